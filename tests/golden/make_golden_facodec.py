"""Writes tests/golden/golden_facodec.npz and keys_facodec_{encoder,decoder}.json from the REAL reference classes
(models/codec/ns3_codec/facodec.py) on the CPU:

    python tests/golden/make_golden_facodec.py /path/to/Amphion

melspec.py imports pyworld, soundfile, librosa and torchaudio's pitch_shift at module level; none of them is used by the classes run here, so
whichever is not installed is stubbed.  The npz holds inputs, outputs and seeds only: the weights regenerate from the seeds (tests/facodec_ref.py: synth_*_state_dict), and the
predictor heads, which inference never runs, keep their own initialisation."""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import codec_ref as C  # noqa: E402
import facodec_ref as R  # noqa: E402

ENC_SEED, DEC_SEED = 11, 23


def stub_imports():
    for name in ("pyworld", "soundfile"):
        sys.modules.setdefault(name, types.ModuleType(name))
    try:
        import librosa.filters  # noqa: F401
    except Exception:
        lr, lrf = types.ModuleType("librosa"), types.ModuleType("librosa.filters")
        lrf.mel = lambda *a, **k: None
        lr.filters = lrf
        sys.modules["librosa"], sys.modules["librosa.filters"] = lr, lrf
    try:
        import torchaudio.functional  # noqa: F401
    except Exception:
        ta, taf = types.ModuleType("torchaudio"), types.ModuleType("torchaudio.functional")
        taf.pitch_shift = lambda *a, **k: None
        ta.functional = taf
        sys.modules["torchaudio"], sys.modules["torchaudio.functional"] = ta, taf


def load_synth(module, sd):
    """the synthetic values under the module's own keys; keys the synthetic dict does not have (the predictor heads) keep their values"""
    full = module.state_dict()
    missing = [k for k in full if k not in sd and not k.startswith(R.PREDICTOR_PREFIXES)]
    extra = [k for k in sd if k not in full]
    assert not missing and not extra, (missing, extra)
    full.update(sd)
    module.load_state_dict(full)
    return module.eval()


def main(amphion_root):
    stub_imports()
    sys.path.insert(0, amphion_root)
    from models.codec.ns3_codec.facodec import FACodecDecoder, FACodecEncoder

    out = {"enc_seed": np.int64(ENC_SEED), "dec_seed": np.int64(DEC_SEED)}
    ehp, dhp = R.small_encoder_hp(), R.small_decoder_hp()
    enc = FACodecEncoder(**ehp)
    dec = FACodecDecoder(**dhp)
    with open(os.path.join(HERE, "keys_facodec_encoder.json"), "w") as f:
        json.dump(list(enc.state_dict()), f, indent=0)
    with open(os.path.join(HERE, "keys_facodec_decoder.json"), "w") as f:
        json.dump(list(dec.state_dict()), f, indent=0)
    load_synth(enc, R.synth_encoder_state_dict(ehp, ENC_SEED))
    load_synth(dec, R.synth_decoder_state_dict(dhp, DEC_SEED))
    with torch.no_grad():
        for T in (230, 240):
            x = C.synth_wave(2, T, 700 + T)
            out[f"x_{T}"] = x.numpy()
            out[f"z_{T}"] = enc(x).numpy()
        z = torch.from_numpy(out["z_240"])
        outs, qs, commit, buf, spk = dec(z, vq=True, eval_vq=True)
        out["fwd_outs"], out["fwd_qs"], out["fwd_spk"] = outs.numpy(), qs.numpy(), spk.numpy()
        for i, b in enumerate(buf):
            out[f"fwd_buf{i}"] = b.numpy()
        out["fwd_commit"] = commit.numpy()
        out["fwd_emb"] = dec.vq2emb(qs).numpy()
        out["fwd_emb_nores"] = dec.vq2emb(qs, use_residual_code=False).numpy()
        out["dec_spk"] = (0.5 * C.synth_latent(2, 256, 1, 801)[:, :, 0]).numpy()
        for n in (1, 7, 33):
            x = C.synth_latent(2, 256, n, 810 + n)
            out[f"dec_x_{n}"] = x.numpy()
            out[f"dec_wav_{n}"] = dec.inference(x, torch.from_numpy(out["dec_spk"])).numpy()
            w = out[f"dec_wav_{n}"]
            print(f"decoder {n} frames: wave {w.shape}, max |w| {np.abs(w).max():.3f}, share beyond 0.99: {(np.abs(w) > 0.99).mean():.3f}")
    np.savez_compressed(os.path.join(HERE, "golden_facodec.npz"), **out)
    print("wrote", {k: getattr(v, "shape", ()) for k, v in out.items()})


if __name__ == "__main__":
    main(sys.argv[1])
