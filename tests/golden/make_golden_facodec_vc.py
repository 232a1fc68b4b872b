"""Writes tests/golden/golden_facodec_vc.npz and keys_facodec_{encoder_v2,decoder_v2,redecoder}.json from the REAL reference classes
(models/codec/ns3_codec/facodec.py: FACodecEncoderV2, FACodecDecoderV2, FACodecRedecoder) on the CPU:

    python tests/golden/make_golden_facodec_vc.py /path/to/Amphion

The import stubs are make_golden_facodec.py's, with one difference: MelSpectrogram calls ``librosa.filters.mel``, and where librosa is not installed
the stub hands the reference THIS project's ``librosa_mel_fn`` (amphion_amd/utils/mel.py), the restatement of librosa 0.9.1's filterbank that
tests/test_oracle_golden.py pins against recorded librosa output.  So the golden mel is the reference's STFT / magnitude / log chain on that
filterbank.  The npz holds inputs, outputs and seeds only: the weights regenerate from the seeds (tests/facodec_vc_ref.py: synth_*_state_dict),
and the predictor heads, which inference never runs, keep their own initialisation.

FACodecRedecoder.forward cannot be run as written: it transposes its [B, T, d] sum to [B, d, T] BEFORE ``timbre_norm`` (facodec.py:726-728), so
LayerNorm(256) meets the time axis and raises unless T == 256 (where it would normalise over time).  ``forward_as_meant`` below runs the real
module's own submodules in forward's own order and summation grouping (facodec.py:698-722) and hands the sum, channel-first, to the real
``inference`` -- the norm over the channel axis, as ``vq2emb`` + ``inference`` apply it.  The ``red_fwd_*`` entries come from it."""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import codec_ref as C  # noqa: E402
import facodec_ref as R  # noqa: E402
import facodec_vc_ref as V  # noqa: E402
from make_golden_facodec import load_synth, stub_imports  # noqa: E402

ENC_SEED, DEC_SEED, RED_SEED = 31, 37, 41
FRAMES = (1, 7, 33)


def stub_librosa_mel():
    from amphion_amd.utils.mel import librosa_mel_fn

    try:
        import librosa.filters  # noqa: F401
    except Exception:
        lr, lrf = types.ModuleType("librosa"), types.ModuleType("librosa.filters")
        lrf.mel = librosa_mel_fn
        lr.filters = lrf
        sys.modules["librosa"], sys.modules["librosa.filters"] = lr, lrf
        print("librosa is not installed: the reference's MelSpectrogram gets amphion_amd.utils.mel.librosa_mel_fn")


def forward_as_meant(red, vq, spk, use_residual_code):
    x_p = 0
    for i in range(red.vq_num_q_p):
        x_p = x_p + red.prosody_embs[i](vq[i])
    x = 0 + red.timbre_cond_prosody_enc(x_p, key_padding_mask=None, condition=spk.unsqueeze(1).expand(-1, x_p.shape[1], -1))
    x_c = 0
    for i in range(red.vq_num_q_c):
        x_c = x_c + red.content_embs[i](vq[red.vq_num_q_p + i])
    x = x + x_c
    if use_residual_code:
        x_r = 0
        for i in range(red.vq_num_q_r):
            x_r = x_r + red.residual_embs[i](vq[red.vq_num_q_p + red.vq_num_q_c + i])
        x = x + x_r
    return red.inference(x.transpose(1, 2), spk)


def main(amphion_root):
    stub_librosa_mel()
    stub_imports()
    sys.path.insert(0, amphion_root)
    from models.codec.ns3_codec.facodec import FACodecDecoderV2, FACodecEncoderV2, FACodecRedecoder

    out = {"enc_seed": np.int64(ENC_SEED), "dec_seed": np.int64(DEC_SEED), "red_seed": np.int64(RED_SEED)}
    ehp, dhp, rhp = R.small_encoder_hp(), R.small_decoder_hp(), V.small_redecoder_hp()
    enc, dec, red = FACodecEncoderV2(**ehp), FACodecDecoderV2(**dhp), FACodecRedecoder(**rhp)
    for name, m in (("encoder_v2", enc), ("decoder_v2", dec), ("redecoder", red)):
        with open(os.path.join(HERE, f"keys_facodec_{name}.json"), "w") as f:
            json.dump(list(m.state_dict()), f, indent=0)
    load_synth(enc, V.synth_encoder_v2_state_dict(ehp, ENC_SEED))
    load_synth(dec, V.synth_decoder_v2_state_dict(dhp, DEC_SEED))
    load_synth(red, V.synth_redecoder_state_dict(rhp, RED_SEED))
    with torch.no_grad():
        # the encoder's block (shared with FACodecEncoder) and the prosody feature at the GPU tests' lengths
        x = C.synth_wave(2, 230, 1230)
        out["x_230"], out["z_230"] = x.numpy(), enc(x).numpy()
        for L in (600, 1000, 1601):
            w = C.synth_wave(2, L, 1300 + L)
            out[f"wave_{L}"] = w.numpy()
            out[f"pf_{L}"] = enc.get_prosody_feature(w).numpy()
        # FACodecDecoderV2.forward at 33 frames
        x, pf = C.synth_latent(2, 256, 33, 1401), V.synth_prosody_feature(2, 33, 1402)
        outs, qs, commit, buf, spk = dec(x, pf, vq=True, eval_vq=True)
        out["fwd_x"], out["fwd_pf"] = x.numpy(), pf.numpy()
        out["fwd_outs"], out["fwd_qs"], out["fwd_spk"], out["fwd_commit"] = outs.numpy(), qs.numpy(), spk.numpy(), commit.numpy()
        out["fwd_buf0"] = buf[0].numpy()
        out["fwd_emb_nores"] = dec.vq2emb(qs, use_residual=False).numpy()
        # waves: V2 inference and the redecoder's three methods
        spk = 0.5 * C.synth_latent(2, 256, 1, 1501)[:, :, 0]
        out["spk"] = spk.numpy()
        for n in FRAMES:
            x = C.synth_latent(2, 256, n, 1510 + n)
            vq = V.synth_codes(rhp, 2, n, 1520 + n)
            out[f"x_{n}"], out[f"vq_{n}"] = x.numpy(), vq.numpy()
            out[f"v2_wav_{n}"] = dec.inference(x, spk).numpy()
            out[f"red_inf_wav_{n}"] = red.inference(x, spk).numpy()
            for res in (False, True):
                out[f"red_fwd_wav_{n}_{int(res)}"] = forward_as_meant(red, vq, spk, res).numpy()
                if n < 33 or res:
                    out[f"red_emb_{n}_{int(res)}"] = red.vq2emb(vq, spk, use_residual=res).numpy()
            w = out[f"red_fwd_wav_{n}_1"]
            print(f"redecoder {n} frames: wave {w.shape}, max |w| {np.abs(w).max():.3f}, share beyond 0.99: {(np.abs(w) > 0.99).mean():.3f}")
    np.savez_compressed(os.path.join(HERE, "golden_facodec_vc.npz"), **out)
    print("wrote", {k: getattr(v, "shape", ()) for k, v in out.items()})


if __name__ == "__main__":
    main(sys.argv[1])
