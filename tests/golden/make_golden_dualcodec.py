#!/usr/bin/env python
"""Golden vectors for DualCodec from the REAL reference classes (models/codec/dualcodec/dualcodec/model_codec/: DualCodec, DAC,
ResidualVectorQuantize, ConvNeXtBlock), CPU, build container only:
    python tests/golden/make_golden_dualcodec.py -> golden_dualcodec.npz, keys_dualcodec.json, keys_dac_rvq.json

The model_codec directory is mounted as a package of its own with the audiotools / easydict stubs of make_golden_dac.py, so the package __init__
(trainers, discriminators) is never executed.  The small net of tests/dualcodec_ref.py: small_hp, built once with is_causal=True and once with
False; B = 2, T = 9 and 33 frames.  The DAC latent is 1024 wide: convnext_decoder's last conv fixes it (see dualcodec_ref).  Inputs and weights
come back from the seeds; only outputs are stored (the [B, 1024, T] quantized latent for T = 9 of the causal net alone, to keep the file small)."""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import make_golden_dac as mgd  # noqa: E402
import make_golden_vocos as mgv  # noqa: E402
import dualcodec_ref as R  # noqa: E402

SEED, B, LENGTHS = 700, 2, (9, 33)


def main():
    mgv.install_stubs()
    torch.manual_seed(0)
    mgd.import_dac_model()
    dm = importlib.import_module("ref_model_codec.dualcodec_model")
    dq = importlib.import_module("ref_model_codec.dac_quantize")
    cnn = importlib.import_module("ref_model_codec.cnn")
    out = {"seed": np.int64(SEED)}
    for causal in (True, False):
        tag = "causal" if causal else "centred"
        hp = R.small_hp(causal)
        model = dm.DualCodec(**hp).eval()
        sd = R.synth_dualcodec_state_dict(hp, SEED)
        have = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
        assert have == [(k, tuple(v.shape)) for k, v in sd.items()], "DualCodec key restatement differs"
        if causal:
            mg.dump_keys("dualcodec", model)
            mg.dump_keys("dac_rvq", model.dac.quantizer)
        model.load_state_dict(sd)
        for T in LENGTHS:
            wave, feats = R.synth_inputs(hp, B, T, SEED + 10 + T)
            with torch.no_grad():
                h = model.convnext_encoder(feats)
                sem_only = model.semantic_quantize(feats)
                sem, ac = model.encode(wave, semantic_repr=feats)
                sem2, ac2 = model.encode(wave, num_quantizers=2, semantic_repr=feats)
                audio = model.decode_from_codes(sem, ac)
                audio_sem = model.decode_from_codes(sem, None)
                semantic = model.convnext_decoder(model.semantic_vq.from_codes(sem)[0])
                z, codes, latents, closs, bloss, first = model.dac.encode(wave, sample_rate=hp["sample_rate"], subtracted_latent=semantic)
            assert torch.equal(sem_only, sem[:, 0]) and torch.equal(codes, ac) and torch.equal(sem2, sem) and torch.equal(ac2, ac[:, :1])
            p = f"{tag}_{T}_"
            out.update({p + "cn_enc": h.numpy(), p + "sem_codes": sem.numpy(), p + "ac_codes": ac.numpy(), p + "wave": audio.numpy(),
                        p + "wave_sem": audio_sem.numpy(), p + "latents": latents.numpy(), p + "losses": np.array([float(closs), float(bloss)])})
            if causal and T == LENGTHS[0]:
                out.update({p + "z": z.numpy(), p + "first": first.numpy()})
            print(tag, T, "wave", tuple(audio.shape), "max", float(audio.abs().max()), "codes", tuple(ac.shape))
        # one block on its own, with a layer scale (gamma present)
        blk = cnn.ConvNeXtBlock(dim=64, intermediate_dim=R.INTERMEDIATE, layer_scale_init_value=0.5, is_causal=causal).eval()
        bsd = R.synth_convnext_block(64, "", SEED + 50, gamma=True)
        assert [(k, tuple(v.shape)) for k, v in blk.state_dict().items()] == [(k, tuple(v.shape)) for k, v in bsd.items()], "block keys differ"
        blk.load_state_dict(bsd)
        x = R.C.synth_latent(B, 64, 33, SEED + 51)
        with torch.no_grad():
            out[f"{tag}_blk_y"] = blk(x).numpy()
    # the quantizer alone, fewer levels
    qhp = dict(D=64, d=8, K=64, N=3, l2=True)
    rvq = dq.ResidualVectorQuantize(input_dim=64, n_codebooks=3, codebook_size=64, codebook_dim=8).eval()
    qsd = R.synth_rvq_state_dict(qhp, SEED + 60)
    assert list(rvq.state_dict()) == list(qsd), "rvq key restatement differs"
    rvq.load_state_dict(qsd)
    z = R.C.synth_latent(B, 64, 33, SEED + 61)
    with torch.no_grad():
        zq, codes, latents, closs, bloss, first = rvq(z, n_quantizers=2)
        back = rvq.from_codes(codes)
    out.update(rvq_zq=zq.numpy(), rvq_codes=codes.numpy(), rvq_latents=latents.numpy(), rvq_first=first.numpy(),
               rvq_losses=np.array([float(closs), float(bloss)]), rvq_from_codes=back[0].numpy(), rvq_z_p=back[1].numpy())
    # the feature preparation as the inference class writes it
    hidden, mean, std = R.synth_hidden(B, 9, 64, SEED + 70)
    out["prep"] = torch.nn.functional.avg_pool1d(((hidden - mean) / std).transpose(1, 2), 2, 2).numpy()
    np.savez_compressed(os.path.join(HERE, "golden_dualcodec.npz"), **out)
    print("bytes", os.path.getsize(os.path.join(HERE, "golden_dualcodec.npz")))


if __name__ == "__main__":
    main()
