"""Writes tests/golden/golden_tokenizers.npz and keys_repcodec.json, keys_coco.json, keys_vevo_repcodec.json from the REAL reference classes
(models/codec/kmeans/repcodec_model.py, models/codec/coco/rep_coco_model.py, models/codec/vevo/vevo_repcodec.py) on the CPU:

    python tests/golden/make_golden_tokenizers.py /path/to/Amphion

The reference imports einops; the other imports are stubbed as for Vocos (make_golden_vocos.install_stubs).  The npz holds outputs and seeds
only: the weights and the inputs regenerate from the seeds (tests/tokenizer_ref.py: synth_*_state_dict, synth_feats)."""
import json
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden_vocos as mgv  # noqa: E402
import tokenizer_ref as R  # noqa: E402

SEED = 53
B = 2


def dump_keys(name, model):
    with open(os.path.join(HERE, f"keys_{name}.json"), "w") as f:
        json.dump(list(model.state_dict()), f, indent=0)


def main(root):
    mgv.install_stubs()
    sys.path.insert(0, root)
    warnings.simplefilter("ignore")
    from models.codec.coco.rep_coco_model import CocoContentStyle
    from models.codec.kmeans.repcodec_model import RepCodec
    from models.codec.vevo.vevo_repcodec import VevoRepCodec

    torch.manual_seed(0)
    out = dict(seed=np.int64(SEED))

    def load(model, sd):
        assert list(model.state_dict()) == list(sd), "the key restatement differs from the reference"
        model.load_state_dict(sd)
        return model.eval()

    dump_keys("repcodec", RepCodec(**dict(R.small_repcodec_hp(), downsample_scale=2)))
    nets = R.golden_models(SEED)
    rep = {K: load(RepCodec(**nets[f"rep{K}"][0]), nets[f"rep{K}"][1]) for K in (64, 8192)}
    coco = CocoContentStyle(cfg=R.coco_cfg(nets["coco"][0]))
    dump_keys("coco", coco)
    load(coco, nets["coco"][1])
    vevo = VevoRepCodec(**nets["vevo"][0])
    dump_keys("vevo_repcodec", vevo)
    load(vevo, nets["vevo"][1])
    vevo.quantizer.initial()

    with torch.no_grad():
        for T in R.GOLDEN_LENGTHS:
            x = R.golden_inputs(T, B)
            for K, m in rep.items():
                codes, zq = m.quantize(x["rep"])
                x_rec, loss, all_idx = m(x["rep"])
                assert codes.shape == (B, T) and all_idx.shape == (1, B, T) and torch.equal(all_idx[0], codes)
                out[f"rep{K}_codes_{T}"] = codes.numpy().astype(np.int16)
                if K == 64:                       # the latent does not depend on the codebooks
                    out[f"rep_z_{T}"] = m.encoder(x["rep"].transpose(1, 2)).transpose(1, 2).numpy()
                    out[f"rep_rec_{T}"] = x_rec.numpy()
            codes, zq = coco.quantize(x["whisper"], x["chroma"])
            w_rec, c_rec, loss, all_idx = coco(x["whisper"], x["chroma"])
            assert w_rec.shape == (B, T, 64) and c_rec.shape == (B, T, 24) and torch.equal(all_idx[0], codes)
            h = coco.whisper_input_layer(x["whisper"]) + coco.chromagram_input_layer(x["chroma"])
            out[f"coco_z_{T}"] = coco.encoder(coco.downsample_layers(h.transpose(1, 2))).transpose(1, 2).numpy()
            out[f"coco_codes_{T}"] = codes.numpy().astype(np.int16)
            out[f"coco_zq_{T}"] = zq.numpy()
            out[f"coco_whisper_{T}"] = w_rec.numpy()
            out[f"coco_chroma_{T}"] = c_rec.numpy()
            z = vevo.projector(vevo.encoder(x["vevo"]))
            y, zq, z2, vqloss, perplexity = vevo(x["vevo"])
            _, idx = vevo.quantizer.codebook.forward_index(z.transpose(2, 1))
            assert torch.equal(z, z2)
            out[f"vevo_z_{T}"] = z.numpy()
            out[f"vevo_codes_{T}"] = idx.numpy().astype(np.int16)
            out[f"vevo_y_{T}"] = y.numpy()
            out[f"vevo_loss_{T}"] = vqloss.numpy()
            out[f"vevo_perplexity_{T}"] = perplexity.numpy()
    path = os.path.join(HERE, "golden_tokenizers.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
