#!/usr/bin/env python
"""Golden vectors for the acoustic codec from the REAL reference classes (models/codec/amphion_codec/codec.py: CodecEncoder, CodecDecoder),
CPU, build container only:   python tests/golden/make_golden_codec.py -> golden_codec.npz, keys_codec_encoder.json, keys_codec_decoder.json

A small encoder (tests/codec_ref.py: small_encoder_hp) at two lengths, one a multiple of the hop and one not, and a small decoder whose
quantizer (small_fvq_hp) encodes the encoder's latent.  Only inputs and outputs are stored: the weights come back from the seeds."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import make_golden_vocos as mgv  # noqa: E402
import codec_ref as C  # noqa: E402

ENC_SEED, DEC_SEED, B, LENGTHS = 71, 72, 2, (230, 240)


def main():
    mgv.install_stubs()
    torch.manual_seed(0)
    from models.codec.amphion_codec.codec import CodecDecoder, CodecEncoder

    ehp, fhp = C.small_encoder_hp(), C.small_fvq_hp()
    enc = CodecEncoder(**ehp).eval()
    mg.dump_keys("codec_encoder", enc)
    sd = C.synth_encoder_state_dict(ehp, ENC_SEED)
    assert list(enc.state_dict()) == list(sd), "encoder key restatement differs from the reference"
    enc.load_state_dict(sd)
    dec = CodecDecoder(**C.decoder_kwargs(fhp)).eval()
    mg.dump_keys("codec_decoder", dec)
    dsd = C.decoder_state_dict(fhp, DEC_SEED)
    assert list(dec.state_dict()) == list(dsd), "decoder key restatement differs from the reference"
    dec.load_state_dict(dsd)
    out = {"enc_seed": np.int64(ENC_SEED), "dec_seed": np.int64(DEC_SEED)}
    for T in LENGTHS:
        x = C.synth_wave(B, T, seed=ENC_SEED + T)
        with torch.no_grad():
            z = enc(x)
            zq, codes, _, _, allq = dec(z, vq=True, eval_vq=True)
            emb = dec.vq2emb(codes)
        out[f"x_{T}"] = x.numpy()
        out[f"z_{T}"] = z.numpy()
        out[f"codes_{T}"] = codes.numpy()
        out[f"zq_{T}"] = zq.numpy()
        out[f"emb_{T}"] = emb.numpy()
        print(T, tuple(z.shape), float(z.abs().max()), tuple(codes.shape))
    np.savez_compressed(os.path.join(HERE, "golden_codec.npz"), **out)


if __name__ == "__main__":
    main()
