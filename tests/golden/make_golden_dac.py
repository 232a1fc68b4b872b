#!/usr/bin/env python
"""Golden vectors for the DAC decoder / encoder stacks from the REAL reference classes (models/codec/dualcodec/dualcodec/model_codec/dac_model.py:
Decoder, Encoder; models/codec/amphion_codec/codec.py: DecoderBlock for the output_padding form), CPU, build container only:
    python tests/golden/make_golden_dac.py -> golden_dac.npz, keys_dac_decoder.json, keys_dac_encoder.json

dac_model.py imports with two tiny stubs (audiotools: AudioSignal and ml.BaseModel = nn.Module; easydict) and its directory mounted as a package
of its own, so that the package __init__ (the DualCodec model, trainers) is never executed.  Two small decoders (tests/dac_ref.py:
small_decoder_hp with odd rates, even_decoder_hp), one small encoder and one Amphion DecoderBlock.  Only inputs and outputs are stored: the
weights come back from the seeds."""
import importlib
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import make_golden_vocos as mgv  # noqa: E402
import dac_ref as D  # noqa: E402

SEEDS = {"small": 81, "even": 82}
LENGTHS = {"small": (1, 7, 33), "even": (33,)}
ENC_SEED, AB_SEED, B = 83, 84, 2


def import_dac_model():
    at, atml, ed = types.ModuleType("audiotools"), types.ModuleType("audiotools.ml"), types.ModuleType("easydict")
    at.AudioSignal = type("AudioSignal", (), {})
    atml.BaseModel = nn.Module
    at.ml = atml
    ed.EasyDict = dict
    sys.modules.update({"audiotools": at, "audiotools.ml": atml, "easydict": ed})
    pkg = types.ModuleType("ref_model_codec")
    pkg.__path__ = [os.path.join(mg.REF, "models", "codec", "dualcodec", "dualcodec", "model_codec")]
    sys.modules["ref_model_codec"] = pkg
    return importlib.import_module("ref_model_codec.dac_model")


def main():
    mgv.install_stubs()
    torch.manual_seed(0)
    dac = import_dac_model()
    from models.codec.amphion_codec.codec import DecoderBlock as AmphionBlock

    out = {}
    for name, hp in (("small", D.small_decoder_hp()), ("even", D.even_decoder_hp())):
        dec = dac.Decoder(**hp).eval()
        if name == "small":
            mg.dump_keys("dac_decoder", dec)
        sd = D.synth_decoder_state_dict(hp, SEEDS[name])
        assert [(k, tuple(v.shape)) for k, v in dec.state_dict().items()] == [(k, tuple(v.shape)) for k, v in sd.items()], "decoder key restatement differs"
        dec.load_state_dict(sd)
        out[f"{name}_seed"] = np.int64(SEEDS[name])
        for T in LENGTHS[name]:
            x = D.C.synth_latent(B, hp["input_channel"], T, SEEDS[name] + T)
            with torch.no_grad():
                y = dec(x)
            out[f"{name}_x_{T}"], out[f"{name}_y_{T}"] = x.numpy(), y.numpy()
            print(name, T, tuple(y.shape), "max", float(y.abs().max()), "rms", float(y.pow(2).mean().sqrt()))
    ehp = D.small_dac_encoder_hp()
    enc = dac.Encoder(**ehp).eval()
    mg.dump_keys("dac_encoder", enc)
    esd = D.synth_dac_encoder_state_dict(ehp, ENC_SEED)
    assert list(enc.state_dict()) == list(esd), "encoder key restatement differs"
    enc.load_state_dict(esd)
    x = D.C.synth_wave(B, 230, ENC_SEED + 1)
    with torch.no_grad():
        z = enc(x)
    out.update(enc_seed=np.int64(ENC_SEED), enc_x=x.numpy(), enc_z=z.numpy())
    # the output_padding form: Amphion's DecoderBlock at an odd stride
    blk = AmphionBlock(64, 32, 3).eval()
    bsd = D.synth_block_state_dict(64, 32, 3, AB_SEED)
    assert [(k, tuple(v.shape)) for k, v in blk.state_dict().items()] == [(k, tuple(v.shape)) for k, v in bsd.items()], "block key restatement differs"
    blk.load_state_dict(bsd)
    x = D.C.synth_latent(B, 64, 33, AB_SEED + 1)
    with torch.no_grad():
        y = blk(x)
    out.update(ab_seed=np.int64(AB_SEED), ab_x=x.numpy(), ab_y=y.numpy())
    print("amphion block", tuple(y.shape))
    np.savez_compressed(os.path.join(HERE, "golden_dac.npz"), **out)


if __name__ == "__main__":
    main()
