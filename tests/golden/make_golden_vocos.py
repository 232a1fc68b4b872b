#!/usr/bin/env python
"""Golden vectors for Vocos from the REAL reference class (models/codec/amphion_codec/vocos.py:824-881), CPU, build container
only:   python tests/golden/make_golden_vocos.py -> golden_vocos.npz, keys_vocos.json

Two small nets (tests/vocos_ref.py: small_hp) with the synthetic weights of vocos_ref.synth_vocos_state_dict, once at
n_fft 256 / hop 64 and once at the recipe's 1920 / 480.  Only inputs and outputs are stored: the weights come back from the seed."""
import os
import sys
import types
from unittest.mock import MagicMock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import vocos_ref as V  # noqa: E402

NETS = {"a": dict(n_fft=256, hop=64, seed=41, B=2, F=21), "b": dict(n_fft=1920, hop=480, seed=42, B=1, F=12)}


def install_stubs():
    mg.install_stubs()
    # vocos.py:14 imports torchaudio's mel-scale helpers for the MDCT / IMDCT heads, which no Vocos path builds
    ta = types.ModuleType("torchaudio")
    taf = types.ModuleType("torchaudio.functional")
    tafff = types.ModuleType("torchaudio.functional.functional")
    tafff._hz_to_mel = MagicMock()
    tafff._mel_to_hz = MagicMock()
    ta.functional, taf.functional = taf, tafff
    sys.modules.update({"torchaudio": ta, "torchaudio.functional": taf, "torchaudio.functional.functional": tafff})


def main():
    install_stubs()
    torch.manual_seed(0)
    from models.codec.amphion_codec.vocos import Vocos

    out = {}
    for tag, c in NETS.items():
        hp = V.small_hp(c["n_fft"], c["hop"])
        m = Vocos(**{k: v for k, v in hp.items()}).eval()
        if tag == "a":
            mg.dump_keys("vocos", m)
        sd = V.synth_vocos_state_dict(hp, c["seed"])
        ref_sd = m.state_dict()
        assert list(ref_sd) == list(V.vocos_param_shapes(hp)), "param key restatement differs from reference"
        assert all(tuple(ref_sd[k].shape) == tuple(v.shape) for k, v in sd.items())
        m.load_state_dict(sd)
        x = V.synth_features(c["B"], hp["input_channels"], c["F"], seed=c["seed"] + 1)
        with torch.no_grad():
            y = m(x)
        out[f"{tag}_x"] = x.numpy()
        out[f"{tag}_y"] = y.numpy()
        out[f"{tag}_n_fft"] = np.int64(c["n_fft"])
        out[f"{tag}_hop"] = np.int64(c["hop"])
        out[f"{tag}_seed"] = np.int64(c["seed"])
        print(tag, tuple(y.shape), float(y.abs().max()))
    np.savez_compressed(os.path.join(HERE, "golden_vocos.npz"), **out)


if __name__ == "__main__":
    main()
