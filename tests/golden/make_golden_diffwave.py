#!/usr/bin/env python
"""Golden vectors for DiffWave from the REAL reference classes (models/vocoders/diffusion/diffwave/diffwave.py and
models/vocoders/diffusion/diffusion_vocoder_inference.py), CPU, build container only:
    python tests/golden/make_golden_diffwave.py -> golden_diffwave.npz, keys_diffwave.json
Weights come back from the seed (tests/diffwave_ref.py: synth_state_dict); only inputs, the recorded noise and outputs are stored."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import diffwave_ref as D  # noqa: E402

# tag -> net, seed, forward batch / frames, sampler frames.  "wide" has the full dilation cycle: d = 512 spans eight 64-column tiles, and
# its one-frame sampler case (L = 256) is shorter than the dilation itself
CASES = {"small": dict(hp=D.SMALL, seed=51, B=2, F=40, Fs=24, full=True), "wide": dict(hp=D.WIDE, seed=52, B=1, F=5, Fs=1, full=False)}


def record_noise(seed, B, L, steps):
    """the draws vocoder_inference makes after torch.manual_seed(seed): randn(B, L), then randn_like per step with n > 0"""
    torch.manual_seed(seed)
    return [torch.randn(B, L) for _ in range(steps)]


def main():
    mg.install_stubs()
    from unittest.mock import MagicMock

    for name in ("json5", "ruamel", "ruamel.yaml"):       # utils/util.py imports them for config files; the sampler needs none
        try:
            __import__(name)
        except ImportError:
            sys.modules[name] = MagicMock()
    try:
        import tqdm  # noqa: F401
    except ImportError:
        sys.modules["tqdm"] = MagicMock(tqdm=lambda x, *a, **k: x)
    from models.vocoders.diffusion.diffwave.diffwave import DiffWave
    from models.vocoders.diffusion.diffusion_vocoder_inference import vocoder_inference

    out = {}
    for tag, c in CASES.items():
        hp = c["hp"]
        cfg = D.make_cfg(**hp)
        m = DiffWave(cfg).eval()
        if tag == "small":
            mg.dump_keys("diffwave", m)
        sd = D.synth_state_dict(hp["C"], hp["N"], hp["n_mel"], hp["u"], c["seed"], out_gain=D.OUT_GAIN[tag])
        assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == list(D.param_shapes(hp["C"], hp["N"], hp["n_mel"], hp["u"]).items())
        m.load_state_dict(sd)
        assert torch.equal(m.diffusion_embedding.embedding, D.embedding_table(50))
        hop = hp["u"][0] * hp["u"][1]
        mel = D.synth_mel(c["B"], hp["n_mel"], c["F"], c["seed"] + 1)
        g = torch.Generator().manual_seed(c["seed"] + 2)
        audio = torch.randn(c["B"], c["F"] * hop, generator=g)
        with torch.no_grad():
            y_int = m(audio, torch.tensor([7]), mel)
            y_flt = m(audio, torch.tensor([10.452], dtype=torch.float32), mel)
        out[f"{tag}_mel"], out[f"{tag}_audio"] = mel.numpy(), audio.numpy()
        out[f"{tag}_y_int"], out[f"{tag}_y_flt"] = y_int.numpy(), y_flt.numpy()
        out[f"{tag}_seed"] = np.int64(c["seed"])
        smel = D.synth_mel(1, hp["n_mel"], c["Fs"], c["seed"] + 3)
        out[f"{tag}_smel"] = smel.numpy()
        for fast in ([True, False] if c["full"] else [True]):
            steps = 6 if fast else 50
            name = f"{tag}_{'fast' if fast else 'full'}"
            torch.manual_seed(c["seed"] + 4)
            wav = vocoder_inference(cfg, m, smel, device="cpu", fast_inference=fast)
            noise = record_noise(c["seed"] + 4, 1, c["Fs"] * hop, steps)
            out[name + "_noise"] = torch.stack(noise).numpy()
            out[name + "_wav"] = wav.numpy()
            print(name, tuple(wav.shape), "clamped", float((wav.abs() == 1).float().mean()))
        print(tag, float(y_int.abs().max()), float(y_int.pow(2).mean().sqrt()))
    np.savez_compressed(os.path.join(HERE, "golden_diffwave.npz"), **out)


if __name__ == "__main__":
    main()
