#!/usr/bin/env python
"""DiffWave sampler on one MI355X: ms per sampler call and x real time for the recipe net (C = 64, N = 30), this library against the
same restatement (tests/diffwave_ref.py) run by torch in fp32 on the same GPU.

    python tools/diffwave_bench.py [--batch 16] [--frames 256] [--full] [--iters 3] [--precision f16x3|f32] [--no-torch]

Layer kernel per dilation: run under `rocprofv3 --kernel-trace --stats` with AMP_LAUNCH_MANIFEST set and join with tools/roofline_table.py."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import diffwave_ref as D  # noqa: E402


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return sorted(ts)[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--full", action="store_true", help="the 50-step schedule (default: the recipe's 6-step fast schedule)")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--precision", default="f16x3")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--sample-rate", type=int, default=24000)
    a = ap.parse_args()
    from amphion_amd import _lib
    from amphion_amd.models.vocoders.diffusion.diffusion_vocoder_inference import vocoder_inference
    from amphion_amd.models.vocoders.diffusion.diffwave.diffwave import DiffWave

    _lib.set_precision(a.precision)
    hp = D.RECIPE
    sd = D.synth_state_dict(hp["C"], hp["N"], hp["n_mel"], hp["u"], 53)
    m = DiffWave(D.make_cfg(**hp))
    m.load_state_dict(sd)
    m = m.to("cuda:0").eval()
    cfg = m.cfg
    mel = D.synth_mel(a.batch, hp["n_mel"], a.frames, 1).to("cuda:0")
    L = a.frames * 256
    steps = 50 if a.full else 6
    noise = [torch.randn(a.batch, L, device="cuda:0") for _ in range(steps)]
    ours = timed(lambda: vocoder_inference(cfg, m, mel, device="cuda:0", fast_inference=not a.full, noise=noise), a.iters)
    seconds = a.batch * L / a.sample_rate
    res = {"batch": a.batch, "frames": a.frames, "steps": steps, "precision": a.precision, "ms": round(ours, 3), "x_real_time": round(seconds * 1e3 / ours, 2)}
    if not a.no_torch:
        sdg = {k: v.to("cuda:0") for k, v in sd.items()}
        table = D.embedding_table(50).to("cuda:0")
        orig = torch.tensor
        with torch.no_grad():
            torch.tensor = lambda *x, **k: orig(*x, **{**k, "device": k.get("device", "cuda:0")})   # the restatement's step tensors
            try:
                ref = timed(lambda: D.sample(sdg, hp, table, cfg, mel, noise, not a.full).cpu(), a.iters)
            finally:
                torch.tensor = orig
        res.update(torch_fp32_ms=round(ref, 3), speedup=round(ref / ours, 3))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
