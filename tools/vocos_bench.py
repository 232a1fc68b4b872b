#!/usr/bin/env python
"""Times the Vocos drop-in (amphion_amd/models/codec/amphion_codec/vocos.py) against an fp32 torch restatement of the same module
on the same GPU, and the pointwise GEMM launches against the nominal f16x3 peak.

    python tools/vocos_bench.py [--iters 20] [--warmup 3] [--json out.json]

Cases: the recipe net (egs/vocoder/vocos/emilia_singnet.json) at B = 16 x F = 256 (82 s of 24 kHz audio) and a single utterance at
F = 250.  Synthetic weights (tests/vocos_ref.py).  Timed with the launch manifest OFF.  The pointwise kernel is timed alone as
REPS launches captured in one graph and replayed between two events (the per-launch figure is GPU time divided by REPS, without
the host's dispatch of each call); its GFLOP come from the launch manifest of a separate child process (--manifest-pass).  The nominal f16x3 peak is the f16
dense MFMA peak / 3 (2.5 PF / 3)."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import vocos_ref as V  # noqa: E402
from amphion_amd.models.codec.amphion_codec.vocos import Vocos, _PwHandle, pw_forward  # noqa: E402

F16X3_PEAK_TF = 2500.0 / 3


def _time(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ts = []
    for _ in range(iters):
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        ts.append(ev[0].elapsed_time(ev[1]))
    ts.sort()
    return ts[len(ts) // 2]


REPS = 20
SIZES = ((16, 256), (1, 250))


def _pw_shapes(hp):
    return ((hp["dim"], hp["intermediate_dim"], 1), (hp["intermediate_dim"], hp["dim"], 2), (hp["dim"], hp["n_fft"] + 2, 0))


def _pw_case(cin, cout, epi, B, F):
    lin = torch.nn.Linear(cin, cout)
    xi = torch.randn(B, cin, F, device="cuda")
    yo = torch.randn(B, cout, F, device="cuda")
    gam = torch.full((cout,), 0.03, device="cuda")
    h = _PwHandle()
    if epi == 2:
        return lambda: pw_forward(h, lin, xi, epi, yo, gamma=gam, res=yo)
    return lambda: pw_forward(h, lin, xi, epi, yo)


def _manifest_pass():
    """one launch of each pointwise case; this process runs with AMP_LAUNCH_MANIFEST set by the parent"""
    hp = V.recipe_hp()
    for B, F in SIZES:
        for cin, cout, epi in _pw_shapes(hp):
            _pw_case(cin, cout, epi, B, F)()
    torch.cuda.synchronize()


def _manifest_rows():
    man = os.path.join(tempfile.mkdtemp(prefix="vocos_bench_"), "manifest.tsv")
    env = dict(os.environ, AMP_LAUNCH_MANIFEST=man)
    subprocess.run([sys.executable, os.path.abspath(__file__), "--manifest-pass"], env=env, check=True, timeout=300)
    with open(man) as f:
        return [ln.rstrip("\n").split("\t") for ln in f if ln.startswith("pw_")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--manifest-pass", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.manifest_pass:
        return _manifest_pass()
    assert not os.environ.get("AMP_LAUNCH_MANIFEST"), "time with the launch manifest off"
    rows = iter(_manifest_rows())
    hp = V.recipe_hp()
    sd = V.synth_vocos_state_dict(hp, 11)
    m = Vocos(**hp)
    m.load_state_dict(sd)
    m = m.cuda().eval()
    sd_dev = {k: v.cuda() for k, v in sd.items()}
    res = {"cases": [], "pw": []}
    for B, F in SIZES:
        x = V.synth_features(B, hp["input_channels"], F, seed=1).cuda()
        with torch.no_grad():
            t_hip = _time(lambda: m(x), a.iters, a.warmup)
            t_ref = _time(lambda: V.vocos_forward(sd_dev, hp, x, dtype=torch.float32), max(3, a.iters // 4), 1)
            err = (m(x).double() - V.vocos_forward(sd_dev, hp, x, dtype=torch.float64)).abs().max().item()
        audio_s = B * F * hp["hop_size"] / 24000.0
        gflop = 2.0 * B * F * (hp["input_channels"] * 7 * hp["dim"] + hp["num_layers"] * 2 * hp["dim"] * hp["intermediate_dim"]
                               + hp["dim"] * (hp["n_fft"] + 2))
        row = dict(B=B, F=F, audio_s=round(audio_s, 2), hip_ms=round(t_hip, 3), torch_fp32_ms=round(t_ref, 3), speedup=round(t_ref / t_hip, 2),
                   x_realtime=round(audio_s / (t_hip / 1e3), 1), tflops=round(gflop / t_hip / 1e9, 1), max_abs_vs_fp64=err)
        res["cases"].append(row)
        print(json.dumps(row))
        # the pointwise launches of this shape, alone
        for cin, cout, epi in _pw_shapes(hp):
            fn = _pw_case(cin, cout, epi, B, F)
            fn()                                                   # create the handle outside the capture
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for _ in range(REPS):
                    fn()
            t = _time(g.replay, max(3, a.iters // 4), 1) / REPS
            name, wgs, gf = next(rows)[:3]
            tf = float(gf) / t
            pr = dict(B=B, F=F, shape=f"{cin}->{cout}", epi=epi, kernel=name, workgroups=int(wgs), gflop=float(gf), ms=round(t, 4),
                      tflops=round(tf, 1), frac_f16x3_peak=round(tf / F16X3_PEAK_TF, 3))
            res["pw"].append(pr)
            print(json.dumps(pr))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
