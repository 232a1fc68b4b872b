#!/usr/bin/env python
"""Times DualCodec's DAC decoder drop-in (amphion_amd/models/codec/dualcodec/dualcodec/model_codec) and its up-sampling op on one GPU, in one
process, alternating with what it is compared against.

    python tools/dac_bench.py [--rounds 10] [--iters 10] [--json out.json] [--skip-decoder]

(a) Snake -> ConvTranspose1d(k = 2 s, stride s): the fused launch (csrc/tconv_f16x3.hip) against amp_snake -> the polyphase transposed conv,
    through the SAME entry point (amp_tconv_forward) with the route switched at create time, same weights, at B = 16 and the columns that 250
    input frames are at that block of the recipe.  Each route is REPS calls in one captured graph; the two graphs are replayed in alternation
    for --rounds rounds; medians with [min, max].  GFLOP / MB are the launcher's own statement (the launch manifest of a child process,
    --manifest-pass; the manifest is off while timing) and give TFLOP/s and TB/s of the fused launch.  A shape the fused kernel is not built
    for is reported as such, with the two launches' time alone.
(b) The 25 Hz recipe decoder (dualcodec_25hz_16384_1024_12vq.yaml: decoder_dim 1536, rates [8, 6, 5, 4], latent 1024) for B = 1 and B = 16 x 250
    frames against the fp32 torch restatement of tests/dac_ref.py, with x real time at 24 kHz and the launch count.  Synthetic weights."""
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

import codec_ref as C  # noqa: E402
import dac_ref as D  # noqa: E402
from amphion_amd import _lib  # noqa: E402
from amphion_amd.models.codec.amphion_codec.codec import _TransposedConv  # noqa: E402
from amphion_amd.models.codec.dualcodec.dualcodec.model_codec import Decoder  # noqa: E402

F16X3_PEAK_TF = 2500.0 / 3
HBM_TBS = 8.0
REPS = 20
SR = 24000
B_OP, FRAMES = 16, 250
# (cin, cout, stride, input columns): blocks 2, 3 and 1 of the 25 Hz recipe at 250 frames; 96 -> 48 is the last block of the 12.5 Hz recipe
# ([2, 8, 6, 5, 4]) at its 125 frames of the same 10 s
OPS = ((384, 192, 5, FRAMES * 8 * 6), (192, 96, 4, FRAMES * 8 * 6 * 5), (96, 48, 4, 125 * 2 * 8 * 6 * 5), (768, 384, 6, FRAMES * 8))


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
    return ts[len(ts) // 2], ts[0], ts[-1]


def _op(cin, cout, s, mode, like=None):
    _lib.check(_lib.lib().amp_set_tconv_fusion(mode))
    try:
        conv = _TransposedConv(cin, cout, s, D.block_padding(s), 0).cuda()
        if like is not None:
            conv.load_state_dict(like.state_dict())
        conv._handle(torch.device("cuda", torch.cuda.current_device()))
    finally:
        _lib.check(_lib.lib().amp_set_tconv_fusion(-1))
    return conv


def _run(conv, x, alpha, out, ws):
    """amp_tconv_forward with every buffer given: nothing is allocated inside a captured graph's calls that the graph does not own"""
    L = _lib.lib()
    B, _, T = x.shape
    _lib.check(L.amp_tconv_forward(conv._handle(x.device), _lib.ptr(x), B, T, _lib.ptr(alpha), _lib.ptr(ws), ws.numel() * 4 if ws is not None else 0,
                                   _lib.ptr(out), _lib.current_stream_ptr(x.device)))


def _manifest_pass():
    with torch.no_grad():
        for cin, cout, s, T in OPS:
            conv = _op(cin, cout, s, 1)
            if conv.fused(torch.device("cuda", 0)):
                conv(torch.randn(B_OP, cin, T, device="cuda"), torch.ones(cin, device="cuda"))
        torch.cuda.synchronize()


def _manifest():
    man = os.path.join(tempfile.mkdtemp(prefix="dac_bench_"), "manifest.tsv")
    subprocess.run([sys.executable, os.path.abspath(__file__), "--manifest-pass"], env=dict(os.environ, AMP_LAUNCH_MANIFEST=man), check=True, timeout=600)
    with open(man) as f:
        rows = [ln.rstrip("\n").split("\t") for ln in f]
    return [r for r in rows if r[0].startswith("tconv_f16x3_kernel")]


def bench_ops(rounds, res):
    man = _manifest()
    dev = torch.device("cuda", torch.cuda.current_device())
    for cin, cout, s, T in OPS:
        fused = _op(cin, cout, s, 1)
        two = _op(cin, cout, s, 0, like=fused)
        built = fused.fused(dev)
        x = torch.randn(B_OP, cin, T, generator=torch.Generator(device="cuda").manual_seed(cin), device="cuda")
        alpha = (0.5 + 1.5 * torch.rand(cin, device="cuda")).contiguous()
        routes = {}
        for name, conv in (("fused", fused), ("two_launch", two)):
            if name == "fused" and not built:
                continue
            out = torch.empty(B_OP, cout, conv.out_len(T), device="cuda")
            need = _lib.lib().amp_tconv_workspace_bytes(conv._handle(dev), B_OP, T)
            ws = torch.empty(need // 4, device="cuda") if need else None
            _run(conv, x, alpha, out, ws)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for _ in range(REPS):
                    _run(conv, x, alpha, out, ws)
            routes[name] = (g, out, ws)
        ts = {k: [] for k in routes}
        for _ in range(rounds):
            for name in routes:
                ts[name].append(_time(routes[name][0].replay, 1, 1)[0] / REPS)
        row = dict(cin=cin, cout=cout, stride=s, B=B_OP, T=T, rounds=rounds)
        for name, v in ts.items():
            v = sorted(v)
            row[name + "_ms"] = round(v[len(v) // 2], 4)
            row[name + "_min_max_ms"] = [round(v[0], 4), round(v[-1], 4)]
        if built:
            mr = next(r for r in man if f"ConvT {cin}->{cout} " in r[4])
            gf, mb, t = float(mr[2]), float(mr[3]), row["fused_ms"]
            row.update(kernel=mr[0], workgroups=int(mr[1]), gflop=gf, mb=mb, tflops=round(gf / t, 1), frac_f16x3_peak=round(gf / t / F16X3_PEAK_TF, 3),
                       flop_per_byte=round(gf * 1e3 / mb, 1), tb_per_s=round(mb / t / 1e3, 2), frac_hbm=round(mb / t / 1e3 / HBM_TBS, 3),
                       fused_over_two_launch=round(t / row["two_launch_ms"], 3))
            assert float((routes["fused"][1] - routes["two_launch"][1]).abs().max()) <= 1e-3 * float(routes["two_launch"][1].abs().max())
        else:
            row["fused"] = "not built"
        res["ops"].append(row)
        print(json.dumps(row), flush=True)
        del routes, x


def bench_decoder(iters, res):
    hp = dict(D.recipe_decoder_hp(), input_channel=1024)
    sd = D.synth_decoder_state_dict(hp, 1)
    dec = Decoder(**hp)
    dec.load_state_dict(sd)
    dec = dec.cuda().eval()
    dsd = {k: v.cuda() for k, v in sd.items()}
    dev = torch.device("cuda", torch.cuda.current_device())
    for B in (1, 16):
        x = C.synth_latent(B, hp["input_channel"], FRAMES, 7).cuda()
        y = dec(x)
        launches = 3
        for i in range(dec.n_blocks):
            blk = dec.model[1 + i].block
            launches += (1 if blk[1].fused(dev) else 2) + sum(1 if u.fused(dev) else 4 for u in list(blk)[2:])
        t = _time(lambda: dec(x), iters, 2)
        tr = _time(lambda: D.decoder_forward(dsd, hp, x, torch.float32), max(3, iters // 3), 1)
        audio = B * y.shape[2] / SR
        row = dict(B=B, frames=FRAMES, samples=int(y.shape[2]), launches=launches, decoder_ms=round(t[0], 3), decoder_min_max_ms=[round(t[1], 3), round(t[2], 3)],
                   torch_fp32_ms=round(tr[0], 3), torch_min_max_ms=[round(tr[1], 3), round(tr[2], 3)], x_realtime=round(audio / t[0] * 1e3, 1),
                   speedup_vs_torch=round(tr[0] / t[0], 2))
        res["decoder"].append(row)
        print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--json", default=None)
    ap.add_argument("--skip-decoder", action="store_true")
    ap.add_argument("--manifest-pass", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.manifest_pass:
        return _manifest_pass()
    assert not os.environ.get("AMP_LAUNCH_MANIFEST"), "time with the launch manifest off"
    res = {"ops": [], "decoder": []}
    with torch.no_grad():
        bench_ops(a.rounds, res)
        if not a.skip_decoder:
            bench_decoder(a.iters, res)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
