"""Times the two kernels of FACodec's voice-conversion classes against the torch sequences they replace, on one GPU:

    python tools/bench_facodec_vc_ops.py [--iters 300] [--rounds 7]

  style LayerNorm   amp_layer_norm_c_style                    vs  amp_layer_norm_c (gamma = 1, beta = 0) -> torch mul -> torch add
                                                                   (FACodecDecoder.inference's route)
  embedding sum     amp_embed_sum_c, N = 2 without init and    vs  N x F.embedding + adds (+ the [B, T, D] stream) -> transpose -> contiguous
                    N = 5 onto a [B, D, T] stream
at the recipe's shape: 256 channels, 500 frames, B = 1 and 16.  Each figure is the median over ``rounds`` of (device events around ``iters``
back-to-back calls) / iters, the two sides alternating round by round after a warm-up of both; at these sizes a call is a few microseconds of
kernel behind a launch, so the figure is the cost of a call in a stream of calls, not kernel time.  The embedding sum is timed at the C entry
(launch only) and through ``hip_ops.embed_sum_c`` (launch + the index check, which synchronises).  Prints one JSON line."""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from amphion_amd import _lib  # noqa: E402
from amphion_amd.modules import hip_ops  # noqa: E402


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / iters          # us per call


def compare(fns, iters, rounds):
    for fn in fns.values():
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(timed(fn, iters))
    return {k: round(statistics.median(v), 2) for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_facodec_vc_ops: needs a ROCm device (a CPU timing says nothing about the kernels)")
    dev = torch.device("cuda:0")
    L = _lib.lib()
    C_, T, K = 256, 500, 1024
    out = {"device": torch.cuda.get_device_name(0), "C": C_, "T": T, "unit": "us per call", "iters": args.iters, "rounds": args.rounds}
    g = torch.Generator().manual_seed(1)
    for B in (1, 16):
        x = torch.randn(B, C_, T, generator=g).to(dev)
        style = torch.randn(B, 2 * C_, generator=g).to(dev)
        gamma, beta = style[:, :C_, None].contiguous(), style[:, C_:, None].contiguous()
        one, zero = torch.ones(C_, device=dev), torch.zeros(C_, device=dev)
        r = compare({"hip": lambda: hip_ops.layer_norm_c_style(x, style),
                     "torch_sequence": lambda: hip_ops.layer_norm_c(x, one, zero) * gamma + beta}, args.iters, args.rounds)
        want = hip_ops.layer_norm_c(x, one, zero) * gamma + beta
        r["max_abs_diff"] = float((hip_ops.layer_norm_c_style(x, style) - want).abs().max())
        out[f"style_layer_norm_B{B}"] = r
        for N, with_init in ((2, False), (5, True)):
            tables = [torch.randn(K, C_, generator=g).to(dev) for _ in range(N)]
            codes = torch.randint(0, K, (N, B, T), generator=g).to(dev)
            init = torch.randn(B, C_, T, generator=g).to(dev) if with_init else None
            init_bt = init.transpose(1, 2).contiguous() if with_init else None
            flag = torch.zeros(1, dtype=torch.int32, device=dev)
            y = torch.empty(B, C_, T, device=dev)
            ptrs = (ctypes.c_void_p * N)(*[w.data_ptr() for w in tables])
            rows = (ctypes.c_int * N)(*[K] * N)
            st = _lib.current_stream_ptr(dev)

            def entry():
                _lib.check(L.amp_embed_sum_c(_lib.ptr(codes), N, ptrs, rows, C_, _lib.ptr(init), B, T, _lib.ptr(y), _lib.ptr(flag), st))

            def torch_seq():
                acc = init_bt
                for n in range(N):
                    e = F.embedding(codes[n], tables[n])
                    acc = e if acc is None else acc + e
                return acc.transpose(1, 2).contiguous()

            r = compare({"hip_entry": entry, "hip_wrapper_with_check": lambda: hip_ops.embed_sum_c(codes, tables, init), "torch_sequence": torch_seq},
                        args.iters, args.rounds)
            r["bit_identical"] = bool(torch.equal(hip_ops.embed_sum_c(codes, tables, init), torch_seq()))
            out[f"embed_sum_N{N}_B{B}"] = r
    print(json.dumps(out))


if __name__ == "__main__":
    main()
