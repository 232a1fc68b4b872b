"""Times Vevo's flow-matching transformer on one GPU at the recipe point (models/vc/vevo/config/Vq8192ToMels.json: mel 128, hidden 1024,
16 layers, 16 heads, MLP 4096, codebook 8192) with synthetic weights, against the same model as torch ops on the same GPU -- the fp32
restatement of tests/fmt_ref.py on the device:

    python tools/bench_fmt.py [--steps 32] [--rounds 3] [--layers 16]

  DiffLlama.forward        one forward at prompt 400 + target 800 frames, B = 1 and B = 4
  reverse_diffusion        the 32-step sampler with classifier-free guidance (64 forwards), same shapes
  amp_rope_attention       vs RoPE in torch + fp32 scaled_dot_product_attention, [B, 16 x 64, 1200]; with its fraction of the f16x3 MFMA
                           peak (838.9 TFLOP/s) counting 4 B H dk T^2 useful flop
  amp_rms_norm_c_adaptive  vs the torch expression
  amp_swiglu               vs silu(gate) * up in torch

Each figure is the median over ``rounds`` of (device events around ``iters`` back-to-back calls) / iters, the two sides alternating round by
round after a warm-up of both -- tools/bench_facodec_vc_ops.py's method.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import fmt_ref as R  # noqa: E402
from amphion_amd import _lib  # noqa: E402
from amphion_amd.models.vc.flow_matching_transformer import FlowMatchingTransformer  # noqa: E402
from amphion_amd.modules import hip_ops  # noqa: E402

PEAK_F16X3 = 2516.6 / 3          # TFLOP/s: dense f16 MFMA / 3 MFMAs per term


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters                  # ms per call


def compare(fns, iters, rounds, warm=2):
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(timed(fn, iters))
    return {k: round(statistics.median(v), 4) for k, v in t.items()}


def synth_model(hp, dev):
    """weights at 1 / sqrt(fan_in) so that the residual stream keeps its magnitude through 16 layers; the adaptive norms near one"""
    g = torch.Generator().manual_seed(7)
    m = FlowMatchingTransformer(**hp)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if "to_weight.bias" in name:
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            elif p.dim() == 2:
                p.copy_(torch.randn(p.shape, generator=g) * (0.5 / p.shape[1] ** 0.5 if "cond_emb" not in name else 0.5))
            else:
                p.copy_(0.02 * torch.randn(p.shape, generator=g))
    return m.to(dev).eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--layers", type=int, default=16)
    ap.add_argument("--prompt", type=int, default=400)
    ap.add_argument("--target", type=int, default=800)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_fmt: needs a ROCm device (a CPU timing says nothing about the kernels)")
    dev = torch.device("cuda:0")
    hp = dict(mel_dim=128, hidden_size=1024, num_layers=args.layers, num_heads=16, cond_codebook_size=8192)
    Tp, Tt = args.prompt, args.target
    T, C, H = Tp + Tt, hp["hidden_size"], hp["num_heads"]
    m = synth_model(hp, dev)
    sd = {k: v.detach() for k, v in m.state_dict().items()}
    out = {"device": torch.cuda.get_device_name(0), "hp": hp, "prompt": Tp, "target": Tt, "unit": "ms per call", "rounds": args.rounds,
           "launches_per_forward": 11 + 8 * args.layers, "precision": _lib.get_precision()}
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for B in (1, 4):
            x = torch.randn(B, T, hp["mel_dim"], generator=g).to(dev)
            t = torch.rand(B, generator=g).to(dev)
            cond = m.cond_emb(torch.randint(0, 8192, (B, T), generator=g).to(dev))
            mask = torch.ones(B, T, device=dev)
            noise = torch.randn(B, Tt, hp["mel_dim"], generator=g).to(dev)
            est = m.diff_estimator
            r = compare({"hip": lambda: est(x, t, cond, mask), "torch_fp32": lambda: R.diffllama_forward(sd, hp, x, t, cond, mask)}, 5, args.rounds)
            r["max_abs_diff"] = float((est(x, t, cond, mask) - R.diffllama_forward(sd, hp, x, t, cond, mask)).abs().max())
            out[f"forward_B{B}"] = r
            r = compare({"hip": lambda: m.reverse_diffusion(cond, x[:, :Tp], n_timesteps=args.steps, cfg=2.0, noise=noise),
                         "torch_fp32": lambda: R.reverse_diffusion(sd, hp, cond, x[:, :Tp], noise, n_timesteps=args.steps, cfg=2.0)}, 1, args.rounds, warm=1)
            out[f"reverse_diffusion_{args.steps}_B{B}"] = r
            # ---- per kernel
            qkv = torch.randn(B, 3 * C, T, generator=g).to(dev)
            cos, sin = hip_ops.rope_tables(T, C // H, dev)
            c2, s2 = torch.cat((cos, cos), -1), torch.cat((sin, sin), -1)

            def torch_attention():
                q, k, v = (y.reshape(B, H, C // H, T).transpose(2, 3) for y in qkv.split(C, 1))
                rope = lambda y: y * c2 + torch.cat((-y[..., 32:], y[..., :32]), -1) * s2
                return F.scaled_dot_product_attention(rope(q), rope(k), v).transpose(2, 3).reshape(B, C, T)

            hip_attention = lambda: hip_ops.rope_attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], H, cos, sin)
            r = compare({"hip": hip_attention, "torch_rope_sdpa_fp32": torch_attention}, 50, args.rounds, warm=5)
            r["max_abs_diff"] = float((hip_attention() - torch_attention()).abs().max())
            r["hip_tflops"] = round(4.0 * B * C * T * T / (r["hip"] * 1e-3) / 1e12, 2)
            r["hip_fraction_of_f16x3_peak"] = round(r["hip_tflops"] / PEAK_F16X3, 4)
            out[f"attention_B{B}"] = r
            h = torch.randn(B, C, T, generator=g).to(dev)
            w = (1.0 + 0.1 * torch.randn(B, C, generator=g)).to(dev)
            out[f"rms_norm_B{B}"] = compare({"hip": lambda: hip_ops.rms_norm_c_adaptive(h, w),
                                             "torch": lambda: w[:, :, None] * (h * torch.rsqrt(h.pow(2).mean(1, keepdim=True) + 1e-6))}, 50,
                                            args.rounds, warm=5)
            gu = torch.randn(B, 8 * C, T, generator=g).to(dev)
            out[f"swiglu_B{B}"] = compare({"hip": lambda: hip_ops.swiglu(gu), "torch": lambda: F.silu(gu[:, :4 * C]) * gu[:, 4 * C:]}, 50,
                                          args.rounds, warm=5)
        _lib.range_check(dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
