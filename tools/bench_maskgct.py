"""Times MaskGCT's two models on one GPU at the recipe points (models/tts/maskgct/config/maskgct.json: T2S hidden 1536 / 16 heads / 16 layers over a
codebook of 8192; S2A 1024 / 16 / 16 over 1024) with synthetic weights: 120 phones, prompt 250, target 500 frames, B = 1 and 4:

    python tools/bench_maskgct.py [--rounds 3] [--layers 16] [--t2s-steps 25] [--s2a-steps 25,10,1,1,1,1,1,1,1,1,1,1]

  step                 one decoding step: the input's embedding sum, both forwards, the guidance, the logits GEMM, the sampler, the re-masking
  reverse_diffusion    the whole sampler at the recipe's step counts (maskgct_utils.py: 25 for T2S; 25, 10, then 1 per layer for S2A; cfg 2.5, rescale 0.75)
  attention_96         amp_rope_attention at dk = 96 against RoPE in torch + fp32 scaled_dot_product_attention, [B, 16 x 96, 870]; with its
                       fraction of the f16x3 MFMA peak (838.9 TFLOP/s) counting 4 B H dk T^2 useful flop
  sampler              amp_mask_sample against the reference's torch ops (topk, scatter_, the noise arithmetic, argmax, softmax, gather) on
                       the same GPU, both from the same channel-first logits; with the share of a step each takes

Each figure is the median over ``rounds`` of (device events around ``iters`` back-to-back calls) / iters, the two sides alternating round by
round after a warm-up of both -- tools/bench_fmt.py's method.  Prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import maskgct_ref as M  # noqa: E402
from amphion_amd import _lib  # noqa: E402
from amphion_amd.models.tts.maskgct import MaskGCT_S2A, MaskGCT_T2S  # noqa: E402
from amphion_amd.modules import hip_ops  # noqa: E402
from bench_fmt import PEAK_F16X3, compare  # noqa: E402


def synth(model, dev):
    """weights at 1 / sqrt(fan_in) so that the residual stream keeps its magnitude through 16 layers; the adaptive norms near one"""
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if "to_weight.bias" in name:
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            elif "_emb" in name:
                p.copy_(0.5 * torch.randn(p.shape, generator=g))
            elif p.dim() == 2:
                p.copy_(torch.randn(p.shape, generator=g) * 0.5 / p.shape[1] ** 0.5)
            else:
                p.copy_(0.02 * torch.randn(p.shape, generator=g))
    return model.to(dev).eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--layers", type=int, default=16)
    ap.add_argument("--phones", type=int, default=120)
    ap.add_argument("--prompt", type=int, default=250)
    ap.add_argument("--target", type=int, default=500)
    ap.add_argument("--t2s-steps", type=int, default=25)
    ap.add_argument("--s2a-steps", default="25,10,1,1,1,1,1,1,1,1,1,1")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_maskgct: needs a ROCm device (a CPU timing says nothing about the kernels)")
    dev = torch.device("cuda:0")
    P, Tp, Tt = args.phones, args.prompt, args.target
    s2a_steps = [int(s) for s in args.s2a_steps.split(",")]
    t2s = synth(MaskGCT_T2S(hidden_size=1536, num_layers=args.layers, num_heads=16, cond_codebook_size=8192), dev)
    s2a = synth(MaskGCT_S2A(num_quantizer=len(s2a_steps), hidden_size=1024, num_layers=args.layers, num_heads=16, codebook_size=1024,
                            cond_codebook_size=8192), dev)
    out = {"device": torch.cuda.get_device_name(0), "phones": P, "prompt": Tp, "target": Tt, "layers": args.layers, "unit": "ms per call",
           "rounds": args.rounds, "t2s_steps": args.t2s_steps, "s2a_steps": s2a_steps, "precision": _lib.get_precision()}
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for B in (1, 4):
            phones = torch.randint(0, 1023, (B, P), generator=g).to(dev)
            sem_prompt = torch.randint(0, 8192, (B, Tp), generator=g).to(dev)
            sem = torch.randint(0, 8192, (B, Tp + Tt), generator=g).to(dev)
            ac_prompt = torch.randint(0, 1024, (B, Tp, len(s2a_steps)), generator=g).to(dev)
            cond = s2a.cond_emb(sem)
            r = {}
            # a whole call with ONE step is one decoding step plus the per-call hoists; two calls' difference is not needed: the hoists are
            # three small launches against 2 x (8 L + 4) of the forwards
            one = [1] + [0] * (len(s2a_steps) - 1)
            r["t2s_step"] = compare({"hip": lambda: t2s.reverse_diffusion(sem_prompt, Tt, phones, n_timesteps=1, cfg=2.5, rescale_cfg=0.75)}, 3,
                                    args.rounds, warm=1)["hip"]
            r["s2a_step"] = compare({"hip": lambda: s2a.reverse_diffusion(cond, ac_prompt, n_timesteps=one, max_layer=1, cfg=2.5, rescale_cfg=0.75)}, 3,
                                    args.rounds, warm=1)["hip"]
            r["t2s_reverse_diffusion"] = compare({"hip": lambda: t2s.reverse_diffusion(sem_prompt, Tt, phones, n_timesteps=args.t2s_steps, cfg=2.5,
                                                                                        rescale_cfg=0.75)}, 1, args.rounds, warm=1)["hip"]
            r["s2a_reverse_diffusion"] = compare({"hip": lambda: s2a.reverse_diffusion(cond, ac_prompt, n_timesteps=s2a_steps, cfg=2.5,
                                                                                        rescale_cfg=0.75)}, 1, args.rounds, warm=1)["hip"]
            out[f"models_B{B}"] = r
            # ---- the dk = 96 attention alone, at the conditional forward's length
            C, H, T = 1536, 16, P + Tp + Tt
            qkv = torch.randn(B, 3 * C, T, generator=g).to(dev)
            cos, sin = hip_ops.rope_tables(T, C // H, dev)
            c2, s2 = torch.cat((cos, cos), -1), torch.cat((sin, sin), -1)

            def torch_attention():
                q, k, v = (y.reshape(B, H, C // H, T).transpose(2, 3) for y in qkv.split(C, 1))
                rope = lambda y: y * c2 + torch.cat((-y[..., 48:], y[..., :48]), -1) * s2
                return F.scaled_dot_product_attention(rope(q), rope(k), v).transpose(2, 3).reshape(B, C, T)

            hip_attention = lambda: hip_ops.rope_attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], H, cos, sin)
            a = compare({"hip": hip_attention, "torch_rope_sdpa_fp32": torch_attention}, 50, args.rounds, warm=5)
            a["max_abs_diff"] = float((hip_attention() - torch_attention()).abs().max())
            a["hip_tflops"] = round(4.0 * B * C * T * T / (a["hip"] * 1e-3) / 1e12, 2)
            a["hip_fraction_of_f16x3_peak"] = round(a["hip_tflops"] / PEAK_F16X3, 4)
            out[f"attention_96_B{B}"] = a
            # ---- the sampler alone
            for tag, V, thres, temp, step_ms in (("t2s", 8192, 0.98, 0.9, r["t2s_step"]), ("s2a", 1024, 0.98, 1.5, r["s2a_step"])):
                k = M.top_k_count(V, thres)
                logits = (torch.randn(B, V, Tt, generator=g) * 4.0).to(dev)
                u = torch.rand(B, Tt, V, generator=g).to(dev)

                def torch_sampler():
                    ids, score, _, _ = M.mask_sample(logits.transpose(1, 2), k, u, temp)
                    return ids, score

                s = compare({"hip": lambda: hip_ops.mask_sample(logits, k, u, temp), "torch_ops": torch_sampler}, 50, args.rounds, warm=5)
                ids_h, ids_t = hip_ops.mask_sample(logits, k, u, temp)[0], torch_sampler()[0]
                s["ids_that_differ"] = int((ids_h != ids_t).sum())
                s["k"] = k
                s["share_of_step_hip"] = round(s["hip"] / step_ms, 4)
                s["share_of_step_torch_ops"] = round(s["torch_ops"] / (step_ms - s["hip"] + s["torch_ops"]), 4)
                out[f"sampler_{tag}_B{B}"] = s
        _lib.range_check(dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
