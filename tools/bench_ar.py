"""Times Vevo's autoregressive transformer on one GPU at the recipe point (models/vc/vevo/config/Vq32ToVq8192.json: hidden 1536, 16 heads of
96, 12 layers, MLP 6144, vocabulary 1056 + 8192 + 20 = 9268) with synthetic weights at 1 / sqrt(fan_in), against torch ops on the same GPU
(DESIGN.md §22):

    python tools/bench_ar.py [--rounds 3] [--layers 12] [--input 200] [--prompt 500] [--new 500]

  generate               200 input tokens, a prompt of 500, 500 new tokens (min_new_tokens = 500: no early EOS on either side) against the fp32
                         restatement of tests/ar_ref.py with a KV cache on the device; ms per decode step = (generate - prefill) / steps
  step parts             the launches of one decode step at L = 1000, each timed alone, times how often the step runs them
  linear CinxCout        every Linear shape of a step: amp_pw_forward_vec against amp_pw_forward at T = 1 ON THE SAME HANDLE (the route this
                         tree would otherwise take), as GB/s of weight bytes (4 per weight: the hi and lo f16 planes, or one fp32), beside
                         the 6.0 - 6.3 TB/s streaming rate of the chip
  decode attention       amp_attention_decode at L = 700 / 1200 against fp32 scaled_dot_product_attention over a torch cache
  prefill attention      amp_rope_attention_causal against amp_rope_attention at T = 700
  sampler                amp_ar_sample against the torch op chain of HF's processors and the race (tests/ar_ref.py: process, race)

Each figure is the median over ``rounds`` of (device events around ``iters`` back-to-back calls) / iters, the two sides alternating round by
round after a warm-up of both -- tools/bench_fmt.py's method.  Prints one JSON line."""
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

import ar_ref as A  # noqa: E402
from amphion_amd import _lib  # noqa: E402
from amphion_amd.models.vc.autoregressive_transformer import AutoregressiveTransformer  # noqa: E402
from amphion_amd.modules import hip_ops  # noqa: E402

STREAM_TBS = (6.0, 6.3)


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
    out = {k: round(statistics.median(v), 5) for k, v in t.items()}
    out["spread"] = {k: round(max(v) - min(v), 5) for k, v in t.items()}
    return out


def synth_model(hp, dev):
    g = torch.Generator().manual_seed(7)
    m = AutoregressiveTransformer(**hp)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if p.dim() == 1:
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            elif "embed_tokens" in name:
                p.copy_(torch.randn(p.shape, generator=g))
            else:
                p.copy_(torch.randn(p.shape, generator=g) / p.shape[1] ** 0.5)
    return m.to(dev).eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--input", type=int, default=200)
    ap.add_argument("--prompt", type=int, default=500)
    ap.add_argument("--new", type=int, default=500)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_ar: needs a ROCm device (a CPU timing says nothing about the kernels)")
    dev = torch.device("cuda:0")
    hp = dict(input_vocab_size=1056, output_vocab_size=8192, hidden_size=1536, intermediate_size=6144, num_hidden_layers=args.layers,
              num_attention_heads=16)
    C, H, I, NL = hp["hidden_size"], hp["num_attention_heads"], hp["intermediate_size"], args.layers
    dk, V = C // H, A.special(hp)["vocab"]
    m = synth_model(hp, dev)
    sd = {k: v.detach() for k, v in m.state_dict().items()}
    out = {"device": torch.cuda.get_device_name(0), "hp": hp, "unit": "ms per call", "rounds": args.rounds, "precision": _lib.get_precision(),
           "stream_rate_TBps": STREAM_TBS}
    g = torch.Generator().manual_seed(1)
    L_ = _lib.lib()
    with torch.no_grad():
        # ---- the whole generate
        ii = torch.randint(0, hp["input_vocab_size"], (1, args.input), generator=g).to(dev)
        po = torch.randint(0, hp["output_vocab_size"], (1, args.prompt), generator=g).to(dev)
        n0 = args.input + 2 + args.prompt + 1
        q = torch.empty(args.new, V).exponential_(generator=g).to(dev)
        kw = dict(max_length=n0 + args.new, min_new_tokens=args.new, temperature=0.8, top_k=50, top_p=0.9, repeat_penalty=1.1)
        hip_gen = lambda: m.generate(ii, prompt_output_ids=po, noise=A.Replay(q), **kw)
        torch_gen = lambda: A.generate(sd, hp, ii, po, A.Replay(q), **kw)
        r = compare({"hip": hip_gen, "torch_fp32_kv_cache": torch_gen}, 1, args.rounds, warm=1)
        a, b = hip_gen(), torch_gen()[0]
        n = min(a.shape[1], b.shape[1])
        r["tokens"], r["leading_equal_tokens"] = int(a.shape[1]), int((a[0, :n] != b[0, :n]).int().cumsum(0).eq(0).sum())
        prompt_ids = torch.cat((m.padding_for_input(ii, torch.ones_like(ii), m.input_eos_token_id, m.input_bos_token_id, m.pad_token_id)[0],
                                m.padding_for_output(po, torch.ones_like(po), m.output_eos_token_id, m.output_bos_token_id, m.pad_token_id)[0][:, :-1]), -1)
        caches = [hip_ops.kv_cache(1, H, dk, n0 + args.new, dev) for _ in range(NL)]
        pre = compare({"hip": lambda: m._prefill(prompt_ids, None, caches, n0 + args.new),
                       "torch_fp32": lambda: A.llama(sd, hp, prompt_ids, cache=[dict() for _ in range(NL)], hidden_only=True)}, 3, args.rounds)
        r["prefill"] = pre
        r["ms_per_decode_step"] = {k: round((r[k] - pre[k2]) / (args.new - 1), 5) for k, k2 in (("hip", "hip"), ("torch_fp32_kv_cache", "torch_fp32"))}
        out["generate"] = r

        # ---- every Linear of a step
        lin = {}
        layer = m.model.model.layers[0]
        qkv_l, gu_l = layer._stacked()
        handles = {"qkv": (layer.self_attn._qkv.get(qkv_l, dev), C, 3 * C, NL), "o_proj": (layer.self_attn._out.get(layer.self_attn.o_proj, dev), C, C, NL),
                   "gate_up": (layer.mlp._gu.get(gu_l, dev), C, 2 * I, NL), "down_proj": (layer.mlp._down.get(layer.mlp.down_proj, dev), I, C, NL),
                   "lm_head": (m.model._head.get(m.model.lm_head, dev), C, V, 1)}
        st = _lib.current_stream_ptr(dev)
        vec_step = gemm_step = 0.0
        for name, (h, cin, cout, count) in handles.items():
            x = torch.randn(1, cin, 1, generator=g).to(dev)
            y = torch.empty(1, cout, 1, device=dev)
            vec = lambda: hip_ops.pw_forward_vec(h, cout, x, out=y)
            gemm = lambda: _lib.check(L_.amp_pw_forward(h, _lib.ptr(x), 0, 1, 1, 0, None, None, _lib.ptr(y), st))
            r = compare({"vec": vec, "gemm_T1": gemm}, 200, args.rounds, warm=10)
            gb = 4.0 * cin * cout / 1e9
            r["weight_GBps"] = {k: round(gb / (r[k] * 1e-3), 1) for k in ("vec", "gemm_T1")}
            yv = vec().clone()
            gemm()
            r["max_abs_diff"] = float((yv - y).abs().max())
            lin[f"{name}_{cin}x{cout}"] = r
            vec_step += count * r["vec"]
            gemm_step += count * r["gemm_T1"]
        lin["per_step_ms"] = {"vec": round(vec_step, 4), "gemm_T1": round(gemm_step, 4)}
        out["linear"] = lin

        # ---- decode attention
        cos, sin = hip_ops.rope_tables(2048, dk, dev)
        att = {}
        for L in (700, 1200):
            kc, vc = torch.randn(1, C, 2048, generator=g).to(dev), torch.randn(1, C, 2048, generator=g).to(dev)
            qd = torch.randn(1, C, 1, generator=g).to(dev)
            kt = kc[:, :, :L].reshape(1, H, dk, L).transpose(2, 3).contiguous()      # a torch cache [B, H, L, dk]
            vt = vc[:, :, :L].reshape(1, H, dk, L).transpose(2, 3).contiguous()
            c2, s2 = torch.cat((cos[L - 1], cos[L - 1])), torch.cat((sin[L - 1], sin[L - 1]))

            def sdpa():
                y = qd.reshape(1, H, 1, dk)
                y = y * c2 + torch.cat((-y[..., dk // 2:], y[..., :dk // 2]), -1) * s2
                return F.scaled_dot_product_attention(y, kt, vt).reshape(1, C, 1)
            hip = lambda: hip_ops.attention_decode(qd, H, cos, sin, L, kc, vc)
            r = compare({"hip": hip, "torch_rope_sdpa_fp32": sdpa}, 200, args.rounds, warm=10)
            r["max_abs_diff"] = float((hip() - sdpa()).abs().max())
            r["hip_cache_GBps"] = round(8.0 * C * L / 1e9 / (r["hip"] * 1e-3), 1)
            att[f"L{L}"] = r
        out["decode_attention"] = att

        # ---- prefill attention, causal against non-causal
        T = 700
        qkv = torch.randn(1, 3 * C, T, generator=g).to(dev)
        pa = lambda causal: hip_ops.rope_attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], H, cos[:T], sin[:T], causal=causal)
        out["prefill_attention_T700"] = compare({"causal": lambda: pa(True), "non_causal": lambda: pa(False)}, 50, args.rounds, warm=5)

        # ---- the other launches of a step, alone
        xcol = torch.randn(1, C, 1, generator=g).to(dev)
        gu = torch.randn(1, 2 * I, 1, generator=g).to(dev)
        qkv1 = torch.randn(1, 3 * C, 1, generator=g).to(dev)
        kc, vc = hip_ops.kv_cache(1, H, dk, 2048, dev)
        parts = compare({"rms_norm": lambda: layer.input_layernorm.forward_cf(xcol), "swiglu": lambda: hip_ops.swiglu(gu),
                         "kv_append": lambda: hip_ops.kv_append(qkv1[:, C:2 * C], qkv1[:, 2 * C:], H, cos, sin, 999, kc, vc),
                         "attention_decode_L1000": lambda: hip_ops.attention_decode(qkv1[:, :C], H, cos, sin, 1000, kc, vc)}, 200, args.rounds, warm=10)
        parts["count_per_step"] = {"rms_norm": 2 * NL + 1, "swiglu": NL, "kv_append": NL, "attention_decode_L1000": NL}
        out["step_parts"] = parts

        # ---- the sampler
        logits = (3.0 * torch.randn(1, V, 1, generator=g)).to(dev)
        ids = torch.randint(0, V, (1, 1024), generator=g).to(dev)
        q1 = q[:1].contiguous()
        hip = lambda: hip_ops.ar_sample(logits, q1, ids, 900, m.output_eos_token_id, True, 0.8, 50, 0.9, 1.1)
        chain = lambda: A.race(A.process(logits[0, :, 0], ids[0, :900], 1.1, m.output_eos_token_id, True, 0.8, 50, 0.9), q1[0])
        r = compare({"hip": hip, "torch_chain": chain}, 100, args.rounds, warm=5)
        r["same_id"] = bool(int(hip()[0, 900]) == chain())
        out["sampler"] = r
    print(json.dumps(out))


if __name__ == "__main__":
    main()
