"""Times VALL-E's AR stage on one GPU at the recipe size (decoder_dim 1024, 16 heads of 64, 12 layers, 1024 audio tokens + EOS) with synthetic
weights, 100 text tokens, a 225-frame prompt and 750 new tokens (forced: no early EOS on any route), against what the tree had before and
against torch ops on the same GPU:

    python tools/valle_bench.py [--rounds 3] [--layers 12] [--text 100] [--prompt 225] [--new 750]

  (a) hip_fused            the model's route: LN folded into the q | k | v, linear1 (+ ReLU) and predict-layer matrix-vector products
                           (amp_pw_forward_vec_ln)
  (b) hip_existing         the same step from the launches that existed: amp_layer_norm_c at T = 1 + amp_pw_forward_vec + a separate ReLU
  (c) torch_kv_cache       tests/valle_ref.py's cached path as torch fp32 ops on the device
  (d) torch_recompute      tests/valle_ref.py's recomputing path as torch fp32 ops on the device: the reference's algorithm (the whole decoder
                           over [text | audio] for every new token)
  (e) prefix_attention     amp_prefix_attention alone at T = text + prompt against amp_cross_attention at the same T
  gemv                     each folded product against its unfolded launches, alone, per shape

A route's total is the host clock around the whole AR stage (it ends in a host read, after a device synchronise); ms per decode step =
(total with ``new`` tokens - total with 0 new tokens) / new.  Medians over ``rounds`` with the routes alternating round by round after a warm-up
of each; ``spread`` is max - min over the rounds.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import valle_ref as V  # noqa: E402
from amphion_amd import _lib  # noqa: E402
from amphion_amd.models.tts.valle import VALLE  # noqa: E402
from amphion_amd.modules import hip_ops  # noqa: E402


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3                # ms


def events(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters                      # ms per call


def compare(fns, rounds, measure, warm=1):
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(measure(fn))
    out = {k: round(statistics.median(v), 5) for k, v in t.items()}
    out["spread"] = {k: round(max(v) - min(v), 5) for k, v in t.items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--text", type=int, default=100)
    ap.add_argument("--prompt", type=int, default=225)
    ap.add_argument("--new", type=int, default=750)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("valle_bench: needs a ROCm device (a CPU timing says nothing about the kernels)")
    dev = torch.device("cuda:0")
    hp = V.make_hp(text_token_num=512, audio_token_num=1024, decoder_dim=1024, nhead=16, num_decoder_layers=args.layers, num_quantizers=1)
    D, H, NL, Vout = hp["decoder_dim"], hp["nhead"], args.layers, hp["audio_token_num"] + 1
    sd = V.synth_state_dict(hp, 7)
    model = VALLE(SimpleNamespace(**hp))
    model.load_state_dict(sd)
    model = model.to(dev)
    sd = V.cast(sd, torch.float32, dev)
    out = {"device": torch.cuda.get_device_name(0), "hp": hp, "text": args.text, "prompt": args.prompt, "new": args.new, "rounds": args.rounds,
           "precision": _lib.get_precision(), "unit": "ms"}
    g = torch.Generator().manual_seed(1)
    x = torch.randint(0, hp["text_token_num"], (1, args.text), generator=g).to(dev)
    x_lens = torch.tensor([args.text])
    y = torch.randint(0, hp["audio_token_num"], (1, args.prompt, 1), generator=g).to(dev)
    forced = torch.randint(0, hp["audio_token_num"], (1, args.new, 1), generator=g)
    q = torch.empty(args.new + 1, Vout).exponential_(generator=g).to(dev)
    with torch.no_grad():
        def hip(n, fused):
            return lambda: model._ar_generate(x, y[..., 0], args.prompt, 10, 0.9, noise=V.Replay(q), teacher=forced[0, :n, 0].tolist(), fused=fused)

        def ref(n, path):
            return lambda: V.inference(sd, hp, x, x_lens, y, x_lens, V.Replay(q), top_k=10, temperature=0.9, path=path, teacher=forced[:, :n])
        full = compare({"hip_fused": hip(args.new, True), "hip_existing": hip(args.new, False), "torch_kv_cache": ref(args.new, "cache"),
                        "torch_recompute": ref(args.new, "recompute")}, args.rounds, wall)
        zero = compare({"hip_fused": hip(0, True), "hip_existing": hip(0, False), "torch_kv_cache": ref(0, "cache"),
                        "torch_recompute": ref(0, "recompute")}, args.rounds, wall, warm=2)
        out["ar_stage_total"] = full
        out["ar_stage_prefill_and_first_step"] = zero
        out["ms_per_decode_step"] = {k: round((full[k] - zero[k]) / args.new, 5) for k in full if k != "spread"}
        a, b = hip(args.new, True)(), hip(args.new, False)()
        out["fused_equals_existing_tokens"] = bool(torch.equal(a, b))

        # ---- (e) the prefill attention alone
        T = args.text + args.prompt
        qkv = torch.randn(1, 3 * D, T, generator=g).to(dev)
        sl = (qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:])
        att = compare({"prefix_attention": lambda: hip_ops.prefix_attention(*sl, H, args.text), "cross_attention": lambda: hip_ops.cross_attention(*sl, H)},
                      args.rounds, lambda fn: events(fn, 50), warm=5)
        att["T"], att["prefix"] = T, args.text
        out["prefill_attention"] = att

        # ---- each folded product against its unfolded launches
        layer = model.ar_decoder.layers[0]
        xcol = torch.randn(1, D, 1, generator=g).to(dev)
        gemv = {}
        for name, h, cout, norm, relu in (("qkv_1024x3072", layer.self_attn._qkv.get(layer.self_attn.in_proj(), dev), 3 * D, layer.norm1, False),
                                          ("linear1_relu_1024x4096", layer._l1.get(layer.linear1, dev), 4 * D, layer.norm2, True),
                                          ("predict_1024x1025", model._ar_head.get(model.ar_predict_layer, dev), Vout, model.ar_decoder.norm, False)):
            ng, nb = norm.affine()
            yo = torch.empty(1, cout, 1, device=dev)
            fused = lambda: hip_ops.pw_forward_vec_ln(h, cout, xcol, ng, nb, norm.eps, relu=relu, out=yo)

            def parts():
                r = hip_ops.pw_forward_vec(h, cout, hip_ops.layer_norm_c(xcol, ng, nb, eps=norm.eps), out=yo)
                return r.relu_() if relu else r
            r = compare({"fused": fused, "norm_vec_relu": parts, "vec_alone": lambda: hip_ops.pw_forward_vec(h, cout, xcol, out=yo)}, args.rounds,
                        lambda fn: events(fn, 200), warm=10)
            r["max_abs_diff"] = float((fused().clone() - parts()).abs().max())
            gemv[name] = r
        out["gemv"] = gemv
    print(json.dumps(out))


if __name__ == "__main__":
    main()
