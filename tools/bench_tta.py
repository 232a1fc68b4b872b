"""Times AudioLDM text-to-audio inference on one GPU at the recipe size (config/audioldm.json: model_channels 256, channel_mult [1, 2, 4], 8 heads,
context 768; AutoencoderKL ch 128, ch_mult [1, 1, 2, 2, 4]) with seeded weights (tests/tta_ref.py: synth_state_dict), against the same model
as torch fp32 ops on the same GPU from the same process:

    python tools/bench_tta.py [--rounds 3] [--tokens 12] [--out profiles/tta_bench_mi355x.json]

  unet_eval_ms      one evaluation of the UNet on [2, 4, 5, 39] (batch 2 = classifier-free guidance) with the context's k | v prepared, against
                    the restatement's ``unet_forward`` on the device with its norms as ``F.group_norm`` and its attention as
                    ``scaled_dot_product_attention`` (torch's fused ops: the written-out forms would inflate a launch-bound baseline)
  split_ms          that evaluation by kind of launch -- convs, norms, attention, GEMMs, T = 1 products, torch glue (cat / crop / embedding) --
                    from device events around every wrapper call of ONE evaluation (the events add gaps: the parts sum to more than the whole)
  conv_ops          every distinct conv of the evaluation: ``amp_conv2d_forward`` (with the stats launch where it normalises on load) against
                    GroupNorm + SiLU + conv2d as torch ops, and the count of each
  decode_ms         ``AutoencoderKL.decode`` at [1, 4, 5, 39] -> [1, 1, 80, 624] against the restatement on the device
  weights           parameters of the UNet, their bytes, and bytes / unet_eval time (the achieved stream rate of the weights)
  distance          the evaluation's and the decoder's distance from the fp64 restatement on the CPU, next to the fp32 CPU evaluation's

Each timing is the median over ``rounds`` of (device events around ``iters`` back-to-back calls) / iters, the two sides alternating round by
round after a warm-up of both -- tools/bench_ns2.py's method.  Prints one JSON line and writes it to ``--out``."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import tta_ref as R  # noqa: E402
from amphion_amd.models.tta.autoencoder import AutoencoderKL  # noqa: E402
from amphion_amd.models.tta.autoencoder import autoencoder as vae_mod  # noqa: E402
from amphion_amd.models.tta.ldm import AudioLDM  # noqa: E402
from amphion_amd.models.tta.ldm import attention as attn_mod  # noqa: E402
from amphion_amd.models.tta.ldm import audioldm as unet_mod  # noqa: E402
from amphion_amd.modules import hip_ops  # noqa: E402


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


def recipe_hp():
    hp = R.small_hp()
    hp.update(model_channels=256, num_heads=8, context_dim=768)
    return hp


def recipe_vae_hp():
    hp = R.small_vae_hp()
    hp.update(ch=128)
    return hp


class Split:
    """device events around every wrapper call of the model's modules while active; ``convs`` also records each conv's geometry"""

    KINDS = {"Conv2d3x3.__call__": "convs", "group_norm_stats": "norms", "group_norm": "norms", "layer_norm_c": "norms", "cross_attention_hd": "attention",
             "geglu": "gemms", "StackedPw.__call__": "gemms", "pw_forward_vec": "t1_products", "silu": "t1_products"}

    def __init__(self):
        self.events, self.convs, self._undo = [], [], []

    def _wrap(self, owner, name, kind, fn):
        def wrapped(*a, **k):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            out = fn(*a, **k)
            e.record()
            self.events.append((kind, s, e))
            if kind == "convs":
                x, w = a[1], a[2]
                self.convs.append((w.shape[1], w.shape[0], x.shape[2], x.shape[3], k.get("stride", 1), bool(k.get("up2", False)), k.get("norm") is not None,
                                   k.get("row_add") is not None, k.get("residual") is not None))
            return out

        self._undo.append((owner, name, getattr(owner, name)))
        setattr(owner, name, wrapped)

    def __enter__(self):
        self._wrap(hip_ops.Conv2d3x3, "__call__", "convs", hip_ops.Conv2d3x3.__call__)
        self._wrap(attn_mod.StackedPw, "__call__", "gemms", attn_mod.StackedPw.__call__)
        for mod in (unet_mod, attn_mod, vae_mod):
            for name in ("group_norm_stats", "group_norm", "layer_norm_c", "cross_attention_hd", "geglu", "pw_forward_vec", "silu"):
                if hasattr(mod, name):
                    self._wrap(mod, name, self.KINDS[name], getattr(mod, name))
        return self

    def __exit__(self, *exc):
        for owner, name, fn in reversed(self._undo):
            setattr(owner, name, fn)
        return False

    def totals(self):
        torch.cuda.synchronize()
        out = {}
        for kind, s, e in self.events:
            out[kind] = out.get(kind, 0.0) + s.elapsed_time(e)
        return {k: round(v, 4) for k, v in out.items()}


def torch_baseline():
    """The restatement as the torch baseline: its GroupNorm written out (six launches) and its attention as softmax + matmul would inflate a
    launch-bound evaluation, so the baseline runs them as torch's own fused ops -- ``F.group_norm`` (except for a group of one value, which it
    refuses) and ``scaled_dot_product_attention``."""
    slow_gn = R.group_norm_ref

    def group_norm(x, gamma, beta, eps, silu=False):
        if x.numel() // (x.shape[0] * 32) < 2:
            return slow_gn(x, gamma, beta, eps, silu)
        y = torch.nn.functional.group_norm(x, 32, gamma, beta, eps)
        return torch.nn.functional.silu(y) if silu else y

    def attention(q, k, v, H, scale=None):
        B, C, Tq = q.shape
        dk = C // H
        qq, kk, vv = (t.reshape(B, H, dk, -1).transpose(2, 3) for t in (q, k, v))
        return torch.nn.functional.scaled_dot_product_attention(qq, kk, vv, scale=scale).transpose(2, 3).reshape(B, C, Tq)

    R.group_norm_ref, R.attention_cf = group_norm, attention


def torch_conv(x, w, b, stride, up2, norm, row, res):
    a = x
    if norm is not None:
        a = torch.nn.functional.silu(torch.nn.functional.group_norm(x, 32, norm[0], norm[1], 1e-5))
    if up2:
        a = torch.nn.functional.interpolate(a, scale_factor=2, mode="nearest")
    y = torch.nn.functional.conv2d(a, w, b, stride=stride, padding=1)
    if row is not None:
        y = y + row[:, :, None, None]
    return y if res is None else y + res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--tokens", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tta_bench_mi355x.json"))
    ap.add_argument("--no-fp64", action="store_true", help="skip the CPU fp64 / fp32 restatement (the distances)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    hp, vhp = recipe_hp(), recipe_vae_hp()
    unet = AudioLDM(R.Cfg(hp))
    sd = R.synth_state_dict({k: v.shape for k, v in unet.state_dict().items()}, 0)
    unet.load_state_dict(sd)
    unet = unet.to(dev).eval()
    vae = AutoencoderKL(R.Cfg(vhp))
    vsd = R.synth_state_dict({k: v.shape for k, v in vae.state_dict().items()}, 1)
    vae.load_state_dict(vsd)
    vae = vae.to(dev).eval()
    slow_refs = (R.group_norm_ref, R.attention_cf)
    torch_baseline()
    sd_dev, vsd_dev = {k: v.to(dev) for k, v in sd.items()}, {k: v.to(dev) for k, v in vsd.items()}
    g = torch.Generator().manual_seed(0)
    x, ctx, z = torch.randn(2, 4, 5, 39, generator=g), torch.randn(2, args.tokens, hp["context_dim"], generator=g), torch.randn(1, 4, 5, 39, generator=g)
    t = torch.tensor([481, 481])
    dx, dctx, dt, dz = x.to(dev), ctx.to(dev), t.to(dev), z.to(dev)
    n_params = sum(v.numel() for v in sd.values())
    res = {"shape": list(x.shape), "tokens": args.tokens, "weights": {"unet_params": n_params, "unet_bytes": 4 * n_params}}
    with torch.no_grad():
        hip_eval = lambda: unet(dx, dt, dctx)
        torch_eval = lambda: R.unet_forward(sd_dev, hp, dx, dt, dctx)
        y = hip_eval()
        res["unet_eval_ms"] = dict(compare({"hip": hip_eval, "torch": torch_eval}, 5, args.rounds, warm=2),
                                   max_abs_difference=float((y - torch_eval()).abs().max()))
        res["weights"]["achieved_gb_per_s"] = round(4 * n_params / (res["unet_eval_ms"]["hip"] * 1e-3) / 1e9, 1)
        with Split() as sp:
            torch.cuda.synchronize()
            whole = timed(hip_eval, 1)
        parts = sp.totals()
        parts["whole_with_events"] = round(whole, 4)
        parts["glue_and_gaps"] = round(whole - sum(v for k, v in parts.items() if k != "whole_with_events"), 4)
        parts["launch_calls"] = {k: sum(1 for e in sp.events if e[0] == k) for k in set(e[0] for e in sp.events)}
        res["split_ms"] = parts
        # every distinct conv of the evaluation, the op against torch's ops
        counts = {}
        for c in sp.convs:
            counts[c] = counts.get(c, 0) + 1
        res["conv_ops"] = []
        for (cin, cout, H, W, stride, up2, norm, row, resid), n in sorted(counts.items()):
            gw = torch.Generator().manual_seed(cin * 7 + cout)
            w = (torch.randn(cout, cin, 3, 3, generator=gw) / (9 * cin) ** 0.5).to(dev)
            b, gam, bet = torch.randn(cout, device=dev), torch.ones(cin, device=dev), torch.zeros(cin, device=dev)
            xx = torch.randn(2, cin, H, W, device=dev)
            Ho, Wo = hip_ops.conv2d_out_size(H, W, stride, up2)
            rr = torch.randn(2, cout, device=dev) if row else None
            rs = torch.randn(2, cout, Ho, Wo, device=dev) if resid else None
            op = hip_ops.Conv2d3x3()
            hip = lambda: op(xx, w, b, stride=stride, up2=up2, norm=(hip_ops.group_norm_stats(xx, 1e-5), gam, bet) if norm else None, row_add=rr, residual=rs)
            tor = lambda: torch_conv(xx, w, b, stride, up2, (gam, bet) if norm else None, rr, rs)
            r = compare({"hip": hip, "torch": tor}, 20, args.rounds)
            res["conv_ops"].append({"cin": cin, "cout": cout, "H": H, "W": W, "stride": stride, "up2": up2, "norm": norm, "count": n, "hip_ms": r["hip"],
                                    "torch_ms": r["torch"], "weight_gb_per_s": round(4 * 9 * cin * cout / (r["hip"] * 1e-3) / 1e9, 1)})
        res["conv_ops_sum_ms"] = {"hip": round(sum(c["hip_ms"] * c["count"] for c in res["conv_ops"]), 4),
                                  "torch": round(sum(c["torch_ms"] * c["count"] for c in res["conv_ops"]), 4)}
        hip_dec = lambda: vae.decode(dz)
        torch_dec = lambda: R.decode_ref(vsd_dev, vhp, dz)
        mel = hip_dec()
        res["decode_ms"] = dict(compare({"hip": hip_dec, "torch": torch_dec}, 3, args.rounds, warm=1), shape=list(mel.shape),
                                max_abs_difference=float((mel - torch_dec()).abs().max()))
        with Split() as sp:
            torch.cuda.synchronize()
            whole = timed(hip_dec, 1)
        parts = sp.totals()
        parts["whole_with_events"] = round(whole, 4)
        res["decode_split_ms"] = parts
        if not args.no_fp64:
            torch.set_num_threads(min(16, os.cpu_count() or 1))
            R.group_norm_ref, R.attention_cf = slow_refs          # the CPU statements as the tests use them
            ref = R.unet_forward(R.cast(sd, torch.float64), hp, x.double(), t, ctx.double())
            cpu = R.unet_forward(sd, hp, x, t, ctx)
            dref = R.decode_ref(R.cast(vsd, torch.float64), vhp, z.double())
            dcpu = R.decode_ref(vsd, vhp, z)
            res["distance"] = {"unet": {"gpu": float((y.double().cpu() - ref).abs().max()), "cpu32": float((cpu.double() - ref).abs().max()),
                                        "ref_absmax": float(ref.abs().max())},
                               "decode": {"gpu": float((mel.double().cpu() - dref).abs().max()), "cpu32": float((dcpu.double() - dref).abs().max()),
                                          "ref_absmax": float(dref.abs().max())}}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
