"""Times NaturalSpeech2 inference on one GPU at the recipe sizes (config/ns2.json: hidden 512 in 8 heads of 64, 6 + 6 encoder layers, filter
2048, k 9, predictors of 30 layers, a WaveNet of 40 layers, latent 128, 32 query tokens, 512 pitch bins) with synthetic weights at
1 / sqrt(fan_in), against the same model as torch fp32 ops on the same GPU from the same process:

    python tools/bench_ns2.py [--rounds 3] [--phones 100] [--prompt 225] [--frames-per-phone 6]

  once per utterance   prompt encoder, query tokens and prior encoder (``inference`` with 0 solver steps) against the restatement of
                       tests/ns2_ref.py on the device; and ``WaveNet.prepare`` (the stacked cterm / k | v / dconst GEMMs), which the torch route
                       has no counterpart of: it forms those terms inside every step
  one solver step      the WaveNet at one step time plus the euler update against the restatement's step on the device
  the layer op         ``amp_ns2_layer_*`` at T = phones x frames-per-phone, with and without FiLM, against the torch ops of one layer

100 phones of 6 frames each (the duration head set to weight 0, bias log 7) and a 225-frame prompt, at B = 1 and B = 8.  Each figure is the
median over ``rounds`` of (device events around ``iters`` back-to-back calls) / iters, the two sides alternating round by round after a warm-up
of both -- tools/bench_fs2.py's method.  Also states the kernel launches of one euler step (counted from the model's structure: in_proj, five
per layer with cross-attention, two per layer, three for the tail, one for the update) and the bytes of cterm and dconst.  Prints one JSON line."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import ns2_ref as R  # noqa: E402
from amphion_amd import _lib  # noqa: E402
from amphion_amd.models.tts.naturalspeech2 import NaturalSpeech2  # noqa: E402
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--phones", type=int, default=100)
    ap.add_argument("--prompt", type=int, default=225)
    ap.add_argument("--frames-per-phone", type=int, default=6)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    hp = R.small_hp(hidden=512, heads=8, enc_layers=6, d_inner=2048, pred_layers=30, wn_layers=40, latent=128, n_query=32, n_bins=512, n_q=1,
                    codebook_size=8)
    sd = R.synth_state_dict(hp, 0)
    sd["prior_encoder.duration_predictor.linear.weight"].zero_()
    sd["prior_encoder.duration_predictor.linear.bias"].fill_(math.log(1.0 + args.frames_per_phone))
    sd_dev = {k: v.to(dev) for k, v in sd.items()}
    model = NaturalSpeech2(R.make_cfg(hp))
    model.load_state_dict(sd, strict=True)
    model = model.to(dev).eval()
    wn = model.diffusion.diff_estimator
    Hd, L, T = hp["hidden"], hp["wn_layers"], args.phones * args.frames_per_phone
    res = {"frames": T, "once_per_utterance_ms": {}, "prepare_ms": {}, "solver_step_ms": {}, "layer_op_ms": {}, "launches_per_step": {}, "bytes": {}}
    n_steps = 200
    h = 1.0 / n_steps
    with torch.no_grad():
        for Bn in (1, 8):
            g = torch.Generator().manual_seed(Bn)
            phone = torch.randint(1, hp["n_vocab"], (Bn, args.phones), generator=g).to(dev)
            lat = torch.randn(Bn, hp["latent"], args.prompt, generator=g).to(dev)
            mask = torch.ones(Bn, args.prompt, device=dev)
            z = torch.randn(Bn, hp["latent"], T, generator=g).to(dev)

            def torch_prior():
                valid = mask.bool()
                ref = torch.nn.functional.linear(lat.transpose(1, 2), sd_dev["prompt_lin.weight"], sd_dev["prompt_lin.bias"])
                ref = R.encoder(sd_dev, "prompt_encoder", hp, ref, valid)
                spk = R.mha(sd_dev, "query_attn", sd_dev["query_emb.weight"][None].expand(Bn, -1, -1), ref, hp["heads"], valid)
                return R.prior(sd_dev, hp, phone, ref, valid), spk

            res["once_per_utterance_ms"][f"B{Bn}"] = compare({
                "hip": lambda: model.inference(ref_latent=lat, phone_id=phone, ref_mask=mask, inference_steps=0, noise=lambda s: z),
                "torch": torch_prior}, 2, args.rounds, warm=1)
            po, spk = torch_prior()
            assert po["prior_out"].shape[1] == T, po["prior_out"].shape
            cond_bf, spk_bf = po["prior_out"].contiguous(), spk.contiguous()
            cond_cf, spk_cf = cond_bf.transpose(1, 2).contiguous(), spk_bf.transpose(1, 2).contiguous()
            times = [1.0 - (i + 0.5) * h for i in range(n_steps)]
            res["prepare_ms"][f"B{Bn}"] = compare({"hip": lambda: wn.prepare(cond_cf, spk_cf, times)}, 3, args.rounds, warm=1)
            state = wn.prepare(cond_cf, spk_cf, times)
            res["bytes"][f"B{Bn}"] = {"cterm": sum(c.numel() for c in state["cterm"]) * 4, "cterm_chunks": len(state["cterm"]),
                                      "dconst": state["dconst"].numel() * 4, "speaker_kv": state["kv"].numel() * 4}
            xt = z / 1.2
            sc = model.diffusion.scalars(times[100], h)
            tt = torch.full((Bn,), times[100], device=dev)

            def hip_step():
                return hip_ops.ns2_ode_step(xt, wn.step(state, xt, 100), xt, *sc)

            def torch_step():
                return R.ode_step(xt, R.wavenet(sd_dev, hp, xt, cond_bf, tt, spk_bf), xt, *sc)

            n_attn = sum(1 for l in wn.layers if l.has_cattn)
            res["launches_per_step"][f"B{Bn}"] = 1 + 5 * n_attn + 2 * L + 3 + 1
            err = float((hip_step() - torch_step()).abs().max())
            res["solver_step_ms"][f"B{Bn}"] = dict(compare({"hip": hip_step, "torch": torch_step}, 5, args.rounds, warm=2), max_abs_difference=err)
            # the layer op alone, a layer with cross-attention's FiLM handed in and one without
            layer = wn.layers[0]
            x = torch.randn(Bn, Hd, T, device=dev)
            xo, sk = torch.empty_like(x), torch.randn(Bn, Hd, T, device=dev)
            film = torch.randn(Bn, 4 * Hd, T, device=dev)
            dc = state["dconst"][100, 0]
            ct = state["cterm"][0][:, :2 * Hd]
            cw, cb = layer.dilated_conv.weight.detach(), layer.dilated_conv.bias.detach()
            ow, ob = layer.out_proj.weight.detach(), layer.out_proj.bias.detach()
            hd, Lb, stream = layer.op_handle(dev), _lib.lib(), _lib.current_stream_ptr(dev)
            wsb = Lb.amp_ns2_layer_workspace_bytes(hd, Bn, T)
            ws = hip_ops._workspace(dev, wsb)
            for name, fm in (("film", film), ("plain", None)):
                def torch_layer():
                    a = R.layer_conv(x, dc[None], cw, cb, 1)
                    return R.layer_tail(x, a, ct, ow, ob, fm, sk)

                # "hip": the checked wrapper; "hip_direct": amp_ns2_layer_forward on resolved addresses, as WaveNet.step calls it
                direct = lambda: Lb.amp_ns2_layer_forward(hd, x.data_ptr(), dc.data_ptr(), 0, ct.data_ptr(), ct.stride(0) if Bn > 1 else 2 * Hd * T,
                                                          None if fm is None else fm.data_ptr(), sk.data_ptr(), Bn, T, xo.data_ptr(), sk.data_ptr(),
                                                          ws.data_ptr(), wsb, stream)
                assert direct() == 0
                res["layer_op_ms"][f"B{Bn}_{name}"] = compare({
                    "hip": lambda: layer._op(x, dc, ct, cw, cb, ow, ob, film=fm, skip=sk, x_out=xo),
                    "hip_direct": direct,
                    "torch": torch_layer}, 20, args.rounds)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
