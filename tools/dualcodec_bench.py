#!/usr/bin/env python
"""Times the DualCodec drop-in (amphion_amd/models/codec/dualcodec/dualcodec/model_codec) on one GPU, in one process, alternating with what it is
compared against.  Synthetic weights; reads nothing outside the repository.

    python tools/dualcodec_bench.py [--rounds 10] [--iters 5] [--json out.json] [--skip-models]

(a) The quantizer entry points with DAC's surrounding passes folded in against the three-step sequences they replace, at the two recipes'
    acoustic quantizers (D 1024, d 8; K 4096 x 7 levels at 125 frames, K 1024 x 11 levels at 250 frames), B = 16:
        amp_fvq_encode_ex(z, sub)          vs   torch z - sub -> amp_fvq_encode -> torch z_q + sub
        amp_fvq_decode_add(codes, add)     vs   amp_fvq_decode -> torch + add
    Each route is REPS calls in one captured graph; the graphs are replayed in alternation for --rounds rounds; medians with [min, max].
(b) wave + semantic features -> codes (DualCodec.encode) and codes -> wave (DualCodec.decode_from_codes) for the hyper-parameters of
    dualcodec_12hz_16384_4096_8vq and dualcodec_25hz_16384_1024_12vq at B = 1 and 16, 10 s of 24 kHz audio, each against the fp32 torch
    restatement of tests/dualcodec_ref.py on the same device (weights folded once, no margin bookkeeping), in alternating rounds, with x real time
    and the number of library launches per call (counted from the modules' routes; torch's two small code-layout copies are not in it).
The launch manifest is off while timing."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402
import torch.nn.functional as Fn  # noqa: E402

import codec_ref as C  # noqa: E402
import dac_ref as D  # noqa: E402
import dualcodec_ref as R  # noqa: E402
from amphion_amd import _lib  # noqa: E402
from amphion_amd.models.codec.dualcodec.dualcodec.model_codec import DualCodec, ResidualVectorQuantize  # noqa: E402

REPS = 20
SR, SECONDS = 24000, 10
B_OP = 16


def _time_once(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1])


def _stats(v):
    v = sorted(v)
    return round(v[len(v) // 2], 4), [round(v[0], 4), round(v[-1], 4)]


def _alternate(routes, rounds, scale=1.0):
    """routes: name -> callable; one warm-up each, then `rounds` rounds of one timed call per route, in turn"""
    for fn in routes.values():
        fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in routes}
    for _ in range(rounds):
        for name, fn in routes.items():
            ts[name].append(_time_once(fn) / scale)
    return {k: _stats(v) for k, v in ts.items()}


# ---- (a) the fused quantizer entry points -------------------------------------------------------------------------------------------------
def bench_quantizer(rounds, res):
    L = _lib.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    p = _lib.ptr
    for name in ("12hz", "25hz"):
        hp = R.recipe_hp(name)
        qhp = R.acoustic_q_hp(hp)
        T = SECONDS * SR // R.hop(hp)
        m = ResidualVectorQuantize(qhp["D"], qhp["N"], qhp["K"], qhp["d"])
        m.load_state_dict(R.synth_rvq_state_dict(qhp, 1))
        m = m.cuda().eval()
        h = m._handle.get(list(m.quantizers), dev)
        n, Dn = qhp["N"], qhp["D"]
        z = C.synth_latent(B_OP, Dn, T, 2).cuda()
        sub = (0.5 * C.synth_latent(B_OP, Dn, T, 3)).cuda()
        codes = torch.empty(n, B_OP, T, dtype=torch.int64, device="cuda")
        zq, tmp, out3 = (torch.empty_like(z) for _ in range(3))
        st = lambda: _lib.current_stream_ptr(dev)       # noqa: E731

        def enc_fused():
            _lib.check(L.amp_fvq_encode_ex(h, p(z), T, p(sub), B_OP, T, n, p(codes), p(zq), None, None, st()))

        def enc_three():
            torch.sub(z, sub, out=tmp)
            _lib.check(L.amp_fvq_encode(h, p(tmp), B_OP, T, n, p(codes), p(zq), None, st()))
            torch.add(zq, sub, out=out3)

        def dec_fused():
            _lib.check(L.amp_fvq_decode_add(h, p(codes), n, B_OP, T, p(sub), p(zq), st()))

        def dec_two():
            _lib.check(L.amp_fvq_decode(h, p(codes), n, B_OP, T, p(tmp), st()))
            torch.add(tmp, sub, out=out3)

        enc_fused()
        torch.cuda.synchronize()
        graphs = {}
        for tag, fn in (("encode_ex", enc_fused), ("encode_three_step", enc_three), ("decode_add", dec_fused), ("decode_then_add", dec_two)):
            fn()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for _ in range(REPS):
                    fn()
            graphs[tag] = g.replay
        t = _alternate(graphs, rounds, scale=REPS)
        row = dict(recipe=name, B=B_OP, T=T, D=Dn, K=qhp["K"], levels=n, rounds=rounds)
        for tag, (med, mm) in t.items():
            row[tag + "_ms"], row[tag + "_min_max_ms"] = med, mm
        row["encode_ex_over_three_step"] = round(row["encode_ex_ms"] / row["encode_three_step_ms"], 3)
        row["decode_add_over_two_step"] = round(row["decode_add_ms"] / row["decode_then_add_ms"], 3)
        res["quantizer"].append(row)
        print(json.dumps(row), flush=True)


# ---- (b) the model ---------------------------------------------------------------------------------------------------------------------------
def _torch_rvq(P, prefix, n, z):
    """the eval-mode residual quantizer as plain fp32 torch ops on folded weights -> (z_q, codes [B, n, T])"""
    zq, residual, codes = torch.zeros_like(z), z, []
    B, _, T = z.shape
    for i in range(n):
        p = f"{prefix}{i}."
        z_e = Fn.conv1d(residual, P[p + "in_proj.weight"], P[p + "in_proj.bias"])
        enc = Fn.normalize(z_e.transpose(1, 2).reshape(B * T, -1))
        cb = Fn.normalize(P[p + "codebook.weight"])
        dist = enc.pow(2).sum(1, keepdim=True) - 2 * enc @ cb.t() + cb.pow(2).sum(1, keepdim=True).t()
        idx = (-dist).max(1)[1].reshape(B, T)
        q = Fn.embedding(idx, P[p + "codebook.weight"]).transpose(1, 2)
        q = Fn.conv1d(z_e + (q - z_e), P[p + "out_proj.weight"], P[p + "out_proj.bias"])
        zq, residual = zq + q, residual - q
        codes.append(idx)
    return zq, torch.stack(codes, 1)


def _torch_encode(P, hp, wave, feats):
    h = R.convnext_encoder(P, hp, feats, torch.float32)
    zq, sem = _torch_rvq(P, "semantic_vq.quantizers.", 1, h)
    semantic = R.convnext_decoder(P, hp, zq, torch.float32)
    z = R.dac_latent(P, hp, wave, torch.float32)
    _, ac = _torch_rvq(P, "dac.quantizer.quantizers.", hp["n_codebooks"], z[..., : semantic.shape[-1]] - semantic)
    return sem, ac


def _launches(m, dev):
    """library launches of one encode / one decode_from_codes, from the routes the handles take"""
    L = m.convnext_layers
    unit = lambda u: 1 if u.fused(dev) else 4          # noqa: E731
    enc = m.dac.encoder
    n_enc = 1 + sum(sum(unit(u) for u in list(enc.block[1 + i].block)[:3]) + 2 for i in range(enc.n_blocks)) + 2
    dec = m.dac.decoder
    n_dec = 3 + sum((1 if dec.model[1 + i].block[1].fused(dev) else 2) + sum(unit(u) for u in list(dec.model[1 + i].block)[2:]) for i in range(dec.n_blocks))
    convnext = 1 + 3 * L
    return dict(encode=convnext + 1 + convnext + n_enc + 1, decode_from_codes=1 + convnext + 1 + n_dec)


def bench_models(rounds, res):
    dev = torch.device("cuda", torch.cuda.current_device())
    for name in ("12hz", "25hz"):
        hp = R.recipe_hp(name)
        sd = R.synth_dualcodec_state_dict(hp, 1)
        m = DualCodec(**hp)
        m.load_state_dict(sd)
        m = m.cuda().eval()
        P = {k: v.cuda() for k, v in D.fold_state_dict(sd).items()}
        T = SECONDS * SR // R.hop(hp)
        for B in (1, 16):
            wave, feats = R.synth_inputs(hp, B, T, 5)
            wave, feats = wave.cuda(), feats.cuda()
            sem, ac = m.encode(wave, sample_rate=SR, semantic_repr=feats)
            y = m.decode_from_codes(sem, ac)
            launches = _launches(m, dev)
            te = _alternate({"hip": lambda: m.encode(wave, sample_rate=SR, semantic_repr=feats), "torch": lambda: _torch_encode(P, hp, wave, feats)}, rounds)
            td = _alternate({"hip": lambda: m.decode_from_codes(sem, ac), "torch": lambda: R.decode_from_codes(P, hp, sem, ac, torch.float32)}, rounds)
            tsem, tac = _torch_encode(P, hp, wave, feats)
            audio = B * SECONDS
            for case, t, n_launch in (("encode", te, launches["encode"]), ("decode_from_codes", td, launches["decode_from_codes"])):
                row = dict(recipe=name, case=case, B=B, frames=T, seconds=SECONDS, launches=n_launch, hip_ms=t["hip"][0], hip_min_max_ms=t["hip"][1],
                           torch_fp32_ms=t["torch"][0], torch_min_max_ms=t["torch"][1], x_realtime=round(audio / t["hip"][0] * 1e3, 1),
                           speedup_vs_torch=round(t["torch"][0] / t["hip"][0], 2))
                if case == "encode":
                    row.update(semantic_code_agreement=round(float((tsem == sem).double().mean()), 4),
                               acoustic_code_agreement=round(float((tac == ac).double().mean()), 4))
                else:
                    row.update(samples=int(y.shape[2]))
                res["models"].append(row)
                print(json.dumps(row), flush=True)
            del wave, feats, sem, ac, y
        del m, P
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=5, help="rounds of the model cases")
    ap.add_argument("--json", default=None)
    ap.add_argument("--skip-models", action="store_true")
    a = ap.parse_args()
    assert not os.environ.get("AMP_LAUNCH_MANIFEST"), "time with the launch manifest off"
    res = {"quantizer": [], "models": []}
    with torch.no_grad():
        bench_quantizer(a.rounds, res)
        if not a.skip_models:
            bench_models(a.iters, res)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
