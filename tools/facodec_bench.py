#!/usr/bin/env python
"""Times FACodec's drop-ins (amphion_amd/models/codec/ns3_codec) and the anti-aliased residual unit on one GPU, in one process, alternating
with what each is compared against.

    python tools/facodec_bench.py [--rounds 10] [--iters 10] [--json out.json] [--skip-recipe]

(a) The residual unit y = x + conv1x1(A2(conv7(A1(x)))), A = Activation1d(SnakeBeta): the fused launch (csrc/aa_unit_f16x3.hip) against the
    handle's own four launches (act1d -> conv -> act1d -> conv + residual), through the SAME entry point (amp_aa_unit_forward) with the route
    switched at create time, same weights, at B = 16 and the columns that 10 s at 16 kHz are at that width of the public recipe.  Each route is
    REPS calls in one captured graph; the two graphs are replayed in alternation for --rounds rounds; medians with [min, max].  GFLOP / MB are
    the launcher's own statement (the launch manifest of a child process, --manifest-pass; the manifest is off while timing) and give TFLOP/s
    and TB/s of the fused launch.
(b) The public-recipe encoder (ngf 32, up_ratios [2, 4, 5, 5], 256 latent channels) and (c) decoder.inference (1024 initial channels,
    up_ratios [5, 5, 4, 2]) for B = 1 and B = 16 x 10 s at 16 kHz against the fp32 torch restatement of tests/facodec_ref.py on the same GPU:
    time, x real time, launches per forward.  Synthetic weights."""
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
import facodec_ref as R  # noqa: E402
from amphion_amd import _lib  # noqa: E402
from amphion_amd.models.codec.ns3_codec import FACodecDecoder, FACodecEncoder  # noqa: E402
from amphion_amd.models.codec.ns3_codec.facodec import ResidualUnit  # noqa: E402

F16X3_PEAK_TF = 2500.0 / 3
HBM_TBS = 8.0
REPS = 20
SR = 16000
SECONDS = 10
B_OP = 16
# (C, columns): the encoder's first block (16 kHz), the decoder's last (16 kHz) and last but one (8 kHz); every dilation of a block
UNITS = tuple((c, t, d) for c, t in ((32, SR * SECONDS), (64, SR * SECONDS), (128, SR * SECONDS // 2)) for d in (1, 3, 9))


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


def _unit(c, d, mode, like=None):
    u = ResidualUnit(c, dilation=d)
    u.load_state_dict(like.state_dict() if like is not None else R.synth_unit_state_dict(c, c + d))
    u = u.cuda().eval()
    _lib.check(_lib.lib().amp_set_aa_unit_fusion(mode))
    try:
        u._handle(torch.device("cuda", torch.cuda.current_device()))
    finally:
        _lib.check(_lib.lib().amp_set_aa_unit_fusion(-1))
    return u


def _manifest_pass():
    with torch.no_grad():
        for c, t, d in UNITS:
            _unit(c, d, 1)(torch.randn(B_OP, c, t, device="cuda"))
        torch.cuda.synchronize()


def _manifest():
    man = os.path.join(tempfile.mkdtemp(prefix="facodec_bench_"), "manifest.tsv")
    subprocess.run([sys.executable, os.path.abspath(__file__), "--manifest-pass"], env=dict(os.environ, AMP_LAUNCH_MANIFEST=man), check=True, timeout=600)
    with open(man) as f:
        rows = [ln.rstrip("\n").split("\t") for ln in f]
    return [r for r in rows if r[0].startswith("aa_unit_f16x3_kernel")]


def bench_units(rounds, res):
    man = _manifest()
    dev = torch.device("cuda", torch.cuda.current_device())
    for c, t, d in UNITS:
        fused = _unit(c, d, 1)
        four = _unit(c, d, 0, like=fused)
        policy = _unit(c, d, -1, like=fused)
        x = torch.randn(B_OP, c, t, generator=torch.Generator(device="cuda").manual_seed(c + d), device="cuda")
        routes = {}
        for name, u in (("fused", fused), ("four_launch", four)):
            out = torch.empty_like(x)
            u.run(x, out)                                    # warm: handles, LDS attribute
            torch.cuda.synchronize()
            need = _lib.lib().amp_aa_unit_workspace_bytes(u._handle(dev), B_OP, t)
            ws = torch.empty(need // 4, device="cuda") if need else None
            h = u._handle(dev)

            def call(h=h, out=out, ws=ws, need=need):
                _lib.check(_lib.lib().amp_aa_unit_forward(h, _lib.ptr(x), B_OP, t, _lib.ptr(out), _lib.ptr(ws), need, _lib.current_stream_ptr(dev)))

            call()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for _ in range(REPS):
                    call()
            routes[name] = (g, out, ws)
        ts = {k: [] for k in routes}
        for _ in range(rounds):
            for name in routes:
                ts[name].append(_time(routes[name][0].replay, 1, 1)[0] / REPS)
        row = dict(C=c, d=d, B=B_OP, T=t, rounds=rounds, policy="fused" if policy.fused(dev) else "four_launch")
        for name, v in ts.items():
            v = sorted(v)
            row[name + "_ms"] = round(v[len(v) // 2], 4)
            row[name + "_min_max_ms"] = [round(v[0], 4), round(v[-1], 4)]
        mr = next(r for r in man if f"aa unit C={c} d={d} " in r[4])
        gf, mb, tf = float(mr[2]), float(mr[3]), row["fused_ms"]
        row.update(kernel=mr[0], workgroups=int(mr[1]), gflop=gf, mb=mb, tflops=round(gf / tf, 1), frac_f16x3_peak=round(gf / tf / F16X3_PEAK_TF, 3),
                   tb_per_s=round(mb / tf / 1e3, 2), frac_hbm=round(mb / tf / 1e3 / HBM_TBS, 3), fused_over_four_launch=round(tf / row["four_launch_ms"], 3))
        assert float((routes["fused"][1] - routes["four_launch"][1]).abs().max()) <= 1e-3 * float(routes["four_launch"][1].abs().max())
        res["units"].append(row)
        print(json.dumps(row), flush=True)
        del routes, x


def _unit_launches(units, dev):
    return sum(1 if u.fused(dev) else 4 for u in units)


def bench_recipe(iters, res):
    dev = torch.device("cuda", torch.cuda.current_device())
    ehp, dhp = R.recipe_encoder_hp(), R.recipe_decoder_hp()
    esd, dsd = R.synth_encoder_state_dict(ehp, 1), R.synth_decoder_state_dict(dhp, 2)
    enc = FACodecEncoder(**ehp)
    enc.load_state_dict(esd)
    enc = enc.cuda().eval()
    dec = FACodecDecoder(**dhp)
    dec.load_state_dict(dsd)
    dec = dec.cuda().eval()
    esd_d = {k: v.cuda() for k, v in esd.items()}
    dsd_d = {k: v.cuda() for k, v in dsd.items() if not k.startswith(("quantizer.", "timbre_encoder."))}
    frames = SR * SECONDS // 200
    for B in (1, 16):
        x = C.synth_wave(B, SR * SECONDS, 5).cuda()
        z = enc(x)
        # first conv; per block 3 units, the activation, repack + conv; the activation and the last conv
        launches = 1 + sum(_unit_launches(list(enc.block[1 + i].block)[:3], dev) + 3 for i in range(enc.n_blocks)) + 2
        t = _time(lambda: enc(x), iters, 2)
        tr = _time(lambda: R.encoder_forward(esd_d, ehp, x, torch.float32), max(3, iters // 3), 1)
        row = dict(B=B, samples=SR * SECONDS, frames=int(z.shape[2]), launches=launches, encoder_ms=round(t[0], 3), encoder_min_max_ms=[round(t[1], 3), round(t[2], 3)],
                   torch_fp32_ms=round(tr[0], 3), torch_min_max_ms=[round(tr[1], 3), round(tr[2], 3)], x_realtime=round(B * SECONDS / t[0] * 1e3, 1),
                   speedup_vs_torch=round(tr[0] / t[0], 2))
        res["encoder"].append(row)
        print(json.dumps(row), flush=True)
        q = C.synth_latent(B, 256, frames, 6).cuda()
        spk = (0.5 * C.synth_latent(B, 256, 1, 7)[:, :, 0]).cuda()
        y = dec.inference(q, spk)
        # timbre_linear, LayerNorm, two element-wise torch ops (* gamma + beta), first conv; per block the activation, the transposed conv (no
        # Snake in front: one launch on either route), 3 units; the activation, the last conv
        launches = 5 + sum(2 + _unit_launches(list(dec.model[1 + i].block)[2:], dev) for i in range(dec.n_blocks)) + 2
        t = _time(lambda: dec.inference(q, spk), iters, 2)
        tr = _time(lambda: R.decoder_inference(dsd_d, dhp, q, spk, torch.float32), max(3, iters // 3), 1)
        row = dict(B=B, frames=frames, samples=int(y.shape[2]), launches=launches, decoder_ms=round(t[0], 3), decoder_min_max_ms=[round(t[1], 3), round(t[2], 3)],
                   torch_fp32_ms=round(tr[0], 3), torch_min_max_ms=[round(tr[1], 3), round(tr[2], 3)], x_realtime=round(B * y.shape[2] / SR / t[0] * 1e3, 1),
                   speedup_vs_torch=round(tr[0] / t[0], 2))
        res["decoder"].append(row)
        print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--json", default=None)
    ap.add_argument("--skip-recipe", action="store_true")
    ap.add_argument("--manifest-pass", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.manifest_pass:
        return _manifest_pass()
    assert not os.environ.get("AMP_LAUNCH_MANIFEST"), "time with the launch manifest off"
    res = {"units": [], "encoder": [], "decoder": []}
    with torch.no_grad():
        bench_units(a.rounds, res)
        if not a.skip_recipe:
            bench_recipe(a.iters, res)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
