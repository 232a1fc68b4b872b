#!/usr/bin/env python
"""Times the Amphion acoustic codec drop-ins (amphion_amd/models/codec/amphion_codec/codec.py) against the fp32 torch restatement of
tests/codec_ref.py on the same GPU, in one process, alternating.

    python tools/codec_bench.py [--iters 10] [--warmup 2] [--json out.json]

Cases: the MaskGCT recipe (encoder d_model 96, strides [3, 4, 5, 8], 12 x 1024 x 8 FVQ, Vocos 512 / 4096 / 30 layers) for one 10-s prompt and
for B = 16 x 10 s of 24 kHz audio: wave -> latent -> codes, and codes -> latent -> wave.  Synthetic weights.  The
fused unit's GFLOP / MB come from the launch manifest of a child process (--manifest-pass); the fused unit at C = 96 and C = 192 and the four launches it
replaces are each timed as REPS calls in one captured graph, in alternation, and the fused one is set against both roofs (f16x3 nominal peak = f16 dense MFMA peak / 3; HBM 8 TB/s)."""
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
import vocos_ref as V  # noqa: E402
from amphion_amd.models.codec.amphion_codec.codec import CodecDecoder, CodecEncoder, ResidualUnit  # noqa: E402

F16X3_PEAK_TF = 2500.0 / 3
HBM_TBS = 8.0
REPS = 20
SR = 24000
SIZES = ((1, 10), (16, 10))
UNITS = ((96, 80000), (192, 20000))      # (C, columns of one 10-s item at that stage)


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
    return ts[len(ts) // 2]


def _models():
    ehp, fhp, vhp = C.recipe_encoder_hp(), C.recipe_fvq_hp(), V.maskgct_decoder_hp()
    esd = C.synth_encoder_state_dict(ehp, 1)
    qsd = C.synth_fvq_state_dict(fhp, 2)
    vsd = V.synth_vocos_state_dict(vhp, 3)
    enc = CodecEncoder(**ehp)
    enc.load_state_dict(esd)
    dec = CodecDecoder(in_channels=fhp["D"], num_quantizers=fhp["N"], codebook_size=fhp["K"], codebook_dim=fhp["d"], quantizer_type="fvq",
                       use_l2_normlize=True, use_vocos=True, vocos_dim=vhp["dim"], vocos_intermediate_dim=vhp["intermediate_dim"],
                       vocos_num_layers=vhp["num_layers"], n_fft=vhp["n_fft"], hop_size=vhp["hop_size"])
    dec.load_state_dict({**{"quantizer." + k: v for k, v in qsd.items()}, **{"model." + k: v for k, v in vsd.items()}})
    dev = lambda sd: {k: v.cuda() for k, v in sd.items()}     # noqa: E731
    return (ehp, fhp, vhp), (dev(esd), dev(qsd), dev(vsd)), enc.cuda().eval(), dec.cuda().eval()


def _unit(Cn, dil=3):
    u = ResidualUnit(Cn, dilation=dil).cuda().eval()
    with torch.no_grad():
        for p in u.parameters():
            if p.shape[-1] == 1 and p.dim() == 3 and p.shape[0] == 1:
                p.uniform_(0.5, 2.0)
    return u


def _manifest_pass():
    hps, sds, enc, dec = _models()
    with torch.no_grad():
        x = C.synth_wave(1, SR, 5).cuda()
        z = enc(x)
        torch.cuda.synchronize()
        for Cn, cols in UNITS:
            _unit(Cn)(torch.randn(16, Cn, cols, device="cuda"))
        torch.cuda.synchronize()


def _manifest():
    man = os.path.join(tempfile.mkdtemp(prefix="codec_bench_"), "manifest.tsv")
    subprocess.run([sys.executable, os.path.abspath(__file__), "--manifest-pass"], env=dict(os.environ, AMP_LAUNCH_MANIFEST=man), check=True, timeout=600)
    with open(man) as f:
        return [ln.rstrip("\n").split("\t") for ln in f]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--json", default=None)
    ap.add_argument("--manifest-pass", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.manifest_pass:
        return _manifest_pass()
    assert not os.environ.get("AMP_LAUNCH_MANIFEST"), "time with the launch manifest off"
    rows = _manifest()
    unit_rows = [r for r in rows if r[0].startswith("codec_unit_f16x3_kernel") and " B=16" in r[4]]
    (ehp, fhp, vhp), (esd, qsd, vsd), enc, dec = _models()
    # first conv + per block (3 units: 1 launch fused, 4 unfused; Snake + space-to-depth, k = 2 conv) + Snake + last conv
    dev0 = torch.device("cuda", torch.cuda.current_device())
    enc_launches = 3 + sum(2 + sum(1 if u.fused(dev0) else 4 for u in list(enc.block[1 + i].block)[:3]) for i in range(enc.n_blocks))
    res = {"encoder_launches": enc_launches, "cases": [], "unit": []}
    print(json.dumps({"encoder_launches_per_forward": enc_launches, "quantize_launches": 1, "vq2emb_launches": 1}))
    with torch.no_grad():
        for B, secs in SIZES:
            x = C.synth_wave(B, SR * secs, 7).cuda()
            z = enc(x)
            _, codes = dec.quantize(z)
            t_enc = _time(lambda: dec.quantize(enc(x)), a.iters, a.warmup)
            t_enc_ref = _time(lambda: C.rvq_forward(qsd, fhp, C.encoder_forward(esd, ehp, x, torch.float32), torch.float32), max(3, a.iters // 3), 1)
            t_q = _time(lambda: dec.quantize(z), a.iters, a.warmup)
            t_q_ref = _time(lambda: C.rvq_forward(qsd, fhp, z, torch.float32), max(3, a.iters // 3), 1)
            t_dec = _time(lambda: dec(dec.vq2emb(codes)), a.iters, a.warmup)
            t_dec_ref = _time(lambda: V.vocos_forward(vsd, vhp, C.vq2emb(qsd, fhp, codes, torch.float32), dtype=torch.float32), max(3, a.iters // 3), 1)
            audio = B * secs
            row = dict(B=B, seconds=secs, frames=int(z.shape[2]),
                       wave_to_codes_ms=round(t_enc, 3), wave_to_codes_torch_ms=round(t_enc_ref, 3), wave_to_codes_x_realtime=round(audio / t_enc * 1e3, 1),
                       quantize_ms=round(t_q, 3), quantize_torch_ms=round(t_q_ref, 3),
                       codes_to_wave_ms=round(t_dec, 3), codes_to_wave_torch_ms=round(t_dec_ref, 3), codes_to_wave_x_realtime=round(audio / t_dec * 1e3, 1))
            res["cases"].append(row)
            print(json.dumps(row))
        # the fused launch against the four launches it replaces: the SAME handle entry (amp_codec_unit_forward) with the route switched at
        # create time, same weights, each as REPS calls in one captured graph, timed in alternation
        from amphion_amd import _lib
        for (Cn, cols), mr in zip(UNITS, unit_rows):
            units = {}
            for name, mode in (("fused", 1), ("four_call", 0)):
                _lib.check(_lib.lib().amp_set_codec_unit_fusion(mode))
                u = _unit(Cn)
                if units:
                    u.load_state_dict(units["fused"][0].state_dict())
                xin = torch.randn(16, Cn, cols, generator=torch.Generator(device="cuda").manual_seed(Cn), device="cuda")
                out = torch.empty_like(xin)
                u.run(xin, out)
                assert u.fused(xin.device) == bool(mode)
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    for _ in range(REPS):
                        u.run(xin, out)
                units[name] = (u, g, xin, out)
            _lib.check(_lib.lib().amp_set_codec_unit_fusion(-1))
            ts = {"fused": [], "four_call": []}
            for _ in range(max(5, a.iters)):
                for name in ("fused", "four_call"):
                    ts[name].append(_time(units[name][1].replay, 1, 1) / REPS)
            med = {k: sorted(v)[len(v) // 2] for k, v in ts.items()}
            t = med["fused"]
            gf, mb = float(mr[2]), float(mr[3])
            tf, tbs = gf / t, mb / t / 1e3
            row = dict(C=Cn, B=16, columns=cols, kernel=mr[0], workgroups=int(mr[1]), gflop=gf, mb=mb, rounds=len(ts["fused"]),
                       fused_ms=round(t, 4), fused_min_max_ms=[round(min(ts["fused"]), 4), round(max(ts["fused"]), 4)],
                       four_call_ms=round(med["four_call"], 4), four_call_min_max_ms=[round(min(ts["four_call"]), 4), round(max(ts["four_call"]), 4)],
                       tflops=round(tf, 1), frac_f16x3_peak=round(tf / F16X3_PEAK_TF, 3), flop_per_byte=round(gf * 1e3 / mb, 1),
                       tb_per_s=round(tbs, 2), frac_hbm=round(tbs / HBM_TBS, 3))
            res["unit"].append(row)
            print(json.dumps(row))
            del units
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
