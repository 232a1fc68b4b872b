#!/usr/bin/env python
"""Times the semantic tokenizers' down-sampling conv (csrc/dsconv_f16x3.hip) and the RepCodec / Coco drop-ins on one GPU, in one process,
alternating with what they are compared against.

    python tools/tokenizer_bench.py [--rounds 10] [--iters 5] [--json out.json] [--skip-models]

(a) Conv1d(1024, 1024, k = 3, stride 2, padding 1) -> GELU at B = 16 x T = 1500 and B = 1 x T = 1500, f16x3: amp_dsconv_forward with the GELU
    epilogue against the route the library offered before it, built here from public entries -- a copy of x with one zero column appended,
    amp_sconv_forward (stride 2, padding 1) with the weight extended by a zero fourth tap, amp_gelu in place.  Each route is REPS calls in one
    captured graph; the two graphs are replayed in alternation for --rounds rounds; medians with [min, max].  GFLOP / MB are the launcher's own
    statement (the launch manifest of a child process, --manifest-pass; the manifest is off while timing).
(b) RepCodec.quantize and CocoContentStyle.quantize at the recipe sizes (maskgct.json's semantic codec; vevosing's Coco at rate 4), B = 1 and
    B = 16 at T = 1500, against the fp32 torch restatement of tests/tokenizer_ref.py on the same GPU, alternating for --rounds rounds of --iters
    calls (device events around each call; the drop-ins' forwards end with a synchronising range check, so they are timed eagerly), with the
    library launches per call (the child's manifest rows plus the backbone's launches that write none).  Synthetic weights."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402
import torch.nn.functional as Fn  # noqa: E402

import tokenizer_ref as R  # noqa: E402
from amphion_amd import _lib  # noqa: E402

F16X3_PEAK_TF = 2500.0 / 3
REPS = 20
T_IN = 1500
OPS = ((1024, 1024, 16), (1024, 1024, 1))       # (cin, cout, B)
MODEL_B = (1, 16)


def _event_ms(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1])


def _stats(v):
    v = sorted(v)
    return round(v[len(v) // 2], 4), [round(v[0], 4), round(v[-1], 4)]


class _Op:
    """both routes of one shape with every buffer allocated up front: nothing is allocated inside a captured graph's calls"""

    def __init__(self, cin, cout, B, T):
        L, p = _lib.lib(), _lib.ptr
        g = torch.Generator().manual_seed(cin + B)
        self.w = (torch.randn(cout, cin, 3, generator=g) / (3 * cin) ** 0.5).contiguous()
        self.b = (0.1 * torch.randn(cout, generator=g)).contiguous()
        self.B, self.T, self.cin, self.cout = B, T, cin, cout
        self.x = torch.randn(B, cin, T, generator=g).cuda()
        self.ds, self.sc = ctypes.c_void_p(), ctypes.c_void_p()
        _lib.check(L.amp_dsconv_create(cin, cout, p(self.w), p(self.b), ctypes.byref(self.ds)))
        w4 = Fn.pad(self.w, (0, 1)).contiguous()
        _lib.check(L.amp_sconv_create(cin, cout, 2, 1, p(w4), p(self.b), ctypes.byref(self.sc)))
        Tout = L.amp_dsconv_out_len(self.ds, T)
        assert Tout == L.amp_sconv_out_len(self.sc, T + 1)
        self.y_new = torch.empty(B, cout, Tout, device="cuda")
        self.y_old = torch.empty(B, cout, Tout, device="cuda")
        self.xp = torch.zeros(B, cin, T + 1, device="cuda")            # the appended column stays zero
        self.need = L.amp_sconv_workspace_bytes(self.sc, B, T + 1)
        self.ws = torch.empty(self.need // 4, device="cuda")

    def new(self):
        _lib.check(_lib.lib().amp_dsconv_forward(self.ds, _lib.ptr(self.x), self.B, self.T, 1, None, 0, _lib.ptr(self.y_new),
                                                 _lib.current_stream_ptr(self.x.device)))

    def old(self):
        L, p = _lib.lib(), _lib.ptr
        st = _lib.current_stream_ptr(self.x.device)
        self.xp[:, :, :self.T].copy_(self.x)
        _lib.check(L.amp_sconv_forward(self.sc, p(self.xp), self.B, self.T + 1, None, p(self.ws), self.need, p(self.y_old), st))
        _lib.check(L.amp_gelu(p(self.y_old), self.y_old.numel(), p(self.y_old), st))

    def close(self):
        _lib.lib().amp_dsconv_destroy(self.ds)
        _lib.lib().amp_sconv_destroy(self.sc)


def _models(B):
    from amphion_amd.models.codec.coco.rep_coco_model import CocoContentStyle
    from amphion_amd.models.codec.kmeans.repcodec_model import RepCodec

    rhp, chp = R.recipe_repcodec_hp(), R.recipe_coco_hp()
    rsd, csd = R.synth_repcodec_state_dict(rhp, 3), R.synth_coco_state_dict(chp, 5, only_quantizer=True)
    rep = RepCodec(**rhp)
    rep.load_state_dict(rsd)
    coco = CocoContentStyle(cfg=R.coco_cfg(chp), construct_only_for_quantizer=True)
    coco.load_state_dict(csd)
    rep, coco = rep.cuda().eval(), coco.cuda().eval()
    x = R.synth_feats(B, T_IN, 1024, 11).cuda()
    c = R.synth_feats(B, T_IN, 24, 12).cuda()
    rsd, csd = {k: v.cuda() for k, v in rsd.items()}, {k: v.cuda() for k, v in csd.items()}
    return {"RepCodec.quantize": (lambda: rep.quantize(x), lambda: R.repcodec_quantize_plain(rsd, rhp, x)),
            "CocoContentStyle.quantize": (lambda: coco.quantize(x, c), lambda: R.coco_quantize_plain(csd, chp, x, c))}


def _count_lines(path):
    with open(path) as f:
        return sum(1 for _ in f)


def _manifest_pass(skip_models):
    man = os.environ["AMP_LAUNCH_MANIFEST"]
    out = {}
    with torch.no_grad():
        for cin, cout, B in OPS:
            op = _Op(cin, cout, B, T_IN)
            op.new()
            op.old()
            torch.cuda.synchronize()
        if not skip_models:
            for B in MODEL_B:
                for name, (hip, _) in _models(B).items():
                    hip()                                    # handles are built on the first call
                    n0 = _count_lines(man)
                    hip()
                    out[f"{name} B={B}"] = _count_lines(man) - n0
    print("LAUNCHES " + json.dumps(out))


def _manifest(skip_models):
    man = os.path.join(tempfile.mkdtemp(prefix="tokenizer_bench_"), "manifest.tsv")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--manifest-pass"] + (["--skip-models"] if skip_models else []),
                       env=dict(os.environ, AMP_LAUNCH_MANIFEST=man), check=True, timeout=900, capture_output=True, text=True)
    launches = json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("LAUNCHES "))[len("LAUNCHES "):])
    with open(man) as f:
        rows = [ln.rstrip("\n").split("\t") for ln in f]
    return rows, launches


def bench_ops(rounds, rows, res):
    for cin, cout, B in OPS:
        op = _Op(cin, cout, B, T_IN)
        graphs = {}
        for name, fn in (("dsconv", op.new), ("sconv_route", op.old)):
            fn()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for _ in range(REPS):
                    fn()
            g.replay()
            torch.cuda.synchronize()
            graphs[name] = g
        ts = {k: [] for k in graphs}
        for _ in range(rounds):
            for name, g in graphs.items():
                ts[name].append(_event_ms(g.replay) / REPS)
        row = dict(cin=cin, cout=cout, B=B, T=T_IN, T_out=int(op.y_new.shape[2]), rounds=rounds, reps_per_graph=REPS)
        for name, v in ts.items():
            row[name + "_ms"], row[name + "_min_max_ms"] = _stats(v)
        at_b = lambda r: f" B={B} " in r[4] + " "          # noqa: E731
        mr = next(r for r in rows if r[0].startswith("dsconv_f16x3_kernel") and at_b(r))
        old_rows = [r for r in rows if at_b(r) and (r[0].startswith("sconv_repack") or " k=2 " in r[4])]
        gf, t = float(mr[2]), row["dsconv_ms"]
        gf_old = sum(float(r[2]) for r in old_rows)
        row.update(kernel=mr[0], workgroups=int(mr[1]), gflop=gf, tflops=round(gf / t, 1), frac_f16x3_peak=round(gf / t / F16X3_PEAK_TF, 3),
                   sconv_route_gflop=gf_old, sconv_route_tflops=round(gf_old / row["sconv_route_ms"], 1), launches=dict(dsconv=1, sconv_route=4),
                   dsconv_over_sconv_route=round(t / row["sconv_route_ms"], 3),
                   faster_beyond_spread=bool(row["dsconv_min_max_ms"][1] < row["sconv_route_min_max_ms"][0]))
        assert float((op.y_new - op.y_old).abs().max()) <= 1e-4 * float(op.y_old.abs().max())
        res["ops"].append(row)
        print(json.dumps(row), flush=True)
        op.close()


def bench_models(rounds, iters, launches, res):
    for B in MODEL_B:
        for name, (hip, plain) in _models(B).items():
            codes, _ = hip()
            pcodes, _ = plain()
            agree = float((codes.reshape(-1) == pcodes.reshape(-1)).double().mean())
            ts = {"hip": [], "torch_fp32": []}
            for _ in range(rounds):
                for key, fn in (("hip", hip), ("torch_fp32", plain)):
                    ts[key].append(sorted(_event_ms(fn) for _ in range(iters))[iters // 2])
            # the backbone's depthwise + LayerNorm launches (one per block) and its two LayerNorms write no manifest row
            rows_ = launches.get(f"{name} B={B}")
            row = dict(model=name, B=B, T=T_IN, rounds=rounds, iters=iters, manifest_rows=rows_,
                       library_launches=None if rows_ is None else rows_ + R.recipe_repcodec_hp()["vocos_num_layers"] + 2,
                       codes_equal_fraction=round(agree, 5))
            for key, v in ts.items():
                row[key + "_ms"], row[key + "_min_max_ms"] = _stats(v)
            row["speedup_vs_torch"] = round(row["torch_fp32_ms"] / row["hip_ms"], 2)
            res["models"].append(row)
            print(json.dumps(row), flush=True)
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--skip-models", action="store_true")
    ap.add_argument("--manifest-pass", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.manifest_pass:
        return _manifest_pass(a.skip_models)
    assert not os.environ.get("AMP_LAUNCH_MANIFEST"), "time with the launch manifest off"
    assert _lib.get_precision() == "f16x3"
    res = {"ops": [], "models": []}
    rows, launches = _manifest(a.skip_models)
    with torch.no_grad():
        bench_ops(a.rounds, rows, res)
        if not a.skip_models:
            bench_models(a.rounds, a.iters, launches, res)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
