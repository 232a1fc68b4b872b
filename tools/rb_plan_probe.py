"""Whole-resblock launch plans at the benchmark shapes (B = 64), op level through amp_resblock_forward_ex (MRF mean mode): zero guards with the
round-5 plan and whole, then real x in the guards (amp_set_rb_guards(1)) under every forced plan (amp_set_rb_split_plan).  Variants alternate in one
process, each looped ~0.7 s so that the package sits at its power cap; every output is compared bitwise with the first.
    python tools/rb_plan_probe.py [rounds]      -> lines on stdout, out/rb_plan_probe.json"""
import ctypes, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from amphion_amd import _lib

L = _lib.lib()
_lib.set_precision("f16x3")
p = lambda t: ctypes.c_void_p(t.data_ptr())
DILS = (1, 3, 5)
B = 64
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
FORMS = [(64, 11, 32768), (64, 7, 32768), (32, 11, 65536), (32, 7, 65536), (64, 3, 32768), (32, 3, 65536)]
VARIANTS = [("g0 today", 0, None), ("g0 (3)", 0, (3,)), ("g1 (3)", 1, (3,)), ("g1 (2,1)", 1, (2, 1)), ("g1 (1,2)", 1, (1, 2)), ("g1 (1,1,1)", 1, (1, 1, 1))]


def rnd(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def setsw(guards, plan):
    _lib.check(L.amp_set_rb_guards(guards))
    if plan is None:
        _lib.check(L.amp_set_rb_split_plan(0, None))
    else:
        _lib.check(L.amp_set_rb_split_plan(len(plan), (ctypes.c_int * 3)(*(list(plan) + [0] * (3 - len(plan))))))


out = {}
for C, k, T in FORMS:
    h1, h2 = [], []
    for hs, ds, s0 in ((h1, DILS, 10), (h2, (1, 1, 1), 30)):
        for i, d in enumerate(ds):
            w, b = rnd(C, C, k, seed=s0 + i, scale=(C * k) ** -0.5).contiguous(), rnd(C, seed=s0 + 10 + i, scale=0.1).contiguous()
            h = ctypes.c_void_p()
            _lib.check(L.amp_conv_create(0, C, C, k, 1, d, (k * d - d) // 2, p(w), p(b), ctypes.byref(h)))
            hs.append(h)
    a1, a2 = (ctypes.c_void_p * 3)(*[h.value for h in h1]), (ctypes.c_void_p * 3)(*[h.value for h in h2])
    x = rnd(B, C, T, seed=5).cuda()
    y = torch.zeros_like(x)
    tmp = torch.zeros((2,) + tuple(x.shape), device="cuda")
    st = _lib.current_stream_ptr(x.device)

    def run():
        _lib.check(L.amp_resblock_forward_ex(a1, a2, 3, p(x), B, T, 0.1, p(y), 2, 3.0, p(tmp), st))

    ref = None
    for r in range(ROUNDS):
        for name, g, plan in VARIANTS:
            setsw(g, plan)
            y.zero_()
            run()
            torch.cuda.synchronize()
            if ref is None:
                ref = y.clone()
            same = bool(torch.equal(ref, y))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.time()
            for _ in range(20):
                run()
            torch.cuda.synchronize()
            per = (time.time() - t0) / 20
            n = max(20, int(0.7 / per))
            e0.record()
            for _ in range(n):
                run()
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / n
            out.setdefault(f"C={C} k={k}", {}).setdefault(name, []).append(round(ms, 4))
            print(f"C={C} k={k} T={T} round {r} {name:12s} {ms:.4f} ms  same_bits={same}", flush=True)
    for h in h1 + h2:
        L.amp_conv_destroy(h)
    del x, y, tmp
    torch.cuda.empty_cache()
setsw(-1, None)
os.makedirs(os.path.join(ROOT, "out"), exist_ok=True)
json.dump(out, open(os.path.join(ROOT, "out", "rb_plan_probe.json"), "w"), indent=1)
for f, d in out.items():
    print(f, {k: (min(v), max(v)) for k, v in d.items()})
