"""The f16x3 range guard in every kernel form that stages operands, op level.

Each f16x3 kernel ORs 1 into the op-level flag word (amp_range_check) when an operand it stages leaves the split-f16 range
(|x| > 4094 after the on-load activation, or infinite).  tests/test_gpu_range_guard.py triggers it in the small-grid conv and the
per-tile pair seam only; the forms below each get, with the decision taken from the fp64 predictor (tests/range_oracle.py):
  a. the exact threshold at the input (4094 passes, nextafter(4094) flags; -40 000 through leaky ReLU 0.1 is -4 000 and passes),
  b. an operand that first leaves the range INSIDE the launch (the pair seam, the x entering pair 1 of a resblock, a Snake output),
  c. values that are never staged (huge outputs, fp32 residuals, the running MRF sum, what lies beyond a ragged utterance) never flag,
  d. every form of the same op takes the same decision, with the same bits when nothing flags,
  e. a single +-inf flags and a single NaN does not, in the interior and next to the sequence end, and the non-finite outputs sit
     where the fp64 reference has them.

Which kernel ran is not inferred from the shape: the cases of a group run in ONE child process with AMP_LAUNCH_MANIFEST set (one
pytest item per group, so the child starts once whatever the number of workers), and the group's test asserts the kernels each
case's launches named.  Reachable forms that have no row here yet, not because they cannot fail: the four-step strips, the
three-in-one grids pair3 / conv_small3, conv_small's gated WN epilogues (amp_wn_forward) and the two-launch resblock split (a
generator-level policy; its manifest work column shows it, tests/test_gpu_resblock.py)."""
import json
import math
import os
import subprocess
import sys
import traceback

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T4094 = 4094.0
NEXT = torch.nextafter(torch.tensor(T4094), torch.tensor(math.inf)).item()     # the next fp32 above 4094: x16 rounds past 65504


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


# ------------------------------------------------------------------------------------------------------------------------------
# child side: the cases.  Every case raises AssertionError on a failure; the kernels it launched are read from the manifest.
# ------------------------------------------------------------------------------------------------------------------------------
def _flag():
    """the op-level word: raised since the last check?  (the check clears it)"""
    from amphion_amd import _lib

    try:
        _lib.range_check()
    except _lib.AmpError as e:
        assert e.status == _lib.AMP_ERR_RANGE, e
        return True
    return False


def _close(y, ref, rel, what):
    err = (y.double() - ref).abs().max().item()
    scale = max(1.0, ref.abs().max().item())
    assert err <= rel * scale, f"{what}: |hip - fp64| = {err:.3e} > {rel:g} x {scale:.3e}"


def _expect(flag, maxima, want, what):
    """the kernel's decision == the predictor's == what the case was built for"""
    from range_oracle import flagged

    assert flagged(maxima) == want, f"{what}: the case is mis-built, predicted maxima {maxima}"
    assert flag == want, f"{what}: flag {flag}, predicted {want} (maxima {maxima})"


def _with_margin(maxima, what):
    from range_oracle import margin

    assert margin(maxima) >= 1.5, f"{what}: within 1.5x of the threshold, maxima {maxima}"


def _switch(name, v):
    from amphion_amd import _lib

    _lib.check(getattr(_lib.lib(), name)(v))


# ---- single convs --------------------------------------------------------------------------------------------------------------
def _conv_form(cin, cout, k, B, T, stride=0):
    """a, c, e on one conv (stride > 0: a ConvTranspose1d with kernel 2 x stride); the reference is item 0's (items are independent)"""
    import functools

    import hip_helpers
    import range_oracle
    from range_oracle import nonfinite_equal

    if stride:
        pad = stride // 2
        w = _rand(cin, cout, k, seed=1, scale=cin ** -0.5)
        kw = dict(transposed=True, stride=stride, padding=pad)
    else:
        pad = (k - 1) // 2
        w = _rand(cout, cin, k, seed=1, scale=(cin * k) ** -0.5)
        kw = dict(padding=pad)
    conv_forward = functools.partial(hip_helpers.conv_forward, **kw)
    conv_ops = functools.partial(range_oracle.conv_ops, **kw)
    b = _rand(cout, seed=2, scale=0.1)
    x0 = _rand(B, cin, T, seed=3)
    _flag()
    for t in (T // 2, T - 2):
        for v, slope, want in ((T4094, 1.0, False), (NEXT, 1.0, True), (-T4094, 1.0, False),
                               (-40000.0, 0.1, False), (-41000.0, 0.1, True)):
            x = x0.clone()
            x[0, 5, t] = v
            y = conv_forward(w, b, x, slope_in=slope)
            ref, m = conv_ops(x[:1], w, b, slope_in=slope)
            what = f"x[{t}] = {v!r} slope {slope}"
            _expect(_flag(), m, want, what)
            if not want:
                _close(y[:1], ref, 5e-6, what)
        for v, want in ((math.inf, True), (-math.inf, True), (math.nan, False)):
            x = x0.clone()
            x[0, 5, t] = v
            y = conv_forward(w, b, x)
            ref, m = conv_ops(x[:1], w, b)
            what = f"x[{t}] = {v}"
            _expect(_flag(), m, want, what)
            assert nonfinite_equal(y[:1], ref, nan=v != v), what
            assert torch.isfinite(y[1:]).all(), what
    # c. never staged: a huge output (weights x 1e4) and a huge fp32 residual
    x = x0 * 0.5
    To = ref.shape[-1]
    y = conv_forward(w * 1e4, b, x, res=torch.full((B, cout, To), 1e7))
    ref, m = conv_ops(x[:1], w * 1e4, b, res=torch.full((1, cout, To), 1e7))
    assert ref.abs().max().item() > 1e6
    _expect(_flag(), m, False, "huge output / residual")
    _close(y[:1], ref, 5e-6, "huge output / residual")


def case_conv_f16x3():
    _conv_form(64, 64, 7, 1, 300)           # 64 rows, two column tiles: the pipelined kernel with half-width tiles


def case_conv_small():
    _conv_form(64, 128, 3, 1, 300)          # 128 rows, a small grid, k = 3: the whole-K kernel


def case_conv_blk():
    _conv_form(16, 256, 3, 4, 16500)        # 256 rows, 4 x 129 tiles of 128 columns >= kConvBlkMinWorkgroups: the row-blocked kernel


def case_conv_blk_kt2():
    _conv_form(64, 128, 4, 1, 49152, stride=2)   # ConvTranspose1d: 256 polyphase rows, 2 taps, 513 tiles of 96 columns: the transposed form


def case_conv_blk_ring_k7():
    _conv_form(16, 256, 7, 4, 16500)        # k = 7, 256 rows: the A-fragment-ring form (conv_blk mode 3, the default)


def case_conv_blk_narrow():
    _conv_form(16, 128, 7, 4, 33000)        # 128 rows, k = 7: two waves along the columns (WN = 2), 4 x 129 tiles of 256 columns


def case_conv_f32_never_flags():
    """exact-fp32 handles have no operand range: nothing they run flags"""
    from amphion_amd import _lib
    from hip_helpers import conv_forward

    _lib.set_precision("f32")
    try:
        w = _rand(64, 64, 7, seed=1, scale=(64 * 7) ** -0.5)
        for v in (1e5, math.inf):
            x = _rand(1, 64, 300, seed=3)
            x[0, 5, 150] = v
            conv_forward(w, None, x, padding=3)
            assert not _flag(), v
    finally:
        _lib.set_precision("f16x3")


def case_conv_ragged_beyond_length():
    """c. what lies beyond a ragged utterance is never staged: +inf / 1e6 there change no valid bit and raise nothing"""
    import ctypes

    from amphion_amd import _lib

    L = _lib.lib()
    cin, cout, k, T = 64, 128, 3, 300
    lens = [300, 177, 2]
    w = _rand(cout, cin, k, seed=1, scale=(cin * k) ** -0.5).contiguous()
    b = _rand(cout, seed=2, scale=0.1).contiguous()
    h = ctypes.c_void_p()
    _lib.check(L.amp_conv_create(0, cin, cout, k, 1, 1, 1, ctypes.c_void_p(w.data_ptr()), ctypes.c_void_p(b.data_ptr()), ctypes.byref(h)))
    try:
        base = _rand(3, cin, T, seed=3).cuda()
        ld = torch.tensor(lens, dtype=torch.int32, device="cuda")
        st = _lib.current_stream_ptr(base.device)
        outs = []
        for fill in (0.0, math.inf, 1e6):
            x = base.clone()
            for i, n in enumerate(lens):
                x[i, :, n:] = fill
            y = torch.full((3, cout, T), math.nan, device="cuda")
            _lib.check(L.amp_conv_forward_ragged(h, ctypes.c_void_p(x.data_ptr()), cin * T, 3, T, ctypes.c_void_p(ld.data_ptr()), 0.1,
                                                 None, 1.0, ctypes.c_void_p(y.data_ptr()), st))
            torch.cuda.synchronize()
            assert not _flag(), fill
            outs.append(y.cpu())
        for i, n in enumerate(lens):
            for o in outs[1:]:
                assert torch.equal(o[i, :, :n], outs[0][i, :, :n]), (i, n)
    finally:
        L.amp_conv_destroy(h)


# ---- fused pairs, strips, whole resblocks ---------------------------------------------------------------------------------------
def _pair_params(C, k, seed=0):
    s = (C * k) ** -0.5
    return (_rand(C, C, k, seed=seed + 1, scale=s), _rand(C, seed=seed + 2, scale=0.1), _rand(C, C, k, seed=seed + 3, scale=s),
            _rand(C, seed=seed + 4, scale=0.1))


def _gain_to(maxima_fn, target):
    """weight gain g with maxima_fn(g) ~= target (a few secant steps: the operand grows nearly linearly with the gain)"""
    g0, m0 = 0.0, maxima_fn(0.0)
    g1 = 1.0
    for _ in range(4):
        m1 = maxima_fn(g1)
        if abs(m1 - target) < 0.02 * target or m1 == m0:
            break
        g0, m0, g1 = g1, m1, g1 + (target - m1) * (g1 - g0) / (m1 - m0)
    return g1


def _pair_form(C, k, d, B, T):
    """a, b (the seam), c, e on amp_pair_forward; item 0 is the reference's"""
    from hip_helpers import pair_forward
    from range_oracle import nonfinite_equal, pair_ops

    w1, b1, w2, b2 = _pair_params(C, k)
    x0 = _rand(B, C, T, seed=5)
    _flag()
    run = lambda x, w1=w1, w2=w2: (pair_forward(w1, b1, w2, b2, x, dilation=d), _flag())
    ref = lambda x, w1=w1, w2=w2: pair_ops(x[:1], w1, b1, w2, b2, dilation=d)
    for t in (T // 2, T - 2):
        for v, want in ((T4094, False), (NEXT, True), (-40000.0, False), (-41000.0, True)):
            x = x0.clone()
            x[0, 5, t] = v
            (y, f), (r, m) = run(x), ref(x)
            what = f"x[{t}] = {v!r}"
            _expect(f, m, want, what)
            if not want:
                _close(y[:1], r, 5e-6, what)
        for v, want in ((math.inf, True), (-math.inf, True), (math.nan, False)):
            x = x0.clone()
            x[0, 5, t] = v
            (y, f), (r, m) = run(x), ref(x)
            _expect(f, m, want, f"x[{t}] = {v}")
            assert nonfinite_equal(y[:1], r, nan=v != v), f"x[{t}] = {v}"
    # b. the seam: c1's output leaves the range while x stays far inside it
    seam = lambda g: ref(x0, w1=w1 * g)[1][1]
    for target, want in ((2.0 * T4094, True), (0.5 * T4094, False)):
        g = _gain_to(seam, target)
        (y, f), (r, m) = run(x0, w1=w1 * g), ref(x0, w1=w1 * g)
        _with_margin(m, f"seam x{g:.3g}")
        assert m[0] < T4094 / 1.5
        _expect(f, m, want, f"seam x{g:.3g}")
        if not want:
            _close(y[:1], r, 5e-6, f"seam x{g:.3g}")
    # c. a huge output (c2 x 1e4) is never staged
    (y, f), (r, m) = run(x0, w2=w2 * 1e4), ref(x0, w2=w2 * 1e4)
    assert r.abs().max().item() > 1e4
    _expect(f, m, False, "huge output")
    _close(y[:1], r, 5e-6, "huge output")


def case_pair_tile():
    _pair_form(64, 3, 1, 1, 300)


def case_pair_strip():
    """C = 128, k = 11: 180 items x 3 one-step strips (>= 512): the A-ring strips"""
    _pair_form(128, 11, 5, 180, 500)


def _rb_params(C, k, n, seed=0):
    ps = [_pair_params(C, k, seed=seed + 10 * p) for p in range(n)]
    return [list(z) for z in zip(*ps)]        # ws1, bs1, ws2, bs2


def _rb_form(mode):
    """a, b (the x entering pair 1 / pair 2, built in registers), c, e on amp_resblock_forward"""
    from hip_helpers import resblock_forward
    from range_oracle import flagged, nonfinite_equal, resblock_ops

    _switch("amp_set_resblock_fusion", mode)
    try:
        _rb_form_cases()
    finally:
        _switch("amp_set_resblock_fusion", -1)


def _rb_form_cases():
    from hip_helpers import resblock_forward
    from range_oracle import nonfinite_equal, resblock_ops

    C, k, dils, B, T = 32, 3, (1, 3, 5), 1, 3000
    ws1, bs1, ws2, bs2 = _rb_params(C, k, 3)
    x0 = _rand(B, C, T, seed=5)
    _flag()

    def run(x, ws2=ws2, n=3):
        return resblock_forward(ws1[:n], bs1[:n], ws2[:n], bs2[:n], x, dilations=dils[:n]), _flag()

    def ref(x, ws2=ws2, n=3):
        return resblock_ops(x, ws1[:n], bs1[:n], ws2[:n], bs2[:n], dilations=dils[:n])

    for t in (T // 2, 1000, T - 2):        # 1000: on a tile seam of the eight-wave form (1000 output columns per tile)
        # a. the exact threshold on a ONE-pair launch of the same kernel: in a longer block the residual carries the spike into the
        #    next pair's input, so the block input would not be the decisive operand; here every other operand is >= 1.5x below it
        for v, want in ((T4094, False), (NEXT, True), (-40000.0, False), (-41000.0, True)):
            x = x0.clone()
            x[0, 5, t] = v
            (y, f), (r, m) = run(x, n=1), ref(x, n=1)
            assert m[0] == (abs(0.1 * v) if v < 0 else v) and max(m[1:]) < T4094 / 1.5, m
            _expect(f, m, want, f"x[{t}] = {v!r}")
            if not want:
                _close(y, r, 5e-6, f"x[{t}] = {v!r}")
        for v, want in ((math.inf, True), (math.nan, False)):
            x = x0.clone()
            x[0, 5, t] = v
            (y, f), (r, m) = run(x), ref(x)
            _expect(f, m, want, f"x[{t}] = {v}")
            assert nonfinite_equal(y, r, nan=v != v), f"x[{t}] = {v}"
    # b. pair p's c2 scaled: the x entering pair p + 1 leaves the range; no conv of pairs 0 .. p stages anything near it
    for p in (0, 1):
        for target, want in ((2.0 * T4094, True), (0.5 * T4094, False)):
            def xin(g, p=p):
                w = list(ws2)
                w[p] = w[p] * g
                return ref(x0, ws2=w)[1][2 * (p + 1)]
            g = _gain_to(xin, target)
            w = list(ws2)
            w[p] = w[p] * g
            (y, f), (r, m) = run(x0, ws2=w), ref(x0, ws2=w)
            _with_margin(m, f"pair {p} c2 x{g:.3g}")
            assert max(m[: 2 * (p + 1)]) < T4094 / 1.5, m
            _expect(f, m, want, f"x into pair {p + 1}")
            if not want:
                _close(y, r, 5e-6, f"x into pair {p + 1}")
    # c. the last pair's c2 x 1e4: a huge output, never staged
    w = list(ws2)
    w[2] = w[2] * 1e4
    (y, f), (r, m) = run(x0, ws2=w), ref(x0, ws2=w)
    _expect(f, m, False, "huge output")
    _close(y, r, 5e-6, "huge output")


def case_rb_form0():
    _rb_form(3)          # four-wave 512-column tiles at C = 32


def case_rb_form1():
    _rb_form(2)          # eight-wave 1024-column tiles


def case_resblock_forms_decide_alike():
    """d. one input through six separate convs, the chain of three pair-kernel launches, and the whole-resblock kernel in both forms:
    the same flag (the predictor's) and, when nothing flags, the same bits from the fused forms (the separate convs round the seam
    through memory in another order, so they are held to the flag only)"""
    from hip_helpers import conv_forward, resblock_forward
    from range_oracle import margin, resblock_ops

    C, k, dils, T = 32, 3, (1, 3, 5), 2100
    decided = set()
    for seed in range(8):
        ws1, bs1, ws2, bs2 = _rb_params(C, k, 3, seed=100 * seed)
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(1, C, T, generator=g) * torch.exp(torch.rand(1, C, 1, generator=g) * 3)
        _, m0 = resblock_ops(x, ws1, bs1, ws2, bs2, dilations=dils)
        s = (0.5 + 1.5 * torch.rand(1, generator=g).item()) * T4094 / max(m0)     # peak 0.5 .. 2 x the threshold
        x = x * s
        _, m = resblock_ops(x, ws1, bs1, ws2, bs2, dilations=dils)
        if margin(m) < 1.01:
            continue
        want = max(m) > T4094
        cur = x
        for w1, b1, w2, b2, d in zip(ws1, bs1, ws2, bs2, dils):
            xt = conv_forward(w1, b1, cur, dilation=d, padding=(k * d - d) // 2, slope_in=0.1)
            cur = conv_forward(w2, b2, xt, padding=(k - 1) // 2, slope_in=0.1, res=cur)
        flags = [_flag()]
        outs = []
        try:
            for mode in (None, 2, 3):
                if mode is None:
                    y = resblock_forward(ws1, bs1, ws2, bs2, x, dilations=dils, fused=False)
                else:
                    _switch("amp_set_resblock_fusion", mode)
                    y = resblock_forward(ws1, bs1, ws2, bs2, x, dilations=dils)
                outs.append(y)
                flags.append(_flag())
        finally:
            _switch("amp_set_resblock_fusion", -1)
        assert flags == [want] * 4, (seed, flags, m)
        if not want:
            assert all(torch.equal(o, outs[0]) for o in outs[1:]), seed
        decided.add(want)
    assert decided == {True, False}, decided


def case_strips_and_tiles_decide_alike():
    """d. the A-ring strips and the per-tile kernel on one input: the same flag, the same bits"""
    from hip_helpers import pair_forward
    from range_oracle import pair_ops

    C, k, d, B, T = 128, 11, 5, 180, 500
    w1, b1, w2, b2 = _pair_params(C, k)
    x = _rand(B, C, T, seed=5)
    seam = lambda g: pair_ops(x[:1], w1 * g, b1, w2, b2, dilation=d)[1][1]
    for g, want in ((1.0, False), (_gain_to(seam, 2 * T4094), True)):
        _, m = pair_ops(x[:1], w1 * g, b1, w2, b2, dilation=d)
        _with_margin(m, f"seam x{g:.3g}")
        outs, flags = [], []
        try:
            for strips in (-1, 0):
                _switch("amp_set_pair_strips", strips)
                outs.append(pair_forward(w1 * g, b1, w2, b2, x, dilation=d))
                flags.append(_flag())
        finally:
            _switch("amp_set_pair_strips", -1)
        assert flags == [want, want], (g, flags, m)
        if not want:
            assert torch.equal(outs[0], outs[1])


# ---- whole AMPBlock (BigVGAN) ----------------------------------------------------------------------------------------------------
def _ampb_params(C, k, n, seed=0):
    s = (C * k) ** -0.5
    ws1 = [_rand(C, C, k, seed=seed + 10 + p, scale=s) for p in range(n)]
    bs1 = [_rand(C, seed=seed + 20 + p, scale=0.1) for p in range(n)]
    ws2 = [_rand(C, C, k, seed=seed + 30 + p, scale=s) for p in range(n)]
    bs2 = [_rand(C, seed=seed + 40 + p, scale=0.1) for p in range(n)]
    alphas = _rand(2 * n, C, seed=seed + 50, scale=0.3)
    betas = _rand(2 * n, C, seed=seed + 51, scale=0.3)
    return ws1, bs1, ws2, bs2, alphas, betas


def _ampb_form(mode):
    """a (through Snake: the predictor decides), b (a Snake output leaves the range, x does not), c (huge output, huge running MRF
    sum), e (+-inf / NaN in the interior and next to the end) on amp_ampblock_forward"""
    from hip_helpers import ampblock_forward
    from oracle import vocoder_oracle as vo
    from range_oracle import ampblock_ops, nonfinite_equal

    _switch("amp_set_ampblock_fusion", mode)
    try:
        _ampb_form_cases()
    finally:
        _switch("amp_set_ampblock_fusion", -1)


def _ampb_form_cases():
    from hip_helpers import ampblock_forward
    from oracle import vocoder_oracle as vo
    from range_oracle import ampblock_ops, nonfinite_equal

    C, k, dils, B, T = 32, 3, (1, 3, 5), 1, 2000
    f = vo.kaiser_sinc_filter1d(0.25, 0.3, 12)
    ws1, bs1, ws2, bs2, al, be = _ampb_params(C, k, 3)
    x0 = _rand(B, C, T, seed=3, scale=1.5)
    _flag()

    def run(x, be=be, ws2=ws2, **kw):
        return ampblock_forward(ws1, bs1, ws2, bs2, al, be, True, f, f, x, dilations=dils, **kw), _flag()

    def ref(x, be=be, ws2=ws2):
        return ampblock_ops(x, ws1, bs1, ws2, bs2, al, be, True, dilations=dils)

    for t in (T // 2, T - 2):
        for v in (1500.0, -1500.0, 9000.0):
            x = x0.clone()
            x[0, 5, t] = v
            (y, fl), (r, m) = run(x), ref(x)
            _with_margin(m, f"x[{t}] = {v}")
            _expect(fl, m, abs(v) > T4094, f"x[{t}] = {v}")
            if abs(v) < T4094:
                _close(y, r, 2e-5, f"x[{t}] = {v}")
        for v in (math.inf, -math.inf, math.nan):
            # the block input is not an operand: Snake turns an infinity into NaN (sin(inf)) before anything is staged, in the
            # kernel as in the reference -- the predictor says no flag, and the NaNs must sit where the reference's do
            x = x0.clone()
            x[0, 5, t] = v
            (y, fl), (r, m) = run(x), ref(x)
            _expect(fl, m, False, f"x[{t}] = {v}")
            assert nonfinite_equal(y, r, nan=v != v), (f"x[{t}] = {v}", (~torch.isfinite(y)).sum().item(), (~torch.isfinite(r)).sum().item())
    # b. a small beta (log scale): Snake's sin^2 / beta reaches thousands while x stays O(1); act 0 (the block input's) and act 3
    #    (inside pair 1, on c1_1's output)
    for s in (0, 3):
        for lb, want in ((-9.0, True), (-7.0, False)):     # 1 / beta = 8 103 / 1 097
            b2 = be.clone()
            b2[s, 7] = lb
            (y, fl), (r, m) = run(x0, be=b2), ref(x0, be=b2)
            _with_margin(m, f"act {s} log beta {lb}")
            assert max(m[:s]) < T4094 / 1.5 if s else True
            _expect(fl, m, want, f"act {s} log beta {lb}")
            if not want:
                _close(y, r, 2e-5, f"act {s} log beta {lb}")
    # c. never staged: the last conv x 1e4, and a running MRF sum of 1e7 (modes 1 and 2)
    w = list(ws2)
    w[2] = w[2] * 1e4
    (y, fl), (r, m) = run(x0, ws2=w), ref(x0, ws2=w)
    _expect(fl, m, False, "huge output")
    _close(y, r, 2e-5, "huge output")
    y0 = torch.full((B, C, T), 1e7)
    for mrf, div in ((1, 1.0), (2, 3.0)):
        (y, fl), (r, m) = run(x0, mode=mrf, div=div, y0=y0), ref(x0)
        _expect(fl, m, False, f"MRF mode {mrf}")
        _close(y, (r + 1e7) / div, 2e-5, f"MRF mode {mrf}")


def case_ampb_form0():
    _ampb_form(3)        # four-wave 512-column tiles at C = 32


def case_ampb_form1():
    _ampb_form(2)        # eight-wave 1024-column tiles


def case_ampblock_forms_decide_alike():
    """d. one input through the separate act1d + conv launches and the whole-AMPBlock kernel: the same flag (the predictor's) and,
    when nothing flags, the same bits"""
    from hip_helpers import ampblock_forward
    from oracle import vocoder_oracle as vo
    from range_oracle import ampblock_ops, margin

    C, k, dils, T = 32, 3, (1, 3, 5), 1200
    f = vo.kaiser_sinc_filter1d(0.25, 0.3, 12)
    _switch("amp_set_ampblock_fusion", 2)
    try:
        decided = _ampb_decide(C, k, dils, T, f)
    finally:
        return decided


def _ampb_decide(C, k, dils, T, f):
    from hip_helpers import ampblock_forward
    from range_oracle import ampblock_ops, margin

    decided = set()
    for seed in range(8):
        ws1, bs1, ws2, bs2, al, be = _ampb_params(C, k, 3, seed=100 * seed)
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(1, C, T, generator=g) * torch.exp(torch.rand(1, C, 1, generator=g) * 3)
        _, m0 = ampblock_ops(x, ws1, bs1, ws2, bs2, al, be, True, dilations=dils)
        x = x * ((0.5 + 1.5 * torch.rand(1, generator=g).item()) * T4094 / max(m0))
        _, m = ampblock_ops(x, ws1, bs1, ws2, bs2, al, be, True, dilations=dils)
        if margin(m) < 1.01:
            continue
        want = max(m) > T4094
        outs, flags = [], []
        for fused in (False, True):
            outs.append(ampblock_forward(ws1, bs1, ws2, bs2, al, be, True, f, f, x, dilations=dils, fused=fused))
            flags.append(_flag())
        assert flags == [want, want], (seed, flags, m)
        if not want:
            assert torch.equal(outs[0], outs[1]), seed
        decided.add(want)
    return decided


# group -> [(case, the kernels its launches must name: exactly this set, or (set, "subset") when other launches may come along)]
GROUPS = {
    "conv": [
        (case_conv_f16x3, {"conv_f16x3_kernel"}),
        (case_conv_small, {"conv_small_kernel"}),
        (case_conv_blk, {"conv_blk_kernel/k3/wn1"}),
        (case_conv_blk_kt2, {"conv_blk_kernel/k2/wn1"}),
        (case_conv_blk_ring_k7, {"conv_blk_kernel/k7/wn1"}),
        (case_conv_blk_narrow, {"conv_blk_kernel/k7/wn2"}),
        (case_conv_f32_never_flags, {"conv_mfma_kernel"}),
        (case_conv_ragged_beyond_length, {"conv_small_kernel"}),
    ],
    "fused": [
        (case_pair_tile, {"pair_f16x3_kernel"}),
        (case_pair_strip, {"pair_strip_kernel"}),
        (case_rb_form0, {"rb_f16x3_kernel/4"}),
        (case_rb_form1, {"rb_f16x3_kernel/8"}),
        (case_resblock_forms_decide_alike, {"conv_f16x3_kernel", "pair_f16x3_kernel", "rb_f16x3_kernel/4", "rb_f16x3_kernel/8"}),
        (case_strips_and_tiles_decide_alike, {"pair_strip_kernel", "pair_f16x3_kernel"}),
    ],
    "ampb": [
        (case_ampb_form0, {"ampb_f16x3_kernel/4"}),
        (case_ampb_form1, {"ampb_f16x3_kernel/8"}),
        (case_ampblock_forms_decide_alike, {"ampb_f16x3_kernel/8", "act1d_kernel", "conv_f16x3_kernel"}),
    ],
}


def _kernel_id(name):
    """manifest name -> base name; the whole-block kernels get /<waves> (WM * WN: 4 = the four-wave form 0, 8 = form 1)"""
    base = name.split("<")[0]
    if base in ("rb_f16x3_kernel", "ampb_f16x3_kernel"):
        args = [int(v) for v in name.split("<")[1].rstrip(">").split(",")]
        return f"{base}/{args[1] * args[2]}"
    if base == "conv_blk_kernel":          # <KT, NI, HALO, CM, RING, WN>
        args = [int(v) for v in name.split("<")[1].rstrip(">").split(",")]
        return f"{base}/k{args[0]}/wn{args[5]}"
    return base


def _child(group, out):
    """run the group's cases in order.  Only a failed assertion moves on to the next case: any other error (a failed launch, a
    HIP error) ends the process at once, after recording what was done, so nothing more is started on a device in doubt."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    torch.set_num_threads(16)
    from amphion_amd import _lib

    _lib.set_precision("f16x3")
    man = os.environ["AMP_LAUNCH_MANIFEST"]
    res = {}
    for case, _ in GROUPS[group]:
        n0 = sum(1 for _ in open(man)) if os.path.exists(man) else 0
        err, fatal = None, None
        try:
            case()
        except AssertionError:
            err = traceback.format_exc()[-3000:]
        except BaseException as e:
            err, fatal = traceback.format_exc()[-3000:], e
        lines = open(man).read().splitlines()[n0:] if os.path.exists(man) else []
        res[case.__name__] = {"err": err, "kernels": sorted({_kernel_id(l.split("\t")[0]) for l in lines})}
        with open(out, "w") as fh:                # after every case: an early end leaves what was done
            json.dump(res, fh)
        if fatal is not None:
            raise fatal


# ------------------------------------------------------------------------------------------------------------------------------
# parent side: ONE test per group, so that each group's child process starts exactly once whatever the number of pytest workers
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("group", list(GROUPS))
def test_range_guard_forms(group, tmp_path):
    out, man = tmp_path / "results.json", tmp_path / "manifest.tsv"
    env = dict(os.environ, AMP_LAUNCH_MANIFEST=str(man), AMP_PRECISION="f16x3", AMP_RB_FUSION="1", AMP_AMPB_FUSION="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), group, str(out)], capture_output=True, text=True, env=env,
                       timeout=600)
    res = json.load(open(out)) if out.exists() else {}
    problems = []
    for case, kernels in GROUPS[group]:
        name = case.__name__
        if name not in res:
            problems.append(f"{name}: not run (the child ended first)")
            continue
        if res[name]["err"] is not None:
            problems.append(f"{name}:\n{res[name]['err']}")
        if set(res[name]["kernels"]) != kernels:
            problems.append(f"{name}: ran {res[name]['kernels']}, not {sorted(kernels)}")
    assert r.returncode == 0 and not problems, f"child exit {r.returncode}\n" + "\n".join(problems) + "\n" + r.stderr[-2000:]


def test_predictor_on_a_hand_worked_pair():
    """CPU: the predictor's operands for y = x + c2(lrelu(c1(lrelu(x)))) with 1 x 1 convs, worked by hand"""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from range_oracle import flagged, margin, nonfinite_equal, pair_ops, resblock_ops, staged_max

    x = torch.tensor([[[-50000.0, 100.0, 3.0]]])
    w1, b1, w2, b2 = torch.full((1, 1, 1), 0.5), torch.zeros(1), torch.full((1, 1, 1), 2.0), torch.ones(1)
    y, m = pair_ops(x, w1, b1, w2, b2, dilation=1, slope=0.1)
    # lrelu(x) = [-5000, 100, 3]; c1 = [-2500, 50, 1.5]; the seam lrelu(c1) = [-250, 50, 1.5]; c2 = [-499, 101, 4]
    assert m == [5000.0, 250.0]
    assert torch.equal(y, torch.tensor([[[-50499.0, 201.0, 7.0]]], dtype=torch.float64))
    assert flagged(m) and margin(m) == 5000.0 / 4094.0
    assert not flagged([4094.0, 250.0]) and flagged([float(NEXT)]) and flagged([math.inf])
    # the second pair stages the first one's output: -50499 through leaky ReLU 0.1
    _, m2 = resblock_ops(x, [w1, w1], [b1, b1], [w2, w2], [b2, b2], dilations=(1, 1), slope=0.1)
    assert m2[:2] == m and abs(m2[2] - 5049.9) < 1e-9
    # NaN is not the guard's business; the non-finite comparison separates NaN from +-inf only on request
    assert staged_max(torch.tensor([math.nan, -3.0])) == 3.0 and not flagged([staged_max(torch.tensor([math.nan]))])
    a, b = torch.tensor([math.nan, 1.0]), torch.tensor([math.inf, 1.0])
    assert nonfinite_equal(a, b) and not nonfinite_equal(a, b, nan=True)


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
