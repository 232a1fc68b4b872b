"""CPU: (1) tests/conv_window_ref.py::conv_window -- the fp64 reference of every large-grid conv test -- is pinned to the full fp64
F.conv1d / F.conv_transpose1d over a sweep of geometries (k < stride included: windows that no input reaches), on whole rows and on
windows that straddle both row ends; (2) the geometry table (tests/conv_geometry.py) holds every axis value it is meant to, so it cannot
shrink unnoticed; (3) tests/recipe_shapes.py keeps its ids and paddings for the recipe layers."""
import itertools
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import conv_geometry as cg  # noqa: E402
from conv_window_ref import conv_full, conv_window, out_len  # noqa: E402
from recipe_shapes import Op, recipe_ops  # noqa: E402

TOL = 1e-12       # fp64 sums of < 200 terms of O(1): rounding is ~1e-14, any slip of the index map is O(1)


def full_reference(x, w, b, res, **kw):
    return conv_full(x, w, b, res=res, **kw)


def _check(transposed, k, stride, dilation, padding, T, g):
    Tout = out_len(T, k, transposed=transposed, stride=stride, dilation=dilation, padding=padding)
    if Tout <= 0:
        return 0
    B, cin, cout = 2, 3, 4
    x = torch.randn(B, cin, T, generator=g, dtype=torch.float64)
    w = torch.randn((cin, cout, k) if transposed else (cout, cin, k), generator=g, dtype=torch.float64)
    b = torch.randn(cout, generator=g, dtype=torch.float64)
    res = torch.randn(B, cout, Tout, generator=g, dtype=torch.float64)
    kw = dict(transposed=transposed, stride=stride, dilation=dilation, padding=padding, slope_in=0.1, slope_out=0.2)
    ref, cond = full_reference(x, w, b, res, **kw)
    rows = [0, 2, 3]
    # the whole row as one window that straddles both ends, and as pieces: a window over the start, single columns, one over the end
    pieces = [(-3, 2)] + [(t, t + 1) for t in range(2, max(2, Tout - 2))] + [(max(2, Tout - 2), Tout + 5)]
    for wins in ([(-5, Tout + 7)], pieces):
        r, c, cols = conv_window(x, w, b, rows=rows, windows=wins, res=res, **kw)
        assert cols.tolist() == list(range(Tout)), (kw, k, T, wins)
        assert (r - ref[:, rows]).abs().max().item() <= TOL, (kw, k, T, wins)
        assert (c - cond[:, rows]).abs().max().item() <= TOL, (kw, k, T, wins)
    # without bias / residual / slopes, one item
    r, c, _ = conv_window(x, w, None, rows=[1], windows=[(0, Tout)], items=[1], transposed=transposed, stride=stride, dilation=dilation,
                          padding=padding)
    ref, cond = full_reference(x, w, None, None, transposed=transposed, stride=stride, dilation=dilation, padding=padding, slope_in=1.0,
                               slope_out=1.0)
    assert (r - ref[1:, 1:2]).abs().max().item() <= TOL and (c - cond[1:, 1:2]).abs().max().item() <= TOL
    return 1


def test_conv_window_matches_full_conv_transpose1d():
    g = torch.Generator().manual_seed(0)
    n = n_short = 0
    for s, k, T in itertools.product((1, 2, 3, 4, 5, 6, 8, 16), (1, 2, 3, 4, 6, 7, 10, 11, 16, 18), (1, 2, 5, 37)):
        for p in sorted({0, 1, 2, 3, 4, max(0, (k - s) // 2), k - 1, k + 2}):
            ok = _check(True, k, s, 1, p, T, g)
            n += ok
            n_short += ok and k < s and p > 0
    assert n >= 852 and n_short >= 64, (n, n_short)


def test_conv_window_matches_full_conv1d():
    g = torch.Generator().manual_seed(1)
    n = 0
    for k, d, T in itertools.product((1, 2, 3, 4, 6, 7, 8, 9, 10, 11), (1, 2, 3, 5), (1, 2, 5, 37)):
        sm = d * (k - 1) // 2
        for p in sorted({0, max(0, sm - 1), sm, sm + 1, d * (k - 1) + 1, d * (k - 1) + 3}):
            n += _check(False, k, 1, d, p, T, g)
    assert n >= 600, n


def test_conv_window_on_the_table_geometries():
    """every case of the table: conv_window on windows over both row ends == the full fp64 conv (small channel counts stand in)"""
    g = torch.Generator().manual_seed(2)
    for case in cg.run_cases():
        op = case.op
        if case.options:
            continue
        T = min(cg.shape(case)[1], 300)
        if op.out_len(T) >= 1:
            assert _check(op.transposed, op.k, op.u or 1, op.d, op.padding, T, g)


# ------------------------------------------------------------------------------------------------------------------------------
# the table holds what it is meant to
# ------------------------------------------------------------------------------------------------------------------------------
def _has(table, **want):
    def ok(r):
        return all((v(r[k]) if callable(v) else r[k] == v) for k, v in want.items())

    return any(ok(r) for r in table)


def test_table_covers_every_axis_value():
    run = [cg.describe(c) for c in cg.run_cases()]
    ct = [r for r in run if r["transposed"]]
    cv = [r for r in run if not r["transposed"]]
    small_ct = [cg.describe(c) for c in cg.CONVT_SMALL]
    large_ct = [cg.describe(c) for c in cg.CONVT_LARGE]
    # ---- ConvTranspose1d ----
    for s in (1, 2, 3, 4, 5, 6, 8, 16):
        assert _has(ct, stride=s), s
    rel = lambda f: [r for r in ct if f(r)]
    assert rel(lambda r: r["k"] < r["stride"]) and rel(lambda r: r["k"] == r["stride"]) and rel(lambda r: r["k"] == 2 * r["stride"])
    assert rel(lambda r: r["k"] == 3 * r["stride"]) and rel(lambda r: r["stride"] > 1 and r["k"] % r["stride"])
    for nt, kt in ((1, 1), (2, 2), (3, 3), (4, 5), (6, 7), (11, 11)):
        assert _has(ct, ntaps=nt, KT=kt), (nt, kt)
    assert _has(ct, padding=0)
    assert rel(lambda r: r["padding"] == (r["k"] - r["stride"]) // 2 and r["k"] > r["stride"] and (r["k"] - r["stride"]) % 2 == 0)
    assert rel(lambda r: r["padding"] == (r["k"] - r["stride"]) // 2 and r["k"] > r["stride"] and (r["k"] - r["stride"]) % 2 == 1)
    for s in (4, 8, 16):
        assert rel(lambda r: r["stride"] == s and r["padding"] % 4 == 0 and r["padding"] > 0), s
        assert rel(lambda r: r["stride"] == s and r["padding"] % 4 != 0), s
    # the largest padding with T_out > 0: one more would leave none
    assert rel(lambda r: 0 < r["Tout"] <= 2 and r["padding"] > r["k"])
    for s in (4, 8):
        for m in (0, 1, 2, 3):       # float4 scatter with every k % 4
            assert rel(lambda r: r["stride"] == s and r["padding"] % 4 == 0 and r["k"] % 4 == m), (s, m)
    assert rel(lambda r: r["stride"] == 2 and r["padding"] % 2 == 0) and rel(lambda r: r["stride"] == 2 and r["padding"] % 2 == 1)
    assert rel(lambda r: r["stride"] > 1 and r["rows"] % 32 == 0)
    for rows in (40, 72, 200):
        assert _has(ct, rows=rows), rows
    # lengths relative to the tile, small grid
    assert _has(small_ct, T=1) and _has(small_ct, T=2)
    for f in (lambda r: r["Tq"] == r["q_tile"] - 1, lambda r: r["Tq"] == r["q_tile"], lambda r: r["Tq"] == r["q_tile"] + 1,
              lambda r: r["Tq"] > 2 * r["q_tile"] and r["Tq"] % r["q_tile"]):
        assert any(f(r) for r in small_ct)
    assert _has(ct, B=1) and _has(ct, B=3)
    assert _has(ct, slope_in=0.1) and _has(ct, bias=False) and rel(lambda r: r["slope_out"] != 1.0) and _has(ct, res=True)
    assert all(r["form"] == "conv_f16x3_kernel" for r in small_ct)
    # large grid: the row-blocked kernel with 2 and 3 (and 7) taps, both chunk modes
    forms = {r["form"].rsplit("/", 1)[0] for r in large_ct}
    assert {"conv_blk_kernel/k2/wn1", "conv_blk_kernel/k3/wn1", "conv_blk_kernel/k7/wn1"} <= forms, forms
    assert all(r["rows"] % 256 == 0 and r["form"].startswith("conv_blk") for r in large_ct)
    assert any(r["KT"] == 2 and r["nchunks"] % 2 == 0 for r in large_ct) and any(r["KT"] == 2 and r["nchunks"] % 2 == 1 for r in large_ct)
    assert any(r["Tq"] % r["q_tile"] for r in large_ct)
    # ---- Conv1d ----
    for k in (2, 4, 6, 8, 9, 10, 3, 7, 11):
        assert _has(cv, k=k), k
    assert _has(cv, dilation=1) and any(r["dilation"] > 1 for r in cv)
    sm = lambda r: r["dilation"] * (r["k"] - 1) // 2
    assert _has(cv, padding=0) and any(r["padding"] == sm(r) - 1 for r in cv) and any(r["padding"] == sm(r) for r in cv)
    assert any(r["padding"] == sm(r) + 1 for r in cv) and any(r["padding"] > r["dilation"] * (r["k"] - 1) for r in cv)
    assert any(r["res"] and r["Tout"] != r["T"] and r["slope_out"] != 1.0 for r in cv)
    assert any(r["halo"] == 128 for r in cv)
    assert any(r["T"] < r["dilation"] * (r["k"] - 1) + 1 and r["Tout"] >= 1 for r in cv)
    assert any(r["form"] == "conv_small_kernel" and r["Tout"] != r["T"] for r in cv) and any(r["form"] == "conv_f16x3_kernel" for r in cv)
    opts = [c for c in cg.CONV_SMALL if c.options]
    assert any(c.options == ((cg.OPT_PAD_REFLECT, 1),) and c.op.padding == c.T - 1 for c in opts)
    assert any(c.options == ((cg.OPT_TANH, 1),) for c in opts)
    # ---- refusals ----
    tags = set().union(*(c.tags for c in cg.REFUSALS))
    assert {"12taps", "dilatedT", "halo129", "Tout0", "reflect", "tanh", "lens"} <= tags
    assert any(c.op.ntaps == 12 for c in cg.REFUSALS)
    assert any(not c.op.u and c.op.halo == 129 for c in cg.REFUSALS)
    assert any(c.op.out_len(c.T) <= 0 and c.op.u for c in cg.REFUSALS) and any(c.op.out_len(c.T) <= 0 and not c.op.u for c in cg.REFUSALS)
    assert any(c.options == ((cg.OPT_PAD_REFLECT, 1),) and not c.op.u and c.op.padding == c.T for c in cg.REFUSALS)
    ids = [c.id for c in cg.all_cases()]
    assert len(ids) == len(set(ids)), sorted(i for i in ids if ids.count(i) > 1)
    assert len(cg.run_cases()) >= 70


def test_float4_tag_is_the_float4_path():
    """the `float4` tag of a ConvTranspose1d case == the kernels' condition for the float4 scatter (stride and padding multiples of 4)"""
    for c in cg.CONVT_SMALL + cg.CONVT_LARGE:
        assert ("float4" in c.tags) == (c.op.u > 1 and c.op.u % 4 == 0 and c.op.padding % 4 == 0), c.id


def test_explicit_padding_leaves_the_recipe_ops_unchanged():
    for op in recipe_ops():
        assert op.pad is None and "p" not in op.name.split("k")[-1]
        assert op.padding == ((op.k - op.u) // 2 if op.u else (op.k * op.d - op.d) // 2)
    assert Op(8, 8, 8, 1, 4).name == "convT8-8u4k8" and Op(8, 8, 8, 1, 4, 0).name == "convT8-8u4k8p0"
    assert Op(8, 8, 3, 2).name == "conv8-8k3d2" and Op(8, 8, 3, 2, 0, 5).padding == 5
