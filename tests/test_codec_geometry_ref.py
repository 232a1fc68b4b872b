"""CPU: (1) the codec geometry table (tests/codec_geometry.py) holds every axis value it is meant to, and -- by the model of the fused
transposed conv written from the kernel's text -- reaches every store branch of tconv_store4 in every stride class, q_first > 0, full and
ragged last tiles and the 4 / 2 / 1 row-block groups, with exactly one owner per output sample; (2) the existing per-element bounds the GPU
sweep holds the ops to (dac_ref.tconv_bound, codec_ref.sconv_bound / unit_bound, facodec_ref.unit_bound) separate right from subtly wrong at
every geometry of the table: the kernels' three-term split-f16 arithmetic and the fp32 restatements meet them, a kernel that lost one
correction term and fp64 mutants with one slip of the index map (padding off by one, the polyphase taps swapped, the column past the end
clamped, the output_padding columns left at the bias, padding filled with the clamped sample, dilation off by one) exceed them."""
import os
import sys

import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import codec_geometry as cg  # noqa: E402
import codec_ref as C  # noqa: E402
import f16x3_emulation as E  # noqa: E402
import facodec_ref as FR  # noqa: E402


# ------------------------------------------------------------------------------------------------------------------------------
# the table holds what it is meant to
# ------------------------------------------------------------------------------------------------------------------------------
def test_table_covers_every_axis_value():
    for table, fused in ((cg.TCONV_FUSED, True), (cg.TCONV_UNFUSED, False)):
        grid = [c for c in table if (c.cin, c.cout) == (32, 16) and c.built]
        assert all(c.fused == fused for c in grid)
        for s in range(2, 9):
            for p in (0, 1, (s + 1) // 2, s - 1, s, s + 1, 2 * s):
                ops = {c.op for c in grid if (c.s, c.p) == (s, p)}
                want = {o for o in (0, 1, min(p, s - 1)) if o < s and o <= p}
                assert ops == want, (s, p, ops, want)
            for c in grid:
                if c.s == s:
                    assert c.Ts == tuple(T for T in (1, 2, 63, 64, 65, 129) if c.out_len(T) > 0) and c.Ts, c.id
            for cout in (1, 3, 33, 40):
                ps = {c.p for c in table if (c.cin, c.cout, c.s) == (32, cout, s)}
                assert (s + 1) // 2 in ps and any(p >= s for p in ps), (s, cout, ps)
        assert any(c.op > 1 for c in grid) and any(c.p == 0 for c in grid) and any(c.p >= c.s for c in grid)
        for cin in (96, 384):
            wide = [c for c in table if c.cin == cin]
            assert {c.s for c in wide} == {4, 6, 7} and all(c.cout == cin // 2 and c.p != (c.s + 1) // 2 for c in wide)
        M = {c.cout * c.s for c in table}
        assert any(m < 32 for m in M) and any(m % 2 for m in M) and any(m % 32 and m > 32 for m in M)
    assert [c.id.replace("unfused", "fused") for c in cg.TCONV_UNFUSED[:len(cg.TCONV_FUSED)]] == [c.id for c in cg.TCONV_FUSED]
    extra = cg.TCONV_UNFUSED[len(cg.TCONV_FUSED):]
    assert {c.s for c in extra} >= {1, 9} and any(c.cin == 48 for c in extra) and all(not c.built and c.fused for c in extra)
    assert any(c.s == 9 and c.op > 1 for c in extra)
    # sconv
    for s in range(1, 9):
        for p in (0, 1, (s + 1) // 2, s, 2 * s - 1):
            for cin in (32, 24):
                c = next(c for c in cg.SCONV if (c.s, c.p, c.cin) == (s, p, cin))
                assert c.cout == 16 and max(1, 2 * s - 2 * p) in c.Ts and 2 * s + 1 in c.Ts and 97 in c.Ts, c.id
                pos = sorted((c.out_len(T) + 1) * s for T in c.Ts)
                assert any(256 - s < v <= 256 for v in pos) and any(257 <= v < 257 + s for v in pos), (c.id, pos)
                assert c.out_len(c.Ts[0]) >= 1 and (c.Ts[0] == 1 or c.out_len(c.Ts[0] - 1) == 0), c.id     # the shortest valid length
                if s > 1:
                    assert any((T + 2 * p) % s for T in c.Ts), c.id
    assert any((c.out_len(T) + 1) * c.s in (256, 257) for c in cg.SCONV for T in c.Ts)
    # units
    for kind, TN, wide in (("codec", 64, 192), ("aa", 54, 128)):
        us = [u for u in cg.UNITS if u.kind == kind and u.fused]
        assert sorted(u.id for u in cg.UNITS if u.kind == kind and not u.fused) == sorted(u.id.replace("/fused", "/unfused") for u in us if u.built)
        assert {u.d for u in us if u.C == 32} == set(range(1, 11)) and {u.d for u in us if u.C == wide} == {2, 8}
        assert all(u.built == (u.d <= 9) for u in us)
        for u in us:
            d = u.d
            assert set(u.Ts) == {1, 3 * d, 3 * d + 1, TN - 1, TN, TN + 1, TN + 3 * d + 1, 2 * TN + 5}, u.id
    assert sum(1 for u in cg.UNITS if u.kind == "aa" and not u.beta and u.fused) == 1
    # refusals
    R = cg.REFUSALS
    assert any(c.kind == "tconv" and c.op >= c.s and c.refuse[:2] == ("create", cg.AMP_ERR_INVALID) for c in R)
    assert any(c.kind == "tconv" and c.p < c.op < c.s and c.refuse[:2] == ("create", cg.AMP_ERR_UNSUPPORTED) for c in R)
    assert any(c.kind == "tconv" and c.op <= c.p and c.op < c.s and c.out_len(c.Ts[0]) <= 0 and c.refuse[:2] == ("forward", cg.AMP_ERR_INVALID) for c in R)
    assert any(c.kind == "tconv" and c.p == 2 * c.s and c.Ts == (1,) for c in R) and any(c.kind == "tconv" and c.out_len(c.Ts[0]) == 0 for c in R)
    assert any(c.kind == "sconv" and c.Ts[0] + 2 * c.p == 2 * c.s - 1 and c.refuse[:2] == ("forward", cg.AMP_ERR_INVALID) for c in R)
    assert any(c.kind == "codec" and c.d < 1 for c in R) and any(c.kind == "aa" and c.d < 1 for c in R)
    assert sorted(c.id for g in cg.GROUPS for c in cg.refusals(g)) == sorted(c.id for c in R)
    ids = [c.id for g in cg.GROUPS.values() for c in g] + [c.id + "/refused" for c in R]
    assert len(ids) == len(set(ids)), sorted(i for i in ids if ids.count(i) > 1)
    print("\ncases per group:", {g: len(v) for g, v in cg.GROUPS.items()}, "refusals:", len(R),
          "calls:", {g: sum(len(c.Ts) * (1 if c.kind in ("codec", "aa") else 2) for c in v) for g, v in cg.GROUPS.items()})


def test_tconv_model_reaches_every_branch_with_one_owner():
    reached = {}
    groups, first, full_last, ragged_last, many_tiles = set(), set(), 0, 0, 0
    n = 0
    for c in cg.TCONV_FUSED:
        assert c.built and c.cin % 32 == 0 and c.cin <= 384 and 2 <= c.s <= 8
        for T in c.Ts:
            m = cg.tconv_model(c.cout, c.s, c.p, c.op, T)
            n += 1
            assert (m["owners"] == 1).all(), (c.id, T, "output samples with", sorted(set(m["owners"].flatten().tolist())), "owners")
            # q_first and the last tile against the definition: the columns that hold any output sample
            q_lo, q_hi = cg.tconv_columns(c.s, c.p, c.op, T)
            assert (m["q_first"], m["q_last"]) == (q_lo, q_hi) and q_hi <= T, (c.id, T, m["q_first"], m["q_last"], q_lo, q_hi)
            assert (m["tiles"] - 1) * cg.TC_TN < q_hi - q_lo + 1 <= m["tiles"] * cg.TC_TN, (c.id, T)
            reached.setdefault(c.s, set()).update(m["branches"])
            groups.update(m["groups"])
            first.add(min(q_lo, 2))
            nq = q_hi - q_lo + 1
            full_last += nq % cg.TC_TN == 0
            ragged_last += nq % cg.TC_TN != 0 and m["tiles"] > 1
            many_tiles += m["tiles"] >= 3
    print(f"\ntconv model over {n} (case, T) pairs: every output sample has one owner; branches reached per stride:")
    for s in sorted(reached):
        print(f"  s = {s} ({'s % 4 == 0' if s % 4 == 0 else 'even' if s % 2 == 0 else 'odd'}): {sorted(reached[s])}")
        assert set(cg.stride_class_branches(s)) <= reached[s], (s, sorted(set(cg.stride_class_branches(s)) - reached[s]))
    assert set(reached) == set(range(2, 9))
    assert groups == {1, 2, 4}, groups                     # the row-block sweep in groups of 4, 2 and 1
    assert first == {0, 1, 2}, first                       # q_first = 0, 1 and >= 2: the first tile starts past column 0
    assert full_last and ragged_last and many_tiles, (full_last, ragged_last, many_tiles)


def test_tconv_row_sweep_visits_every_quad_once_and_the_model_sees_a_second_owner():
    for M in (1, 31, 33, 64, 65, 231, 320, 1344, 1536):
        rows, _ = cg.tconv_row_quads(M)
        assert sorted(rows) == list(range(0, (M + 31) // 32 * 32, 4)), M
    # the model is not blind: a sweep that visits one row block twice, or skips one, shows in the owner counts
    keep = cg.tconv_row_quads
    try:
        cg.tconv_row_quads = lambda M: (keep(M)[0] + [0], keep(M)[1])
        assert cg.tconv_model(16, 4, 2, 0, 65)["owners"].max() == 2
        cg.tconv_row_quads = lambda M: (keep(M)[0][1:], keep(M)[1])
        assert cg.tconv_model(16, 4, 2, 0, 65)["owners"].min() == 0
    finally:
        cg.tconv_row_quads = keep
    assert (cg.tconv_model(16, 4, 2, 0, 65)["owners"] == 1).all()


# ------------------------------------------------------------------------------------------------------------------------------
# the bounds separate right from subtly wrong
# ------------------------------------------------------------------------------------------------------------------------------
def _worst(y, ref, tol):
    return float(((y.double() - ref).abs() / tol).max())


def snake32(x, alpha):
    a = alpha.float()
    return x + (1.0 / (a + 1e-9)) * torch.sin(a * x).pow(2)


def tconv_poly(a, w, b, s, p, op, shift=0, swap=False, clamp=False, op_bias=False):
    """the polyphase form the kernel computes, in fp64, with one optional slip: y[o, t] = b[o] + sum_c w[c, o, r] a[c, q] + w[c, o, r + s] a[c, q - 1],
    u = t + p (+ shift), q = u div s, r = u mod s; columns outside [0, T) read 0 (clamp: column T reads a[T - 1]).  Computed as the
    un-cropped transposed conv full[u], u in [0, (T + 1) s), which holds exactly these two taps per u, and indexed at u; beyond it: the bias."""
    Bn, cin, T = a.shape
    Tout = cg.tconv_out_len(T, s, p, op)
    if swap:
        w = torch.cat([w[:, :, s:], w[:, :, :s]], dim=2)
    if clamp:
        a = torch.cat([a, a[:, :, -1:]], dim=2)            # tap 0 of column T; its tap 1 lands at u >= (T + 1) s, which no output reads
    full = F.conv_transpose1d(a, w, None, stride=s)[:, :, :(T + 1) * s]
    u = torch.arange(Tout) + p + shift
    ok = (u >= 0) & (u < full.shape[2])
    y = b[None, :, None] + full[:, :, u.clamp(0, full.shape[2] - 1)] * ok
    if op_bias and op:
        y[:, :, Tout - op:] = b[None, :, None]
    return y


def test_tconv_bound_separates_right_from_wrong():
    cases = [c for c in cg.TCONV_FUSED + cg.TCONV_UNFUSED[len(cg.TCONV_FUSED):] if c.cin == 32]
    assert len(cases) >= 170
    n = 0
    three_worst, mutants = 0.0, {}
    for c in cases:
        P = cg.tensors(c)
        w, b = P["w"], P["b"]
        kw = dict(transposed=True, stride=c.s, padding=c.p, output_padding=c.op)
        for T in c.Ts:
            x = cg.inputs(c, T)
            for with_alpha in (True, False):
                alpha = P["alpha"] if with_alpha else None
                ref, tol = cg.reference(c, P, x, with_alpha)
                n += 1
                a64 = C.snake(x.double(), alpha) if with_alpha else x.double()
                assert float((tconv_poly(a64, w, b, c.s, c.p, c.op) - ref).abs().max()) <= 1e-12, (c.id, T)
                a32 = snake32(x, alpha) if with_alpha else x
                r3 = _worst(E.conv(a32, w.float(), b.float(), terms=3, **kw), ref, tol)
                three_worst = max(three_worst, r3)
                assert r3 <= 1.0, (c.id, T, with_alpha, "three-term", r3)
                got = {t: _worst(E.conv(a32, w.float(), b.float(), terms=t, **kw), ref, tol) for t in ("no_wh_xlo", "no_wlo_xhi")}
                got["padding+1"] = _worst(tconv_poly(a64, w, b, c.s, c.p, c.op, shift=1), ref, tol)
                got["padding-1"] = _worst(tconv_poly(a64, w, b, c.s, c.p, c.op, shift=-1), ref, tol)
                got["taps swapped"] = _worst(tconv_poly(a64, w, b, c.s, c.p, c.op, swap=True), ref, tol)
                if (cg.tconv_out_len(T, c.s, c.p, c.op) - 1 + c.p) // c.s == T:          # some output sample lies in column q = T
                    got["column T clamped"] = _worst(tconv_poly(a64, w, b, c.s, c.p, c.op, clamp=True), ref, tol)
                if c.op:
                    got["output_padding at bias"] = _worst(tconv_poly(a64, w, b, c.s, c.p, c.op, op_bias=True), ref, tol)
                for name, r in got.items():
                    assert r > 1.0, (c.id, T, with_alpha, name, r)
                    mutants[name] = min(mutants.get(name, r), r)
    print(f"\ntconv, {n} (case, T, alpha) points: three-term worst error / bound {three_worst:.3f}; smallest mutant error / bound:",
          {k: round(v, 2) for k, v in mutants.items()})
    assert set(mutants) == {"no_wh_xlo", "no_wlo_xhi", "padding+1", "padding-1", "taps swapped", "column T clamped", "output_padding at bias"}


def test_emulation_output_padding_is_the_transposed_convs():
    g = torch.Generator().manual_seed(5)
    x, w, b = torch.randn(2, 8, 9, generator=g), torch.randn(8, 5, 6, generator=g), torch.randn(5, generator=g)
    for op in (0, 1, 2):
        y = E.conv(x, w, b, transposed=True, stride=3, padding=2, output_padding=op)
        ref = F.conv_transpose1d(x.double(), w.double(), b.double(), stride=3, padding=2, output_padding=op)
        assert y.shape == ref.shape and ref.shape[2] == cg.tconv_out_len(9, 3, 2, op)
        assert float((y.double() - ref).abs().max()) <= 1e-5
    assert torch.equal(E.conv(x, w, b, transposed=True, stride=3, padding=2), E.conv(x, w, b, transposed=True, stride=3, padding=2, output_padding=0))


def test_sconv_bound_separates_right_from_wrong():
    n, right_worst, mutants = 0, 0.0, {}
    for c in cg.SCONV:
        P = cg.tensors(c)
        w, b = P["w"], P["b"]
        for T in c.Ts:
            x = cg.inputs(c, T)
            Tout = c.out_len(T)
            for with_alpha in (True, False):
                alpha = P["alpha"] if with_alpha else None
                ref, tol = cg.reference(c, P, x, with_alpha)
                assert ref.shape[2] == Tout
                n += 1
                a32 = snake32(x, alpha) if with_alpha else x
                r = _worst(F.conv1d(a32, w.float(), b.float(), stride=c.s, padding=c.p), ref, tol)
                right_worst = max(right_worst, r)
                assert r <= 1.0, (c.id, T, with_alpha, "fp32 restatement", r)
                a64 = C.snake(x.double(), alpha) if with_alpha else x.double()
                got = {"padding+1": _worst(F.conv1d(F.pad(a64, (c.p + 1, c.p + 1)), w, b, stride=c.s)[:, :, :Tout], ref, tol)}
                if c.p:
                    got["padding-1"] = _worst(F.conv1d(F.pad(a64, (c.p - 1, c.p + c.s)), w, b, stride=c.s)[:, :, :Tout], ref, tol)
                    got["padding clamped"] = _worst(F.conv1d(F.pad(a64, (c.p, c.p), mode="replicate"), w, b, stride=c.s), ref, tol)
                for name, v in got.items():
                    assert v > 1.0, (c.id, T, with_alpha, name, v)
                    mutants[name] = min(mutants.get(name, v), v)
    print(f"\nsconv, {n} (case, T, alpha) points: fp32 restatement worst error / bound {right_worst:.3f}; smallest mutant error / bound:",
          {k: round(v, 2) for k, v in mutants.items()})
    assert set(mutants) == {"padding+1", "padding-1", "padding clamped"}


def _unit(case, P, x, dil=None, clamp=False):
    """the unit in x's dtype with conv7 at dilation `dil` (default: the case's) and, for clamp, its padding filled with the clamped activation"""
    d = case.d if dil is None else dil
    if case.kind == "codec":
        act1, act2 = (lambda v: C.snake(v, P["0.alpha"])), (lambda v: C.snake(v, P["2.alpha"]))
        w1, b1, w2, b2 = P["1.weight"], P["1.bias"], P["3.weight"], P["3.bias"]
    else:
        act1 = lambda v: FR.activation1d(v, P["block.0.act.alpha"], P.get("block.0.act.beta"))
        act2 = lambda v: FR.activation1d(v, P["block.2.act.alpha"], P.get("block.2.act.beta"))
        w1, b1, w2, b2 = P["block.1.weight"], P["block.1.bias"], P["block.3.weight"], P["block.3.bias"]
    s1 = act1(x)
    if clamp:
        v = F.conv1d(F.pad(s1, (3 * d, 3 * d), mode="replicate"), w1, b1, dilation=d)
    else:
        v = F.conv1d(s1, w1, b1, dilation=d, padding=3 * d)
    return x + F.conv1d(act2(v), w2, b2)


def test_unit_bounds_separate_right_from_wrong():
    for kind in ("codec", "aa"):
        n, right_worst, mutants = 0, 0.0, {}
        for c in cg.UNITS:
            if c.kind != kind or not c.fused:                # (the unfused entries repeat the fused ones' geometry)
                continue
            P = cg.tensors(c)
            P32 = {k: v.float() for k, v in P.items()}
            for T in c.Ts:
                x = cg.inputs(c, T)
                ref, tol = cg.reference(c, P, x)
                n += 1
                assert float((_unit(c, P, x.double()) - ref).abs().max()) <= 1e-12
                r = _worst(_unit(c, P32, x), ref, tol)
                right_worst = max(right_worst, r)
                assert r <= 1.0, (c.id, T, "fp32 restatement", r)
                got = {"padding clamped": _worst(_unit(c, P, x.double(), clamp=True), ref, tol)}
                if T > c.d:                                # else only the centre tap of conv7 reads the item at either dilation
                    got["dilation+1"] = _worst(_unit(c, P, x.double(), dil=c.d + 1), ref, tol)
                if T > c.d and c.d > 1:
                    got["dilation-1"] = _worst(_unit(c, P, x.double(), dil=c.d - 1), ref, tol)
                for name, v in got.items():
                    assert v > 1.0, (c.id, T, name, v)
                    mutants[name] = min(mutants.get(name, v), v)
        print(f"\n{kind} unit, {n} (case, T) points: fp32 restatement worst error / bound {right_worst:.3f}; smallest mutant error / bound:",
              {k: round(v, 2) for k, v in mutants.items()})
        assert set(mutants) == {"padding clamped", "dilation+1", "dilation-1"}
