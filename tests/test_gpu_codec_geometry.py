"""amp_tconv_* / amp_sconv_* / amp_codec_unit_* / amp_aa_unit_* over their whole documented geometry (tests/codec_geometry.py), through the C
ABI, against fp64.

The codec recipes only ever make these handles at padding ceil(stride / 2), output_padding stride % 2 and dilations 1 / 3 / 9; the header
documents any padding >= 0, output_padding < stride and <= padding, any cout, any stride, dilations up to 9 fused and beyond unfused.  Here
  tconv_fused    strides 2..8 x paddings {0, 1, ceil(s / 2), s - 1, s, s + 1, 2 s} x output_paddings {0, 1, min(p, s - 1)}, rows M = cout s
                 below 32 / odd / no multiple of 32, cin 96 and 384: every store branch of tconv_store4 per stride class, q_first > 0, the
                 4 / 2 / 1 row-block groups (tests/test_codec_geometry_ref.py asserts that the table reaches them);
  tconv_unfused  the same geometries on snake -> ConvTranspose1d, plus strides 1 and 9 and cin = 48, which are not built for fusion;
  sconv          strides 1..8 x paddings {0, 1, ceil(s / 2), s, 2 s - 1} x cin {32, 24}, T no multiple of the stride, the shortest valid T,
                 and (T_out + 1) s on either side of the repack kernel's 256-thread block;
  units          every dilation 1..9 fused and on the four launches, dilation 10 (must fall back), C = 192 / 128, lengths around the tile
                 (64 / 54 columns) and the 3 d halo, SnakeBeta and plain Snake.
Every call goes through the helpers of tests/hip_helpers.py: y inside a NaN-filled buffer whose sentinels must stay untouched, every element
finite, the shape against amp_*_out_len and the closed form, every element against fp64 under the EXISTING per-element bounds
(dac_ref.tconv_bound, codec_ref.sconv_bound / unit_bound, facodec_ref.unit_bound; error / bound <= 1; no new tolerance), and the launches of
every call from AMP_LAUNCH_MANIFEST.  The unfused routes run under both precisions and calibrate each bound at each geometry.  The refusal
cases must raise the listed status with a message naming the argument, before any launch.  Once per group: item b of a B = 3 call equals
the B = 1 call bit for bit, and the range flag is clean at the end.

One child process per (group, precision), the runner of tests/test_gpu_recipe_shapes.py: results after every case, only a failed assertion
moves on to the next case, anything else ends the child and the remaining cases are reported as not run."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import codec_geometry as cg  # noqa: E402
from recipe_shapes import Op  # noqa: E402
from test_gpu_recipe_shapes import _child, _kernel_id, _run_group  # noqa: E402

DEV = "cuda:0"


def _manifest_lines():
    man = os.environ["AMP_LAUNCH_MANIFEST"]
    return open(man).read().splitlines() if os.path.exists(man) else []


# ------------------------------------------------------------------------------------------------------------------------------
# what each call must launch: [(kernel id, first words of the manifest's description)]
# ------------------------------------------------------------------------------------------------------------------------------
def _convt(case):
    return Op(case.cin, case.cout, 2 * case.s, 1, case.s, case.p)


def tconv_fused_expected(case, precision):
    return bool(case.fused and case.built and precision == "f16x3")


def tconv_launches(case, T, precision, with_alpha, batch=cg.B):
    if tconv_fused_expected(case, precision):
        return [("tconv_f16x3_kernel", "snake + ConvT")]
    return ([("snake_kernel", "Snake")] if with_alpha else []) + [(_convt(case).form(batch, T, precision)[0], "ConvT")]


def sconv_launches(case, T, precision, batch=cg.B):
    U = case.out_len(T) + 1
    return [("sconv_repack_kernel", "snake + space-to-depth"), (Op(case.cin * case.s, case.cout, 2, 1, 0, 0).form(batch, U, precision)[0], "conv")]


def unit_launches(case, T, fused, precision, batch=cg.B):
    if fused:
        return [(f"{case.kind}_unit_f16x3_kernel", "")]
    act = ("snake_kernel", "Snake") if case.kind == "codec" else ("act1d_kernel", "Activation1d")
    c1, c2 = Op(case.C, case.C, 7, case.d), Op(case.C, case.C, 1, 1)
    return [act, (c1.form(batch, T, precision)[0], "conv"), act, (c2.form(batch, T, precision)[0], "conv")]


def _check_launches(what, lines, expected):
    got = [(_kernel_id(l), l.split("\t")[-1]) for l in lines]
    ok = len(got) == len(expected) and all(g[0] == e[0] and g[1].startswith(e[1]) for g, e in zip(got, expected))
    assert ok, f"{what}: launched {got}, expected {expected}"


def _ratio(what, y, ref, tol, Tout_lib, Tout_closed):
    assert tuple(y.shape) == tuple(ref.shape) and y.shape[2] == Tout_lib == Tout_closed, (what, tuple(y.shape), tuple(ref.shape), Tout_lib, Tout_closed)
    assert torch.isfinite(y).all(), what
    frac = ((y.double() - ref).abs() / tol)
    r = float(frac.max())
    if not r <= 1.0:
        at = [int(v) for v in (frac == frac.max()).nonzero()[0]]
        raise AssertionError(f"{what}: |hip - fp64| / bound = {r:.3f} > 1 at (item, row, t) = {at} of {tuple(y.shape)}: the bound's derivation "
                             "or the kernel is wrong at this geometry")
    return r


# ------------------------------------------------------------------------------------------------------------------------------
# child side: one case = one handle, with / without the activation, every length
# ------------------------------------------------------------------------------------------------------------------------------
def run_tconv(case, precision):
    from hip_helpers import tconv_forward

    P = cg.tensors(case)
    xs = [cg.inputs(case, T) for T in case.Ts]
    worst = 0.0
    for with_alpha in (True, False):
        info = {}
        n0 = len(_manifest_lines())
        ys = tconv_forward(P["w"], P["b"], xs, P["alpha"] if with_alpha else None, stride=case.s, padding=case.p, output_padding=case.op,
                           fusion=1 if case.fused else 0, info=info)
        lines = _manifest_lines()[n0:]
        assert info["fused"] == int(tconv_fused_expected(case, precision)), f"{case.id} [{precision}]: amp_tconv_fused() = {info['fused']}"
        expected = [e for T in case.Ts for e in tconv_launches(case, T, precision, with_alpha)]
        _check_launches(f"{case.id} alpha={with_alpha}", lines, expected)
        for T, x, y in zip(case.Ts, xs, ys):
            ref, tol = cg.reference(case, P, x, with_alpha)
            worst = max(worst, _ratio(f"{case.id} alpha={with_alpha} B={cg.B} T={T} [{precision}]", y, ref, tol, info["out_len"][T], case.out_len(T)))
    return worst


def run_sconv(case, precision):
    from hip_helpers import sconv_forward

    P = cg.tensors(case)
    xs = [cg.inputs(case, T) for T in case.Ts]
    worst = 0.0
    for with_alpha in (True, False):
        info = {}
        n0 = len(_manifest_lines())
        ys = sconv_forward(P["w"], P["b"], xs, P["alpha"] if with_alpha else None, stride=case.s, padding=case.p, info=info)
        lines = _manifest_lines()[n0:]
        _check_launches(f"{case.id} alpha={with_alpha}", lines, [e for T in case.Ts for e in sconv_launches(case, T, precision)])
        for T, x, y in zip(case.Ts, xs, ys):
            ref, tol = cg.reference(case, P, x, with_alpha)
            worst = max(worst, _ratio(f"{case.id} alpha={with_alpha} B={cg.B} T={T} [{precision}]", y, ref, tol, info["out_len"][T], case.out_len(T)))
    return worst


def _unit_forward(case, P, xs, fusion, info):
    from hip_helpers import aa_unit_forward, codec_unit_forward

    if case.kind == "codec":
        from codec_ref import folded

        return codec_unit_forward(P["0.alpha"], folded(P, "1."), P["1.bias"], P["2.alpha"], folded(P, "3."), P["3.bias"], xs, dilation=case.d,
                                  fusion=fusion, info=info)
    import facodec_ref as FR
    from codec_ref import folded

    f = FR.FILT.reshape(-1)
    return aa_unit_forward(P["block.0.act.alpha"], P.get("block.0.act.beta"), folded(P, "block.1."), P["block.1.bias"],
                           P["block.2.act.alpha"], P.get("block.2.act.beta"), folded(P, "block.3."), P["block.3.bias"], f, f, xs,
                           dilation=case.d, logscale=True, fusion=fusion, info=info)


def unit_fused_expected(case, precision):
    return bool(case.fused and case.built and precision == "f16x3")


def run_unit(case, precision):
    P = cg.tensors(case)
    xs = [cg.inputs(case, T) for T in case.Ts]
    fused = unit_fused_expected(case, precision)
    info = {}
    n0 = len(_manifest_lines())
    ys = _unit_forward(case, P, xs, 1 if case.fused else 0, info)
    lines = _manifest_lines()[n0:]
    assert info["fused"] == int(fused), f"{case.id} [{precision}]: amp_{case.kind}_unit_fused() = {info['fused']}"
    _check_launches(case.id, lines, [e for T in case.Ts for e in unit_launches(case, T, fused, precision)])
    worst = 0.0
    for T, x, y in zip(case.Ts, xs, ys):
        ref, tol = cg.reference(case, P, x)
        worst = max(worst, _ratio(f"{case.id} B={cg.B} T={T} [{precision}]", y, ref, tol, T, T))
    return worst


def run_case(case, precision):
    return {"tconv": run_tconv, "sconv": run_sconv}.get(case.kind, run_unit)(case, precision)


def run_refusal(case):
    from amphion_amd._lib import AmpError
    from hip_helpers import sconv_forward, tconv_forward

    stage, status, word = case.refuse
    n0 = len(_manifest_lines())
    err = None
    try:
        if case.kind == "tconv":
            g = torch.Generator().manual_seed(1)
            tconv_forward(torch.randn(case.cin, case.cout, 2 * case.s, generator=g), torch.zeros(case.cout), cg.inputs(case, case.Ts[0]), None,
                          stride=case.s, padding=case.p, output_padding=case.op, fusion=1 if case.fused else 0)
        elif case.kind == "sconv":
            g = torch.Generator().manual_seed(1)
            sconv_forward(torch.randn(case.cout, case.cin, 2 * case.s, generator=g), torch.zeros(case.cout), cg.inputs(case, case.Ts[0]), None,
                          stride=case.s, padding=case.p)
        else:
            _unit_forward(case, cg.tensors(case), [cg.inputs(case, case.Ts[0])], 1, {})
    except AmpError as e:
        err = e
    assert err is not None, f"{case.id}: ran; it must be refused at {stage} with status {status}"
    assert err.status == status and word in str(err), f"{case.id}: refused with {err} (expected status {status}, a message naming '{word}')"
    assert len(_manifest_lines()) == n0, f"{case.id}: a kernel was launched before the refusal"
    return None


# the case of each group whose B = 3 call must hold the B = 1 call of item 1 bit for bit
BATCH_CASE = {"tconv_fused": lambda c: (c.s, c.p, c.op, c.cout) == (3, 4, 2, 16), "tconv_unfused": lambda c: (c.s, c.p, c.op, c.cout) == (3, 4, 2, 16),
              "sconv": lambda c: (c.s, c.p, c.cin) == (3, 2, 32), "units": lambda c: (c.kind, c.C, c.d, c.fused) == ("codec", 32, 2, True)}
BATCH_T = 130


def run_batch_independence(group, precision):
    from hip_helpers import sconv_forward, tconv_forward

    case = next(c for c in cg.GROUPS[group] if BATCH_CASE[group](c))
    P = cg.tensors(case)
    x3 = cg.inputs(case, BATCH_T, batch=3)
    xs = [x3, x3[1:2].contiguous()]
    if case.kind == "tconv":
        y3, y1 = tconv_forward(P["w"], P["b"], xs, P["alpha"], stride=case.s, padding=case.p, output_padding=case.op, fusion=1 if case.fused else 0)
    elif case.kind == "sconv":
        y3, y1 = sconv_forward(P["w"], P["b"], xs, P["alpha"], stride=case.s, padding=case.p)
    else:
        y3, y1 = _unit_forward(case, P, xs, 1, {})
    assert torch.equal(y3[1], y1[0]), f"{case.id} [{precision}]: item 1 of a B = 3 call differs from the B = 1 call"
    if group == "units" and precision == "f16x3":               # the anti-aliased unit as well
        aa = next(c for c in cg.UNITS if (c.kind, c.C, c.d, c.beta, c.fused) == ("aa", 32, 2, True, True))
        Pa = cg.tensors(aa)
        xa = cg.inputs(aa, BATCH_T, batch=3)
        y3, y1 = _unit_forward(aa, Pa, [xa, xa[1:2].contiguous()], 1, {})
        assert torch.equal(y3[1], y1[0]), f"{aa.id} [{precision}]: item 1 of a B = 3 call differs from the B = 1 call"
    return None


def run_range_check():
    from amphion_amd import _lib

    _lib.range_check(DEV)
    return None


def _case_kernels(case, precision):
    """the kernel ids a case's launches must name, over both activation settings / both routes and every length"""
    if case.kind == "tconv":
        return {e[0] for T in case.Ts for a in (True, False) for e in tconv_launches(case, T, precision, a)}
    if case.kind == "sconv":
        return {e[0] for T in case.Ts for e in sconv_launches(case, T, precision)}
    return {e[0] for T in case.Ts for e in unit_launches(case, T, unit_fused_expected(case, precision), precision)}


def group_cases(group, precision):
    """[(case id, callable returning error / bound or None, the kernel ids its launches must name)] -- the runner's table form"""
    cases = cg.GROUPS[group]
    if group == "tconv_fused" and precision == "f32":
        # the fused kernel is not built under f32: one case shows that the handle says so and runs the two launches
        cases = [c for c in cases if (c.s, c.p, c.op, c.cout) == (4, 2, 0, 16)]
    if group == "units" and precision == "f32":
        # every unit is the four launches under f32: the handles asked for them, dilation 10, and one built geometry of each unit asked for the
        # fused launch, which must say that it fell back
        cases = [c for c in cases if not c.fused or not c.built or (c.C, c.d, c.beta) == (32, 1, True)]
    out = [(c.id, (lambda c=c: run_case(c, precision)), _case_kernels(c, precision)) for c in cases]
    out += [(c.id + "/refused", (lambda c=c: run_refusal(c)), set()) for c in cg.refusals(group)]
    if not (group == "tconv_fused" and precision == "f32"):
        bc = next(c for c in cg.GROUPS[group] if BATCH_CASE[group](c))
        if bc.kind == "tconv":
            ks = {e[0] for B in (3, 1) for e in tconv_launches(bc, BATCH_T, precision, True, B)}
        elif bc.kind == "sconv":
            ks = {e[0] for B in (3, 1) for e in sconv_launches(bc, BATCH_T, precision, B)}
        else:
            ks = {e[0] for B in (3, 1) for e in unit_launches(bc, BATCH_T, unit_fused_expected(bc, precision), precision, B)}
            if precision == "f16x3":
                ks |= {"aa_unit_f16x3_kernel"}
        out.append((f"{group}/batch_independence", (lambda: run_batch_independence(group, precision)), ks))
    out.append((f"{group}/range_check", run_range_check, set()))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("group", ["tconv_fused", "tconv_unfused", "sconv", "units"])
def test_codec_geometry(group, conv_precision, tmp_path):
    _run_group(group, conv_precision, tmp_path, cases_fn=group_cases, script=__file__, title="codec geometry", bound=1.0)


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2], sys.argv[3], cases_fn=group_cases)
