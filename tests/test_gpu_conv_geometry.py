"""amp_conv_create / amp_conv_forward over their whole geometry (tests/conv_geometry.py), through the C ABI, against fp64.

The recipes only ever run ConvTranspose1d with padding (k - stride) // 2, stride in {2, 4, 8} and k a multiple of the stride, and Conv1d with
'same' padding and k in {1, 3, 5, 7, 11}; the header documents any such geometry.  Here every stride 1..16, k below / equal to / no multiple of
the stride, every padding class, the zero-padded tap counts, paddings other than 'same', the 128-column halo limit, T from 1 to several
ragged tiles and the two per-conv options run at two grids:
  small  every output sample against the full fp64 F.conv1d / F.conv_transpose1d (tests/conv_window_ref.py::conv_full);
  large  ConvTranspose1d whose GEMM rows are a multiple of 256, sized so that the launch policy takes the row-blocked kernel: the windowed
         fp64 reference on probe rows x (both row ends, tile seams with and without the padding shift, a random spot, and the whole last
         2 * stride + 8 columns) of items 0 and B - 1, plus isfinite over the whole NaN-pre-filled output (a dropped store is a NaN).
Both arithmetics meet |hip - fp64| / cond <= BOUND, the bound tests/test_recipe_numerics.py derives.  Which kernel ran, that it ran once and
that the manifest labels it by the handle's `transposed` are asserted from AMP_LAUNCH_MANIFEST.  The refusal cases must raise the listed
status with a message that names the argument, before any launch.

One child process per (grid, precision), the runner of tests/test_gpu_recipe_shapes.py: results after every case, only a failed assertion
moves on to the next case, anything else ends the child and the remaining cases are reported as not run."""
import ctypes
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import conv_geometry as cg  # noqa: E402
from test_gpu_recipe_shapes import BOUND, _child, _noise, _run_group  # noqa: E402


def _manifest_lines():
    man = os.environ["AMP_LAUNCH_MANIFEST"]
    return open(man).read().splitlines() if os.path.exists(man) else []


def _tensors(case):
    op = case.op
    B, T = case.shape()
    g = torch.Generator().manual_seed(op.cin * 131 + op.cout * 7 + op.k * 3 + op.d + op.u + 17 * op.padding)
    if op.u:
        w = torch.randn(op.cin, op.cout, op.k, generator=g) * max(1.0, op.cin * op.k / op.u) ** -0.5
    else:
        w = torch.randn(op.cout, op.cin, op.k, generator=g) * (op.cin * op.k) ** -0.5
    b = torch.randn(op.cout, generator=g) * 0.1 if case.bias else None
    x = _noise(B * op.cin * T, 1).view(B, op.cin, T)
    Tout = op.out_len(T)
    res = _noise(B * op.cout * Tout, 2).view(B, op.cout, Tout) if case.res and Tout > 0 else None
    kw = dict(transposed=op.transposed, stride=op.u or 1, dilation=op.d, padding=op.padding, slope_in=case.slope_in, slope_out=case.slope_out)
    return w, b, x, res, kw


def _merge(windows, Tout):
    out = []
    for t0, t1 in sorted((max(0, a), min(Tout, b)) for a, b in windows):
        if t1 <= t0:
            continue
        if out and t0 <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], t1))
        else:
            out.append((t0, t1))
    return out


def run_case(case, precision):
    """one geometry: returns the largest error ratio; raises AssertionError on a wrong shape, a NaN, a wrong label or a ratio above BOUND"""
    from conv_window_ref import conv_full, conv_window, error_ratio, pick, probe_rows, probe_windows
    from hip_helpers import conv_forward

    op = case.op
    B, T = case.shape()
    Tout = op.out_len(T)
    w, b, x, res, kw = _tensors(case)
    n0 = len(_manifest_lines())
    y = conv_forward(w, b, x, res=res, options=case.options, **kw)
    launches = [l.split("\t")[-1] for l in _manifest_lines()[n0:]]
    want = "ConvT" if op.transposed else "conv"
    assert len(launches) == 1 and launches[0].split(" ")[0] == want, f"{case.id}: launches {launches}, expected one '{want} ...'"
    assert y.shape == (B, op.cout, Tout), (case.id, tuple(y.shape), Tout)
    bad = (~torch.isfinite(y)).nonzero()
    assert bad.numel() == 0, (f"{case.id}: {bad.shape[0]} of {y.numel()} outputs were not written or are not finite; columns "
                              f"{sorted(set(bad[:, 2].tolist()))[:12]} of T_out = {Tout}")
    opts = dict(case.options)
    if case.grid == "small":
        ref, cond = conv_full(x, w, b, res=res, reflect=bool(opts.get(cg.OPT_PAD_REFLECT)), tanh=bool(opts.get(cg.OPT_TANH)), **kw)
        r = error_ratio(y, ref, cond)
    else:
        _, rows_per_group, tile = op.form(B, T, precision)
        tile = tile or 128
        rows = probe_rows(op.cout, rows_per_group, up=op.u or 1, seed=op.cin + op.k)
        wins = probe_windows(Tout, tile, seed=op.cout + op.k)
        # a transposed conv's tiles start at q0 * stride - padding: the same seams, shifted by the padding
        wins += [(t0 - op.padding, t1 - op.padding) for t0, t1 in wins]
        wins += [(Tout - (2 * (op.u or 1) + 8), Tout), (0, 2 * (op.u or 1) + 8)]
        wins = _merge(wins, Tout)
        items = sorted({0, B - 1})
        ref, cond, cols = conv_window(x, w, b, rows=rows, windows=wins, items=items, res=res, **kw)
        r = error_ratio(pick(y, items, rows, cols), ref, cond)
    assert r <= BOUND, f"{case.id} B={B} T={T}: |hip - fp64| / cond = {r:.3e} > {BOUND:g}"
    return r


def _ragged_forward(case):
    """amp_conv_forward_ragged with a lens vector on this geometry (the refusal cases: the call must not launch)"""
    from amphion_amd import _lib

    L = _lib.lib()
    op = case.op
    w, b, x, _, kw = _tensors(case)
    h = ctypes.c_void_p()
    w = w.contiguous()
    _lib.check(L.amp_conv_create(int(op.transposed), op.cin, op.cout, op.k, op.u or 1, op.d, op.padding, ctypes.c_void_p(w.data_ptr()),
                                 ctypes.c_void_p(b.contiguous().data_ptr()), ctypes.byref(h)))
    try:
        xd = x.contiguous().cuda()
        B, _, T = xd.shape
        lens = torch.full((B,), T, dtype=torch.int32, device="cuda")
        y = torch.full((B, op.cout, max(1, op.out_len(T))), float("nan"), device="cuda")
        _lib.check(L.amp_conv_forward_ragged(h, ctypes.c_void_p(xd.data_ptr()), 0, B, T, ctypes.c_void_p(lens.data_ptr()), 1.0, None, 1.0,
                                             ctypes.c_void_p(y.data_ptr()), _lib.current_stream_ptr(xd.device)))
        torch.cuda.synchronize()
    finally:
        L.amp_conv_destroy(h)


def run_refusal(case):
    from amphion_amd._lib import AmpError
    from hip_helpers import conv_forward

    stage, status, word = case.refuse
    n0 = len(_manifest_lines())
    err = None
    try:
        if stage == "ragged":
            _ragged_forward(case)
        else:
            w, b, x, res, kw = _tensors(case)
            conv_forward(w, b, x, res=res, options=case.options, **kw)
    except AmpError as e:
        err = e
    assert err is not None, f"{case.id}: ran; it must be refused at {stage} with status {status}"
    assert err.status == status and word in str(err), f"{case.id}: refused with {err} (expected status {status}, a message naming '{word}')"
    assert len(_manifest_lines()) == n0, f"{case.id}: a kernel was launched before the refusal"
    return None


def group_cases(group, precision):
    """[(case id, callable returning the error ratio or None, the kernel ids its launches must name)] -- the runner's table form"""
    out = []
    for case in cg.all_cases():
        if case.refuse is not None:
            if group == "small":
                out.append((case.id + "/refused", (lambda case=case: run_refusal(case)), set()))
        elif case.grid == group:
            B, T = case.shape()
            out.append((case.id, (lambda case=case: run_case(case, precision)), {case.op.form(B, T, precision)[0]}))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("group", ["small", "large"])
def test_conv_geometry(group, conv_precision, tmp_path):
    _run_group(group, conv_precision, tmp_path, cases_fn=group_cases, script=__file__, title="conv geometry")


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2], sys.argv[3], cases_fn=group_cases)
