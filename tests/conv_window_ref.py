"""fp64 reference of one Conv1d / ConvTranspose1d on chosen output rows x column windows, and the probe sets for it.

A full fp64 reference of a batch-grid conv is out of reach on the host (C = 768, k = 11 over a grid that reaches the row-blocked
kernel is more than 1e11 MAC).  Every output sample depends only on its own receptive field, so the reference is computed on the
input slice that reaches each window, for the chosen output channels only.  The arithmetic follows tests/hip_helpers.conv_forward
(include/amphion_hip.h, amp_conv_forward):

    y = lrelu(conv(lrelu(x, slope_in), w) + b + res, slope_out)

`cond` is the same sum over absolute values, |conv|(|lrelu(x)|, |w|) + |b| + |res|: the size of the terms that make up each output.
The error measure |hip - ref| / cond is then relative to each output's own condition, so one bound holds whatever the cancellation.
"""
import random

import torch
import torch.nn.functional as F


def _lrelu(x, slope):
    return x if slope == 1.0 else torch.where(x >= 0, x, x * slope)


def out_len(T, k, *, transposed=False, stride=1, dilation=1, padding=0):
    if transposed:
        return (T - 1) * stride - 2 * padding + k
    return T + 2 * padding - dilation * (k - 1)


def conv_window(x, w, b=None, *, rows, windows, items=None, transposed=False, stride=1, dilation=1, padding=0, slope_in=1.0,
                res=None, slope_out=1.0):
    """fp64 output and condition of one conv at y[items][:, rows][:, :, cols].

    x [B, Cin, T], w [Cout, Cin, k] (transposed: [Cin, Cout, k]), b [Cout] or None, res [B, Cout, Tout] or None.
    rows: output channels; windows: (t0, t1) column ranges of the output; items: batch items (default all).
    Returns (ref, cond, cols): [len(items), len(rows), len(cols)] float64 each and the LongTensor of output columns."""
    B, _, T = x.shape
    k = w.shape[2]
    items = list(range(B)) if items is None else list(items)
    rows = torch.as_tensor(list(rows), dtype=torch.long)
    Tout = out_len(T, k, transposed=transposed, stride=stride, dilation=dilation, padding=padding)
    xs = _lrelu(x[items].double(), slope_in)
    wr = (w[:, rows] if transposed else w[rows]).double()
    refs, conds, cols = [], [], []
    for t0, t1 in windows:
        t0, t1 = max(0, t0), min(Tout, t1)
        if t1 <= t0:
            continue
        if not transposed:
            # y[t] = sum_j w[:, :, j] . x[t - padding + j * dilation]: the window reads x[t0 - padding, t1 - 1 - padding + (k - 1) d]
            i0, i1 = t0 - padding, t1 - 1 - padding + (k - 1) * dilation
            lo, hi = max(0, i0), min(T - 1, i1)
            sl = torch.zeros(len(items), x.shape[1], i1 - i0 + 1, dtype=torch.float64)
            if hi >= lo:
                sl[:, :, lo - i0: hi - i0 + 1] = xs[:, :, lo: hi + 1]
            r = F.conv1d(sl, wr, dilation=dilation)
            c = F.conv1d(sl.abs(), wr.abs(), dilation=dilation)
        else:
            # y[t] = sum over i * stride - padding + j = t of x[i] w[i, :, j]: inputs i in [ceil((t0 + p - k + 1) / s), floor((t1 - 1 + p) / s)]
            i0 = max(0, -((k - 1 - t0 - padding) // stride))
            i1 = min(T - 1, (t1 - 1 + padding) // stride)
            r = torch.zeros(len(items), len(rows), t1 - t0, dtype=torch.float64)
            c = torch.zeros_like(r)
            if i1 >= i0:                                      # else no input reaches the window (k < stride): bias + residual only
                sl = xs[:, :, i0: i1 + 1]
                base = i0 * stride - padding                  # global column of the slice's local output 0
                rs = F.conv_transpose1d(sl, wr, stride=stride)
                cs = F.conv_transpose1d(sl.abs(), wr.abs(), stride=stride)
                # the slice's outputs cover [base, base + len): with k < stride that may start after t0 or end before t1
                g0, g1 = max(t0, base), min(t1, base + rs.shape[-1])
                if g1 > g0:
                    r[:, :, g0 - t0: g1 - t0] = rs[:, :, g0 - base: g1 - base]
                    c[:, :, g0 - t0: g1 - t0] = cs[:, :, g0 - base: g1 - base]
        refs.append(r[:, :, : t1 - t0])
        conds.append(c[:, :, : t1 - t0])
        cols.append(torch.arange(t0, t1))
    ref, cond, cols = torch.cat(refs, -1), torch.cat(conds, -1), torch.cat(cols)
    if b is not None:
        bb = b.double()[rows].view(1, -1, 1)
        ref, cond = ref + bb, cond + bb.abs()
    if res is not None:
        rr = res[items][:, rows][:, :, cols].double()
        ref, cond = ref + rr, cond + rr.abs()
    return _lrelu(ref, slope_out), cond, cols


def conv_full(x, w, b=None, *, transposed=False, stride=1, dilation=1, padding=0, slope_in=1.0, res=None, slope_out=1.0, reflect=False,
              tanh=False):
    """fp64 (ref, cond) of the WHOLE output, straight from torch's conv: what conv_window is pinned to (tests/test_conv_geometry_ref.py)
    and the reference of the small-grid geometry cases.  reflect: the padding mirrors (nn.ReflectionPad1d + unpadded conv); tanh: on the
    output (cond stays that of the sum: |tanh(a) - tanh(b)| <= |a - b|)."""
    xa = _lrelu(x.double(), slope_in)
    wd = w.double()
    if transposed:
        r = F.conv_transpose1d(xa, wd, stride=stride, padding=padding)
        c = F.conv_transpose1d(xa.abs(), wd.abs(), stride=stride, padding=padding)
    else:
        if reflect:
            xa, padding = F.pad(xa, (padding, padding), mode="reflect"), 0
        r = F.conv1d(xa, wd, dilation=dilation, padding=padding)
        c = F.conv1d(xa.abs(), wd.abs(), dilation=dilation, padding=padding)
    if b is not None:
        r, c = r + b.double().view(1, -1, 1), c + b.double().abs().view(1, -1, 1)
    if res is not None:
        r, c = r + res.double(), c + res.double().abs()
    r = _lrelu(r, slope_out)
    return (torch.tanh(r) if tanh else r), c


def pick(y, items, rows, cols):
    """y[items][:, rows][:, :, cols] of a full output"""
    return y[list(items)][:, torch.as_tensor(list(rows))][:, :, cols]


def error_ratio(y, ref, cond):
    """largest |y - ref| / cond (fp64): the error of each output relative to the size of its terms"""
    return ((y.double() - ref).abs() / cond.clamp_min(1e-300)).max().item()


def probe_rows(cout, group_rows, *, up=1, n_random=3, seed=0):
    """output channels to probe: the first and last row of each GEMM row group that holds real rows, the last real row next to the
    padding, and a few random ones.  GEMM rows are polyphase for a transposed conv (row m = channel m // up, phase m % up)."""
    M = cout * up
    rows = set()
    for g0 in range(0, M, group_rows):
        rows.add(g0 // up)
        rows.add((min(g0 + group_rows, M) - 1) // up)
    rows.add(cout - 1)
    rng = random.Random(seed)
    rows.update(rng.randrange(cout) for _ in range(n_random))
    return sorted(r for r in rows if 0 <= r < cout)


def probe_windows(Tout, tile, *, width=8, n_seams=3, seed=0):
    """column windows: the sequence start and end, tile seams (multiples of the launch's tile width `tile`, first, middle and last)
    and one random interior spot"""
    ws = [(0, width), (Tout - width, Tout)]
    seams = [s for s in range(tile, Tout, tile)]
    if seams:
        pick_s = sorted({seams[0], seams[len(seams) // 2], seams[-1]})[:n_seams]
        ws += [(s - width // 2, s + width // 2) for s in pick_s]
    rng = random.Random(seed)
    if Tout > 4 * width:
        t = rng.randrange(width, Tout - 2 * width)
        ws.append((t, t + width))
    # merge overlaps (the reference would otherwise report a column twice)
    out = []
    for t0, t1 in sorted((max(0, a), min(Tout, b)) for a, b in ws):
        if out and t0 <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], t1))
        else:
            out.append((t0, t1))
    return out
