"""amp_evq_* / amp_lstm_* / amp_dsconv_* / amp_elu_pad / amp_gelu over their whole documented geometry, through the C ABI, against fp64
(tests/tokenizer_geometry.py holds the tables; tests/test_tokenizer_geometry_ref.py shows on the CPU what they reach and that the rules below
catch a kernel with one slip).  The model tests of tests/test_gpu_speechtokenizer.py and tests/test_gpu_tokenizers.py sit at D and H multiples of
4, K of 5 / 64 / 1024, input_size == hidden, at most two layers and two K steps of the down-sampling conv; everything else runs here alone.

No new tolerance:
  fp32 kernels (LSTM recurrence, elu_pad, gelu, the evq tensors)   error <= max(4 x |fp32 restatement - fp64|, 1e-6 max|ref64|)
  amp_lstm_forward under both precisions                           the same with the floor 1e-4
  codes        equal to fp64's on every (level, frame) speechtokenizer_ref.margin_rule decides; the undecided share, on the reference alone,
               is at most 0.02; every (level, frame), decided or not: the chosen row's fp64 distance is within tau of the fp64 minimum
  amp_dsconv   tokenizer_ref.dsconv_bound, error / bound <= 1; under f32 also bit-equal to the three-launch route
Every output tensor and the LSTM workspace (exactly amp_lstm_workspace_bytes long) lies between sentinels and starts out as sentinels; every
case asserts that an item's bits are those of its B = 1 run.  The worst error / bound of each case is printed."""
import ctypes
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import range_oracle  # noqa: E402
import speechtokenizer_ref as R  # noqa: E402
import tokenizer_geometry as tg  # noqa: E402
import tokenizer_ref as TR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
INT_SENTINEL = -0x5A5A5A5A5A5A
T4094 = 4094.0
NEXT = torch.nextafter(torch.tensor(T4094), torch.tensor(math.inf)).item()


def _L():
    from amphion_amd import _lib

    return _lib


def _H():
    import speechtokenizer_hip as H

    return H


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return _L().current_stream_ptr(torch.device(DEV))


class Guarded:
    """a device tensor of `shape`, `offset` floats off a 16-byte boundary, between two runs of GUARD sentinel elements (NaN, INT_SENTINEL for
    the codes, or `fill`); the tensor itself starts out as sentinels too, so a dropped store shows"""

    def __init__(self, shape, dtype=torch.float32, offset=0, fill=None):
        self.n = int(np.prod(shape))
        self.fill = fill if fill is not None else (float("nan") if dtype.is_floating_point else INT_SENTINEL)
        assert (self.n + 2 * GUARD + offset) * torch.empty((), dtype=dtype).element_size() <= tg.DEVICE_TENSOR_CAP, (shape, "DEVICE_TENSOR_CAP")
        self.buf = torch.full((self.n + 2 * GUARD + offset,), self.fill, dtype=dtype, device=DEV)
        self.lo = GUARD + offset
        self.t = self.buf[self.lo:self.lo + self.n].view(*shape)
        if dtype == torch.float32:
            assert self.t.data_ptr() % 16 == 4 * (offset % 4)

    def _is_sentinel(self, part):
        return torch.isnan(part) if self.fill != self.fill else part == self.fill

    def check_guards(self, what):
        torch.cuda.synchronize()
        for name, part in (("in front of", self.buf[:self.lo]), ("behind", self.buf[self.lo + self.n:])):
            hit = (~self._is_sentinel(part)).nonzero().flatten().tolist()
            assert not hit, f"{what}: the sentinel elements {hit[:8]} {name} the tensor were written"

    def check(self, what):
        self.check_guards(what)
        bad = self._is_sentinel(self.t).nonzero()
        assert bad.numel() == 0, f"{what}: {bad.shape[0]} of {self.n} outputs were not written; first at {bad[:4].tolist()} of {tuple(self.t.shape)}"
        return self.t


def bound(ref64, ref32, floor):
    return tg.lstm_bound(ref64, ref32, floor)


def check(name, got, ref64, ref32, floor, quiet=False):
    got = got.detach().cpu().double()
    assert got.shape == ref64.shape, (name, got.shape, ref64.shape)
    assert torch.isfinite(got).all(), name
    err, tol = float((got - ref64).abs().max()), bound(ref64, ref32, floor)
    ratio = err / tol if tol else 0.0
    if not quiet:
        print(f"    {name}: error {err:.3g}, bound {tol:.3g} ({ratio:.3f})")
    assert err <= tol, (name, err, tol)
    return ratio


# ------------------------------------------------------------------------------------------------------------------------------
# amp_evq
# ------------------------------------------------------------------------------------------------------------------------------
def evq_encode(q, z, st, n_q, want_zq=True, want_all=True, what="encode"):
    """amp_evq_encode on a device tensor -> (codes [n, B, T], zq or None, all_zq or None), every output guarded"""
    Bn, D, T = z.shape
    n = n_q - st
    out = [Guarded((n, Bn, T), torch.int64), Guarded((Bn, D, T)) if want_zq else None, Guarded((n, Bn, D, T)) if want_all else None]
    _L().check(_L().lib().amp_evq_encode(q.h, _p(z), Bn, T, st, n_q, *[_p(g.t) if g else None for g in out], _stream()))
    return tuple(g.check(f"{what} {tag}") if g else None for g, tag in zip(out, ("codes", "zq", "all_zq")))


def evq_decode(q, codes, st, what="decode"):
    n, Bn, T = codes.shape
    out = Guarded((Bn, q.D, T))
    _L().check(_L().lib().amp_evq_decode(q.h, _p(codes), n, st, Bn, T, _p(out.t), _stream()))
    return out.check(what)


def check_evq(q, ref, tag):
    """every rule of the header on one encode; -> the worst error / bound of its tensors"""
    cbs, z, st, n_q, r64, tau, decided = (ref[k] for k in ("cbs", "z", "st", "n_q", "r64", "tau", "decided"))
    print(f"{tag}: tau {tau:.3e}, smallest fp64 margin {float(r64['margin'].min()):.3e}, undecided frames {ref['undecided']:.4f}")
    assert ref["undecided"] <= tg.UNDECIDED_CAP, "the fp64 reference itself leaves too many frames undecided"
    zd = z.to(DEV)
    codes, zq, allq = evq_encode(q, zd, st, n_q, what=tag)
    ch = codes.cpu()
    assert codes.dtype == torch.int64 and int(ch.min()) >= 0 and int(ch.max()) < q.K, tag
    same = ch == r64["codes"]
    assert bool(same[decided].all()), f"{tag}: {int((~same & decided).sum())} decided codes differ from fp64's"
    excess = tg.evq_excess(cbs, z, ch, st)
    assert float(excess.max()) <= tau, f"{tag}: a chosen row is {float(excess.max()):.3e} above the fp64 minimum (tau {tau:.3e})"
    f64 = R.evq_forward(cbs, z, torch.float64, st, n_q, codes=ch)
    f32 = R.evq_forward(cbs, z, torch.float32, st, n_q, codes=ch)
    worst = max(check(f"{tag} zq", zq, f64["zq"], f32["zq"], 1e-6), check(f"{tag} all_zq", allq, f64["all_q"], f32["all_q"], 1e-6))
    acc = torch.zeros_like(allq[0])
    for lvl in allq:
        acc = acc + lvl
    assert torch.equal(acc, zq), f"{tag}: all_zq does not sum to zq in level order"
    dec = evq_decode(q, codes, st, what=tag + " decode")
    assert q.check() == 0, tag
    worst = max(worst, check(f"{tag} decode", dec, R.evq_decode(cbs, ch, torch.float64, st), R.evq_decode(cbs, ch, torch.float32, st), 1e-6))
    # the optional outputs left out
    for want_zq, want_all in ((False, True), (True, False), (False, False)):
        c2, q2, a2 = evq_encode(q, zd, st, n_q, want_zq, want_all, what=f"{tag} zq={want_zq} all_zq={want_all}")
        assert torch.equal(c2, codes) and (q2 is None or torch.equal(q2, zq)) and (a2 is None or torch.equal(a2, allq)), (tag, want_zq, want_all)
    # an item's bits are those of its B = 1 run
    for b in range(z.shape[0]):
        c1, q1, a1 = evq_encode(q, zd[b:b + 1].contiguous(), st, n_q, what=f"{tag} item {b}")
        assert torch.equal(c1[:, 0], codes[:, b]) and torch.equal(q1[0], zq[b]) and torch.equal(a1[:, 0], allq[:, b]), (tag, b)
    return worst


@pytest.mark.parametrize("case", tg.EVQ, ids=lambda c: c.id)
def test_evq_geometry(case):
    H = _H()
    worst = 0.0
    for T in case.Ts:
        ref = tg.evq_reference(case, T)
        q = H.Evq(ref["cbs"])
        worst = max(worst, check_evq(q, ref, f"evq {case.id} B={tg.B} T={T}"))
        if T == 17 and case.N >= 2:
            for st, n_q in ((1, case.N), (0, case.N - 1)):
                worst = max(worst, check_evq(q, tg.evq_reference(case, T, st, n_q), f"evq {case.id} T={T} levels [{st}, {n_q})"))
    print(f"evq {case.id}: worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("case", tg.EVQ_TIES, ids=lambda c: c.id)
def test_evq_ties_resolve_to_the_lowest_index(case):
    """every codebook row twice: the distances tie exactly, inside a thread's own rows, between threads of a wave or between waves"""
    H = _H()
    full, half, z = tg.evq_tie_inputs(case, case.Ts[0])
    zd = z.to(DEV)
    codes = evq_encode(H.Evq(full), zd, 0, case.N)[0]
    assert int(codes.max()) < case.K // 2 and int(codes.min()) >= 0, case.id
    assert torch.equal(codes, evq_encode(H.Evq(half), zd, 0, case.N)[0]), case.id


def test_evq_decode_flag_on_a_padded_row():
    H, case = _H(), tg.EVQ_FLAG
    T = case.Ts[0]
    cbs, _ = tg.evq_inputs(case, T)
    q = H.Evq(cbs)
    codes = torch.randint(0, case.K, (case.N, tg.B, T), generator=torch.Generator().manual_seed(3))
    dec = evq_decode(q, codes.to(DEV), 0)
    assert q.check() == 0
    check("decode of random codes at D = 1023", dec, R.evq_decode(cbs, codes, torch.float64), R.evq_decode(cbs, codes, torch.float32), 1e-6)
    zero = codes.clone()
    zero[1, 2, 16] = 0
    want = evq_decode(q, zero.to(DEV), 0)
    for bad in (case.K, -1, 2 ** 40):
        c = codes.clone()
        c[1, 2, 16] = bad
        got = evq_decode(q, c.to(DEV), 0, what=f"decode with the code {bad}")
        assert q.check() == _L().AMP_ERR_INVALID, bad
        assert torch.equal(got, want), bad
        assert q.check() == 0, bad                                    # the check cleared it


# ------------------------------------------------------------------------------------------------------------------------------
# amp_lstm
# ------------------------------------------------------------------------------------------------------------------------------
def _workspace(m, Bn, T):
    need = _L().lib().amp_lstm_workspace_bytes(m.h, Bn, T)
    assert need > 0 and need % 4 == 0
    return Guarded((need // 4,)), need


def lstm_recur(m, gx, skip=None, what="recur"):
    """amp_lstm_recur of layer 0 on device tensors; y and the exactly sized, NaN-filled workspace are guarded"""
    Bn, _, T = gx.shape
    y = Guarded((Bn, m.ndir * m.H, T))
    ws, _ = _workspace(m, Bn, T)
    rc = _L().lib().amp_lstm_recur(m.h, 0, _p(gx), Bn, T, _p(skip), _p(y.t), _p(ws.t), _stream())
    assert rc == 0, f"{what}: amp_lstm_recur returned {rc}: {_L().lib().amp_last_error().decode()}"
    ws.check_guards(what + " workspace")
    return y.check(what)


def lstm_forward(m, x, what="forward"):
    Bn, _, T = x.shape
    y = Guarded((Bn, _L().lib().amp_lstm_out_channels(m.h), T))
    ws, need = _workspace(m, Bn, T)
    _L().check(_L().lib().amp_lstm_forward(m.h, _p(x), Bn, T, _p(y.t), _p(ws.t), need, _stream()))
    ws.check_guards(what + " workspace")
    return y.check(what)


def check_recur(m, w_hh, gx, skip, tag, items=None):
    ref64 = R.lstm_recur(w_hh.double(), gx.double(), None if skip is None else skip.double())
    ref32 = R.lstm_recur(w_hh, gx, skip)
    gxd, skd = gx.to(DEV), None if skip is None else skip.to(DEV)
    y = lstm_recur(m, gxd, skd, what=tag)
    ratio = check(tag, y, ref64, ref32, 1e-6, quiet=True)
    for b in range(gx.shape[0]) if items is None else items:
        y1 = lstm_recur(m, gxd[b:b + 1].contiguous(), None if skd is None else skd[b:b + 1].contiguous(), what=f"{tag} item {b}")
        assert torch.equal(y1[0], y[b]), f"{tag}: item {b} differs from its B = 1 run"
    return ratio


@pytest.mark.parametrize("Hn", tg.LSTM_H)
def test_lstm_recur_hidden_axis(Hn):
    H = _H()
    worst = 0.0
    for bidir in (False, True):
        w = tg.lstm_weights(Hn, Hn, 1, bidir, 40 + Hn)
        m = H.Lstm(Hn, Hn, 1, bidir, False, *w)
        w_hh = torch.stack(w[1], 0)
        for T in tg.LSTM_H_T:
            _, gx, skip = tg.recur_case(Hn, bidir, T, tg.B, 1000 * Hn + T)
            for sk in (None, skip):
                r = check_recur(m, w_hh, gx, sk, f"recur H={Hn} bidir={bidir} T={T} skip={sk is not None}")
                worst = max(worst, r)
    print(f"lstm recur H={Hn}: worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("Hn", tg.LSTM_B_H)
def test_lstm_recur_batch_axis(Hn):
    H = _H()
    w = tg.lstm_weights(Hn, Hn, 1, True, 500 + Hn)
    m = H.Lstm(Hn, Hn, 1, True, False, *w)
    w_hh = torch.stack(w[1], 0)
    worst = 0.0
    for Bn in tg.LSTM_B:
        _, gx, skip = tg.recur_case(Hn, True, tg.LSTM_B_T, Bn, 600 + Hn + Bn)
        r = check_recur(m, w_hh, gx, skip, f"recur H={Hn} B={Bn} (tile {tg.lstm_tile(Bn)})")
        print(f"    recur H={Hn} B={Bn}: error / bound {r:.3f}")
        worst = max(worst, r)
    print(f"lstm recur H={Hn} over B: worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("Hn,T", tg.LSTM_LONG)
def test_lstm_recur_many_steps(Hn, T):
    H = _H()
    w, gx, _ = tg.recur_case(Hn, True, T, 2, 700 + Hn)
    m = H.Lstm(Hn, Hn, 1, True, False, *w)
    r = check_recur(m, torch.stack(w[1], 0), gx, None, f"recur H={Hn} T={T}")
    print(f"lstm recur H={Hn} T={T}: error / bound = {r:.3f}")


def test_lstm_recur_saturated_gates():
    H = _H()
    Hn, T, scale = tg.LSTM_SATURATED
    w, gx, skip = tg.recur_case(Hn, True, T, tg.B, 800, scale=scale)
    m = H.Lstm(Hn, Hn, 1, True, False, *w)
    r = check_recur(m, torch.stack(w[1], 0), gx, skip, f"recur H={Hn} T={T} gx x {scale:g}")
    print(f"lstm recur H={Hn} T={T} gx x {scale:g}: error / bound = {r:.3f}")
    # +-200 in chosen gate rows: the gate is exactly 0 or 1 (tests/tokenizer_geometry.py: saturated_gx)
    gx, zero, held = tg.saturated_gx(Hn, 5, tg.B, 7)
    w = tg.lstm_weights(Hn, Hn, 1, False, 8)
    m = H.Lstm(Hn, Hn, 1, False, False, *w)
    w_hh = torch.stack(w[1], 0)
    r = check_recur(m, w_hh, gx, None, "recur with +-200 in gate rows")
    y = lstm_recur(m, gx.to(DEV)).cpu()
    assert bool((y[:, zero[0]:zero[1]] == 0).all()), "an output gate at -200 is not exactly 0"
    assert bool((y[:, held[0]:held[1], 1:] == y[:, held[0]:held[1], :1]).all()), "f = +200, i = -200, o = +200 does not hold tanh(c_0) bit for bit"
    assert bool((y[:, held[0]:held[1], 0] != 0).any())
    print(f"lstm recur with +-200 in gate rows: error / bound = {r:.3f}")


def test_lstm_recur_at_the_64_kb_launch():
    """H = 1024 with B = 9: the tile of 16 items asks for 16 * 1024 * 4 = 65 536 B of dynamic LDS, exactly the default limit"""
    H = _H()
    Hn, Bn, T = tg.LSTM_64KB
    assert tg.lstm_lds_bytes(Hn, Bn) == 64 * 1024
    w, gx, skip = tg.recur_case(Hn, True, T, Bn, 99)
    m = H.Lstm(Hn, Hn, 1, True, False, *w)
    r = check_recur(m, torch.stack(w[1], 0), gx, skip, f"recur H={Hn} bidir B={Bn} T={T}")
    print(f"lstm recur H={Hn} B={Bn} T={T}: error / bound = {r:.3f}")


@pytest.mark.parametrize("Hn", tg.LSTM_FLIP_H)
def test_lstm_reverse_direction_is_the_flipped_forward_direction(Hn):
    H = _H()
    w = tg.lstm_weights(Hn, Hn, 1, True, 7 + Hn, same_dirs=True)
    m = H.Lstm(Hn, Hn, 1, True, False, *w)
    half = torch.randn(tg.B, 4 * Hn, 7, generator=torch.Generator().manual_seed(Hn))
    y = lstm_recur(m, torch.cat([half, half.flip(2)], 1).contiguous().to(DEV))
    assert torch.equal(y[:, :Hn], y[:, Hn:].flip(2))


def _forward_case(In, Hn, L, bidir, skip, precision, Ts):
    H = _H()
    w = tg.lstm_weights(In, Hn, L, bidir, 300 + In + Hn + L)
    m = H.Lstm(In, Hn, L, bidir, skip, *w)
    P = tg.lstm_named(w, L, bidir)
    P64 = {k: v.double() for k, v in P.items()}
    worst = 0.0
    for T in Ts:
        x = torch.randn(tg.B, In, T, generator=torch.Generator().manual_seed(10 * Hn + T))
        ref64, ref32 = R.slstm(P64, "", x.double(), L, bidir, skip), R.slstm(P, "", x, L, bidir, skip)
        tag = f"lstm In={In} H={Hn} L={L} bidir={bidir} skip={skip} T={T} [{precision}]"
        xd = x.to(DEV)
        y = lstm_forward(m, xd, what=tag)
        worst = max(worst, check(tag, y, ref64, ref32, 1e-4, quiet=True))
        for b in range(tg.B):
            assert torch.equal(lstm_forward(m, xd[b:b + 1].contiguous(), what=f"{tag} item {b}")[0], y[b]), (tag, b)
    _L().range_check(DEV)
    print(f"lstm forward In={In} H={Hn} L={L} bidir={bidir} skip={skip} [{precision}]: worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("In,Hn,L,bidir,skip", tg.LSTM_FORWARD)
def test_lstm_forward_geometry(conv_precision, In, Hn, L, bidir, skip):
    _forward_case(In, Hn, L, bidir, skip, conv_precision, tg.LSTM_FORWARD_T)


@pytest.mark.parametrize("In,Hn,L,bidir,skip", tg.LSTM_CREATE_EDGES)
def test_lstm_create_accepts_the_edges(conv_precision, In, Hn, L, bidir, skip):
    _forward_case(In, Hn, L, bidir, skip, conv_precision, (2,))


def _flag(dev=DEV):
    """the op-level range word: raised since the last check?  (the check clears it)"""
    _lib = _L()
    try:
        _lib.range_check(dev)
    except _lib.AmpError as e:
        assert e.status == _lib.AMP_ERR_RANGE, e
        return True
    return False


def test_lstm_forward_range_flag_through_the_projection():
    """f16x3: the projection stages x itself; 4094 fits the split form, the next fp32 does not"""
    H = _H()
    In, Hn = 7, 12
    w = tg.lstm_weights(In, Hn, 1, True, 31)
    m = H.Lstm(In, Hn, 1, True, False, *w)
    x0 = torch.randn(tg.B, In, 7, generator=torch.Generator().manual_seed(32))
    _flag()
    base = lstm_forward(m, x0.to(DEV))
    assert not _flag()
    for v in (T4094, NEXT, -T4094, -NEXT):
        x = x0.clone()
        x[1, In - 1, 3] = v
        want = range_oracle.flagged([range_oracle.staged_max(x)])
        assert want == (abs(v) > T4094)
        y = lstm_forward(m, x.to(DEV), what=f"x = {v!r}")
        assert _flag() == want, f"x = {v!r}: the flag is not {want}"
        assert torch.equal(y[0], base[0]) and torch.equal(y[2], base[2]), v


# ------------------------------------------------------------------------------------------------------------------------------
# amp_elu_pad, amp_gelu
# ------------------------------------------------------------------------------------------------------------------------------
def _elementwise_check(tag, got, ref64, ref32):
    """equal non-finite positions (NaN where NaN, the same infinity where infinite), the fp32 rule on the finite part"""
    got = got.cpu().double()
    fin = torch.isfinite(ref64)
    assert torch.equal(torch.isnan(got), torch.isnan(ref64)), tag
    inf = torch.isinf(ref64)
    assert torch.equal(torch.isinf(got), inf) and torch.equal(got[inf], ref64[inf]), tag
    if not bool(fin.any()):
        return 0.0
    both = fin & torch.isfinite(ref32.double())
    e32 = float((ref32.double() - ref64)[both].abs().max()) if bool(both.any()) else 0.0
    tol = max(4.0 * e32, 1e-6 * float(ref64[fin].abs().max()))
    err = float((got - ref64)[fin].abs().max())
    assert err <= tol, (tag, err, tol)
    return err / tol if tol else 0.0


def _elu_pad(x, pl, pr, elu, alpha, ox, oy):
    """amp_elu_pad with x `ox` and y `oy` floats off a 16-byte boundary; y guarded"""
    Bn, C, T = x.shape
    xg = Guarded((Bn, C, T), offset=ox)
    xg.t.copy_(x)
    y = Guarded((Bn, C, T + pl + pr), offset=oy)
    _L().check(_L().lib().amp_elu_pad(_p(xg.t), Bn, C, T, pl, pr, int(elu), float(alpha), _p(y.t), _stream()))
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("pl,pr", tg.ELU_PADS)
def test_elu_pad_geometry(pl, pr):
    worst = 0.0
    for T in tg.elu_lengths(pl, pr):
        for C in tg.ELU_C:
            g = torch.Generator().manual_seed(1000 * pl + 100 * pr + 10 * T + C)
            x = 2.0 * torch.randn(tg.ELU_B, C, T, generator=g)
            plain = R.pad1d_reflect(x, pl, pr)
            ref64, ref32 = R.pad1d_reflect(Fn.elu(x.double(), 0.5), pl, pr), R.pad1d_reflect(Fn.elu(x, 0.5), pl, pr)
            one = None
            for ox in tg.OFFSETS:
                for oy in tg.OFFSETS:
                    tag = f"elu_pad pads ({pl}, {pr}) T={T} C={C} x+{ox} y+{oy}"
                    assert torch.equal(_elu_pad(x, pl, pr, False, 1.0, ox, oy).check(tag).cpu(), plain), tag + ": the reflect part is bit-exact"
                    y = _elu_pad(x, pl, pr, True, 0.5, ox, oy).check(tag)
                    worst = max(worst, _elementwise_check(tag, y, ref64, ref32))
                    one = y.clone() if one is None else one
                    assert torch.equal(y, one), tag + ": the bits depend on the alignment"
            y1 = _elu_pad(x[1:2].contiguous(), pl, pr, True, 0.5, 0, 0).check("B = 1")
            assert torch.equal(y1[0], one[1]), (pl, pr, T, C)
    print(f"elu_pad pads ({pl}, {pr}): worst error / bound = {worst:.3f}")


def _with_specials(x, seed):
    """x with tokenizer_geometry.special_values() at random places"""
    sv = tg.special_values()
    flat = x.clone().flatten()
    at = torch.randperm(flat.numel(), generator=torch.Generator().manual_seed(seed))[:sv.numel()]
    flat[at] = sv
    return flat.view_as(x)


def test_elu_pad_special_values():
    for pl, pr in ((33, 64), (0, 0), (7, 0)):
        for alpha in (1.0, 0.5):
            x = _with_specials(2.0 * torch.randn(tg.ELU_B, 3, 130, generator=torch.Generator().manual_seed(pl)), 5 + pr)
            ref64, ref32 = R.pad1d_reflect(Fn.elu(x.double(), alpha), pl, pr), R.pad1d_reflect(Fn.elu(x, alpha), pl, pr)
            assert bool((ref64 == -alpha).any()) and bool(torch.isnan(ref64).any()) and bool(torch.isinf(ref64).any())
            for ox, oy in ((0, 0), (1, 3)):
                tag = f"elu_pad specials pads ({pl}, {pr}) alpha={alpha} x+{ox} y+{oy}"
                y = _elu_pad(x, pl, pr, True, alpha, ox, oy)
                y.check_guards(tag)                                   # (a NaN output is a sentinel too: only the guards are looked at)
                r = _elementwise_check(tag, y.t, ref64, ref32)
                print(f"    {tag}: error / bound {r:.3f}")
                plain = _elu_pad(x, pl, pr, False, alpha, ox, oy)
                plain.check_guards(tag)
                want = R.pad1d_reflect(x, pl, pr)
                got = plain.t.cpu()
                assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(got[~torch.isnan(want)], want[~torch.isnan(want)]), tag


@pytest.mark.parametrize("n", tg.GELU_N)
def test_gelu_geometry(n):
    L = _L().lib()
    worst = 0.0
    for special in (False, True):
        x = 3.0 * torch.randn(n, generator=torch.Generator().manual_seed(n))
        if special:
            if n < tg.special_values().numel():
                continue
            x = _with_specials(x, n)
        ref64, ref32 = Fn.gelu(x.double()), Fn.gelu(x)
        one = None
        for ox in tg.OFFSETS:
            for oy in tg.OFFSETS:
                tag = f"gelu n={n} x+{ox} y+{oy} specials={special}"
                xg, y = Guarded((n,), offset=ox), Guarded((n,), offset=oy)
                xg.t.copy_(x)
                _L().check(L.amp_gelu(_p(xg.t), n, _p(y.t), _stream()))
                y.check_guards(tag)
                if not special:
                    y.check(tag)
                worst = max(worst, _elementwise_check(tag, y.t, ref64, ref32))
                one = y.t.clone() if one is None else one
                assert torch.equal(torch.isnan(y.t), torch.isnan(one)) and torch.equal(y.t[~torch.isnan(one)], one[~torch.isnan(one)]), tag
            # in place, a guarded tensor holding x
            _L().check(L.amp_gelu(_p(xg.t), n, _p(xg.t), _stream()))
            xg.check_guards(f"gelu n={n} x+{ox} in place")
            assert torch.equal(torch.isnan(xg.t), torch.isnan(one)) and torch.equal(xg.t[~torch.isnan(one)], one[~torch.isnan(one)]), (n, ox)
    print(f"gelu n={n}: worst error / bound = {worst:.3f}")


# ------------------------------------------------------------------------------------------------------------------------------
# amp_dsconv: one child process per (group, precision) with AMP_LAUNCH_MANIFEST set, so that the tile that ran is read, not inferred
# ------------------------------------------------------------------------------------------------------------------------------
def _manifest_lines():
    man = os.environ["AMP_LAUNCH_MANIFEST"]
    return open(man).read().splitlines() if os.path.exists(man) else []


class _RawDevice:
    """device memory that does not come from torch's caching allocator: the exact-fp32 route's workspace of one table row is larger than
    tokenizer_geometry.DEVICE_TENSOR_CAP, and the sweep leaves the allocator's large-block pool as it found it"""

    def __init__(self, nbytes):
        path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)       # the HIP runtime torch loaded
        self.hip = ctypes.CDLL(path)
        self.hip.hipMalloc.argtypes, self.hip.hipFree.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t], [ctypes.c_void_p]
        self.p = ctypes.c_void_p()
        assert self.hip.hipMalloc(ctypes.byref(self.p), nbytes) == 0 and self.p.value

    def free(self):
        torch.cuda.synchronize()
        assert self.hip.hipFree(self.p) == 0


def ds_forward(conv, x, gelu, what="dsconv"):
    """amp_dsconv_forward on a device tensor; y guarded"""
    _lib = _L()
    L = _lib.lib()
    Bn, _, T = x.shape
    y = Guarded((Bn, conv.cout, L.amp_dsconv_out_len(conv.h, T)))
    need = L.amp_dsconv_workspace_bytes(conv.h, Bn, T)
    raw = ws = None
    if need > tg.DEVICE_TENSOR_CAP:
        raw = _RawDevice(need)
    elif need:
        ws = torch.empty(need // 4, device=DEV)
    wp = raw.p if raw else _p(ws)
    try:
        _lib.check(L.amp_dsconv_forward(conv.h, _p(x), Bn, T, int(gelu), wp, need, _p(y.t), _stream()))
        return y.check(what)
    finally:
        if raw:
            raw.free()


def _ds_tile_of(lines, what):
    """the launches of one f16x3 call: exactly one dsconv_f16x3_kernel<GELU, MI, NI> -> (GELU, MI, NI)"""
    names = [l.split("\t")[0] for l in lines]
    assert len(names) == 1 and names[0].startswith("dsconv_f16x3_kernel<"), f"{what}: launched {names}"
    return tuple(int(v) for v in names[0].split("<")[1].rstrip(">").split(","))


def run_ds_case(case, precision):
    from test_gpu_tokenizers import DsConv, three_step_route

    w, b = tg.ds_tensors(case)
    conv = DsConv(w, b)
    worst = 0.0
    for T in case.Ts:
        x = tg.ds_input(case, T)
        xd = x.to(DEV)
        for gelu in (False, True):
            tag = f"dsconv {case.id} T={T} gelu={gelu} [{precision}]"
            ref, tol = TR.dsconv_bound(w.double(), b.double(), x.double(), gelu)
            n0 = len(_manifest_lines())
            y = ds_forward(conv, xd, gelu, what=tag)
            lines = _manifest_lines()[n0:]
            assert tuple(y.shape) == tuple(ref.shape) == (case.B, case.cout, (T - 1) // 2 + 1) and torch.isfinite(y).all(), tag
            ratio = float(((y.cpu().double() - ref).abs() / tol.clamp_min(1e-30)).max())
            print(f"    {tag}: worst error / bound = {ratio:.3f}", file=sys.stderr)
            worst = max(worst, ratio)
            assert ratio <= 1.0, (tag, ratio)
            if precision == "f32":
                assert any(l.startswith("dsconv_zero_col_kernel") for l in lines) and not any(l.startswith("dsconv_f16x3") for l in lines), tag
                assert torch.equal(y, three_step_route(w, b, xd, gelu)), tag + ": not the three-launch route's bits"
            else:
                assert _ds_tile_of(lines, tag) == (int(gelu),) + case.tile(T), f"{tag}: ran {_ds_tile_of(lines, tag)}, the table expects {case.tile(T)}"
        y = ds_forward(conv, xd, True)
        for i in range(case.B):                       # an item's bits depend neither on what it is batched with nor on the tile width
            n0 = len(_manifest_lines())
            y1 = ds_forward(conv, xd[i:i + 1].contiguous(), True, what=f"{case.id} T={T} item {i}")
            if precision != "f32":
                assert _ds_tile_of(_manifest_lines()[n0:], "B = 1")[1:] == case.tile(T, 1) == (1, 1)
            assert torch.equal(y1[0], y[i]), (case.id, T, i)
    assert not _flag()
    return worst


def _ds_range_setup():
    from test_gpu_tokenizers import DsConv

    case = tg.DS_RANGE
    w, b = tg.ds_tensors(case)
    return case, w, b, DsConv(w, b), tg.ds_input(case, case.Ts[0])


DS_RANGE_AT = {"interior": (5, 4), "column 0": (70, 0), "column T - 1": (2, -1), "the last channel of a ragged K step": (128, 4)}


def run_ds_range_threshold(where):
    """one element of item 1 at 4094 passes, its nextafter flags; with nothing flagged the other items keep their bits"""
    case, w, b, conv, x0 = _ds_range_setup()
    ch, t = DS_RANGE_AT[where]
    _flag()
    base = ds_forward(conv, x0.to(DEV), True)
    assert not _flag()
    for v in (T4094, NEXT, -T4094, -NEXT):
        x = x0.clone()
        x[1, ch, t] = v
        want = range_oracle.flagged([range_oracle.staged_max(x)])
        assert want == (abs(v) > T4094), "the case is mis-built"
        y = ds_forward(conv, x.to(DEV), True, what=f"{where}: {v!r}")
        assert _flag() == want, f"{where}: x = {v!r}: the flag is not {want}"
        assert torch.equal(y[0], base[0]) and torch.equal(y[2], base[2]), (where, v)
        if not want:
            ref, tol = TR.dsconv_bound(w.double(), b.double(), x.double(), True)
            assert float(((y.cpu().double() - ref).abs() / tol).max()) <= 1.0, (where, v)
    return None


def run_ds_range_nonfinite():
    """a single +-inf flags, a single NaN does not; the non-finite outputs sit where fp64 has them and the other items keep their bits"""
    case, w, b, conv, x0 = _ds_range_setup()
    _flag()
    base = ds_forward(conv, x0.to(DEV), False)
    for ch, t in DS_RANGE_AT.values():
        for v in (math.inf, -math.inf, math.nan):
            x = x0.clone()
            x[1, ch, t] = v
            want = range_oracle.flagged([range_oracle.staged_max(x)])
            assert want == (v == v)
            yg = Guarded((case.B, case.cout, (case.Ts[0] - 1) // 2 + 1))
            xd = x.to(DEV)
            _L().check(_L().lib().amp_dsconv_forward(conv.h, _p(xd), case.B, case.Ts[0], 0, None, 0, _p(yg.t), _stream()))
            yg.check_guards(f"x = {v}")
            assert _flag() == want, f"x[1, {ch}, {t}] = {v}: the flag is not {want}"
            ref = TR.dsconv(w.double(), b.double(), x.double(), False)
            assert range_oracle.nonfinite_equal(yg.t.cpu(), ref, nan=v != v), (ch, t, v)
            assert torch.equal(yg.t[0], base[0]) and torch.equal(yg.t[2], base[2]), (ch, t, v)
    return None


def run_ds_range_unstaged():
    """input columns -1 and >= T are selected to 0 and only their load address is clamped: with 1e6 in every element in front of the tensor and
    behind it (what a load without the clamp would reach from the first and the last row) nothing flags and no bit changes"""
    case, w, b, conv, x0 = _ds_range_setup()
    _flag()
    base = ds_forward(conv, x0.to(DEV), True)
    for T in (case.Ts[0], case.Ts[0] - 1):            # T odd: column T is staged as 0; T even: the window ends at T - 1
        x = x0[..., :T].contiguous()
        want = ds_forward(conv, x.to(DEV), True)
        xg = Guarded(tuple(x.shape), fill=1e6)
        xg.t.copy_(x)
        y = ds_forward(conv, xg.t, True, what=f"T={T} between 1e6")
        assert not _flag(), f"T={T}: a value that is never staged raised the flag"
        assert torch.equal(y, want) and (T != case.Ts[0] or torch.equal(y, base)), T
    return None


def ds_group_cases(group, precision):
    """[(case id, callable returning error / bound or None, whether it applies)] -- the table form of tests/test_gpu_recipe_shapes.py's runner"""
    if group == "dsconv":
        return [(c.id, (lambda c=c: run_ds_case(c, precision)), None) for c in tg.DSCONV]
    out = [(f"threshold/{k}", (lambda k=k: run_ds_range_threshold(k)), None) for k in DS_RANGE_AT]
    return out + [("nonfinite", run_ds_range_nonfinite, None), ("unstaged", run_ds_range_unstaged, None)]


def _run_children(group, precision, tmp_path):
    out, man = tmp_path / "results.json", tmp_path / "manifest.tsv"
    env = dict(os.environ, AMP_LAUNCH_MANIFEST=str(man), AMP_PRECISION=precision)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), group, precision, str(out)], capture_output=True, text=True, env=env, timeout=600)
    res = json.load(open(out)) if out.exists() else {}
    problems, table = [], []
    for name, _, _ in ds_group_cases(group, precision):
        if name not in res:
            problems.append(f"{name}: not run (the child ended first)")
            continue
        c = res[name]
        if c["err"] is not None:
            problems.append(f"{name}:\n{c['err']}")
        table.append(f"{precision:6s} {name:44s} {' + '.join(c['kernels']):60s} {'-' if c['ratio'] is None else format(c['ratio'], '.3f'):>7s}")
    print(f"\n# tokenizer geometry, group {group}, {precision}: case, kernels, largest error / bound\n" + "\n".join(table))
    print(r.stderr[-6000:])
    assert r.returncode == 0 and not problems, f"child exit {r.returncode}\n" + "\n".join(problems) + "\n" + r.stderr[-2000:]


def test_dsconv_geometry(conv_precision, tmp_path):
    _run_children("dsconv", conv_precision, tmp_path)


def test_dsconv_range_guard(tmp_path):
    _run_children("dsrange", "f16x3", tmp_path)


if __name__ == "__main__":
    from test_gpu_recipe_shapes import _child

    _child(sys.argv[1], sys.argv[2], sys.argv[3], cases_fn=ds_group_cases)
