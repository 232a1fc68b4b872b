"""Op-level parity of the sixteen VITS entry points that were reached only through whole modules: each one against the plain
statement of the same operation in tests/vits_ops_ref.py (pinned to the oracle by tests/test_vits_ops_ref.py), over one grid of
time lengths on both sides of the 256-thread block, the 1 024-column row block and two row blocks, channel counts that are no
multiple of 4 or 8, and ragged lengths around the row-block edges.

Bounds.  Ops that move data or do ONE fp32 operation per element are compared bit for bit with that operation in torch on the
CPU.  Ops with transcendentals or reductions are compared with fp64: layer_norm / dwconv / attention / spline at the bounds
tests/test_gpu_vits_infer.py::test_ops_vs_oracle already uses; wn_gate / posterior_sample / gauss_sample / affine_reverse, which
had no bound, at 4 x the error of THE SAME FORMULA evaluated by torch in fp32 on the CPU on the same inputs, scaled by
max(1, |ref|max) -- room for another, still few-ulp expf / tanhf; a wrong operand or mask is orders above it.  Every batch holds
at least 20 000 elements so that the CPU's maximum error is a maximum over enough draws to stand for its arithmetic.

Padding.  Where include/amphion_hip.h says the columns beyond a length are ignored or written as zero they hold NaN here; where
it states that the mask is a factor (the callers pass specified memory) they hold ordinary numbers."""
import math
import zlib

import pytest
import torch

import vits_ops_ref as ref

pytestmark = pytest.mark.gpu

T_GRID = [1, 255, 256, 257, 1023, 1024, 1025, 2049, 3000]
C_GRID = [7, 24, 192]
EDGES = (1023, 1025, 2047, 2049)            # just below / above one and two 1 024-column row blocks
MIN_ELEMS = 20000
NAN = float("nan")


def _ragged(T, zero, most=None):
    v = sorted({T, 1, T - 1} | {e for e in EDGES if e < T}, reverse=True)
    v = [n for n in v if n >= 1]
    if most is not None and len(v) > most:   # keep T, T - 1, the edge values next to them and 1
        v = v[:most - 1] + [1]
    return v + ([0] if zero else [])


def _cases(T, row_elems, zero=True, none=True, most=None, min_elems=MIN_ELEMS):
    """-> [(lens or None, B)]: no lengths, all full, ragged; the batch repeated until it holds ``min_elems`` elements"""
    out = []
    for lens in ([None] if none else []) + [[T, T], _ragged(T, zero, most)]:
        n = 2 if lens is None else len(lens)
        reps = max(1, -(-min_elems // (n * row_elems)))
        out.append((None if lens is None else lens * reps, n * reps))
    return out


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


def _lens_dev(lens):
    return None if lens is None else torch.tensor(lens, dtype=torch.int32).cuda()


def _valid(lens, B, C, T):
    return ref.seq_mask(lens, B, T).expand(B, C, T)


def _poison(x, lens):
    """NaN in the columns t >= lens[b]"""
    if lens is None:
        return x
    return x.masked_fill(~_valid(lens, *x.shape), NAN)


def _f64(t):
    return t.double() if isinstance(t, torch.Tensor) and t.is_floating_point() else t


def _bounded(name, got, fn, args, where=None):
    """the kernel against fn in fp64, allowed 4 x the error of fn in fp32 on the CPU, scaled by max(1, |ref|max)"""
    want = fn(*[_f64(a) for a in args])
    cpu = fn(*args)
    assert cpu.dtype == torch.float32 and got.shape == want.shape
    sel = (lambda t: t) if where is None else (lambda t: t[where])
    e_cpu = (sel(cpu).double() - sel(want)).abs().max().item()
    e_gpu = (sel(got.cpu()).double() - sel(want)).abs().max().item()
    scale = max(1.0, sel(want).abs().max().item())
    print(f"\n[vits ops] {name}: kernel {e_gpu:.3e}, torch fp32 on the CPU {e_cpu:.3e}, |ref|max {scale:.3g}")
    assert e_cpu > 0, "the CPU's fp32 evaluation is exact here: the case sizes no bound"
    assert e_gpu <= 4 * e_cpu * scale, (name, e_gpu, e_cpu, scale)


# ---- wn_gate -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", T_GRID)
@pytest.mark.parametrize("H", C_GRID)                    # a is [B, 2H, T]: 384 rows per item at the recipe's 192
def test_wn_gate(H, T):
    from amphion_amd.modules import hip_ops

    g = _gen("gate", H, T)
    B = max(3, -(-MIN_ELEMS // (H * T)))
    a = torch.randn(B, 2 * H, T, generator=g) * 2
    n_layers, layer = 3, 1
    cond = torch.randn(B, 2 * H * n_layers, 1, generator=g)             # cond_layer(g) as WN holds it
    out = torch.full((B, H, T), NAN).cuda()
    hip_ops.wn_gate(a.cuda(), None, out)
    _bounded(f"wn_gate H={H} T={T}", out, ref.wn_gate, (a, None))
    # WN's slice of the condition: a view that starts at this layer's rows and keeps the batch stride of all layers
    cd = cond.cuda()
    g_l = cd[:, layer * 2 * H:, 0]
    assert g_l.stride(0) == 2 * H * n_layers and g_l.data_ptr() != cd.data_ptr()
    out = torch.full((B, H, T), NAN).cuda()
    hip_ops.wn_gate(a.cuda(), g_l, out)
    _bounded(f"wn_gate H={H} T={T} cond", out, ref.wn_gate, (a, cond[:, layer * 2 * H:(layer + 1) * 2 * H, 0]))


# ---- wn_accumulate -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", T_GRID)
@pytest.mark.parametrize("H", C_GRID)
def test_wn_accumulate(H, T):
    from amphion_amd.modules import hip_ops

    g = _gen("acc", H, T)
    for lens, B in _cases(T, H * T, min_elems=1):
        ld = _lens_dev(lens)
        for first, last in ((True, False), (False, False), (False, True), (True, True)):
            x, out = torch.randn(B, H, T, generator=g), torch.randn(B, H, T, generator=g)
            rs = torch.randn(B, H if last else 2 * H, T, generator=g)
            xd = x.cuda()
            od = torch.full((B, H, T), NAN).cuda() if first else out.cuda()     # `first` starts from zero: it does not read out
            hip_ops.wn_accumulate(xd, od, rs.cuda(), ld, first, last)
            wx, wo = ref.wn_accumulate(x, out, rs, lens, first, last)
            assert torch.equal(od.cpu(), wo), (lens is None, first, last)
            assert torch.equal(xd.cpu(), wx), (lens is None, first, last)
            if lens is not None and not last:
                assert (xd.cpu()[~_valid(lens, B, H, T)] == 0).all()


# ---- sequence_mask / flip_channels / add_channel_bias ---------------------------------------------------------------------
@pytest.mark.parametrize("T", T_GRID)
@pytest.mark.parametrize("C", C_GRID + [384])
def test_sequence_mask_flip_and_channel_bias(C, T):
    from amphion_amd.modules import hip_ops

    g = _gen("mask", C, T)
    for lens, B in _cases(T, C * T, none=False, min_elems=1):
        x = torch.randn(B, C, T, generator=g)
        got = hip_ops.sequence_mask_(_poison(x, lens).cuda(), _lens_dev(lens)).cpu()       # NaN beyond the lengths: assigned, not multiplied
        assert torch.equal(got, ref.sequence_mask(x, lens))
        assert torch.equal(got[_valid(lens, B, C, T)], x[_valid(lens, B, C, T)]) and (got[~_valid(lens, B, C, T)] == 0).all()
        assert torch.equal(hip_ops.flip_channels(x.cuda()).cpu(), ref.flip_channels(x))
        cb = torch.randn(B, C, 1, generator=g)
        assert torch.equal(hip_ops.add_channel_bias_(x.cuda(), cb.cuda()).cpu(), ref.add_channel_bias(x, cb))


# ---- coupling_apply ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", T_GRID)
@pytest.mark.parametrize("h", C_GRID)                    # x is [B, 2h, T]
def test_coupling_apply(h, T):
    from amphion_amd.modules import hip_ops

    g = _gen("coupling", h, T)
    for lens, B in _cases(T, h * T, min_elems=1):
        x, m = torch.randn(B, 2 * h, T, generator=g), torch.randn(B, h, T, generator=g)
        mp = _poison(m, lens)                            # m is unspecified beyond the length (a ragged conv skips those tiles)
        for reverse in (False, True):
            got = hip_ops.coupling_apply_(x.cuda(), mp.cuda(), _lens_dev(lens), reverse).cpu()
            assert torch.equal(got, ref.coupling_apply(x, mp, lens, reverse)), (lens is None, reverse)
            assert torch.equal(got[:, :h], x[:, :h])
            if lens is not None:
                assert (got[:, h:][~_valid(lens, B, h, T)] == 0).all()


# ---- posterior_sample / affine_reverse / gauss_sample --------------------------------------------------------------------
@pytest.mark.parametrize("T", T_GRID)
@pytest.mark.parametrize("C", C_GRID)                    # stats is [B, 2C, T]
def test_posterior_sample(C, T):
    from amphion_amd.modules import hip_ops

    g = _gen("post", C, T)
    for lens, B in _cases(T, C * T):
        stats = torch.cat([torch.randn(B, C, T, generator=g), torch.randn(B, C, T, generator=g) * 0.7 - 0.5], 1)
        eps = torch.randn(B, C, T, generator=g)
        got = hip_ops.posterior_sample(stats.cuda(), eps.cuda(), _lens_dev(lens))
        _bounded(f"posterior_sample C={C} T={T} B={B}", got, ref.posterior_sample, (stats, eps, lens))
        if lens is not None:
            assert (got.cpu()[~_valid(lens, B, C, T)] == 0).all()


@pytest.mark.parametrize("T", T_GRID)
@pytest.mark.parametrize("C", [2] + C_GRID)              # 2: the duration predictor's flows
def test_affine_reverse(C, T):
    from amphion_amd.modules import hip_ops

    g = _gen("affine", C, T)
    for lens, B in _cases(T, C * T):
        x = torch.randn(B, C, T, generator=g) * 2
        m, logs = torch.randn(C, generator=g), torch.randn(C, generator=g) * 0.7
        got = hip_ops.affine_reverse(x.cuda(), m.cuda(), logs.cuda(), _lens_dev(lens))
        _bounded(f"affine_reverse C={C} T={T} B={B}", got, ref.affine_reverse, (x, m, logs, lens))
        if lens is not None:
            assert (got.cpu()[~_valid(lens, B, C, T)] == 0).all()


@pytest.mark.parametrize("T", T_GRID)
@pytest.mark.parametrize("C", C_GRID)
def test_gauss_sample(C, T):
    from amphion_amd.modules import hip_ops

    g = _gen("gauss", C, T)
    B = max(3, -(-MIN_ELEMS // (C * T)))
    m, logs, noise = torch.randn(B, C, T, generator=g), torch.randn(B, C, T, generator=g) * 0.7 - 0.5, torch.randn(B, C, T, generator=g)
    for scale in (0.667, 1.0):
        got = hip_ops.gauss_sample(m.cuda(), logs.cuda(), noise.cuda(), scale)
        _bounded(f"gauss_sample C={C} T={T} scale={scale}", got, ref.gauss_sample, (m, logs, noise, scale))


# ---- embed_tokens --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", T_GRID)
@pytest.mark.parametrize("hidden", C_GRID)
def test_embed_tokens(hidden, T):
    from amphion_amd.modules import hip_ops

    g = _gen("embed", hidden, T)
    n_vocab = 53
    w = torch.randn(n_vocab, hidden, generator=g) * hidden**-0.5
    for lens, B in _cases(T, hidden * T, min_elems=1):
        tok = torch.randint(0, n_vocab, (B, T), generator=g)
        got = hip_ops.embed_tokens(tok.cuda(), w.cuda(), _lens_dev(lens), math.sqrt(hidden)).cpu()
        assert torch.equal(got, ref.embed_tokens(tok, w, lens, math.sqrt(hidden))), lens is None
        if lens is not None:       # ids beyond the length may be anything: they are clamped, then masked
            for bad in (2**40, -7):
                wild = tok.masked_fill(~ref.seq_mask(lens, B, T)[:, 0], bad)
                assert torch.equal(hip_ops.embed_tokens(wild.cuda(), w.cuda(), _lens_dev(lens), math.sqrt(hidden)).cpu(), got)


# ---- layer_norm_c_ragged -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", T_GRID)
@pytest.mark.parametrize("C", C_GRID)
def test_layer_norm_ragged(C, T):
    from amphion_amd.modules import hip_ops

    g = _gen("ln", C, T)
    for lens, B in _cases(T, C * T, none=False, min_elems=1):
        ld = _lens_dev(lens)
        x, r, p = (torch.randn(B, C, T, generator=g) for _ in range(3))
        gm, bt = 1 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
        valid = _valid(lens, B, C, T)
        xp, rp, pp = (_poison(t, lens).cuda() for t in (x, r, p))
        # the three forms and bounds of test_ops_vs_oracle: plain and with a residual 2e-5; residual, GELU and `+ post` 1e-5
        for res, post, gelu, tol in ((None, None, False, 2e-5), (rp, None, False, 2e-5), (rp, pp, True, 1e-5)):
            got = hip_ops.layer_norm_c(xp, gm.cuda(), bt.cuda(), res=res, post=post, gelu=gelu, lens=ld).cpu()
            want = ref.layer_norm_c_ragged(x.double(), r.double() if res is not None else None, gm.double(), bt.double(),
                                           p.double() if post is not None else None, lens, gelu=gelu)
            err = (got.double() - want).abs().max().item()
            print(f"\n[vits ops] layer_norm_c_ragged C={C} T={T} res={res is not None} gelu={gelu}: {err:.3e}")
            assert err <= tol, (res is not None, gelu, err)
            assert (got[~valid] == 0).all()


# ---- dwconv --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", T_GRID)
@pytest.mark.parametrize("C", C_GRID)
def test_dwconv(C, T):
    from amphion_amd.modules import hip_ops

    g = _gen("dw", C, T)
    for lens, B in _cases(T, C * T, min_elems=1):
        x = torch.randn(B, C, T, generator=g)
        for K, d in ((3, 1), (3, 9), (5, 2)):
            w, b = torch.randn(C, 1, K, generator=g), torch.randn(C, generator=g)
            got = hip_ops.dwconv(_poison(x, lens).cuda(), w.cuda(), b.cuda(), _lens_dev(lens), d).cpu()   # x * mask: nothing beyond is read
            err = (got.double() - ref.dwconv(x.double(), w.double(), b.double(), lens, d)).abs().max().item()
            print(f"\n[vits ops] dwconv C={C} T={T} K={K} d={d}: {err:.3e}")
            assert err <= 1e-5, (K, d, err)
        got = hip_ops.dwconv(x.cuda(), w.cuda(), None, _lens_dev(lens), d).cpu()                           # no bias
        assert (got.double() - ref.dwconv(x.double(), w.double(), None, lens, d)).abs().max().item() <= 1e-5


# ---- spline_flow ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", T_GRID)
def test_spline_flow(T):
    from amphion_amd.modules import hip_ops

    g = _gen("spline", T)
    K = 10
    for lens, B in _cases(T, T, min_elems=4000):
        z = torch.randn(B, 2, T, generator=g) * 3
        h = torch.randn(B, 3 * K - 1, T, generator=g)
        for inverse in (True, False):
            for flip in (False, True):
                got = hip_ops.spline_flow(z.cuda(), h.cuda(), _lens_dev(lens), K, 64, 5.0, inverse, flip_in=flip, flip_out=flip).cpu()
                want = ref.spline_flow(z.double(), h.double(), lens, K, 64, 5.0, inverse, flip_in=flip, flip_out=flip)
                err = (got.double() - want).abs().max().item()
                print(f"\n[vits ops] spline_flow T={T} B={B} inverse={inverse} flip={flip}: {err:.3e}")
                assert err <= 2e-4, (inverse, flip, err)
                if lens is not None:
                    assert (got[~_valid(lens, B, 2, T)] == 0).all()


# ---- rel_attention_strided -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", T_GRID)
@pytest.mark.parametrize("C,H", [(7, 1), (24, 2), (192, 2)])       # dk = 7: the one-query kernel; 12 and 96: the tiled one while it fits
def test_rel_attention_strided(C, H, T):
    from amphion_amd.modules import hip_ops

    g = _gen("attn", C, T)
    window = 4
    for lens, B in _cases(T, C * T, zero=False, most=4, min_elems=1):
        x = torch.randn(B, C, T, generator=g)
        ek, ev = (torch.randn(2 * window + 1, C // H, generator=g) * 0.3 for _ in range(2))
        q, k, v, _ = ref.attention_operands(x)
        qkv = torch.cat([q, k, v], 1).contiguous().cuda()               # the merged projection's output: three slices of one tensor
        got = hip_ops.rel_attention_qkv(qkv, ek.cuda(), ev.cuda(), _lens_dev(lens), H, window).cpu()
        want = ref.rel_attention(x.double(), ek, ev, lens, H, window)
        valid = _valid(lens, B, C, T)                                   # valid queries
        err = (got.double() - want)[valid].abs().max().item()
        print(f"\n[vits ops] rel_attention_strided C={C} H={H} T={T} B={B}: {err:.3e}")
        assert torch.isfinite(got[valid]).all() and err <= 2e-5, err


# ---- durations / expand_path_strided -------------------------------------------------------------------------------------
def _logw(n, length_scale, g):
    """log((n + u) / length_scale), u in [0.05, 0.95]: exp(logw) * length_scale stays at least 0.05 from an integer, its ceil is n + 1"""
    u = 0.05 + 0.9 * torch.rand(n.shape, generator=g, dtype=torch.float64)
    return torch.log((n.double() + u) / length_scale).float()


@pytest.mark.parametrize("T,big", [(1, 3), (257, 3), (1025, 6), (2049, 100), (3000, 6)])
@pytest.mark.parametrize("length_scale", [1.0, 1.1])
def test_durations_exact(T, big, length_scale):
    """ceil makes this exact or off by one, so the inputs stay away from the integers and everything is asserted exactly.  Zero
    durations: every masked token, and (below) exp(logw) that underflows to 0.  ``big`` = 100 at T = 2 049 takes the running sum
    beyond 2^16."""
    from amphion_amd.modules import hip_ops

    g = _gen("dur", T, length_scale)
    lens = _ragged(T, zero=True)
    B = len(lens)
    n = torch.randint(0, big, (B, 1, T), generator=g)
    logw = _logw(n, length_scale, g)
    logw[:, :, ::5] = -200.0                                             # expf underflows to exactly 0: ceil(0) = 0 frames
    n[:, :, ::5] = -1
    mask = ref.seq_mask(lens, B, T, torch.int64)
    want_w = (n + 1) * mask
    want_cum = torch.cumsum(want_w[:, 0], -1)
    if T == 2049:
        assert want_cum[0, -1].item() > 2**16
    w_ceil, cum, ylen = hip_ops.durations(logw.cuda(), _lens_dev(lens), length_scale)
    assert torch.equal(w_ceil.cpu(), want_w.float())
    assert torch.equal(cum.cpu().long(), want_cum)
    assert torch.equal(ylen.cpu().long(), want_cum[:, -1].clamp_min(1))
    # and the reference's own lines agree with the construction (in fp32, as the reference runs: exp(-200) is 0 there, not in fp64)
    rw, rc, ry = ref.durations(logw, lens, length_scale)
    assert torch.equal(rw.long(), want_w) and torch.equal(rc, want_cum) and torch.equal(ry, want_cum[:, -1].clamp_min(1))
    # no lengths
    w_ceil, cum, ylen = hip_ops.durations(logw.cuda(), None, length_scale)
    assert torch.equal(w_ceil.cpu(), (n + 1).float()) and torch.equal(cum.cpu().long(), torch.cumsum(n[:, 0] + 1, -1))


@pytest.mark.parametrize("Tx", T_GRID)
@pytest.mark.parametrize("D", [7, 40, 192])
def test_expand_path_strided(D, Tx):
    """both halves of a [B, 2D, Tx] tensor read in place, over many 64-frame blocks, against generate_path + matmul (one non-zero term
    per output: exact)"""
    from amphion_amd import _lib
    from amphion_amd.modules import hip_ops

    g = _gen("expand", D, Tx)
    xl = _ragged(Tx, zero=True, most=4)
    B = len(xl)
    w = torch.randint(0, 4, (B, 1, Tx), generator=g) * ref.seq_mask(xl, B, Tx, torch.int64)     # zero durations among them
    cum = torch.cumsum(w[:, 0], -1)
    yl = cum[:, -1].clamp_min(1)
    ty = int(yl.max())
    stats = torch.randn(B, 2 * D, Tx, generator=g)
    sd = stats.cuda()
    cd, xd, yd = cum.to(torch.int32).cuda(), _lens_dev(xl), yl.to(torch.int32).cuda()
    for half in (0, 1):
        src = sd[:, half * D:(half + 1) * D]
        assert not src.is_contiguous() or B == 1
        out, attn = hip_ops.expand_path(src, cd, xd, yd, ty, want_attn=(half == 0))
        want, path = ref.expand_path(stats[:, half * D:(half + 1) * D], w.float(), xl, yl, ty)
        assert torch.equal(out.cpu(), want), half
        if attn is not None:
            assert torch.equal(attn.cpu(), path)
    # the entry point itself with the stride spelled out, and without x lengths (NULL = all Tx)
    out = torch.full((1, D, int(yl[0])), NAN).cuda()
    _lib.check(_lib.lib().amp_expand_path_strided(_lib.ptr(sd[:1, D:]), 2 * D * Tx, _lib.ptr(cd[:1]), None, _lib.ptr(yd[:1]), 1, D, Tx,
                                                  int(yl[0]), _lib.ptr(out), None, _lib.current_stream_ptr(sd.device)))
    want, _ = ref.expand_path(stats[:1, D:], w[:1].float(), None, yl[:1], int(yl[0]))
    assert torch.equal(out.cpu(), want)


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_grid_limits_are_refused_not_truncated():
    """B * C rows ride on gridDim.y (65 535 at most) in amp_dwconv, amp_affine_reverse and amp_embed_tokens: one row more is
    AMP_ERR_INVALID with the entry point's message, and nothing is launched -- the output keeps what it held."""
    from amphion_amd import _lib

    L = _lib.lib()
    B, C, T = 256, 256, 2                                                # 65 536 rows
    x = torch.randn(B, C, T).cuda()
    st = _lib.current_stream_ptr(x.device)
    w, b = torch.randn(C, 1, 3).cuda(), torch.randn(C).cuda()
    tok = torch.zeros(B, T, dtype=torch.int64).cuda()
    emb = torch.randn(5, C).cuda()
    calls = {
        "amp_dwconv": lambda y: L.amp_dwconv(_lib.ptr(x), _lib.ptr(w), _lib.ptr(b), None, B, C, T, 3, 1, _lib.ptr(y), st),
        "amp_affine_reverse": lambda y: L.amp_affine_reverse(_lib.ptr(x), _lib.ptr(b), _lib.ptr(b), None, B, C, T, _lib.ptr(y), st),
        "amp_embed_tokens": lambda y: L.amp_embed_tokens(_lib.ptr(tok), _lib.ptr(emb), None, B, T, C, 5, 1.0, _lib.ptr(y), st),
    }
    for name, call in calls.items():
        y = torch.full((B, C, T), 7.0).cuda()
        status = call(y)
        assert status == -1, (name, status)                              # AMP_ERR_INVALID
        assert L.amp_last_error().decode().startswith(name + ": bad argument"), name
        with pytest.raises(_lib.AmpError, match=name):
            _lib.check(status)
        torch.cuda.synchronize()
        assert (y == 7.0).all(), name
    # one row fewer is inside the limit
    y = torch.full((B * C - 1, 1, T), 7.0).cuda()
    _lib.check(L.amp_affine_reverse(_lib.ptr(x), _lib.ptr(b[:1]), _lib.ptr(b[:1]), None, B * C - 1, 1, T, _lib.ptr(y), st))
    _bounded("affine_reverse at 65 535 rows", y, ref.affine_reverse, (x.cpu().reshape(-1, 1, T)[:B * C - 1], b[:1].cpu(), b[:1].cpu(), None))
