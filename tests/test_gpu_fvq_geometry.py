"""amp_fvq_* over the whole documented geometry (D <= 1024, d <= 32, K <= 16384, N <= 32) and amp_semantic_prepare around its 64 x 32 tile, through
the C ABI, against fp64 (tests/fvq_geometry.py holds the tables; tests/test_fvq_geometry_ref.py shows on the CPU what they reach and that the
rules below catch a kernel with one slip).

Every other quantizer case of the suite has d = 8, K and D multiples of 16 and N <= 12: fvq_encode_kernel<16> and <32>, zero-padded rows (d < DP),
threads that scan no row (K < 16) or unequal counts, ragged D, N = 32, the 136-KB encode and the 66-KB decode LDS requests run here alone.
For every encode case and length (B = 3, T = 1 / 17 / 50), with the existing rules and no new tolerance:
  codes        equal to fp64's on every (level, frame) the margin rule of codec_ref decides; the undecided share is printed (it is 0);
  zq, latents  within max(4 x the fp32 restatement's own error against fp64, 1e-6 max|z|) on decided frames; the ratio is printed;
  all_zq       sums to zq in level order, bit for bit;
  every (level, frame), decided or not: along the GPU's own codes, the chosen row's fp64 distance exceeds the fp64 minimum by at most tau;
  decode       amp_fvq_decode of the GPU's codes within the same rule of fp64 vq2emb and of encode's zq; amp_fvq_decode_add bit for bit
               decode + add; amp_fvq_check clean;
  every output lies between sentinels that must stay untouched (T = 17 and 50 leave 15 and 14 frames of the last tile past the end).
The folded forms (row stride T + 3, sub), fewer levels, batch independence, exact ties (every row twice; d = 1 with l2), the decode flag at the
66-KB request, the refusals at the edge of the range, and amp_semantic_prepare at every crossing of its tile follow."""
import ctypes
import os
import sys
import time

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import codec_ref as C  # noqa: E402
import dualcodec_ref as R  # noqa: E402
import fvq_geometry as fg  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
INT_SENTINEL = -0x5A5A5A5A5A5A


def _L():
    from amphion_amd import _lib

    return _lib


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return _L().current_stream_ptr(torch.device(DEV))


class Guarded:
    """a device tensor of `shape` between two runs of GUARD sentinel elements (NaN, or INT_SENTINEL for the codes); the tensor itself starts
    out as sentinels too, so a dropped store shows"""

    def __init__(self, shape, dtype=torch.float32):
        self.n = int(np.prod(shape))
        self.fill = float("nan") if dtype.is_floating_point else INT_SENTINEL
        self.buf = torch.full((self.n + 2 * GUARD,), self.fill, dtype=dtype, device=DEV)
        self.t = self.buf[GUARD:GUARD + self.n].view(*shape)

    def _is_sentinel(self, part):
        return torch.isnan(part) if self.buf.dtype.is_floating_point else part == INT_SENTINEL

    def check(self, what):
        torch.cuda.synchronize()
        for name, part in (("in front of", self.buf[:GUARD]), ("behind", self.buf[GUARD + self.n:])):
            hit = (~self._is_sentinel(part)).nonzero().flatten().tolist()
            assert not hit, f"{what}: the sentinel elements {hit[:8]} {name} the tensor were written"
        bad = self._is_sentinel(self.t).nonzero()
        assert bad.numel() == 0, f"{what}: {bad.shape[0]} of {self.n} outputs were not written; first at {bad[:4].tolist()} of {tuple(self.t.shape)}"
        return self.t


class Handle:
    """amp_fvq_create from a folded state_dict (fvq_geometry.weights); destroyed on exit"""

    def __init__(self, hp, sd):
        self.hp, self.h = hp, ctypes.c_void_p()
        args, keep = fg.create_args(fg.model_weights(sd, hp))
        _L().check(_L().lib().amp_fvq_create(hp["D"], hp["d"], hp["K"], hp["N"], int(hp["l2"]), *args, ctypes.byref(self.h)))
        del keep                                                     # the library has its own copy

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        _L().lib().amp_fvq_destroy(self.h)

    def encode_ex(self, z, T, sub=None, n=None, stride=None, what="encode_ex"):
        """amp_fvq_encode_ex on device tensors -> (codes [n, B, T], zq, all_zq, latents), every output guarded"""
        hp = self.hp
        Bn = z.shape[0]
        n = hp["N"] if n is None else n
        stride = z.shape[2] if stride is None else stride
        out = [Guarded((n, Bn, T), torch.int64), Guarded((Bn, hp["D"], T)), Guarded((n, Bn, hp["D"], T)), Guarded((Bn, n * hp["d"], T))]
        _L().check(_L().lib().amp_fvq_encode_ex(self.h, _p(z), stride, _p(sub), Bn, T, n, *[_p(g.t) for g in out], _stream()))
        return tuple(g.check(f"{what} {tag}") for g, tag in zip(out, ("codes", "zq", "all_zq", "latents")))

    def encode(self, z, n=None, what="encode"):
        """amp_fvq_encode on a contiguous device tensor -> (codes, zq, all_zq)"""
        hp = self.hp
        Bn, _, T = z.shape
        n = hp["N"] if n is None else n
        out = [Guarded((n, Bn, T), torch.int64), Guarded((Bn, hp["D"], T)), Guarded((n, Bn, hp["D"], T))]
        _L().check(_L().lib().amp_fvq_encode(self.h, _p(z), Bn, T, n, *[_p(g.t) for g in out], _stream()))
        return tuple(g.check(f"{what} {tag}") for g, tag in zip(out, ("codes", "zq", "all_zq")))

    def decode(self, codes, add=None, n=None, use_add_entry=None, what="decode"):
        n_, Bn, T = codes.shape
        n = n_ if n is None else n
        out = Guarded((Bn, self.hp["D"], T))
        L = _L().lib()
        if add is not None or use_add_entry:
            _L().check(L.amp_fvq_decode_add(self.h, _p(codes), n, Bn, T, _p(add), _p(out.t), _stream()))
        else:
            _L().check(L.amp_fvq_decode(self.h, _p(codes), n, Bn, T, _p(out.t), _stream()))
        return out.check(what)

    def flag(self):
        return _L().lib().amp_fvq_check(self.h, _stream())


def _ratio(tag, what, got, ref, which, zmax):
    """error / bound of `got` against fp64 on the frames decided at every level, under the suite's rule"""
    bound, mask = fg.restatement_bound(ref, which, zmax)
    if not bool(mask.any()):
        return 0.0
    err = float((got.cpu().double() - ref["r64"][which])[mask].abs().max())
    print(f"    {what}: err {err:.3e}, bound {bound:.3e}, ratio {err / bound:.3f}")
    assert err <= bound, (tag, what, err, bound)
    return err / bound


# ------------------------------------------------------------------------------------------------------------------------------
# every encode case at every length
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fg.ALL_ENCODE, ids=lambda c: c.name)
def test_fvq_geometry(case):
    hp = case.hp
    t_gpu = 0.0
    with Handle(hp, fg.weights(case)) as h:
        for T in case.Ts:
            tag = f"{case.id} B={fg.B} T={T}"
            ref = fg.reference(case, T)
            sd, z, r64, tau, decided = ref["sd"], ref["z"], ref["r64"], ref["tau"], ref["decided"]
            print(f"{tag}: tau {tau:.3e}, smallest fp64 margin {float(r64['margin'].min()):.3e}, undecided frames {ref['undecided']:.4f}")
            if case.margin:
                assert ref["undecided"] <= fg.UNDECIDED_CAP, "the fp64 reference itself leaves too many frames undecided for this seed"
            zmax = float(z.abs().max())
            t0 = time.perf_counter()
            zd = z.to(DEV)
            codes, zq, allq, lat = h.encode_ex(zd, T, what=tag)
            c2, q2, a2 = h.encode(zd, what=tag)
            t_gpu += time.perf_counter() - t0
            assert torch.equal(c2, codes) and torch.equal(q2, zq) and torch.equal(a2, allq), f"{tag}: the NULL forms of encode_ex are not amp_fvq_encode"
            codes_c = codes.cpu()
            assert codes.dtype == torch.int64 and int(codes_c.min()) >= 0 and int(codes_c.max()) < case.K, tag
            # ---- the margin rule: codes on decided (level, frame)s, zq and latents on the frames decided at every level ----
            if case.margin:
                same = (codes_c == r64["codes"])
                assert bool(same[decided].all()), f"{tag}: {int((~same[decided]).sum())} decided codes differ from fp64's"
                _ratio(tag, "zq", zq, ref, "zq", zmax)
                _ratio(tag, "latents", lat, ref, "latents", zmax)
            # ---- all_zq sums to zq in level order ----
            acc = torch.zeros_like(allq[0])
            for q in allq:
                acc = acc + q
            assert torch.equal(acc, zq), f"{tag}: all_zq does not sum to zq"
            # ---- every (level, frame): near-optimal in fp64 along the GPU's own trajectory ----
            excess = fg.excess_over_minimum(sd, hp, z, codes_c)
            print(f"    near-optimality: largest fp64 excess over the minimum {float(excess.max()):.3e} (tau {tau:.3e})")
            assert float(excess.max()) <= tau, f"{tag}: a chosen row is {float(excess.max()):.3e} above the fp64 minimum at (level, frame) {(excess == excess.max()).nonzero()[0].tolist()}"
            # ---- decode of the GPU's codes ----
            t0 = time.perf_counter()
            dec = h.decode(codes, what=tag + " decode")
            add = torch.randn(fg.B, case.D, T, generator=torch.Generator().manual_seed(case.seed + T)).to(DEV)
            dec_add = h.decode(codes, add, what=tag + " decode_add")
            dec_null = h.decode(codes, None, use_add_entry=True, what=tag + " decode_add(NULL)")
            t_gpu += time.perf_counter() - t0
            assert torch.equal(dec_add, dec + add) and torch.equal(dec_null, dec), f"{tag}: decode_add is not decode + add"
            assert h.flag() == 0, tag
            v64 = C.vq2emb(sd, hp, codes_c, torch.float64)
            e32 = float((C.vq2emb(sd, hp, codes_c, torch.float32).double() - v64).abs().max())
            b_dec = max(4 * e32, 1e-6 * zmax)
            err = float((dec.cpu().double() - v64).abs().max())
            b_enc = fg.restatement_bound(ref, "zq", zmax)[0]
            err_enc = float((dec - zq).abs().max())
            print(f"    decode: vs fp64 {err:.3e} (bound {b_dec:.3e}, ratio {err / b_dec:.3f}); vs encode's zq {err_enc:.3e} (bound {b_enc:.3e})")
            assert err <= b_dec and err_enc <= b_enc, tag
            # ---- for the record: the numpy model of the kernel (not a bit claim: its fma rounds twice) ----
            if case.K <= 1000:
                m = fg.fvq_model(hp, fg.model_weights(sd, hp), z.numpy())
                print(f"    model of the kernel: {int((m['codes'] != codes_c.numpy()).sum())} of {codes_c.numel()} codes differ, "
                      f"zq differs in {int((m['zq'] != zq.cpu().numpy()).sum())} of {zq.numel()} elements")
    print(f"{case.id}: {t_gpu * 1e3:.1f} ms in the library's calls and their copies")


# ------------------------------------------------------------------------------------------------------------------------------
# the folded forms, fewer levels, batch independence
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fg.PER_DP)
def test_folded_forms_are_the_separate_passes(name):
    """row stride T + 3 (the three columns past the crop hold NaN: they are never read) and sub, against crop / subtract -> amp_fvq_encode -> add"""
    case, T = fg.by_name(name), 17
    g = torch.Generator().manual_seed(case.seed + 1)
    wide = torch.full((fg.B, case.D, T + 3), float("nan"))
    wide[..., :T] = fg.latent(case, T)
    sub = torch.randn(fg.B, case.D, T, generator=g)
    wd, sd_ = wide.to(DEV), sub.to(DEV)
    with Handle(case.hp, fg.weights(case)) as h:
        codes, zq, allq, lat = h.encode_ex(wd, T, sd_, stride=T + 3, what=case.id + " folded")
        zc = (wd[..., :T] - sd_).contiguous()
        c3, q3, a3 = h.encode(zc, what=case.id + " plain")
        assert torch.equal(codes, c3) and torch.equal(zq, q3 + sd_) and torch.equal(allq, a3)
        lat3 = h.encode_ex(zc, T, what=case.id + " plain ex")[3]
        assert torch.equal(lat, lat3)
        # the stride alone, and sub alone
        c4, q4, a4, l4 = h.encode_ex(wd, T, None, stride=T + 3, what=case.id + " stride")
        c5, q5, a5 = h.encode(wd[..., :T].contiguous(), what=case.id + " crop")
        assert torch.equal(c4, c5) and torch.equal(q4, q5) and torch.equal(a4, a5)
        assert torch.isfinite(zq).all() and torch.isfinite(q4).all() and torch.isfinite(l4).all()


def test_fewer_levels_are_a_prefix():
    case, T = fg.by_name("largest_N"), 17
    zd = fg.latent(case, T).to(DEV)
    with Handle(case.hp, fg.weights(case)) as h:
        full = h.encode_ex(zd, T)
        for n in (1, case.N - 1):
            part = h.encode_ex(zd, T, n=n, what=f"n={n}")
            assert part[0].shape[0] == n and torch.equal(part[0], full[0][:n]) and torch.equal(part[2], full[2][:n])
            assert torch.equal(part[3], full[3][:, :n * case.d])
            acc = torch.zeros_like(part[1])
            for q in full[2][:n]:
                acc = acc + q
            assert torch.equal(part[1], acc)
            dec = h.decode(full[0], n=n, what=f"decode n={n}")
            assert torch.equal(dec, h.decode(full[0][:n].contiguous(), what=f"decode of {n} levels"))
        assert h.flag() == 0


@pytest.mark.parametrize("name", fg.PER_DP)
def test_batch_independence(name):
    case, T = fg.by_name(name), 17
    zd = fg.latent(case, T).to(DEV)
    with Handle(case.hp, fg.weights(case)) as h:
        full = h.encode_ex(zd, T)
        one = h.encode_ex(zd[:1].contiguous(), T)
        assert torch.equal(one[0][:, 0], full[0][:, 0]) and torch.equal(one[1][0], full[1][0]) and torch.equal(one[2][:, 0], full[2][:, 0])
        assert torch.equal(one[3][0], full[3][0])
        assert torch.equal(h.decode(one[0])[0], h.decode(full[0])[0])


# ------------------------------------------------------------------------------------------------------------------------------
# exact ties
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fg.TIES, ids=lambda c: c.name)
def test_ties_resolve_to_the_lowest_index(case):
    """every codebook row twice: distances tie exactly, within a thread's own rows or between threads (tests/fvq_geometry.py)"""
    T = case.Ts[0]
    sd, hhp, half = fg.tie_weights(case)
    zd = fg.latent(case, T).to(DEV)
    with Handle(case.hp, sd) as h:
        codes = h.encode_ex(zd, T)[0]
    assert int(codes.max()) < case.K // 2 and int(codes.min()) >= 0
    with Handle(hhp, half) as h2:
        assert torch.equal(codes, h2.encode_ex(zd, T)[0])


def test_sign_case_resolves_to_the_lowest_index():
    """d = 1 with l2: every distance is exactly 0 or 4 (tests/fvq_geometry.py), so the code is the lowest index whose sign is that of the z_e the
    kernel itself reports; fp64 along the same codes sees the same exact distances, and the reported z_e is fp64's under the latents' rule"""
    case = fg.SIGN
    T = case.Ts[0]
    sd, z = fg.weights(case), fg.latent(case, T)
    W = fg.model_weights(sd, case.hp)
    with Handle(case.hp, sd) as h:
        codes, zq, allq, lat = h.encode_ex(z.to(DEV), T)
    codes_c, lat_c = codes.cpu(), lat.cpu()
    for l in range(case.N):
        want = fg.sign_rule_codes(W["cb"][l][:, 0], lat_c[:, l, :].numpy())
        assert np.array_equal(codes_c[l].numpy(), want), l
    assert float(fg.excess_over_minimum(sd, case.hp, z, codes_c).max()) == 0.0
    r64 = C.rvq_forward(sd, case.hp, z, torch.float64, codes=codes_c)
    r32 = C.rvq_forward(sd, case.hp, z, torch.float32, codes=codes_c)
    l64 = fg.latents_of(sd, case.hp, z, r64["all_q"], torch.float64)
    e32 = float((fg.latents_of(sd, case.hp, z, r32["all_q"], torch.float32).double() - l64).abs().max())
    bound = max(4 * e32, 1e-6 * float(z.abs().max()))
    err = float((lat_c.double() - l64).abs().max())
    print(f"sign case latents: err {err:.3e}, bound {bound:.3e}")
    assert err <= bound


# ------------------------------------------------------------------------------------------------------------------------------
# the decode flag at the LDS request above 64 KB
# ------------------------------------------------------------------------------------------------------------------------------
def test_decode_flag_at_the_largest_lds_request():
    case, T = fg.DECODE_LDS, 17
    assert fg.decode_lds_bytes(case.N, case.d) > 64 * 1024
    sd = fg.weights(case)
    g = torch.Generator().manual_seed(case.seed + 2)
    codes = torch.randint(0, case.K, (case.N, fg.B, T), generator=g)
    zmax = float(fg.latent(case, T).abs().max())
    with Handle(case.hp, sd) as h:
        dec = h.decode(codes.to(DEV))
        v64 = C.vq2emb(sd, case.hp, codes, torch.float64)
        e32 = float((C.vq2emb(sd, case.hp, codes, torch.float32).double() - v64).abs().max())
        err = float((dec.cpu().double() - v64).abs().max())
        print(f"decode of random codes at n = d = 32: err {err:.3e}, fp32 restatement {e32:.3e}")
        assert err <= max(4 * e32, 1e-6 * zmax) and h.flag() == 0
        zero = codes.clone()
        zero[31, 2, 16] = 0
        want = h.decode(zero.to(DEV))
        for bad in (case.K, -1, 2 ** 40):
            c = codes.clone()
            c[31, 2, 16] = bad
            got = h.decode(c.to(DEV), what=f"decode with the code {bad}")
            assert h.flag() == fg.AMP_ERR_INVALID, bad
            assert torch.equal(got, want), bad
            assert h.flag() == 0, bad                                 # the check cleared it


# ------------------------------------------------------------------------------------------------------------------------------
# refusals at the edge of the range
# ------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    L = _L().lib()
    for (D, d, K, N), given, poison, status, word in fg.CREATE_REFUSALS:
        args, keep = fg.create_args(fg.refusal_weights(D, d, K, N, poison), given)
        h = ctypes.c_void_p()
        rc = L.amp_fvq_create(D, d, K, N, 1, *args, ctypes.byref(h))
        msg = L.amp_last_error().decode()
        assert rc == status and word in msg and not h.value, ((D, d, K, N), given, poison, rc, msg)
    case, T = fg.by_name("dp8_padded_ragged"), 17
    zd = fg.latent(case, T).to(DEV)
    sub = torch.zeros_like(zd)
    codes = torch.full((case.N + 1, fg.B, T), INT_SENTINEL, dtype=torch.int64, device=DEV)
    zq = torch.full_like(zd, float("nan"))
    with Handle(case.hp, fg.weights(case)) as h:
        def ex(z=zd, stride=T, sub_=None, n=case.N, q=zq):
            return L.amp_fvq_encode_ex(h.h, _p(z), stride, _p(sub_), fg.B, T, n, _p(codes), _p(q), None, None, _stream())

        assert ex(stride=T - 1) == fg.AMP_ERR_INVALID and b"stride" in L.amp_last_error()
        assert ex(q=zd) == fg.AMP_ERR_INVALID and b"alias" in L.amp_last_error()
        assert ex(sub_=zq) == fg.AMP_ERR_INVALID and b"alias" in L.amp_last_error()
        assert L.amp_fvq_encode(h.h, _p(zd), fg.B, T, case.N, _p(codes), _p(zd), None, _stream()) == fg.AMP_ERR_INVALID
        for n in (0, case.N + 1, -1):
            assert ex(n=n) == fg.AMP_ERR_INVALID and b"n_quantizers" in L.amp_last_error(), n
            assert L.amp_fvq_decode(h.h, _p(codes), n, fg.B, T, _p(zq), _stream()) == fg.AMP_ERR_INVALID, n
        assert L.amp_fvq_encode_ex(h.h, _p(zd), T, None, 0, T, case.N, _p(codes), _p(zq), None, None, _stream()) == fg.AMP_ERR_INVALID
        assert L.amp_fvq_encode_ex(h.h, _p(zd), T, None, fg.B, 0, case.N, _p(codes), _p(zq), None, None, _stream()) == fg.AMP_ERR_INVALID
        assert L.amp_fvq_encode_ex(h.h, None, T, None, fg.B, T, case.N, _p(codes), _p(zq), None, None, _stream()) == fg.AMP_ERR_INVALID
        assert L.amp_fvq_encode_ex(h.h, _p(zd), T, None, fg.B, T, case.N, None, _p(zq), None, None, _stream()) == fg.AMP_ERR_INVALID
        torch.cuda.synchronize()
        assert bool((codes == INT_SENTINEL).all()) and bool(torch.isnan(zq).all()), "a refused call wrote its outputs"
        assert ex(sub_=sub) == 0                                     # and the handle still serves
        torch.cuda.synchronize()
        assert bool((codes[:case.N] != INT_SENTINEL).all()) and bool(torch.isfinite(zq).all())


# ------------------------------------------------------------------------------------------------------------------------------
# amp_semantic_prepare
# ------------------------------------------------------------------------------------------------------------------------------
def _prepare(hidden, mean, std, f, what):
    """amp_semantic_prepare on CPU tensors.  hidden lies between NaN sentinels: the ABI's row stride is C itself, so a channel index at or past
    C would land in the next frame -- and, at the last frame of the last item, in the sentinels; nothing read from there may reach the output"""
    Bn, T, Cn = hidden.shape
    hg = Guarded((Bn, T, Cn))
    hg.t.copy_(hidden)
    dev = [None if t is None else t.to(DEV) for t in (mean, std)]
    out = Guarded((Bn, Cn, T // f))
    _L().check(_L().lib().amp_semantic_prepare(_p(hg.t), _p(dev[0]), _p(dev[1]), Bn, T, Cn, f, _p(out.t), _stream()))
    y = out.check(what)
    assert torch.isfinite(y).all(), what
    return y.cpu()


@pytest.mark.parametrize("stats", [True, False], ids=["normalised", "raw"])
@pytest.mark.parametrize("Bn,T,Cn,f", fg.SEMANTIC)
def test_semantic_prepare_geometry(Bn, T, Cn, f, stats):
    tag = f"semantic prepare B={Bn} T={T} C={Cn} f={f} stats={stats}"
    hidden, mean, std = R.synth_hidden(Bn, T, Cn, 700 + 10 * T + f + Cn)
    if not stats:
        mean = std = None
    hmax = float(hidden.abs().max())

    def check(m, s, what):
        ref = R.prepare_semantic_features(hidden, m, s, f, torch.float64)
        e32 = float((R.prepare_semantic_features(hidden, m, s, f, torch.float32).double() - ref).abs().max())
        bound = max(4 * e32, 1e-6 * hmax)
        y = _prepare(hidden, m, s, f, tag)
        err = float((y.double() - ref).abs().max())
        print(f"{tag} {what}: err {err:.3e}, fp32 restatement {e32:.3e}, bound {bound:.3e}, ratio {err / bound:.3f}")
        assert y.shape == (Bn, Cn, T // f) and err <= bound, (tag, what, err, bound)
        return y

    y = check(mean, std, "both" if stats else "neither")
    if stats:
        check(mean, None, "mean alone")
        check(None, std, "std alone")
    # the dropped tail frames are never read
    if T % f:
        spoiled = hidden.clone()
        spoiled[:, T - T % f:] = float("nan")
        assert torch.equal(_prepare(spoiled, mean, std, f, tag + " spoiled tail"), y)
    assert torch.equal(_prepare(hidden[:1].contiguous(), mean, std, f, tag + " B=1")[0], y[0])
