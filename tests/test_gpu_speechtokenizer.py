"""SpeechTokenizer on the MI355X (csrc/seanet.hip, csrc/lstm.hip, csrc/evq.hip and the drop-ins of amphion_amd/models/codec/speechtokenizer)
against the fp64 restatement of tests/speechtokenizer_ref.py and the golden outputs of the real reference classes.

Bounds, with e32 the fp32 restatement's own error against fp64 on the same inputs:
    exact-fp32 ops (amp_elu_pad, amp_lstm_recur, amp_evq_* tensors)                      max(4 e32, 1e-6 max|ref64|)
    anything containing f16x3 GEMMs (amp_lstm_forward, encoder, decoder, end to end)      max(4 e32, 1e-4 max|ref64|)
Quantizer codes: identical to fp64 on every DECIDED (level, frame) pair (speechtokenizer_ref.margin_rule), nothing compared elsewhere; tensors
are compared with the fp64 reference FOLLOWING the kernel's codes, so that an undecided frame does not hide the rest."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import speechtokenizer_hip as H  # noqa: E402
import speechtokenizer_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = H.DEV
GOLDEN = os.path.join(ROOT, "tests", "golden")
LSTM_T = (1, 2, 7, 33)


def bound(ref64, ref32, floor):
    return max(4.0 * float((ref32.double() - ref64).abs().max()), floor * float(ref64.abs().max()))


def check(name, got, ref64, ref32, floor):
    got = got.cpu().double()
    assert got.shape == ref64.shape, (name, got.shape, ref64.shape)
    assert torch.isfinite(got).all(), name
    err, tol = float((got - ref64).abs().max()), bound(ref64, ref32, floor)
    print(f"    {name}: error {err:.3g}, bound {tol:.3g} ({err / tol if tol else 0:.3f})")
    assert err <= tol, (name, err, tol)
    return err / tol if tol else 0.0


# ---- amp_elu_pad ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pl,pr", [(0, 0), (3, 3), (1, 1), (2, 1), (4, 3), (3, 10)])
def test_elu_pad(pl, pr):
    for T in (1, 2, 3, 4, 7, 65, 257):                       # crosses T <= max(pad) for every pad
        for C in (1, 5, 64):
            g = torch.Generator().manual_seed(1000 * pl + 100 * pr + 10 * T + C)
            x = 2.0 * torch.randn(2, C, T, generator=g)
            plain = H.elu_pad(x.to(DEV), pl, pr, False).cpu()
            assert torch.equal(plain, R.pad1d_reflect(x, pl, pr)), ("the reflect part is bit-exact", pl, pr, T, C)
            for alpha in (1.0, 0.5):
                ref64 = R.pad1d_reflect(Fn.elu(x.double(), alpha), pl, pr)
                ref32 = R.pad1d_reflect(Fn.elu(x, alpha), pl, pr)
                got = H.elu_pad(x.to(DEV), pl, pr, True, alpha).cpu().double()
                assert got.shape == ref64.shape
                err, tol = float((got - ref64).abs().max()), bound(ref64, ref32, 1e-6)
                assert err <= tol, (pl, pr, T, C, alpha, err, tol)
    # in place with zero pads: the residual block's plain ELU
    if pl == pr == 0:
        from amphion_amd import _lib
        x = torch.randn(2, 5, 7).to(DEV)
        want = H.elu_pad(x, 0, 0, True)
        _lib.check(_lib.lib().amp_elu_pad(_lib.ptr(x), 2, 5, 7, 0, 0, 1, 1.0, _lib.ptr(x), None))
        torch.cuda.synchronize()
        assert torch.equal(x, want)


def test_elu_pad_takes_any_4_byte_alignment():
    """x and y one, two and three floats off a 16-byte boundary: the 16-byte accesses are taken only where the address allows"""
    from amphion_amd import _lib

    g = torch.Generator().manual_seed(5)
    x = 2.0 * torch.randn(2, 5, 64, generator=g)
    for off_x in (1, 2, 3):
        for off_y in (0, 1):
            for pl, pr in ((0, 0), (3, 1), (4, 4)):
                bx = torch.zeros(off_x + x.numel(), device=DEV)
                xv = bx[off_x:].view(2, 5, 64)
                xv.copy_(x)
                by = torch.full((off_y + 2 * 5 * (64 + pl + pr) + 4,), float("nan"), device=DEV)
                yv = by[off_y:off_y + 2 * 5 * (64 + pl + pr)].view(2, 5, 64 + pl + pr)
                assert xv.data_ptr() % 16 == 4 * off_x and yv.data_ptr() % 16 == 4 * off_y
                _lib.check(_lib.lib().amp_elu_pad(_lib.ptr(xv), 2, 5, 64, pl, pr, 0, 1.0, _lib.ptr(yv), None))
                torch.cuda.synchronize()
                assert torch.equal(yv.cpu(), R.pad1d_reflect(x, pl, pr)), (off_x, off_y, pl, pr)
                assert bool(torch.isnan(by[off_y + yv.numel():]).all()) and bool(torch.isnan(by[:off_y]).all())


def test_lstm_recur_refuses_an_unaligned_workspace():
    from amphion_amd import _lib

    w, gx, _ = recur_case(8, False, 2, 1, 3)
    m = H.Lstm(8, 8, 1, False, False, *w)
    ws = torch.zeros(256, device=DEV)
    y = torch.zeros(1, 8, 2, device=DEV)
    gxd = gx.to(DEV)
    L = _lib.lib()
    assert L.amp_lstm_recur(m.h, 0, _lib.ptr(gxd), 1, 2, None, _lib.ptr(y), _lib.ptr(ws[1:]), None) == _lib.AMP_ERR_INVALID
    assert b"16-byte aligned" in L.amp_last_error()
    assert L.amp_lstm_recur(m.h, 1, _lib.ptr(gxd), 1, 2, None, _lib.ptr(y), _lib.ptr(ws), None) == _lib.AMP_ERR_INVALID      # layer 1 of 1
    assert L.amp_lstm_recur(m.h, 0, _lib.ptr(gxd), 1, 2, None, _lib.ptr(y), _lib.ptr(ws), None) == 0
    torch.cuda.synchronize()


# ---- amp_lstm_recur ------------------------------------------------------------------------------------------------------------------
def lstm_weights(In, Hn, layers, bidir, seed, same_dirs=False):
    """nn.LSTM's four lists at U(+-1/sqrt(H)); same_dirs: the reverse direction gets the forward direction's weights"""
    g = torch.Generator().manual_seed(seed)
    ndir = 2 if bidir else 1
    out = [[], [], [], []]
    for layer in range(layers):
        cin = In if layer == 0 else ndir * Hn
        for d in range(ndir):
            if d and same_dirs:
                for lst in out:
                    lst.append(lst[-1].clone())
                continue
            for lst, shape in zip(out, ((4 * Hn, cin), (4 * Hn, Hn), (4 * Hn,), (4 * Hn,))):
                lst.append((2 * torch.rand(shape, generator=g) - 1) / Hn ** 0.5)
    return out


def recur_case(Hn, bidir, T, B, seed, same_dirs=False):
    ndir = 2 if bidir else 1
    w = lstm_weights(Hn, Hn, 1, bidir, seed, same_dirs)
    g = torch.Generator().manual_seed(seed + 1)
    gx = torch.randn(B, ndir * 4 * Hn, T, generator=g)
    skip = torch.randn(B, Hn, T, generator=g)
    return w, gx, skip


@pytest.mark.parametrize("bidir", [False, True])
@pytest.mark.parametrize("Hn", [5, 20, 32, 96])
def test_lstm_recur_vs_fp64(Hn, bidir):
    w, _, _ = recur_case(Hn, bidir, 1, 1, 40 + Hn)
    m = H.Lstm(Hn, Hn, 1, bidir, False, *w)
    w_hh = torch.stack(w[1], 0)
    worst = 0.0
    for T in LSTM_T:
        _, gx, skip = recur_case(Hn, bidir, T, 3, 1000 * Hn + T)
        for sk in (None, skip):
            ref64 = R.lstm_recur(w_hh.double(), gx.double(), None if sk is None else sk.double())
            ref32 = R.lstm_recur(w_hh, gx, sk)
            y = m.recur(0, gx.to(DEV), None if sk is None else sk.to(DEV))
            worst = max(worst, check(f"recur H={Hn} bidir={bidir} T={T} skip={sk is not None}", y, ref64, ref32, 1e-6))
            for b in range(3):                               # each item bit-equal to its B = 1 run
                y1 = m.recur(0, gx[b:b + 1].contiguous().to(DEV), None if sk is None else sk[b:b + 1].contiguous().to(DEV))
                assert torch.equal(y1[0], y[b]), (Hn, bidir, T, b)
    print(f"lstm recur H={Hn} bidir={bidir}: worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("Hn", [5, 96])
def test_lstm_reverse_direction_at_one_step_is_the_forward_direction(Hn):
    w, _, _ = recur_case(Hn, True, 1, 2, 7 + Hn, same_dirs=True)
    m = H.Lstm(Hn, Hn, 1, True, False, *w)
    g = torch.Generator().manual_seed(Hn)
    half = torch.randn(2, 4 * Hn, 1, generator=g)
    y = m.recur(0, torch.cat([half, half], 1).to(DEV))
    assert torch.equal(y[:, :Hn], y[:, Hn:])
    # and over more steps the reverse direction is the forward direction of the time-flipped input
    half = torch.randn(2, 4 * Hn, 7, generator=g)
    y = m.recur(0, torch.cat([half, half.flip(2)], 1).contiguous().to(DEV))
    assert torch.equal(y[:, :Hn], y[:, Hn:].flip(2))


@pytest.mark.parametrize("B", [5, 8, 9, 17])
def test_lstm_recur_batch_tiles(B):
    """the kernel walks the batch in tiles of 1, 4, 8 or 16 items by B: every tile width, a full tile and a tail, H with and without 16-byte rows"""
    for Hn in (20, 70):
        w, gx, skip = recur_case(Hn, True, 7, B, 500 + Hn + B)
        m = H.Lstm(Hn, Hn, 1, True, False, *w)
        w_hh = torch.stack(w[1], 0)
        y = m.recur(0, gx.to(DEV), skip.to(DEV))
        check(f"recur H={Hn} B={B}", y, R.lstm_recur(w_hh.double(), gx.double(), skip.double()), R.lstm_recur(w_hh, gx, skip), 1e-6)
        for b in (0, B - 1):
            y1 = m.recur(0, gx[b:b + 1].contiguous().to(DEV), skip[b:b + 1].contiguous().to(DEV))
            assert torch.equal(y1[0], y[b]), (Hn, B, b)


def test_lstm_recur_recipe_grid():
    """H = 1024, bidirectional: the grid and the 16-byte weight loads of the public recipe"""
    Hn = 1024
    w, gx, skip = recur_case(Hn, True, 3, 2, 99)
    m = H.Lstm(Hn, Hn, 1, True, False, *w)
    w_hh = torch.stack(w[1], 0)
    y = m.recur(0, gx.to(DEV), skip.to(DEV))
    check("recur H=1024 bidir T=3 B=2", y, R.lstm_recur(w_hh.double(), gx.double(), skip.double()), R.lstm_recur(w_hh, gx, skip), 1e-6)
    y1 = m.recur(0, gx[1:2].contiguous().to(DEV), skip[1:2].contiguous().to(DEV))
    assert torch.equal(y1[0], y[1])


# ---- amp_lstm_forward ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layers,bidir", [(1, False), (1, True), (2, False), (2, True)])
@pytest.mark.parametrize("Hn", [20, 96])
def test_lstm_forward_vs_fp64(conv_precision, Hn, layers, bidir):
    """SLSTM in the conv layout, skip folded in; layer 1 of a bidirectional stack reads 2H channels"""
    from amphion_amd import _lib

    w = lstm_weights(Hn, Hn, layers, bidir, 300 + Hn + layers)
    m = H.Lstm(Hn, Hn, layers, bidir, True, *w)
    ndir = 2 if bidir else 1
    P = {}
    for layer in range(layers):
        for d in range(ndir):
            sfx = f"_l{layer}" + ("_reverse" if d else "")
            for name, lst in zip(("weight_ih", "weight_hh", "bias_ih", "bias_hh"), w):
                P[name + sfx] = lst[layer * ndir + d]
    P64 = {k: v.double() for k, v in P.items()}
    worst = 0.0
    for T in LSTM_T:
        g = torch.Generator().manual_seed(10 * Hn + T)
        x = torch.randn(3, Hn, T, generator=g)
        ref64, ref32 = R.slstm(P64, "", x.double(), layers, bidir), R.slstm(P, "", x, layers, bidir)
        y = m.forward(x.to(DEV))
        worst = max(worst, check(f"lstm H={Hn} L={layers} bidir={bidir} T={T} [{conv_precision}]", y, ref64, ref32, 1e-4))
        for b in (0, 2):
            assert torch.equal(m.forward(x[b:b + 1].contiguous().to(DEV))[0], y[b]), (Hn, layers, bidir, T, b)
    _lib.range_check(DEV)
    print(f"lstm forward H={Hn} L={layers} bidir={bidir} [{conv_precision}]: worst error / bound = {worst:.3f}")


# ---- amp_evq_* -----------------------------------------------------------------------------------------------------------------------
def check_evq(q, cbs, z, st, n_q, name):
    r64, _, tau, decided = R.margin_rule(cbs, z, st, n_q)
    codes, zq, allq = q.encode(z.to(DEV), st, n_q)
    codes_h = codes.cpu()
    assert int(codes_h.min()) >= 0 and int(codes_h.max()) < q.K
    same = codes_h == r64["codes"]
    assert bool(same[decided].all()), (name, int((~same & decided).sum()))
    undecided = 1.0 - float(decided[-1].double().mean())
    assert undecided <= 0.05, (name, undecided)
    # tensors: the fp64 / fp32 restatements following the kernel's codes
    f64 = R.evq_forward(cbs, z, torch.float64, st, n_q, codes=codes_h)
    f32 = R.evq_forward(cbs, z, torch.float32, st, n_q, codes=codes_h)
    check(f"{name} zq", zq, f64["zq"], f32["zq"], 1e-6)
    check(f"{name} all_zq", allq, f64["all_q"], f32["all_q"], 1e-6)
    out = q.decode(codes, st)
    assert q.check() == 0
    check(f"{name} decode", out, R.evq_decode(cbs, codes_h, torch.float64, st), R.evq_decode(cbs, codes_h, torch.float32, st), 1e-6)
    print(f"{name}: tau = {tau:.3g}, undecided at the last level {100 * undecided:.2f} %, codes off fp64 on undecided pairs: {int((~same).sum())}")
    return codes


@pytest.mark.parametrize("D,K,N", [(8, 5, 4), (32, 64, 8), (1024, 1024, 8)])
def test_evq_vs_fp64(D, K, N):
    q = None
    for T in (1, 31, 33, 65):
        cbs, z = R.quantizer_case(D, K, N, T)
        q = H.Evq(cbs)
        codes = check_evq(q, cbs, z, 0, N, f"evq D={D} K={K} N={N} T={T}")
        # a frame never depends on what it is batched with
        c1, zq1, _ = q.encode(z[1:2].contiguous().to(DEV), 0, N)
        assert torch.equal(c1[:, 0], codes[:, 1])
    cbs, z = R.quantizer_case(D, K, N, 33, s=0.05)
    check_evq(H.Evq(cbs), cbs, z, 0, N, f"evq D={D} K={K} N={N} T=33 s=0.05")
    # st = 1 starts level 1 from the whole input; n_q < N stops early
    cbs, z = R.quantizer_case(D, K, N, 33)
    q = H.Evq(cbs)
    c_st = check_evq(q, cbs, z, 1, N, f"evq D={D} K={K} N={N} st=1")
    c_full = check_evq(q, cbs, z, 0, N - 1, f"evq D={D} K={K} N={N} n_q={N - 1}")
    assert tuple(c_st.shape) == (N - 1, 2, 33) and not torch.equal(c_st, c_full)


def test_evq_equal_rows_return_the_lower_index():
    cbs, z = R.quantizer_case(32, 64, 2, 33)
    cbs[0][41] = cbs[0][9]
    cbs[0][63] = cbs[0][62]
    z[0, :, 5] = cbs[0][41]
    z[1, :, 32] = cbs[0][63] * 1.01
    codes, _, _ = H.Evq(cbs).encode(z.to(DEV), 0, 2)
    assert int(codes[0, 0, 5]) == 9 and int(codes[0, 1, 32]) == 62


def test_evq_equal_rows_across_waves_and_passes():
    """K = 1024: rows 4 kp + 256 pass + u belong to wave kp // 16.  Equal rows in two waves of one pass (40 | 100), in two passes (9 | 700) and in
    one thread's two passes (13 | 269): the tie goes through the shuffle tree, the LDS stage of the four waves and the ascending scan"""
    cbs, z = R.quantizer_case(32, 1024, 1, 33)
    pairs = ((40, 100), (9, 700), (13, 269), (1023, 5))
    for i, (a, b) in enumerate(pairs):
        cbs[0][max(a, b)] = cbs[0][min(a, b)]
        z[i % 2, :, 3 + 7 * i] = cbs[0][a] * (1.0 + 0.01 * i)
    codes, _, _ = H.Evq(cbs).encode(z.to(DEV), 0, 1)
    for i, (a, b) in enumerate(pairs):
        assert int(codes[0, i % 2, 3 + 7 * i]) == min(a, b), (a, b, int(codes[0, i % 2, 3 + 7 * i]))
    r64 = R.evq_forward(cbs, z, torch.float64)
    assert all(int(r64["codes"][0, i % 2, 3 + 7 * i]) == min(a, b) for i, (a, b) in enumerate(pairs))


def test_evq_level_range_is_judged_by_the_library():
    """0 <= st < n_q <= N and st + n <= N at the C entry points themselves (the Python drop-in raises before it gets there)"""
    from amphion_amd import _lib

    L, p = _lib.lib(), _lib.ptr
    cbs, z = R.quantizer_case(8, 5, 4, 7)
    q = H.Evq(cbs)
    zd = z.to(DEV)
    codes = torch.zeros((4, 2, 7), dtype=torch.int64, device=DEV)
    out = torch.zeros((2, 8, 7), device=DEV)
    for st, n_q in ((2, 2), (3, 2), (-1, 2), (0, 5), (4, 5), (0, 0)):
        assert L.amp_evq_encode(q.h, p(zd), 2, 7, st, n_q, p(codes), None, None, None) == _lib.AMP_ERR_INVALID, (st, n_q)
        assert b"amp_evq_encode: levels" in L.amp_last_error()
    for n, st in ((0, 0), (5, 0), (2, 3), (1, 4), (1, -1)):
        assert L.amp_evq_decode(q.h, p(codes), n, st, 2, 7, p(out), None) == _lib.AMP_ERR_INVALID, (n, st)
    assert L.amp_evq_encode(q.h, p(zd), 2, 7, 3, 4, p(codes), None, None, None) == 0 and L.amp_evq_decode(q.h, p(codes), 1, 3, 2, 7, p(out), None) == 0
    torch.cuda.synchronize()
    assert q.check() == 0


def test_evq_out_of_range_code_sets_the_flag():
    from amphion_amd import _lib

    cbs, z = R.quantizer_case(32, 64, 3, 7)
    q = H.Evq(cbs)
    codes = torch.randint(0, 64, (3, 2, 7))
    bad = codes.clone()
    bad[1, 0, 3], bad[2, 1, 6] = 64, -1
    out = q.decode(bad.to(DEV), 0)
    assert q.check() == _lib.AMP_ERR_INVALID and b"outside" in _lib.lib().amp_last_error()
    row0 = bad.clone()
    row0[1, 0, 3], row0[2, 1, 6] = 0, 0
    assert torch.equal(out, q.decode(row0.to(DEV), 0))
    assert q.check() == 0                                         # the check cleared the flag
    q.decode(codes.to(DEV), 0)
    assert q.check() == 0
    from amphion_amd.models.codec.speechtokenizer.modules.quantization import ResidualVectorQuantizer
    m = ResidualVectorQuantizer(dimension=32, n_q=3, bins=64)
    for i, c in enumerate(cbs):
        m.vq.layers[i]._codebook.embed.copy_(c)
        m.vq.layers[i]._codebook.inited.fill_(1.0)
    m = m.to(DEV).eval()
    with pytest.raises(_lib.AmpError):
        m.decode(bad.to(DEV))
    assert torch.equal(m.decode(codes.to(DEV)), q.decode(codes.to(DEV), 0))


# ---- the model -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "golden_speechtokenizer.npz"))


@pytest.fixture(scope="module")
def small(gold):
    hp = R.small_hp()
    return hp, R.synth_state_dict(hp, int(gold["seed"]))


def build(hp, sd):
    from amphion_amd.models.codec.speechtokenizer import SpeechTokenizer

    m = SpeechTokenizer(hp)
    m.load_state_dict(sd)
    return m.to(DEV).eval()


def near_gold(name, got, g, ref64, ref32, floor):
    """the golden tensor is the reference's own fp32 evaluation: it may sit its own rounding away from fp64"""
    got, g = got.cpu().double(), torch.from_numpy(g).double()
    tol = bound(ref64, ref32, floor) + float((g - ref64).abs().max())
    assert float((got - g).abs().max()) <= tol, (name, float((got - g).abs().max()), tol)


@pytest.mark.parametrize("n", [47, 48, 49, 480])
def test_small_model_vs_fp64_and_golden(conv_precision, gold, small, n):
    from amphion_amd import _lib

    hp, sd = small
    m = build(hp, sd)
    cbs = R.codebooks_of(sd, hp)
    x = torch.from_numpy(gold[f"x_{n}"])
    tag = f"n={n} [{conv_precision}]"
    # encoder
    e = m.encoder(x.to(DEV))
    e64, e32 = R.encoder_forward(sd, hp, x, torch.float64), R.encoder_forward(sd, hp, x, torch.float32)
    check(f"encoder {tag}", e, e64, e32, 1e-4)
    near_gold("latent", e, gold[f"z_{n}"], e64, e32, 1e-4)
    # quantizer, from the HIP latent
    codes = m.encode(x.to(DEV))
    eh = e.cpu()
    r64, _, tau, decided = R.margin_rule(cbs, eh)
    assert bool((codes.cpu() == r64["codes"])[decided].all())
    # against the golden codes: a pair counts when its fp64 margin also covers the latent's distance from the reference's, which moves a
    # difference of two distances by at most 2 |delta|_2 |e_k - e_j|_2 <= 4 |delta|_2 max_k |e_k|_2 at every level
    delta = (eh.double() - torch.from_numpy(gold[f"z_{n}"]).double()).norm(dim=1)                      # [B, T]
    slack = tau + 4.0 * delta * max(float(c.double().norm(dim=1).max()) for c in cbs)
    g64 = R.evq_forward(cbs, torch.from_numpy(gold[f"z_{n}"]), torch.float64)
    sure = torch.cumprod((g64["margin"] > slack[None]).to(torch.int64), dim=0).bool()
    gcodes = torch.from_numpy(gold[f"codes_{n}"]).long()
    assert bool((codes.cpu() == gcodes)[sure].all())
    print(f"    codes {tag}: {int(sure.sum())} of {sure.numel()} pairs compared with the golden codes, {int((codes.cpu() != gcodes).sum())} differ")
    assert torch.equal(m.encode(x.to(DEV), st=1), m.quantizer.encode(e, st=1)) and m.encode(x.to(DEV), n_q=2).shape[0] == 2
    # decode, from the golden codes
    w = m.decode(gcodes.to(DEV))
    w64, w32 = R.model_decode(sd, hp, gcodes, torch.float64), R.model_decode(sd, hp, gcodes, torch.float32)
    check(f"decode {tag}", w, w64, w32, 1e-4)
    near_gold("decode", w, gold[f"dec_{n}"], w64, w32, 1e-4)
    # forward: every stage against fp64 run from the HIP stage before it
    o, commit, feat = m(x.to(DEV))
    assert commit.shape == () and float(commit) == 0.0
    hc = codes.cpu()
    f64, f32 = R.evq_forward(cbs, eh, torch.float64, codes=hc), R.evq_forward(cbs, eh, torch.float32, codes=hc)
    qh = m.quantizer.decode(codes)
    check(f"quantized {tag}", qh, f64["zq"], f32["zq"], 1e-6)
    check(f"feature {tag}", feat, R.feature(sd, f64["all_q"][0], torch.float64), R.feature(sd, f32["all_q"][0], torch.float32), 1e-4)
    check(f"decoder {tag}", o, R.decoder_forward(sd, hp, qh.cpu(), torch.float64), R.decoder_forward(sd, hp, qh.cpu(), torch.float32), 1e-4)
    assert tuple(o.shape) == (2, 1, -(-n // 48) * 48) and tuple(feat.shape) == (2, -(-n // 48), 24)
    # forward against the golden file: made whenever the device walked the golden codes -- and it must have, where every pair is sure
    if bool(sure.all()):
        assert torch.equal(hc, gcodes)
    if not torch.equal(hc, gcodes):
        pytest.fail(f"forward {tag}: {int((hc != gcodes).sum())} codes off the golden ones on pairs the margin leaves open: the golden "
                    "forward / feature comparison cannot be made for this input")
    e2e64, e2e32 = R.model_forward(sd, hp, x, torch.float64), R.model_forward(sd, hp, x, torch.float32)
    assert torch.equal(e2e64["codes"], gcodes)
    near_gold("forward", o, gold[f"fwd_o_{n}"], e2e64["o"], e2e32["o"], 1e-4)
    near_gold("feature", feat, gold[f"fwd_feat_{n}"], e2e64["feature"], e2e32["feature"], 1e-4)
    fl = m.forward_feature(x.to(DEV))
    assert len(fl) == hp["n_q"]
    check(f"forward_feature {tag}", torch.stack(fl), f64["all_q"], f32["all_q"], 1e-6)
    _lib.range_check(DEV)


@pytest.mark.parametrize("which", ["encoder", "decoder"])
def test_stack_with_two_residual_layers_and_true_skip(conv_precision, which):
    """routes the model configurations never take: a dilated residual conv (reflect staging with pads 2, 2) and true_skip (res = x)"""
    from amphion_amd import _lib
    from amphion_amd.models.codec.speechtokenizer.modules import SEANetDecoder, SEANetEncoder

    hp = R.stack_hp()
    sd = R.synth_stack_state_dict(hp, which, 3)
    m = (SEANetEncoder if which == "encoder" else SEANetDecoder)(dimension=16, n_filters=8, n_residual_layers=2, ratios=[3, 2], lstm=1,
                                                                   true_skip=True, dilation_base=2)
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    for T in (1, 2, 5, 37):                                  # T <= 2 crosses the small-input rule of the dilated conv's pads
        g = torch.Generator().manual_seed(T)
        x = torch.randn(2, 1 if which == "encoder" else 16, T, generator=g)
        y = m(x.to(DEV))
        check(f"{which} stack T={T} [{conv_precision}]", y, R.stack_forward(sd, hp, which, x, torch.float64),
              R.stack_forward(sd, hp, which, x, torch.float32), 1e-4)
    _lib.range_check(DEV)


def test_one_sample_input(gold, small):
    hp, sd = small
    m = build(hp, sd)
    x = torch.from_numpy(gold["x_1"])
    e = m.encoder(x.to(DEV))
    check("encoder n=1", e, R.encoder_forward(sd, hp, x, torch.float64), R.encoder_forward(sd, hp, x, torch.float32), 1e-4)


def test_recipe_frame_counts():
    """319 / 320 / 321 samples are 1 / 1 / 2 frames at the public recipe; the last one against fp64"""
    hp = R.recipe_hp()
    sd = R.synth_state_dict(hp, 5)
    m = build(hp, sd)
    for n, frames in ((319, 1), (320, 1), (321, 2)):
        x = R.synth_wave(1, n, n)
        e = m.encoder(x.to(DEV))
        assert tuple(e.shape) == (1, 1024, frames)
        codes = m.encode(x.to(DEV))
        assert tuple(codes.shape) == (8, 1, frames) and tuple(m.decode(codes).shape) == (1, 1, 320 * frames)
    check("recipe encoder n=321", e, R.encoder_forward(sd, hp, x, torch.float64), R.encoder_forward(sd, hp, x, torch.float32), 1e-4)
    qh = m.quantizer.decode(codes)
    check("recipe decoder n=321", m.decoder(qh), R.decoder_forward(sd, hp, qh.cpu(), torch.float64),
          R.decoder_forward(sd, hp, qh.cpu(), torch.float32), 1e-4)


def test_state_dict_round_trip_and_refusals(small):
    from amphion_amd.models.codec.speechtokenizer import SpeechTokenizer

    hp, sd = small
    m = build(hp, sd)
    back = m.state_dict()
    assert list(back) == list(sd) and all(torch.equal(back[k].cpu(), sd[k]) for k in sd)
    m2 = SpeechTokenizer(hp)
    m2.load_state_dict({k: v.cpu() for k, v in back.items()})
    m2 = m2.to(DEV).eval()
    x = R.synth_wave(2, 100, 3).to(DEV)
    assert torch.equal(m2.encode(x), m.encode(x))
    m.train()
    for call in (lambda: m(x), lambda: m.encode(x), lambda: m.decode(torch.zeros(4, 2, 3, dtype=torch.int64, device=DEV))):
        with pytest.raises(NotImplementedError):
            call()
    m.eval()
    with pytest.raises(RuntimeError):
        m.encode(x.cpu())
    with pytest.raises(ValueError):
        m.encode(x, st=4)
