"""The geometry tables of the tokenizer kernels of include/amphion_hip.h -- amp_evq_* (csrc/evq.hip: D <= 1024, K <= 4096, N <= 32), amp_lstm_*
(csrc/lstm.hip: hidden <= 1024, input_size <= 2048, num_layers <= 4), amp_dsconv_* and amp_gelu (csrc/dsconv_f16x3.hip) and amp_elu_pad
(csrc/seanet.hip) -- where every other case of the suite sits at a model's shapes.  Plain data and pure numpy / torch-CPU functions, no GPU and
nothing of the package: tests/test_tokenizer_geometry_ref.py checks the tables on the CPU, tests/test_gpu_tokenizer_geometry.py runs every case
through the C ABI.

evq_model() and lstm_model() restate evq_encode_kernel and lstm_step_kernel in numpy fp32, operation by operation: the thread-to-row and
lane-to-column maps, the fmaf chains and their order, the scans, the shuffle trees.  A fused multiply-add is emulated as one fp64 product (exact:
24 + 24 bits) and one fp64 sum rounded to fp32 -- two roundings where the hardware has one, so a model claims "the suite's rules hold", not bit
equality.  The `mutant` argument applies ONE slip of the kernel's text; the CPU tests show that the tables catch each of them."""
from dataclasses import dataclass

import numpy as np

import speechtokenizer_ref as R

B = 3
UNDECIDED_CAP = 0.02                             # the cap of tests/fvq_geometry.py
DEVICE_TENSOR_CAP = 1 << 20                      # tests/fvq_geometry.py: DEVICE_TENSOR_CAP, for the reason written there
EVQ_TF = 16                                      # frames per workgroup of both evq kernels
f32 = np.float32


def fma(a, b, c):
    """fmaf on fp32 arrays: the product is exact in fp64, the sum is rounded to fp64 and then to fp32"""
    return (np.asarray(a, f32).astype(np.float64) * np.asarray(b, f32).astype(np.float64) + np.asarray(c, f32).astype(np.float64)).astype(f32)


# ------------------------------------------------------------------------------------------------------------------------------
# amp_evq
# ------------------------------------------------------------------------------------------------------------------------------
EVQ_LENGTHS = (1, 16, 17, 50)                    # one frame; exactly one tile; a second tile with one frame; four tiles, the last with 2
EVQ_SHORT = (1, 16, 17, 35)                      # where all_zq at T = 50 would pass DEVICE_TENSOR_CAP: three tiles, the last with 3 frames


@dataclass(frozen=True)
class Evq:
    D: int
    K: int
    N: int
    decay: bool = True                           # speechtokenizer_ref.synth_codebooks' 0.6^level; False: every level randn (N = 32)
    Ts: tuple = EVQ_LENGTHS

    @property
    def id(self):
        return f"D{self.D}K{self.K}N{self.N}"

    @property
    def DP(self):
        return (self.D + 3) & ~3

    @property
    def padded(self):
        return self.D < self.DP


EVQ = [
    Evq(1, 1, 1), Evq(3, 5, 2), Evq(5, 7, 3), Evq(7, 3, 2), Evq(6, 1, 3), Evq(13, 37, 4), Evq(30, 257, 3), Evq(130, 129, 4),
    Evq(1022, 33, 2, Ts=EVQ_SHORT), Evq(1023, 16, 2, Ts=EVQ_SHORT), Evq(1024, 4096, 1), Evq(16, 4096, 2), Evq(18, 4095, 2),
    Evq(257, 1000, 8, Ts=EVQ_SHORT), Evq(6, 260, 2),
    Evq(8, 16, 32, decay=False), Evq(5, 33, 32, decay=False),
]
# exact ties, every codebook row twice (rows K/2 .. copy rows 0 .. K/2 - 1).  Row k belongs to thread kp = (k % 256) / 4, pass k / 256
EVQ_TIES = [Evq(5, 10, 2, Ts=(17,)),             # 5 apart: the neighbouring threads of one wave, one pass
            Evq(6, 520, 2, Ts=(17,)),            # 260 apart: the next thread, the next pass
            Evq(130, 64, 2, Ts=(17,)),           # 32 apart: threads 8 apart in one wave
            Evq(5, 1024, 1, Ts=(17,)),           # 512 apart: the same thread two passes on (the scan's strict <)
            Evq(5, 4, 2, Ts=(17,)),              # 2 apart: the same thread, the same pass
            Evq(5, 256, 1, Ts=(17,))]            # 128 apart: threads 32 apart, so two waves apart (the LDS stage)


def evq_tie_relation(case):
    """where a row's copy K/2 further on lives: the set of "thread" | "wave" | "waves" over the rows k < K/2"""
    h, out = case.K // 2, set()
    for k in range(h):
        a, b = (k % 256) // 4, ((k + h) % 256) // 4
        out.add("thread" if a == b else "wave" if a // 16 == b // 16 else "waves")
    return out
EVQ_FLAG = Evq(1023, 16, 2, Ts=(17,))            # the decode flag where the channel loop takes four passes over a padded row


def evq_by_id(name):
    return next(c for c in EVQ + EVQ_TIES if c.id == name)


def evq_inputs(case, T, batch=B):
    """-> (codebooks [N] x [K, D], z [batch, D, T])"""
    import torch

    if case.decay:
        return R.quantizer_case(case.D, case.K, case.N, T, B=batch)
    seed = 7000 + 131 * case.D + 17 * case.K + T
    g = torch.Generator().manual_seed(seed)
    cbs = [torch.randn(case.K, case.D, generator=g).float() for _ in range(case.N)]
    return cbs, torch.randn(batch, case.D, T, generator=torch.Generator().manual_seed(seed + 1)).float()


def evq_tie_inputs(case, T):
    """-> (codebooks with rows K/2 .. equal to rows 0 .. K/2 - 1, their first halves, z)"""
    cbs, z = evq_inputs(case, T)
    h = case.K // 2
    assert 2 * h == case.K
    full = []
    for c in cbs:
        c = c.clone()
        c[h:] = c[:h]
        full.append(c)
    return full, [c[:h].contiguous() for c in full], z


_EVQ_REF = {}


def evq_reference(case, T, st=0, n_q=None):
    """speechtokenizer_ref.margin_rule of (case, T) on levels [st, n_q), computed once and left unchanged"""
    key = (case, T, st, n_q)
    if key not in _EVQ_REF:
        cbs, z = evq_inputs(case, T)
        r64, _, tau, decided = R.margin_rule(cbs, z, st, n_q)
        _EVQ_REF[key] = dict(cbs=cbs, z=z, r64=r64, tau=tau, decided=decided, undecided=1.0 - float(decided[-1].double().mean()), st=st,
                             n_q=case.N if n_q is None else n_q)
    return _EVQ_REF[key]


def evq_excess(cbs, z, codes, st=0):
    """walk fp64 along `codes` [n, B, T]: at every (level, frame), the fp64 distance of the chosen row above the fp64 minimum -> [n, B * T]"""
    import torch

    f64 = R.evq_forward(cbs, z, torch.float64, st, st + codes.shape[0], codes=codes)
    return torch.stack([d.max(1).values - d.gather(1, c.reshape(-1, 1)).squeeze(1) for d, c in zip(f64["dist"], codes)])   # dist: larger is closer


def evq_rule_failures(ref, out):
    """what the GPU test asserts of an encode, applied to `out` = dict(codes [n, B, T] int64 numpy, zq, all_zq numpy) -> the rules broken"""
    import torch

    cbs, z, st, n_q = ref["cbs"], ref["z"], ref["st"], ref["n_q"]
    K = cbs[0].shape[0]
    codes = torch.from_numpy(np.ascontiguousarray(out["codes"]))
    if int(codes.min()) < 0 or int(codes.max()) >= K:
        return ["code range"]
    bad = []
    if not bool((codes == ref["r64"]["codes"])[ref["decided"]].all()):
        bad.append("codes")
    if not float(evq_excess(cbs, z, codes, st).max()) <= ref["tau"]:
        bad.append("near-optimality")
    f64 = R.evq_forward(cbs, z, torch.float64, st, n_q, codes=codes)
    f32_ = R.evq_forward(cbs, z, torch.float32, st, n_q, codes=codes)
    for key, name in (("zq", "zq"), ("all_q", "all_zq")):
        got = torch.from_numpy(np.ascontiguousarray(out[name])).double()
        bound = max(4.0 * float((f32_[key].double() - f64[key]).abs().max()), 1e-6 * float(f64[key].abs().max()))
        if not float((got - f64[key]).abs().max()) <= bound:            # (a NaN fails)
            bad.append(name)
    acc = np.zeros_like(out["all_zq"][0])
    for q in out["all_zq"]:
        acc = (acc + q).astype(f32)
    if not np.array_equal(acc, out["zq"]):
        bad.append("all_zq does not sum to zq")
    return bad


# pad_not_zeroed        the residual's columns D .. DP - 1 keep what LDS held
# scan_le               `dist <= best` in a thread's scan
# merge_prefers_higher  the shuffle tree and the wave stage take the higher index on equal distances
# guard_dropped         `if (k0 + u < K)` gone: the clamped row K - 1 is scored again under the indices K .. with sum e^2 read past the level
# update_stride_D       the residual update runs to DP and reads its row at code * D, the host's unpadded stride
# st_from_residual      level st starts from the residual the levels before it leave, not from the whole input
EVQ_MUTANTS = ("pad_not_zeroed", "scan_le", "merge_prefers_higher", "guard_dropped", "update_stride_D", "st_from_residual")


def _merge(a, b, higher):
    """`if (ob < best || (ob == best && oi < bi)) take the other`: a = (best, bi) of this lane, b of the other"""
    take = (b[0] < a[0]) | ((b[0] == a[0]) & ((b[1] > a[1]) if higher else (b[1] < a[1])))
    return np.where(take, b[0], a[0]), np.where(take, b[1], a[1])


def evq_model(cbs, z, st=0, n_q=None, mutant=None):
    """evq_encode_kernel on z [B, D, T] (numpy fp32), codebooks [N][K, D] -> dict(codes [n, B, T] int64, zq [B, D, T], all_zq [n, B, D, T]).
    Frames are independent in the kernel, so they are walked together."""
    assert mutant is None or mutant in EVQ_MUTANTS
    cbs = [np.asarray(c, f32) for c in cbs]
    N, (K, D) = len(cbs), cbs[0].shape
    n_q = N if n_q is None else n_q
    DP = (D + 3) & ~3
    Bn, _, T = z.shape
    F = Bn * T
    # amp_evq_create: rows zero-padded to DP floats, sum e^2 as one fmaf chain over D.  Flat, with a level of zeros behind the last one: what a
    # read past row K - 1 of the last level finds is anything; zeros are as good
    cb = np.zeros((N + 1, K, DP), f32)
    cn2 = np.zeros((N + 1, K), f32)
    for l in range(N):
        cb[l, :, :D] = cbs[l]
        s = np.zeros(K, f32)
        for j in range(D):
            s = fma(cbs[l][:, j], cbs[l][:, j], s)
        cn2[l] = s
    cb_flat, cn2_flat = cb.reshape(-1), cn2.reshape(-1)
    Rz = np.full((F, DP), np.nan if mutant == "pad_not_zeroed" else 0.0, f32)      # what LDS held before is anything: NaN is the value that tells
    Rz[:, :D] = np.transpose(np.asarray(z, f32), (0, 2, 1)).reshape(F, D)
    Q = np.zeros((F, DP), f32)
    fr = np.arange(F)
    codes, allq = [], []
    first = 0 if mutant == "st_from_residual" else st
    with np.errstate(all="ignore"):
        for lvl in range(first, n_q):
            x2 = np.zeros(F, f32)
            for c in range(D):
                x2 = fma(Rz[:, c], Rz[:, c], x2)
            # every row the 64 threads kp visit: k = 4 kp + 256 pass + u, the row READ clamped to K - 1, the index and sum e^2 taken at k
            npass = (K + 255) // 256
            k_all = np.arange(npass * 256)
            guard = k_all < K
            if mutant == "guard_dropped":
                guard = (k_all // 4) * 4 < K                                       # the loop still ends with `k0 < K`
            rows = cb[lvl][np.minimum(k_all, K - 1)]                               # [k, DP]
            x2x = (f32(2) * Rz).astype(f32)
            dot = np.zeros((F, len(k_all)), f32)
            for c in range(DP):
                dot = fma(x2x[:, c, None], rows[None, :, c], dot)
            dist = ((x2[:, None] - dot).astype(f32) + cn2_flat[np.minimum(lvl * K + k_all, cn2_flat.size - 1)][None, :]).astype(f32)
            seen = guard[None, :] & ~np.isnan(dist)                                # a row past the guard is not visited; a NaN never passes
            dist = np.where(seen, dist, np.inf)
            # thread kp scans its rows ascending (pass, then u) with a strict <, from best = +inf, bi = 0
            order = (np.arange(npass)[:, None] * 256 + np.arange(4)[None, :]).reshape(-1)          # of kp = 0
            best = np.empty((64, F), f32)
            bi = np.empty((64, F), np.int64)
            for kp in range(64):
                ks = order + 4 * kp
                sub = dist[:, ks]
                if mutant == "scan_le":
                    eq = (sub == sub.min(1, keepdims=True)) & seen[:, ks]          # `<=`: the last of the smallest (+inf <= +inf as well)
                    i = sub.shape[1] - 1 - np.argmax(eq[:, ::-1], axis=1)
                    hit = eq.any(1)
                else:
                    i = np.argmin(sub, axis=1)
                    hit = sub[fr, i] < np.inf
                best[kp] = np.where(hit, sub[fr, i], np.inf)
                bi[kp] = np.where(hit, ks[i], 0)
            # the sixteen row groups of a wave through the xor tree (lane offsets 4 .. 32 are kp offsets 1 .. 8), then the four waves in order
            hi = mutant == "merge_prefers_higher"
            kp = np.arange(64)
            for o in (1, 2, 4, 8):
                other = (kp & ~15) | ((kp & 15) ^ o)
                best, bi = _merge((best, bi), (best[other], bi[other]), hi)
            top = (best[0], bi[0])
            for w in range(1, 4):
                top = _merge(top, (best[16 * w], bi[16 * w]), hi)
            code = top[1]
            # residual -= row, sum += row, over c < D
            stride, upto = (D, DP) if mutant == "update_stride_D" else (DP, D)
            base = lvl * K * DP
            s = cb_flat[np.minimum(base + code[:, None] * stride + np.arange(upto)[None, :], cb_flat.size - 1)]
            Rz[:, :upto] = (Rz[:, :upto] - s).astype(f32)
            if lvl < st:
                continue                                                           # (st_from_residual: the levels before st only leave a residual)
            Q[:, :upto] = (Q[:, :upto] + s).astype(f32)
            codes.append(code)
            allq.append(s[:, :D].copy())
    unflat = lambda t: np.ascontiguousarray(np.transpose(t.reshape(Bn, T, -1), (0, 2, 1)))      # noqa: E731
    return dict(codes=np.stack(codes).reshape(len(codes), Bn, T), zq=unflat(Q[:, :D]), all_zq=np.stack([unflat(s) for s in allq]))


# ------------------------------------------------------------------------------------------------------------------------------
# amp_lstm
# ------------------------------------------------------------------------------------------------------------------------------
LSTM_H = (1, 2, 3, 4, 63, 64, 65, 252, 256, 260, 257, 1023)      # H < 4: inactive waves; H = 63 / 64 / 65: the scalar path's second pass; H / 4 =
LSTM_H_T = (1, 2, 3)                                             # 63 / 64 / 65: the 16-byte path's; 257 and 1023: the scalar path at depth
LSTM_B = (1, 2, 4, 5, 8, 9, 16, 17, 33)                          # every tile width full, with a tail, and three tiles
LSTM_B_H = (12, 70)
LSTM_B_T = 3
LSTM_LONG = ((20, 257), (21, 257))                               # (H, T) at B = 2: both parities of the state ping-pong over many steps
LSTM_SATURATED = (96, 33, 30.0)                                  # (H, T, the factor on gx)
LSTM_64KB = (1024, 9, 2)                                         # (H, B, T), bidirectional: BT = 16 with a tail, 16 * 1024 * 4 = 65 536 B of LDS
#                                                                  (T = 2: at T = 3 the exactly sized workspace, state + gx, passes DEVICE_TENSOR_CAP)
LSTM_FLIP_H = (257, 260)
# amp_lstm_forward: (input_size, hidden, layers, bidirectional, skip)
LSTM_FORWARD = [(7, 12, 1, True, False), (130, 20, 2, False, False), (3, 64, 2, True, False), (2048, 4, 1, False, False)] + \
               [(Hn, Hn, L, bd, True) for L in (3, 4) for Hn in (12, 20) for bd in (False, True)]
LSTM_FORWARD_T = (1, 2, 7)
LSTM_CREATE_EDGES = [(1024, 1024, 1, False, False), (4, 4, 4, True, True)]      # the accept side of hidden <= 1024 and num_layers <= 4


def lstm_tile(Bn):
    return 1 if Bn == 1 else 4 if Bn <= 4 else 8 if Bn <= 8 else 16


def lstm_lds_bytes(Hn, Bn):
    return lstm_tile(Bn) * Hn * 4


def lstm_weights(In, Hn, layers, bidir, seed, same_dirs=False):
    """nn.LSTM's four lists (w_ih, w_hh, b_ih, b_hh; l0, l0_reverse, l1, ..) at U(+-1/sqrt(H)); same_dirs: the reverse direction gets the
    forward direction's weights"""
    import torch

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


def lstm_named(w, layers, bidir):
    """the four lists as nn.LSTM names them (what speechtokenizer_ref.slstm reads)"""
    ndir = 2 if bidir else 1
    P = {}
    for layer in range(layers):
        for d in range(ndir):
            sfx = f"_l{layer}" + ("_reverse" if d else "")
            for name, lst in zip(("weight_ih", "weight_hh", "bias_ih", "bias_hh"), w):
                P[name + sfx] = lst[layer * ndir + d]
    return P


def recur_case(Hn, bidir, T, Bn, seed, same_dirs=False, scale=1.0):
    """-> (the four weight lists of one layer with input_size = H, gx [B, ndir * 4H, T], skip [B, H, T])"""
    import torch

    ndir = 2 if bidir else 1
    w = lstm_weights(Hn, Hn, 1, bidir, seed, same_dirs)
    g = torch.Generator().manual_seed(seed + 1)
    gx = scale * torch.randn(Bn, ndir * 4 * Hn, T, generator=g)
    skip = torch.randn(Bn, Hn, T, generator=g)
    return w, gx, skip


def saturated_gx(Hn, T, Bn, seed):
    """unidirectional gx with +-200 in chosen gate rows (expf overflows to inf: the gate is exactly 0 or 1).  Units [0, H/4): o = -200 at every
    step, so y = 0 exactly.  Units [H/4, H/2): o = +200 at every step and, from step 1 on, f = +200 and i = -200, so c stays c_0 and
    y_t = tanh(c_0) at every step, bit for bit.  -> (gx, the two unit ranges)"""
    import torch

    gx = torch.randn(Bn, 4 * Hn, T, generator=torch.Generator().manual_seed(seed))
    q = Hn // 4
    gx[:, 3 * Hn:3 * Hn + q] = -200.0
    gx[:, 3 * Hn + q:3 * Hn + 2 * q] = 200.0
    gx[:, Hn + q:Hn + 2 * q, 1:] = 200.0
    gx[:, q:2 * q, 1:] = -200.0
    return gx, (0, q), (q, 2 * q)


def lstm_bound(ref64, ref32, floor):
    return max(4.0 * float((ref32.double() - ref64).abs().max()), floor * float(ref64.abs().max()))


# dir1_not_reversed        direction 1 walks t = step
# h_store_to_prev          the state's two buffers confused: h is stored to the buffer it was read from.  (Swapping h_prev and h_next in BOTH the
#                          load and the store is no slip -- the ping-pong is symmetric -- so the confusion modelled is the one-sided one: the
#                          next step then reads what was written two steps before, or the NaN the workspace starts with)
# gate_order               the rows taken as i, g, f, o
# tail_from_previous_tile  a tail tile (nb < BT) behind a full one stages the full one's rows of h
# quad_stride              the 16-byte path's `k4 += 64` written as a stride of 64 COLUMNS, 16 quads: quads are multiplied twice once H / 4 > 16
# skip_both_layers         amp_lstm_forward adds the skip at every layer's store
LSTM_MUTANTS = ("dir1_not_reversed", "h_store_to_prev", "gate_order", "tail_from_previous_tile", "quad_stride", "skip_both_layers")


def _lane_columns(Hn, mutant=None):
    """-> (cols [64, L], live [64, L]): the columns of W_hh / h a lane multiplies, in its chain's order.  H % 4 == 0: lane l owns the quads
    l, l + 64, .. (columns 4 k4 .. 4 k4 + 3 in order); else the columns l, l + 64, .."""
    lists = []
    for lane in range(64):
        if Hn % 4 == 0:
            step = 16 if mutant == "quad_stride" else 64       # the slip: `k4 += 64 / 4`, a stride in columns applied to quads
            lists.append([4 * k4 + e for k4 in range(lane, Hn // 4, step) for e in range(4)])
        else:
            lists.append(list(range(lane, Hn, 64)))
    L = max(1, max(len(v) for v in lists))
    cols, live = np.zeros((64, L), np.int64), np.zeros((64, L), bool)
    for lane, v in enumerate(lists):
        cols[lane, :len(v)] = v
        live[lane, :len(v)] = True
    return cols, live


def lstm_model(w_hh, gx, skip=None, mutant=None):
    """amp_lstm_recur's launches on numpy fp32: w_hh [ndir, 4H, H], gx [B, ndir * 4H, T], skip [B, H, T] or None -> y [B, ndir * H, T].  The
    state buffers start as NaN, as the tests' workspace does."""
    assert mutant is None or mutant in LSTM_MUTANTS
    w_hh, gx = np.asarray(w_hh, f32), np.asarray(gx, f32)
    ndir, _, Hn = w_hh.shape
    Bn, _, T = gx.shape
    BT = lstm_tile(Bn)
    cols, live = _lane_columns(Hn, mutant)
    y = np.full((Bn, ndir * Hn, T), np.nan, f32)
    hbuf = [np.full((ndir, Bn, Hn), np.nan, f32) for _ in range(2)]
    cst = np.full((ndir, Bn, Hn), np.nan, f32)
    order = (0, 2, 1, 3) if mutant == "gate_order" else (0, 1, 2, 3)
    sig = lambda v: (f32(1) / (f32(1) + np.exp(-v, dtype=f32))).astype(f32)      # noqa: E731
    with np.errstate(all="ignore"):
        for step in range(T):
            h_prev, h_next = hbuf[step & 1], hbuf[(step + 1) & 1]
            if mutant == "h_store_to_prev":
                h_next = h_prev
            new_h = h_next.copy()
            for d in range(ndir):
                t = T - 1 - step if (d and mutant != "dir1_not_reversed") else step
                W = w_hh[d].reshape(4, Hn, Hn)
                for b0 in range(0, Bn, BT):
                    nb = min(BT, Bn - b0)
                    src = b0 - BT if (mutant == "tail_from_previous_tile" and nb < BT and b0) else b0
                    s = np.zeros((nb, 4, Hn), f32)
                    if step:
                        hs = h_prev[d, src:src + nb]                                       # [nb, H]
                        part = np.zeros((nb, 4, Hn, 64), f32)
                        for i in range(cols.shape[1]):
                            wv = np.where(live[:, i], W[:, :, cols[:, i]], f32(0))          # [4, H, 64]
                            hv = np.where(live[:, i], hs[:, cols[:, i]], f32(0))            # [nb, 64]
                            part = fma(wv[None], hv[:, None, None, :], part)
                        lanes = np.arange(64)
                        for o in (32, 16, 8, 4, 2, 1):
                            part = (part + part[..., lanes ^ o]).astype(f32)
                        s = part[..., 0]
                    g = gx[b0:b0 + nb, d * 4 * Hn:(d + 1) * 4 * Hn, t].reshape(nb, 4, Hn)
                    v = (g + s).astype(f32)
                    ig, fg, gg, og = sig(v[:, order[0]]), sig(v[:, order[1]]), np.tanh(v[:, order[2]]).astype(f32), sig(v[:, order[3]])
                    cp = cst[d, b0:b0 + nb] if step else np.zeros((nb, Hn), f32)
                    cn = ((fg * cp).astype(f32) + (ig * gg).astype(f32)).astype(f32)
                    hn = (og * np.tanh(cn).astype(f32)).astype(f32)
                    cst[d, b0:b0 + nb] = cn
                    new_h[d, b0:b0 + nb] = hn
                    y[b0:b0 + nb, d * Hn:(d + 1) * Hn, t] = hn if skip is None else (hn + np.asarray(skip, f32)[b0:b0 + nb, :, t]).astype(f32)
            h_next[...] = new_h
    return y


def lstm_forward_model(P, x, layers, bidir, skip, mutant=None):
    """amp_lstm_forward with lstm_model as the recurrence and a torch fp32 projection; P as lstm_named gives it"""
    import torch

    h = x
    for layer in range(layers):
        w_ih, w_hh, b = R.lstm_weights(P, "", layer, bidir)
        gx = R.lstm_input_projection(w_ih, b, h)
        last = layer == layers - 1
        sk = x if (skip and (last or mutant == "skip_both_layers")) else None
        h = torch.from_numpy(lstm_model(w_hh.numpy(), gx.numpy(), None if sk is None else sk.numpy(), mutant))
    return h


# ------------------------------------------------------------------------------------------------------------------------------
# amp_dsconv
# ------------------------------------------------------------------------------------------------------------------------------
DS_KC = 64                                        # channels per K step
DS_BIG_MIN = 256                                  # workgroups of the 128-column tile from which the launcher takes it


@dataclass(frozen=True)
class Ds:
    cin: int
    cout: int
    B: int
    Ts: tuple

    @property
    def id(self):
        return f"{self.cin}to{self.cout}B{self.B}"

    @property
    def steps(self):
        return (self.cin + DS_KC - 1) // DS_KC

    def big(self, T, batch=None):
        """does ds_launch take the 128-column tile?"""
        Tout = (T - 1) // 2 + 1
        return (self.B if batch is None else batch) * ((Tout + 127) // 128) * ((self.cout + 127) // 128) >= DS_BIG_MIN

    def tile(self, T, batch=None):
        """(MI, NI) of dsconv_f16x3_kernel<GELU, MI, NI>"""
        return (2, 2) if self.big(T, batch) else (1, 1)


DSCONV = [Ds(1, 1, 2, (1, 2, 5)), Ds(63, 33, 2, (7, 8)), Ds(65, 31, 2, (7, 8)), Ds(129, 96, 2, (128, 129, 130)), Ds(200, 70, 3, (255, 256, 257)),
          Ds(320, 64, 1, (9,)), Ds(200, 4090, 8, (13, 14))]
DS_RANGE = Ds(129, 33, 3, (9,))                   # the range guard: three K steps, the last with one channel


def ds_tensors(case):
    import torch

    g = torch.Generator().manual_seed(9000 + 7 * case.cin + case.cout)
    w = torch.randn(case.cout, case.cin, 3, generator=g) / (3 * case.cin) ** 0.5
    return w, 0.1 * torch.randn(case.cout, generator=g)


def ds_input(case, T, batch=None):
    import torch

    return torch.randn(case.B if batch is None else batch, case.cin, T, generator=torch.Generator().manual_seed(9100 + case.cin + 13 * T))


def ds_window_model(x, w, TN, clamp=False):
    """the even / odd plane indexing of dsconv_f16x3_kernel on one row x [T] with the taps w [3], in fp64: window column j of a tile at q0 is
    input column 2 q0 - 1 + j; odd j is E[j >> 1] at staged column j >> 1, even j is O[j >> 1] at staged column TN + (j >> 1); output q reads
    O[q], E[q], O[q + 1].  Input columns -1 and >= T are selected to 0 (clamp: the slip that keeps the clamped load's value)"""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    T = len(x)
    Tout = (T - 1) // 2 + 1
    y = np.zeros(Tout)
    for q0 in range(0, Tout, TN):
        staged = np.zeros(2 * TN + 1)
        for j in range(2 * TN + 1):
            t = 2 * q0 - 1 + j
            ok = 0 <= t < T
            v = x[min(max(t, 0), T - 1)]
            col = (j >> 1) if (j & 1) else TN + (j >> 1)
            staged[col] = v if (ok or clamp) else 0.0
        for q in range(min(TN, Tout - q0)):
            y[q0 + q] = w[0] * staged[TN + q] + w[1] * staged[q] + w[2] * staged[TN + q + 1]
    return y


# ------------------------------------------------------------------------------------------------------------------------------
# amp_elu_pad, amp_gelu
# ------------------------------------------------------------------------------------------------------------------------------
ELU_PADS = ((0, 5), (7, 0), (0, 1), (33, 64), (64, 33), (16, 16))
ELU_C = (1, 3)
ELU_B = 2
GELU_N = (2, 3, 4, 7, 8, 1023, 1024, 1025, 1027)
OFFSETS = (0, 1, 2, 3)                            # floats off a 16-byte boundary


def elu_lengths(pl, pr):
    m = max(pl, pr)
    return tuple(sorted({1, 2, m, m + 1, m + 2, 130}))


def special_values():
    """-0.0, +-denormal, -100, -1e30, +-inf, NaN"""
    import torch

    return torch.tensor([-0.0, 1e-40, -1e-40, -100.0, -1e30, float("inf"), float("-inf"), float("nan")], dtype=torch.float32)
