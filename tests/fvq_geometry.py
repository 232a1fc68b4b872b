"""The geometry table of the integer-deciding codec kernels of include/amphion_hip.h -- amp_fvq_* (csrc/fvq.hip) over the whole documented range
D <= 1024, d <= 32, K <= 16384, N <= 32, and amp_semantic_prepare (csrc/semantic_prepare.hip) around its 64-channel x 32-frame tile -- where every
other quantizer case of the suite sits at d = 8, K a multiple of 16, D a multiple of 16 and N <= 12.  Plain data and pure functions, no GPU and
nothing of the package: tests/test_fvq_geometry_ref.py checks the table on the CPU, tests/test_gpu_fvq_geometry.py runs every case through the
C ABI.

An encode case is one handle (D, d, K, N, l2), projections exactly when D != d; it runs at every length of `Ts` with B = 3.  fvq_model() restates
csrc/fvq.hip's encode kernel in numpy fp32, operation by operation: the fmaf chains and their order, the four-part shuffle tree of in_project,
each thread's ascending scan with a strict <, the part / wave merge with the lower index winning on equality, the straight-through form and the
zero-padded rows of DP = 8 / 16 / 32 floats.  A fused multiply-add is emulated as one fp64 product (exact: 24 + 24 bits) and one fp64 sum rounded
to fp32 -- two roundings where the hardware has one, so the model claims "the same codes on every decided frame", not bit equality.  Its
`mutant` argument applies ONE slip of the kernel's text; the CPU tests show that the suite's rules catch each of them on this table.
"""
from dataclasses import dataclass

import numpy as np

AMP_ERR_INVALID, AMP_ERR_UNSUPPORTED = -1, -4
FVQ_TF = 16                                      # frames per workgroup of both fvq kernels; a thread scans k = part16, part16 + 16, ..
SP_TC, SP_TT = 64, 32                            # channels x output frames per workgroup of semantic_prepare_kernel
B = 3
LENGTHS = (1, 17, 50)                            # one frame; a ragged second tile; four tiles, the last with 2 frames.  B * T <= 150
MAX_D, MAX_d, MAX_K, MAX_N = 1024, 32, 16384, 32
UNDECIDED_CAP = 0.02                             # the cap of tests/test_gpu_codec.py::check_encode
# no device tensor of the sweep exceeds torch's small-block limit, so the sweep leaves the caching allocator's large-block pool exactly as it found
# it: the tests that poison freed memory on purpose (tests/test_gpu_vits_longform.py) depend on which cached large blocks they are handed back
DEVICE_TENSOR_CAP = 1 << 20


def row_pad(d):
    """amp_fvq_create: codebook rows are zero-padded to DP floats"""
    return 8 if d <= 8 else 16 if d <= 16 else 32


def encode_lds_bytes(D, d):
    """fvq_lds_bytes(D, DP): residual and sum [D][16] each, z_e and its normalised form [DP][16] each, 10 rows of 16 words of merge state"""
    return (2 * D * FVQ_TF + 2 * row_pad(d) * FVQ_TF + FVQ_TF * 10) * 4


def decode_lds_bytes(n, d):
    """fvq_decode_run: the code rows of all levels [n][d][16] and the codes [n][16]"""
    return (n * d + n) * FVQ_TF * 4


@dataclass(frozen=True)
class Enc:
    name: str
    D: int
    d: int
    K: int
    N: int
    l2: bool
    seed: int
    Ts: tuple = LENGTHS
    margin: bool = True                          # False: the fp64 reference need not decide it; only the near-optimality rule applies to its codes

    @property
    def id(self):
        return f"{self.name}/D{self.D}d{self.d}K{self.K}N{self.N}{'/l2' if self.l2 else ''}"

    @property
    def hp(self):
        return dict(D=self.D, d=self.d, K=self.K, N=self.N, l2=self.l2)

    @property
    def DP(self):
        return row_pad(self.d)

    @property
    def padded(self):
        return self.d < self.DP

    @property
    def identity(self):
        return self.D == self.d


ENCODE = [
    Enc("dp8_padded_ragged", 20, 5, 37, 2, True, 500),           # <8>, padded rows, ragged D and K
    Enc("dp8_identity_smallK", 4, 4, 7, 3, False, 501),          # <8>, identity, K < 16: nine of the sixteen scanning threads of a frame scan nothing
    Enc("dp16_full", 48, 16, 100, 3, True, 502),                 # <16>, d == DP
    Enc("dp16_padded_K16", 33, 9, 16, 2, False, 503),            # <16>, padded, ragged D, every thread scans exactly one row
    Enc("dp16_identity_padded", 12, 12, 50, 2, True, 504),       # <16>, identity, padded
    Enc("dp32_full", 96, 32, 256, 2, True, 505),                 # <32>, d == DP
    Enc("dp32_padded", 130, 17, 129, 4, False, 506),             # <32>, padded, D % 4 == 2
    Enc("dp32_identity", 32, 32, 64, 2, True, 507),              # <32>, identity
    Enc("largest_lds", 1024, 32, 33, 2, True, 508, (1, 17, 35)),  # the encode kernel's largest LDS request, 135 808 B (T: see DEVICE_TENSOR_CAP)
    Enc("largest_K_narrow", 16, 8, 16384, 1, True, 509),
    Enc("largest_K_wide", 32, 32, 16384, 1, True, 510),          # a 2-MB codebook
    Enc("largest_N", 24, 6, 16, 32, True, 511),                  # (l2 = False leaves 5.9 % undecided at T = 17: not under the margin rule)
    Enc("deep_and_wide", 64, 24, 1000, 8, True, 512),
    Enc("smallest_d", 3, 1, 5, 2, False, 513),
    Enc("degenerate", 1, 1, 1, 1, True, 514),
]
# the decode kernel's LDS request above the 64-KB default needs d = 32 and N = 32 together: 67 584 B
DECODE_LDS = Enc("decode_lds", 32, 32, 16, 32, True, 515, margin=False)
ALL_ENCODE = ENCODE + [DECODE_LDS]

# exact ties.  Every codebook row twice (rows K/2 .. equal rows 0 .. K/2 - 1): one case per DP, a padded one among them.  K/2 = 18 and 50 put a row
# and its copy into different threads (the shuffle / LDS merge must prefer the lower index), K/2 = 128 and 32 into the same thread (the scan's <).
TIES = [
    Enc("ties_dp8_padded", 20, 5, 36, 2, True, 520, (17,)),
    Enc("ties_dp16_full", 48, 16, 100, 3, True, 521, (17,)),
    Enc("ties_dp16_identity_padded", 12, 12, 64, 2, True, 522, (17,)),
    Enc("ties_dp32_full", 96, 32, 256, 2, True, 523, (17,)),
]
# d = 1 with l2: every row normalises to exactly +1 or -1 (sqrt(x * x) = |x| and x / |x| = +-1 are exact in binary floating point), z_e too, so a
# distance is exactly (1 - 2) + 1 = 0 where the signs agree and (1 + 2) + 1 = 4 where not: the code is the lowest index whose sign is z_e's, 0 if none
SIGN = Enc("sign_d1_l2", 3, 1, 5, 2, True, 524, (17,), margin=False)

# one case per DP for the folded forms (row stride T + 3 and sub) and for batch independence
PER_DP = ("dp8_padded_ragged", "dp16_padded_K16", "dp32_full")


def by_name(name):
    return next(c for c in ALL_ENCODE + TIES + [SIGN] if c.name == name)


# (argument tuple D, d, K, N; which projection arrays are given "all" | "none" | "in_only" | "no_bias"; codebook poison; status; word of the message)
CREATE_REFUSALS = [
    ((MAX_D + 1, 8, 16, 1), "all", None, AMP_ERR_UNSUPPORTED, "outside the kernel"),
    ((64, MAX_d + 1, 16, 1), "all", None, AMP_ERR_UNSUPPORTED, "outside the kernel"),
    ((64, 8, MAX_K + 1, 1), "all", None, AMP_ERR_UNSUPPORTED, "outside the kernel"),
    ((64, 8, 16, MAX_N + 1), "all", None, AMP_ERR_UNSUPPORTED, "outside the kernel"),
    ((0, 8, 16, 1), "all", None, AMP_ERR_INVALID, "D=0"),
    ((64, 0, 16, 1), "all", None, AMP_ERR_INVALID, "d=0"),
    ((64, 8, 0, 1), "all", None, AMP_ERR_INVALID, "K=0"),
    ((64, 8, 16, 0), "all", None, AMP_ERR_INVALID, "N=0"),
    ((-1, 8, 16, 1), "all", None, AMP_ERR_INVALID, "D=-1"),
    ((64, 8, 16, -2), "all", None, AMP_ERR_INVALID, "N=-2"),
    ((64, 8, 16, 2), "in_only", None, AMP_ERR_INVALID, "come together"),
    ((64, 8, 16, 2), "no_bias", None, AMP_ERR_INVALID, "come together"),
    ((64, 8, 16, 2), "none", None, AMP_ERR_INVALID, "identity"),
    ((8, 8, 16, 2), "none", float("nan"), AMP_ERR_INVALID, "non-finite"),
    ((64, 8, 16, 2), "all", float("inf"), AMP_ERR_INVALID, "non-finite"),
    ((64, 8, 16, 2), "all", float("-inf"), AMP_ERR_INVALID, "non-finite"),
]


# ------------------------------------------------------------------------------------------------------------------------------
# amp_semantic_prepare: (B, T, C, factor), each with and without the statistics
# ------------------------------------------------------------------------------------------------------------------------------
SEMANTIC = [
    (2, 1, 1, 1),            # one element
    (2, 33, 1, 1),           # C = 1, a second time tile with one frame
    (2, 63, 63, 2),          # To = 31, the last frame dropped
    (2, 160, 63, 5),         # To = 32: exactly one time tile
    (2, 64, 64, 2),          # one full tile both ways
    (2, 7, 64, 5),           # To = 1, two frames dropped
    (2, 99, 65, 3),          # To = 33, a second channel tile with one channel
    (2, 101, 65, 3),         # the same with two frames dropped
    (2, 66, 65, 2),
    (2, 70, 130, 1),         # To = 70: three time tiles, the last with 6 frames; three channel tiles, the last with 2
    (2, 155, 130, 5),        # To = 31
    (3, 352, 130, 5),        # B = 3, To = 70, two frames dropped
]


# ------------------------------------------------------------------------------------------------------------------------------
# tensors and fp64 / fp32 references of an encode case (torch on the CPU; imported on use)
# ------------------------------------------------------------------------------------------------------------------------------
QP = "quantizers."


def weights(case):
    """the case's state_dict as codec_ref's quantizer functions read it, fp32, with the projections FOLDED (`weight` in place of weight_g /
    weight_v: the values the library is given, so fp64, fp32 and the kernel all start from the same numbers)"""
    import codec_ref as C

    sd = C.synth_fvq_state_dict(case.hp, case.seed)
    out = {}
    for k, v in sd.items():
        if k.endswith("weight_g"):
            out[k[:-2]] = C.folded({n: t.double() for n, t in sd.items()}, k[:-8]).float().contiguous()
        elif not k.endswith("weight_v"):
            out[k] = v
    return out


def tie_weights(case):
    """-> (state_dict with rows K/2 .. equal to rows 0 .. K/2 - 1, hp and state_dict of the half codebook)"""
    sd = weights(case)
    h = case.K // 2
    assert 2 * h == case.K
    half = {}
    for k, v in sd.items():
        if k.endswith("codebook.weight"):
            v = v.clone()
            v[h:] = v[:h]
            sd[k] = v
            half[k] = v[:h].contiguous()
        else:
            half[k] = v
    return sd, dict(case.hp, K=h), half


def latent(case, T, batch=B):
    import codec_ref as C

    return C.synth_latent(batch, case.D, T, case.seed + 100 + 7 * T + batch)


def latents_of(sd, hp, z, all_q, dtype):
    """every level's z_e [B, n * d, T] (torch.cat(latents, 1) of DualCodec's ResidualVectorQuantize) along the trajectory whose per-level z_q are all_q"""
    import codec_ref as C
    import torch
    import torch.nn.functional as Fn

    P = {k: v.to(dtype) for k, v in sd.items()}
    residual = z.to(dtype)
    lat = []
    for i in range(all_q.shape[0]):
        p = f"{QP}{i}."
        lat.append(Fn.conv1d(residual, C.folded(P, p + "in_project."), P[p + "in_project.bias"]) if hp["D"] != hp["d"] else residual)
        residual = residual - all_q[i].to(dtype)
    return torch.cat(lat, 1)


_REF = {}


def reference(case, T):
    """the CPU references of (case, T), computed once and left unchanged: codec_ref.margin_rule's fp64 run, its fp32 restatement along the fp64
    codes, tau, the decided mask, both runs' latents, and the undecided share of frames"""
    import codec_ref as C
    import torch

    key = (case.name, T)
    if key not in _REF:
        sd, z = weights(case), latent(case, T)
        r64, r32, tau, decided = C.margin_rule(sd, case.hp, z)
        r64["latents"] = latents_of(sd, case.hp, z, r64["all_q"], torch.float64)
        r32["latents"] = latents_of(sd, case.hp, z, r32["all_q"], torch.float32)
        undecided = 1.0 - float(decided[-1].double().mean())
        _REF[key] = dict(sd=sd, z=z, r64=r64, r32=r32, tau=tau, decided=decided, undecided=undecided)
    return _REF[key]


def restatement_bound(ref, which, zmax):
    """the suite's rule for zq / latents on the frames decided at every level: max(4 x the fp32 restatement's own error against fp64, 1e-6 max|z|).
    -> (bound, mask)"""
    r64, r32 = ref["r64"][which], ref["r32"][which]
    mask = ref["decided"][-1][:, None, :].expand_as(r64)
    e32 = float((r32.double() - r64)[mask].abs().max()) if bool(mask.any()) else 0.0
    return max(4 * e32, 1e-6 * zmax), mask


def excess_over_minimum(sd, hp, z, codes):
    """walk fp64 along `codes` [n, B, T]: at every (level, frame), the fp64 distance of the chosen row minus the fp64 minimum -> [n, B * T]"""
    import codec_ref as C
    import torch

    f64 = C.rvq_forward(sd, hp, z, torch.float64, codes.shape[0], codes=codes)
    return torch.stack([d.gather(1, c.reshape(-1, 1)).squeeze(1) - d.min(1).values for d, c in zip(f64["dist"], codes)])


# ------------------------------------------------------------------------------------------------------------------------------
# the encode kernel in numpy fp32, from the text of csrc/fvq.hip
# ------------------------------------------------------------------------------------------------------------------------------
MUTANTS = ("stride_d", "scan_start_plus_1", "scan_le", "merge_prefers_higher", "padding_not_zeroed")
f32 = np.float32


def fma(a, b, c):
    """fmaf on fp32 arrays: the product is exact in fp64, the sum is rounded to fp64 and then to fp32"""
    return (np.asarray(a, f32).astype(np.float64) * np.asarray(b, f32).astype(np.float64) + np.asarray(c, f32).astype(np.float64)).astype(f32)


def model_weights(sd, hp):
    """the host arrays amp_fvq_create receives: w_in [N, d, D], b_in [N, d], cb [N, K, d], w_out [N, D, d], b_out [N, D] (projections None for identity)"""
    N, proj = hp["N"], hp["D"] != hp["d"]
    g = lambda key: np.stack([sd[f"{QP}{i}.{key}"].numpy().astype(f32) for i in range(N)])      # noqa: E731
    W = dict(cb=g("codebook.weight"), w_in=None, b_in=None, w_out=None, b_out=None)
    if proj:
        W.update(w_in=g("in_project.weight")[..., 0], b_in=g("in_project.bias"), w_out=g("out_project.weight")[..., 0], b_out=g("out_project.bias"))
    return W


def _normalise_rows(r, l2):
    """amp_fvq_create's host loop: -> (rows the distance is taken to, their sums of squares)"""
    if l2:
        n2 = np.zeros(r.shape[0], f32)
        for j in range(r.shape[1]):
            n2 = fma(r[:, j], r[:, j], n2)
        nrm = np.sqrt(n2)
        inv = np.where(nrm > f32(1e-12), nrm, f32(1e-12)).astype(f32)
        nr = (r / inv[:, None]).astype(f32)
    else:
        nr = r
    s = np.zeros(r.shape[0], f32)
    for j in range(r.shape[1]):
        s = fma(nr[:, j], nr[:, j], s)
    return nr, s


def _merge(a, b, higher):
    """`if (ob < best || (ob == best && oi < bi)) take the other`: a = (best, bi) of this lane, b of the other"""
    take = (b[0] < a[0]) | ((b[0] == a[0]) & ((b[1] > a[1]) if higher else (b[1] < a[1])))
    return np.where(take, b[0], a[0]), np.where(take, b[1], a[1])


def fvq_model(hp, W, z, sub=None, n=None, mutant=None):
    """fvq_encode_kernel<DP> on z [B, D, T] (numpy fp32; sub [B, D, T] or None) -> dict(codes [n, B, T] int64, zq [B, D, T], all_zq [n, B, D, T],
    latents [B, n * d, T]).  Frames are independent in the kernel, so they are walked together."""
    assert mutant is None or mutant in MUTANTS
    D, d, K, l2 = hp["D"], hp["d"], hp["K"], hp["l2"]
    n = hp["N"] if n is None else n
    DP = row_pad(d)
    stride = d if mutant == "stride_d" else DP
    Bn, _, T = z.shape
    F = Bn * T
    flat = lambda t: np.ascontiguousarray(np.transpose(np.asarray(t, f32), (0, 2, 1)).reshape(F, D))      # noqa: E731
    R = flat(z)
    if sub is not None:
        R = (R - flat(sub)).astype(f32)
    Q = np.zeros((F, D), f32)
    codes, allq, lat = [], [], []
    with np.errstate(all="ignore"):
        for l in range(n):
            # ---- z_e = in_project(residual): part p sums channels p, p + 4, .. as one chain; the parts meet as (s0 + s1) + (s2 + s3) ----
            if W["w_in"] is not None:
                parts = []
                for p in range(4):
                    s = np.zeros((F, d), f32)
                    for c in range(p, D, 4):
                        s = fma(W["w_in"][l][None, :, c], R[:, c, None], s)
                    parts.append(s)
                E = (((parts[0] + parts[1]).astype(f32) + (parts[2] + parts[3]).astype(f32)).astype(f32) + W["b_in"][l][None, :]).astype(f32)
            else:
                E = R[:, :d].copy()
            # ---- F.normalize(z_e) and sum e^2 ----
            if l2:
                n2 = np.zeros(F, f32)
                for j in range(d):
                    n2 = fma(E[:, j], E[:, j], n2)
                nrm = np.sqrt(n2)
                inv = np.where(nrm > f32(1e-12), nrm, f32(1e-12)).astype(f32)
                v = (E / inv[:, None]).astype(f32)
            else:
                v = E
            e2 = np.zeros(F, f32)
            for j in range(d):
                e2 = fma(v[:, j], v[:, j], e2)
            EN = np.full((F, DP), np.nan if mutant == "padding_not_zeroed" else 0.0, f32)     # what LDS held before is anything: NaN is the value that tells
            EN[:, :d] = v
            e = (f32(2) * EN).astype(f32)
            # ---- the padded codebook of the level and all K distances ----
            nr, cn2 = _normalise_rows(W["cb"][l], l2)
            cbn = np.zeros((K, DP), f32)
            cbn[:, :d] = nr
            cb = np.zeros((K, DP), f32)
            cb[:, :d] = W["cb"][l]
            at = np.arange(K)[:, None] * stride + np.arange(DP)[None, :]               # row k is read at k * stride .. + DP of the flat array
            rows = cbn.reshape(-1)[at]
            dot = np.zeros((F, K), f32)
            for j in range(DP):
                dot = fma(e[:, j, None], rows[None, :, j], dot)
            dist = ((e2[:, None] - dot).astype(f32) + cn2[None, :]).astype(f32)
            # ---- thread part16 scans k = part16, part16 + 16, .. ascending with a strict <, from best = +inf, bi = 0 ----
            cand = []
            for p16 in range(16):
                ks = np.arange(p16 + (1 if mutant == "scan_start_plus_1" else 0), K, 16)
                best, bi = np.full(F, np.inf, f32), np.zeros(F, np.int64)
                if len(ks):
                    sub_d = dist[:, ks]
                    sub_d = np.where(np.isnan(sub_d), np.inf, sub_d)                      # a NaN never passes `dist < best`
                    if mutant == "scan_le":
                        i = sub_d.shape[1] - 1 - np.argmin(sub_d[:, ::-1], axis=1)        # `<=`: the last of the smallest
                        hit = np.ones(F, bool)                                           # (+inf <= +inf as well)
                    else:
                        i = np.argmin(sub_d, axis=1)                                     # the first of the smallest
                        hit = sub_d[np.arange(F), i] < np.inf
                    best = np.where(hit, sub_d[np.arange(F), i], best).astype(f32)
                    bi = np.where(hit, ks[i], bi)
                cand.append((best, bi))
            # ---- the four parts of a wave through the shuffle tree (xor 16, then xor 32), then the four waves in order ----
            hi = mutant == "merge_prefers_higher"
            waves = [_merge(_merge(cand[4 * w], cand[4 * w + 1], hi), _merge(cand[4 * w + 2], cand[4 * w + 3], hi), hi) for w in range(4)]
            top = waves[0]
            for w in range(1, 4):
                top = _merge(top, waves[w], hi)
            code = top[1]
            # ---- z_e + (codebook[code] - z_e), out_project, residual and sum ----
            raw = cb.reshape(-1)[code[:, None] * stride + np.arange(d)[None, :]]
            q = (E + (raw - E).astype(f32)).astype(f32)
            if W["w_out"] is not None:
                s = np.zeros((F, D), f32)
                for j in range(d):
                    s = fma(W["w_out"][l][None, :, j], q[:, j, None], s)
                s = (s + W["b_out"][l][None, :]).astype(f32)
            else:
                s = q
            R = (R - s).astype(f32)
            Q = (Q + s).astype(f32)
            codes.append(code)
            allq.append(s)
            lat.append(E)
    unflat = lambda t: np.transpose(t.reshape(Bn, T, -1), (0, 2, 1))      # noqa: E731
    zq = unflat(Q)
    if sub is not None:
        zq = (zq + np.asarray(sub, f32)).astype(f32)
    return dict(codes=np.stack(codes).reshape(n, Bn, T), zq=zq, all_zq=np.stack([unflat(s) for s in allq]),
                latents=np.concatenate([unflat(e) for e in lat], axis=1))


def sign_rule_codes(cb_level, z_e):
    """d = 1 with l2: the lowest index whose sign is z_e's, 0 when no row has it.  cb_level [K] and z_e [...] hold no zero"""
    cb_level, z_e = np.asarray(cb_level), np.asarray(z_e)
    assert (cb_level != 0).all() and (z_e != 0).all()
    same = np.sign(cb_level)[None, :] == np.sign(z_e).reshape(-1, 1)
    return np.where(same.any(1), same.argmax(1), 0).reshape(z_e.shape)


# ------------------------------------------------------------------------------------------------------------------------------
# amp_fvq_create's arguments from host arrays (ctypes alone: the library handle is the caller's)
# ------------------------------------------------------------------------------------------------------------------------------
def create_args(W, given="all"):
    """-> ((in_w, in_b, codebook, out_w, out_b) arrays of per-level pointers or None, the arrays to keep alive).  given: "all" what W holds |
    "none" no projection array | "in_only" in_project without out_project | "no_bias" both weights without their biases"""
    import ctypes

    keep = []

    def arr(a):
        if a is None:
            return None
        rows = [np.ascontiguousarray(r, f32) for r in a]
        keep.extend(rows)
        return (ctypes.c_void_p * len(rows))(*[r.ctypes.data for r in rows])

    wi, bi, wo, bo = (W[k] for k in ("w_in", "b_in", "w_out", "b_out"))
    if given == "none":
        wi = bi = wo = bo = None
    elif given == "in_only":
        wo = bo = None
    elif given == "no_bias":
        bi = bo = None
    else:
        assert given == "all"
    return (arr(wi), arr(bi), arr(W["cb"]), arr(wo), arr(bo)), keep


def refusal_weights(D, d, K, N, poison=None):
    """finite host arrays for a create that must be refused: the true sizes where they lie inside the kernel's range, one element where not (a
    size outside the range is refused before anything is read); poison: the value of one codebook entry of the last level"""
    inside = 1 <= D <= MAX_D and 1 <= d <= MAX_d and 1 <= K <= MAX_K and 1 <= N <= MAX_N
    Dn, dn, Kn, Nn = (D, d, K, N) if inside else (1, 1, 1, 1)
    g = np.random.default_rng(7)
    W = dict(w_in=g.standard_normal((Nn, dn, Dn)).astype(f32), b_in=g.standard_normal((Nn, dn)).astype(f32),
             cb=g.standard_normal((Nn, Kn, dn)).astype(f32), w_out=g.standard_normal((Nn, Dn, dn)).astype(f32),
             b_out=g.standard_normal((Nn, Dn)).astype(f32))
    if poison is not None:
        W["cb"][-1, Kn // 2, dn - 1] = poison
    return W
