"""The geometry table of the codec ops of include/amphion_hip.h -- amp_tconv_*, amp_sconv_*, amp_codec_unit_*, amp_aa_unit_* -- over the whole
range the header documents, well outside the single point of it the codec recipes use (padding ceil(stride / 2), output_padding stride % 2,
dilations 1 / 3 / 9).  Plain data and pure functions, no GPU: tests/test_codec_geometry_ref.py checks the table and the bounds on the CPU,
tests/test_gpu_codec_geometry.py runs every case through the C ABI.

A case is one handle: it runs with and without the activation parameter where the op has one, at every length of `Ts`, with B = 2.
`refuse` cases must raise instead of launching: (stage, status, word the message must hold).

tconv_model() restates, from the text of csrc/tconv_f16x3.hip and of amp_tconv_forward, how the fused transposed conv tiles its columns,
which rows each wave sweeps and which of tconv_store4's store branches every (row quad, column) takes; it returns the branches reached
and the number of owners of every output sample.
"""
from dataclasses import dataclass, field

import numpy as np

AMP_ERR_INVALID, AMP_ERR_UNSUPPORTED = -1, -4
TC_TN = 64                                       # columns per workgroup of tconv_f16x3_kernel
CU_TN, AA_TN = 64, 54                            # output columns per workgroup of the codec unit / the anti-aliased unit
UNIT_MAX_FUSED_DILATION = 9
B = 2


def ceil_half(s):
    return (s + 1) // 2


def tconv_out_len(T, s, p, op):
    return (T - 1) * s - 2 * p + 2 * s + op


def sconv_out_len(T, s, p):
    n = T + 2 * p - 2 * s
    return 0 if n < 0 else n // s + 1


# ------------------------------------------------------------------------------------------------------------------------------
# case types
# ------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Tconv:
    cin: int
    cout: int
    s: int
    p: int
    op: int
    fused: bool                                  # amp_set_tconv_fusion(1 / 0) before the handle is made
    Ts: tuple = ()
    built: bool = True                           # the fused kernel is built for this (cin, s) under f16x3
    refuse: tuple = None
    kind: str = field(default="tconv", repr=False)

    @property
    def id(self):
        return f"tconv{self.cin}-{self.cout}s{self.s}p{self.p}op{self.op}/{'fused' if self.fused else 'unfused'}"

    def out_len(self, T):
        return tconv_out_len(T, self.s, self.p, self.op)


@dataclass(frozen=True)
class Sconv:
    cin: int
    cout: int
    s: int
    p: int
    Ts: tuple = ()
    refuse: tuple = None
    kind: str = field(default="sconv", repr=False)

    @property
    def id(self):
        return f"sconv{self.cin}-{self.cout}s{self.s}p{self.p}"

    def out_len(self, T):
        return sconv_out_len(T, self.s, self.p)


@dataclass(frozen=True)
class Unit:
    kind: str                                    # "codec" (amp_codec_unit_*: Snake1d) | "aa" (amp_aa_unit_*: Activation1d)
    C: int
    d: int
    Ts: tuple = ()
    fused: bool = True                           # amp_set_*_unit_fusion(1 / 0) before the handle is made
    beta: bool = True                            # aa only: SnakeBeta (False: plain Snake, beta = NULL)
    refuse: tuple = None

    @property
    def id(self):
        return (f"{self.kind}_unit{self.C}d{self.d}" + ("" if self.beta or self.kind == "codec" else "/snake")
                + ("/fused" if self.fused else "/unfused"))

    @property
    def built(self):
        """the fused kernel is built for this unit under f16x3"""
        return self.C % 32 == 0 and self.C <= (192 if self.kind == "codec" else 128) and 1 <= self.d <= UNIT_MAX_FUSED_DILATION

    @property
    def TN(self):
        return CU_TN if self.kind == "codec" else AA_TN


# ------------------------------------------------------------------------------------------------------------------------------
# tconv
# ------------------------------------------------------------------------------------------------------------------------------
TCONV_LENGTHS = (1, 2, 63, 64, 65, 129)


def tconv_paddings(s):
    return sorted({0, 1, ceil_half(s), s - 1, s, s + 1, 2 * s})


def tconv_output_paddings(s, p):
    """{0, 1, min(p, s - 1)} where the header allows them: output_padding < stride and <= padding"""
    return sorted(o for o in {0, 1, min(p, s - 1)} if o < s and o <= p)


def _lengths(s, p, op, Ts=TCONV_LENGTHS):
    return tuple(T for T in Ts if tconv_out_len(T, s, p, op) > 0)


def _tconv_grid(fused):
    out = []
    for s in range(2, 9):
        for p in tconv_paddings(s):
            for op in tconv_output_paddings(s, p):
                out.append(Tconv(32, 16, s, p, op, fused, _lengths(s, p, op)))
        # rows M = cout * s below 32, odd, no multiple of 32; 4 / 2 / 1 row-block groups.  At the recipe padding and at one padding >= s
        for cout in (1, 3, 33, 40):
            for p, op in ((ceil_half(s), s % 2), (s + 2, min(s - 1, 2))):
                out.append(Tconv(32, cout, s, p, op, fused, _lengths(s, p, op, (1, 64, 65))))
    # wide inputs (the K loop over 6 / 24 chunks per tap, the 100-KB window) at strides 4, 6, 7 and paddings the recipes never use
    for cin, s, p, op in ((96, 4, 5, 1), (96, 6, 0, 0), (96, 7, 9, 6), (384, 4, 3, 2), (384, 6, 7, 5), (384, 7, 2, 0)):
        out.append(Tconv(cin, cin // 2, s, p, op, fused, _lengths(s, p, op, (1, 65))))
    return out


TCONV_FUSED = _tconv_grid(True)
TCONV_UNFUSED = _tconv_grid(False) + [
    # not built for fusion: strides 1 and 9, cin no multiple of 32 -- amp_set_tconv_fusion(1) must still give the two launches
    Tconv(32, 16, 1, 0, 0, True, _lengths(1, 0, 0), built=False),
    Tconv(32, 16, 1, 1, 0, True, _lengths(1, 1, 0), built=False),
    Tconv(32, 16, 1, 2, 0, True, _lengths(1, 2, 0), built=False),
    Tconv(32, 16, 9, 0, 0, True, _lengths(9, 0, 0), built=False),
    Tconv(32, 16, 9, 5, 1, True, _lengths(9, 5, 1), built=False),
    Tconv(32, 16, 9, 10, 8, True, _lengths(9, 10, 8), built=False),
    Tconv(32, 16, 9, 18, 3, True, _lengths(9, 18, 3), built=False),
    Tconv(48, 16, 4, 2, 0, True, _lengths(4, 2, 0), built=False),
    Tconv(48, 24, 6, 7, 5, True, _lengths(6, 7, 5), built=False),
    Tconv(48, 16, 3, 0, 0, True, _lengths(3, 0, 0), built=False),
]


# ------------------------------------------------------------------------------------------------------------------------------
# sconv
# ------------------------------------------------------------------------------------------------------------------------------
REPACK_BLOCK = 256                               # threads per block of sconv_repack_kernel: one per padded position j < (T_out + 1) * s


def sconv_paddings(s):
    return sorted({0, 1, ceil_half(s), s, 2 * s - 1})


def sconv_lengths(s, p):
    """the shortest valid length (T + 2 p >= 2 s, T >= 1), 2 s + 1, 97, and the two lengths that put the repack kernel's (T_out + 1) * s
    positions of a row on either side of its 256-thread block: the largest multiple of s that is <= 256 (256 itself for s = 1, 2, 4, 8)
    and the next one (>= 257: a second block with few live threads).  T = U s - 2 p is the shortest length with T_out + 1 = U; the longest,
    s - 1 more, leaves s - 1 samples at the end that no output reads."""
    U = REPACK_BLOCK // s
    Ts = {max(1, 2 * s - 2 * p), 2 * s + 1, 97, U * s - 2 * p, (U + 1) * s - 2 * p, (U + 1) * s - 2 * p + s - 1}
    return tuple(sorted(T for T in Ts if T >= 1 and sconv_out_len(T, s, p) > 0))


SCONV = [Sconv(cin, 16, s, p, sconv_lengths(s, p)) for s in range(1, 9) for p in sconv_paddings(s) for cin in (32, 24)]


# ------------------------------------------------------------------------------------------------------------------------------
# the residual units
# ------------------------------------------------------------------------------------------------------------------------------
def unit_lengths(d, TN):
    return tuple(sorted({1, 3 * d, 3 * d + 1, TN - 1, TN, TN + 1, TN + 3 * d + 1, 2 * TN + 5}))


def _units():
    """every geometry asked for the fused launch (dilation 10 is not built: the handle must fall back to the four launches) and, where the fused
    kernel is built, for the four launches as well"""
    geo = ([("codec", 32, d, True) for d in range(1, 11)] + [("codec", 192, d, True) for d in (2, 8)]
           + [("aa", 32, d, True) for d in range(1, 11)] + [("aa", 128, d, True) for d in (2, 8)] + [("aa", 32, 4, False)])
    out = []
    for kind, C, d, beta in geo:
        u = Unit(kind, C, d, unit_lengths(d, CU_TN if kind == "codec" else AA_TN), True, beta)
        out.append(u)
        if u.built:
            out.append(Unit(kind, C, d, u.Ts, False, beta))
    return out


UNITS = _units()


# ------------------------------------------------------------------------------------------------------------------------------
# refusals: each raises _lib.AmpError with this status and a message holding this word, before any launch
# ------------------------------------------------------------------------------------------------------------------------------
REFUSALS = [
    Tconv(32, 16, 4, 4, 4, True, (8,), refuse=("create", AMP_ERR_INVALID, "output_padding")),        # output_padding >= stride
    Tconv(32, 16, 2, 3, 2, False, (8,), refuse=("create", AMP_ERR_INVALID, "output_padding")),
    Tconv(32, 16, 4, 1, 2, True, (8,), refuse=("create", AMP_ERR_UNSUPPORTED, "output_padding")),    # output_padding > padding
    Tconv(32, 16, 8, 0, 1, False, (8,), refuse=("create", AMP_ERR_UNSUPPORTED, "output_padding")),
    Tconv(32, 16, 4, 8, 0, True, (1,), refuse=("forward", AMP_ERR_INVALID, "T_out")),                # padding 2 s, T = 1: T_out = -8
    Tconv(32, 16, 3, 6, 2, False, (2,), refuse=("forward", AMP_ERR_INVALID, "T_out")),               # T_out = -1
    Tconv(32, 16, 5, 5, 0, True, (1,), refuse=("forward", AMP_ERR_INVALID, "T_out")),                # T_out = 0 exactly
    Sconv(32, 16, 4, 0, (7,), refuse=("forward", AMP_ERR_INVALID, "T_out")),                         # T + 2 p = 2 s - 1
    Sconv(32, 16, 8, 3, (9,), refuse=("forward", AMP_ERR_INVALID, "T_out")),
    Sconv(24, 16, 3, 1, (1,), refuse=("forward", AMP_ERR_INVALID, "T_out")),
    Unit("codec", 32, 0, (8,), refuse=("create", AMP_ERR_INVALID, "dilation")),
    Unit("codec", 32, -1, (8,), refuse=("create", AMP_ERR_INVALID, "dilation")),
    Unit("aa", 32, 0, (8,), refuse=("create", AMP_ERR_INVALID, "dilation")),
]

GROUPS = {"tconv_fused": TCONV_FUSED, "tconv_unfused": TCONV_UNFUSED, "sconv": SCONV, "units": UNITS}


def refusals(group):
    kinds = {"tconv_fused": (), "tconv_unfused": ("tconv",), "sconv": ("sconv",), "units": ("codec", "aa")}[group]
    return [c for c in REFUSALS if c.kind in kinds]


# ------------------------------------------------------------------------------------------------------------------------------
# the fused tconv's tiling and store branches, from the kernel's text
# ------------------------------------------------------------------------------------------------------------------------------
BRANCHES_S4 = ("float4", "float2x2", "scalar4", "edge4/lo", "edge4/hi")      # s % 4 == 0
BRANCHES_S2 = ("float2", "scalar2", "edge2/lo", "edge2/hi")                  # other even s
BRANCHES_S1 = ("scalar1",)                                                   # odd s


def stride_class_branches(s):
    return BRANCHES_S4 if s % 4 == 0 else BRANCHES_S2 if s % 2 == 0 else BRANCHES_S1


def tconv_row_quads(M):
    """the first rows m0 of the register quads tconv_rows stores, in the kernel's order, over both wm: wave (wm, .) sweeps the row blocks
    wm, wm + 2, .. in groups of 4, then 2, then 1; a lane half `hi` holds rows 4 hi + 8 j .. + 3 of a 32-row block.  -> (m0 list, the
    group sizes used)"""
    NRB = (M + 31) // 32
    m0s, groups = [], []
    for wm in (0, 1):
        rb = wm
        blocks = []
        while rb + 6 < NRB:
            blocks += [rb, rb + 2, rb + 4, rb + 6]
            groups.append(4)
            rb += 8
        if rb + 2 < NRB:
            blocks += [rb, rb + 2]
            groups.append(2)
            rb += 4
        if rb < NRB:
            blocks.append(rb)
            groups.append(1)
        for blk in blocks:
            assert blk < NRB
            for hi in (0, 1):
                for j in range(4):
                    m0s.append(blk * 32 + 4 * hi + 8 * j)
    return m0s, groups


def tconv_model(cout, s, p, op, T, batch=B):
    """-> dict(Tout, q_first, q_last, tiles, groups, branches {name: count}, owners int array [batch, cout, Tout]).
    y is taken as 16-byte aligned (the test helpers place it so); an element's byte alignment is then that of its flat index."""
    Tout = tconv_out_len(T, s, p, op)
    assert Tout > 0
    M = cout * s
    # amp_tconv_forward / launch_tconv
    q_first = p // s
    q_last = (Tout - 1 + p) // s
    nq = q_last - q_first + 1
    tiles = (nq + TC_TN - 1) // TC_TN
    m0s, groups = tconv_row_quads(M)
    m0 = np.array([m for m in m0s if m < M], dtype=np.int64)                 # `if (m0 >= a.M) return`
    q = q_first + np.arange(tiles * TC_TN, dtype=np.int64)                   # q0 + wn * 32 + l31 over the tiles of one item
    item = np.arange(batch, dtype=np.int64)[:, None, None]
    owners = np.zeros((batch, cout, Tout), dtype=np.int64)
    branches = {}

    def note(name, mask):
        n = int(mask.sum())
        if n:
            branches[name] = branches.get(name, 0) + n

    def write(o, t, mask):
        """one scalar lane of a store: rows o [m], samples t [m, q], mask [batch, m, q]"""
        ii, oo, tt = np.broadcast_arrays(item, o[None, :, None] if o.ndim == 1 else o, t[None])
        assert (tt[mask] >= 0).all() and (tt[mask] < Tout).all() and (oo[mask] < cout).all()
        np.add.at(owners, (ii[mask], oo[mask], tt[mask]), 1)

    tb = q * s - p                                                            # [q]
    o = m0 // s
    r = m0 - o * s
    full = np.ones((batch, len(m0), len(q)), dtype=bool)
    if s % 4 == 0:
        assert (r % 4 == 0).all() and (r + 3 < s).all() and M % 4 == 0
        t0 = tb[None, :] + r[:, None]                                         # [m, q]
        idx = (item * cout + o[None, :, None]) * Tout + t0[None]              # flat index of d
        inb = ((t0 >= 0) & (t0 + 3 < Tout))[None] & full
        a16, a8 = idx % 4 == 0, idx % 2 == 0
        note("float4", inb & a16)
        note("float2x2", inb & ~a16 & a8)
        note("scalar4", inb & ~a8)
        for e in range(4):
            write(o, t0 + e, inb)
        edge = ~inb
        lanes = [edge & ((t0 + e >= 0) & (t0 + e < Tout))[None] for e in range(4)]
        some = lanes[0] | lanes[1] | lanes[2] | lanes[3]
        note("edge4/lo", some & (t0 < 0)[None])
        note("edge4/hi", some & (t0 + 3 >= Tout)[None])
        for e in range(4):
            write(o, t0 + e, lanes[e])
    elif s % 2 == 0:
        assert (r % 2 == 0).all() and M % 2 == 0
        oo, rr = o.copy(), r.copy()
        for h in range(2):
            live = (m0 + 2 * h < M)[None, :, None] & full
            assert (rr + 1 < s).all()
            t0 = tb[None, :] + rr[:, None]
            idx = (item * cout + oo[None, :, None]) * Tout + t0[None]
            inb = ((t0 >= 0) & (t0 + 1 < Tout))[None] & full
            vec = live & inb & (idx % 2 == 0)
            note("float2", vec)
            note("scalar2", live & inb & ~vec)
            lanes = [live & ~vec & ((t0 + e >= 0) & (t0 + e < Tout))[None] for e in range(2)]
            some = (lanes[0] | lanes[1]) & ~inb
            note("edge2/lo", some & (t0 < 0)[None])
            note("edge2/hi", some & (t0 + 1 >= Tout)[None])
            write(oo, t0, vec)
            write(oo, t0 + 1, vec)
            for e in range(2):
                write(oo, t0 + e, lanes[e])
            rr = rr + 2
            wrap = rr >= s
            rr = np.where(wrap, 0, rr)
            oo = oo + wrap
    else:
        oo, rr = o.copy(), r.copy()
        for e in range(4):
            live = (m0 + e < M)[None, :, None] & full
            t1 = tb[None, :] + rr[:, None]
            ok = live & ((t1 >= 0) & (t1 < Tout))[None]
            note("scalar1", ok)
            write(np.minimum(oo, cout - 1), t1, ok)
            assert not (ok & (oo >= cout)[None, :, None]).any()
            rr = rr + 1
            wrap = rr >= s
            rr = np.where(wrap, 0, rr)
            oo = oo + wrap
    return dict(Tout=Tout, q_first=q_first, q_last=q_last, tiles=tiles, groups=groups, branches=branches, owners=owners)


def tconv_columns(s, p, op, T):
    """from the definition alone (u = t + p, q = u div s over t in [0, T_out)): the first and last column any output sample lies in"""
    Tout = tconv_out_len(T, s, p, op)
    qs = [(t + p) // s for t in (0, Tout - 1)]
    return qs[0], qs[1]


# ------------------------------------------------------------------------------------------------------------------------------
# tensors, fp64 references and the existing per-element bounds of a case (torch on the CPU; imported on use)
# ------------------------------------------------------------------------------------------------------------------------------
def _seed(case):
    if case.kind in ("tconv", "sconv"):
        return 1000 + 97 * case.s + 13 * case.p + 7 * case.cin + case.cout + (31 * case.op if case.kind == "tconv" else 5)
    return 2000 + 11 * case.d + case.C + (1 if case.kind == "aa" else 0)


def tensors(case):
    """the case's parameters in fp64, the conv weights folded and rounded to the fp32 values the library is given.  tconv / sconv:
    dict(w, b, alpha [1, cin, 1]); units: the unit's state_dict (codec_ref.unit_param_shapes / facodec_ref.unit_param_shapes) with
    `weight` in place of weight_g / weight_v; the betas dropped for plain Snake"""
    import codec_ref as C

    def fold(sd):
        out = {}
        for k, v in sd.items():
            if k.endswith("weight_g"):
                out[k[:-2]] = C.folded(sd, k[:-8]).float().double()
            elif not k.endswith("weight_v"):
                out[k] = v
        return out

    if case.kind == "tconv":
        import dac_ref as D

        shapes = {"a.alpha": (1, case.cin, 1)}
        D._wnT(shapes, "c.", case.cin, case.cout, 2 * case.s)
    elif case.kind == "sconv":
        shapes = {"a.alpha": (1, case.cin, 1)}
        C._wn(shapes, "c.", case.cout, case.cin, 2 * case.s)
    elif case.kind == "codec":
        return fold({k: v.double() for k, v in C._synth(C.unit_param_shapes(case.C), _seed(case)).items()})
    else:
        import facodec_ref as FR

        sd = fold({k: v.double() for k, v in FR.synth_unit_state_dict(case.C, _seed(case)).items()})
        return sd if case.beta else {k: v for k, v in sd.items() if not k.endswith("act.beta")}
    sd = fold({k: v.double() for k, v in C._synth(shapes, _seed(case)).items()})
    return dict(w=sd["c.weight"], b=sd["c.bias"], alpha=sd["a.alpha"])


def inputs(case, T, batch=B):
    import codec_ref as C

    return C.synth_latent(batch, case.cin if case.kind in ("tconv", "sconv") else case.C, T, _seed(case) + 3 * T + batch)


def reference(case, P, x, with_alpha=True):
    """(fp64 output, per-element bound) of one call: dac_ref.tconv_bound, codec_ref.sconv_bound / unit_bound, facodec_ref.unit_bound"""
    import codec_ref as C

    x = x.double()
    if case.kind == "tconv":
        import dac_ref as D

        return D.tconv_bound(P["w"], P["b"], P["alpha"] if with_alpha else None, x, case.s, case.p, case.op)
    if case.kind == "sconv":
        return C.sconv_bound(P["w"], P["b"], P["alpha"] if with_alpha else None, x, case.s, case.p)
    if case.kind == "codec":
        return C.unit_bound(P, x, case.d)
    import facodec_ref as FR

    return FR.unit_bound(P, x, case.d)
