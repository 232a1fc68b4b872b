"""The geometry table of amp_conv_create / amp_conv_forward: Conv1d and ConvTranspose1d over stride, kernel size, padding, dilation, length
and batch, well outside the corner the vocoder recipes use (tests/recipe_shapes.py).  Plain data and pure functions: the CPU tests
(tests/test_conv_geometry_ref.py) pin the fp64 reference on these geometries and assert that every axis value below occurs, the GPU test
(tests/test_gpu_conv_geometry.py) runs every case through the C ABI.

A case names its length either directly or relative to the launch's tile (`tiles`, `delta`: the GEMM columns of the launch are
tiles * tile + delta, the tile width from Op.form()), so that "one tile - 1 / one tile / one tile + 1 / ragged last tile" stay what they
say if the launch policy moves.  `refuse` cases must raise instead of launching: (stage, status, word the message must hold).
"""
from dataclasses import dataclass, field

from recipe_shapes import Op

AMP_ERR_INVALID, AMP_ERR_UNSUPPORTED = -1, -4
OPT_PAD_REFLECT, OPT_TANH = 1, 2


@dataclass(frozen=True)
class Case:
    op: Op
    B: int = 1
    T: int = 0                                   # input length; 0: from (tiles, delta)
    tiles: int = 0
    delta: int = 0
    grid: str = "small"
    bias: bool = True
    res: bool = False
    slope_in: float = 0.1
    slope_out: float = 1.0
    options: tuple = ()                          # amp_conv_set_option pairs
    refuse: tuple = None                         # (stage: create | option | forward | ragged, amp_status, word in the message)
    tags: frozenset = field(default_factory=frozenset)

    @property
    def id(self):
        B, T = self.shape()
        return f"{self.op.name}/B{B}T{T}" + ("/" + "+".join(sorted(self.tags)) if self.tags else "")

    def q_tile(self):
        """GEMM columns per workgroup tile of this case's launch (f16x3): the tile in output columns / the polyphase factor"""
        B, T = self.B, self.T or 64
        tile = self.op.form(B, T)[2]
        return tile // (self.op.u if self.op.u > 1 else 1)

    def shape(self):
        """(B, T)"""
        if self.T:
            return self.B, self.T
        if self.grid == "large":
            return large_shape(self)
        op = self.op
        Tq = self.tiles * self.q_tile() + self.delta
        # GEMM columns: T + ntaps - 1 for a polyphase ConvTranspose1d, T_out otherwise
        T = Tq - (op.ntaps - 1) if op.u > 1 else Tq - (op.out_len(0))
        assert T >= 1 and op.out_len(T) >= 1, (self.op, T)
        return self.B, T


def _t(op, **kw):
    return Case(op, **kw)


def _ct(cin, cout, k, s, p, **kw):
    return Case(Op(cin, cout, k, 1, s, p), **kw)


def _c(cin, cout, k, d, p, **kw):
    return Case(Op(cin, cout, k, d, 0, p), **kw)


def same(k, d=1):
    return d * (k - 1) // 2


# ------------------------------------------------------------------------------------------------------------------------------
# ConvTranspose1d, small grid (one short item or three: the half-width conv_f16x3 tiles), cin <= 64
# ------------------------------------------------------------------------------------------------------------------------------
CONVT_SMALL = [
    # ---- stride 1: runs as the equivalent Conv1d (flipped taps, padding k - 1 - p) ----
    _ct(16, 24, 3, 1, 1, T=37),
    _ct(16, 24, 4, 1, 0, B=3, T=2),
    _ct(8, 40, 7, 1, 5, tiles=1, delta=1),
    _ct(8, 8, 5, 1, 6, T=40),                                  # padding > k - 1: the equivalent Conv1d has a negative padding
    _ct(16, 128, 3, 1, 1, B=3, tiles=3, delta=17),             # full 128-row blocks and whole tiles: the kernels' unpredicated store path
    _ct(8, 16, 11, 1, 5, T=70),                                # 11 taps
    # ---- stride 2: the 8-byte store path, even and odd padding ----
    _ct(24, 40, 6, 2, 2, T=50),                                # k = 3 stride, even padding, rows 80: padded last block
    _ct(32, 16, 4, 2, 1, B=3, tiles=2, delta=9),               # odd padding, rows 32: the vector path in every block
    _ct(16, 20, 3, 2, 0, T=1),                                 # k no multiple of the stride, padding 0, T = 1
    _ct(16, 16, 2, 2, 0, tiles=1, delta=0),                    # k == stride
    _ct(16, 16, 1, 2, 0, T=33),                                # k < stride: every other output is bias only
    _ct(16, 16, 8, 2, 3, T=41, bias=False),                    # 4 taps -> 5
    _ct(8, 16, 12, 2, 5, T=19, slope_out=0.2),                 # 6 taps -> 7
    _ct(8, 16, 22, 2, 10, T=30),                               # 11 taps
    _ct(16, 32, 5, 2, 2, T=64, res=True),                      # k - stride odd with even padding, residual
    # ---- stride 3, 5, 6: no vector path ----
    _ct(16, 8, 7, 3, 2, T=29),
    _ct(8, 24, 3, 3, 0, B=3, T=2),
    _ct(8, 8, 2, 3, 0, T=21),                                  # k < stride
    _ct(8, 12, 9, 3, 3, tiles=1, delta=-1),                    # k = 3 stride
    _ct(8, 8, 10, 5, 2, T=37),                                 # k = 2 stride, k - stride odd, rows 40
    _ct(8, 8, 4, 5, 0, T=13, bias=False),                      # k < stride
    _ct(8, 12, 12, 6, 3, T=25),                                # rows 72
    # ---- stride 4: float4 path (padding % 4 == 0) with k % 4 = 0, 1, 2, 3; generic path (padding % 4 != 0) ----
    _ct(16, 8, 8, 4, 0, T=3, tags={"float4"}),
    _ct(16, 16, 9, 4, 0, T=3, tags={"float4"}),
    _ct(16, 8, 6, 4, 0, T=3, tags={"float4"}),
    _ct(32, 8, 7, 4, 0, B=3, tiles=2, delta=5, tags={"float4"}),
    _ct(16, 16, 12, 4, 4, tiles=1, delta=1, tags={"float4"}),   # k = 3 stride, padding (k - stride) // 2 = 4
    _ct(16, 16, 10, 4, 4, T=3, slope_out=0.2, tags={"float4"}),
    _ct(16, 8, 8, 4, 2, T=35),                                 # (k - stride) // 2 = 2: generic path
    _ct(16, 8, 7, 4, 1, T=35),                                 # k - stride odd
    _ct(16, 10, 8, 4, 0, T=20, tags={"float4"}),               # rows 40: float4 in block 0, the padded block 1 on the generic path
    _ct(16, 8, 3, 4, 0, T=9, tags={"float4"}),                 # k < stride at a float4 stride
    _ct(16, 8, 8, 4, 11, T=5),                                 # the largest padding with T_out > 0 (T_out = 2)
    _ct(16, 8, 10, 4, 12, T=7, tags={"float4"}),               # large padding on the float4 path (T_out = 10)
    # ---- stride 8 ----
    _ct(16, 25, 16, 8, 4, B=3, T=9, tags={"float4"}),          # rows 200: padded last block
    _ct(16, 4, 18, 8, 4, T=3, tags={"float4"}),                # k % 4 = 2
    _ct(64, 8, 21, 8, 8, T=17, tags={"float4"}),               # k % 4 = 1, three taps
    _ct(16, 8, 19, 8, 4, T=5, tags={"float4"}),                # k % 4 = 3
    _ct(16, 8, 16, 8, 3, T=33),                                # padding % 4 != 0
    _ct(16, 8, 12, 8, 0, tiles=1, delta=0, tags={"float4"}),   # k no multiple of the stride
    _ct(16, 16, 16, 8, 4, B=1, tiles=1, delta=-1, res=True, tags={"float4"}),
    # ---- stride 16 ----
    _ct(8, 4, 32, 16, 8, T=11, tags={"float4"}),
    _ct(8, 2, 20, 16, 2, T=11),
    _ct(8, 6, 35, 16, 12, T=6, tags={"float4"}),               # k % 4 = 3, rows 96
]

# ------------------------------------------------------------------------------------------------------------------------------
# ConvTranspose1d, large grid: rows a multiple of 256 and enough tiles for the row-blocked kernel (conv_blk /k2, /k3, /k7)
# ------------------------------------------------------------------------------------------------------------------------------
CONVT_LARGE = [
    _ct(32, 64, 16, 8, 4, B=3, grid="large", tags={"float4"}),            # /k2, two chunks per round (nchunks even)
    _ct(48, 64, 18, 8, 4, B=3, grid="large", tags={"float4"}),            # /k3, k % 4 = 2
    _ct(48, 64, 6, 4, 0, B=3, grid="large", tags={"float4"}),             # /k2, one chunk per round (nchunks odd), k % 4 = 2
    _ct(16, 64, 7, 4, 0, B=3, grid="large", tags={"float4"}),             # /k2, k % 4 = 3
    _ct(32, 64, 9, 4, 0, B=1, grid="large", tags={"float4"}),             # /k3, k % 4 = 1
    _ct(32, 32, 16, 8, 3, B=3, grid="large"),                             # /k2, generic scatter
    _ct(32, 128, 4, 2, 1, B=3, grid="large"),                             # /k2, 8-byte stores, odd padding
    _ct(16, 128, 5, 2, 2, B=3, grid="large", slope_out=0.2),              # /k3, 8-byte stores, even padding
    _ct(16, 16, 32, 16, 8, B=3, grid="large", bias=False, tags={"float4"}),   # /k2, stride 16
    _ct(16, 64, 22, 4, 0, B=1, grid="large", tags={"float4"}),            # /k7 (6 taps -> 7), k % 4 = 2
]

# ------------------------------------------------------------------------------------------------------------------------------
# Conv1d, small grid: the zero-padded tap counts, paddings other than 'same', the halo limit
# ------------------------------------------------------------------------------------------------------------------------------
CONV_SMALL = [
    _c(16, 24, 2, 1, 0, T=37, slope_in=1.0),
    _c(16, 96, 4, 1, same(4), T=100),                          # 'same' of an even k: T_out = T - 1
    _c(24, 128, 6, 2, same(6, 2), B=3, tiles=2, delta=3),      # 6 taps -> 7: not the whole-K kernel
    _c(16, 32, 8, 1, same(8) + 1, T=50, res=True, slope_out=0.2),
    _c(8, 16, 9, 3, same(9, 3) - 1, T=77),
    _c(8, 16, 10, 1, 0, T=30),
    _c(16, 128, 3, 1, 0, B=3, tiles=1, delta=1),               # 'valid', whole-K kernel
    _c(16, 128, 7, 2, same(7, 2) + 1, T=90, res=True, slope_out=0.2),     # T_out = T + 2 with a residual of that length
    _c(16, 128, 11, 1, same(11) - 1, tiles=1, delta=-1),
    _c(16, 80, 3, 2, 5, T=44, res=True, slope_out=0.2),        # padding > dilation (k - 1): the first and last outputs are bias only
    _c(32, 128, 3, 1, same(3), tiles=1, delta=0),
    _c(16, 16, 7, 1, same(7), T=1),
    _c(16, 16, 11, 1, same(11), T=2, bias=False),
    _c(8, 16, 3, 64, 64, T=300),                               # receptive field exactly the 128-column halo
    _c(8, 16, 2, 128, 64, T=300),
    _c(8, 16, 7, 4, 12, T=5),                                  # T shorter than the receptive field (25), T_out = 5
    _c(8, 16, 4, 3, 4, T=3),                                   # T_out = 2
    _c(16, 24, 7, 2, 6, T=7, options=((OPT_PAD_REFLECT, 1),), slope_in=1.0, tags={"reflect"}),   # p = T - 1, the largest allowed
    _c(16, 3, 4, 1, 2, T=45, options=((OPT_TANH, 1),), tags={"tanh"}),
]

# ------------------------------------------------------------------------------------------------------------------------------
# refusals: each raises _lib.AmpError with this status and a message holding this word, before any launch
# ------------------------------------------------------------------------------------------------------------------------------
REFUSALS = [
    _ct(8, 8, 24, 2, 11, T=16, refuse=("create", AMP_ERR_UNSUPPORTED, "taps"), tags={"12taps"}),
    _ct(8, 8, 12, 1, 5, T=16, refuse=("create", AMP_ERR_UNSUPPORTED, "taps"), tags={"12taps"}),
    Case(Op(8, 8, 4, 2, 2, 1), T=16, refuse=("create", AMP_ERR_UNSUPPORTED, "dilat"), tags={"dilatedT"}),
    _c(8, 16, 2, 129, 64, T=300, refuse=("create", AMP_ERR_UNSUPPORTED, "halo"), tags={"halo129"}),
    _c(8, 16, 3, 1, 129, T=300, refuse=("create", AMP_ERR_UNSUPPORTED, "padding"), tags={"halo129"}),
    _ct(16, 8, 8, 4, 12, T=5, refuse=("forward", AMP_ERR_INVALID, "T_out"), tags={"Tout0"}),
    _c(8, 16, 7, 1, 0, T=6, refuse=("forward", AMP_ERR_INVALID, "T_out"), tags={"Tout0"}),
    _c(16, 24, 7, 2, 6, T=6, options=((OPT_PAD_REFLECT, 1),), refuse=("forward", AMP_ERR_INVALID, "reflection"), tags={"reflect"}),
    _ct(16, 8, 8, 4, 2, T=16, options=((OPT_PAD_REFLECT, 1),), refuse=("option", AMP_ERR_UNSUPPORTED, "transposed"), tags={"reflect"}),
    _ct(16, 8, 8, 4, 2, T=16, options=((OPT_TANH, 1),), refuse=("option", AMP_ERR_UNSUPPORTED, "transposed"), tags={"tanh"}),
    _ct(16, 8, 8, 4, 2, T=16, refuse=("ragged", AMP_ERR_UNSUPPORTED, "lengths"), tags={"lens"}),
    _ct(16, 8, 3, 1, 1, T=16, refuse=("ragged", AMP_ERR_UNSUPPORTED, "lengths"), tags={"lens"}),
    _c(16, 8, 3, 1, 0, T=16, refuse=("ragged", AMP_ERR_UNSUPPORTED, "lengths"), tags={"lens"}),
]

BLK_MIN_TILES_FACTOR = 1.25


def large_shape(case):
    """(B, T) of a large-grid case: 1.25 x the smallest length at which the launch policy takes the row-blocked kernel, plus a ragged
    last tile (as tests/test_gpu_recipe_shapes.py sizes its large grid)"""
    op, B = case.op, case.B
    T0 = next(T for T in range(16, 1 << 20, 16) if op.form(B, T)[0].startswith("conv_blk"))
    T = int(T0 * BLK_MIN_TILES_FACTOR) + 7
    assert op.form(B, T)[0] == op.form(B, T0)[0], op
    return B, T


def shape(case):
    return case.shape()


def run_cases():
    return CONVT_SMALL + CONVT_LARGE + CONV_SMALL


def all_cases():
    return run_cases() + REFUSALS


def describe(case):
    """the axis values of one case, for the coverage test"""
    op = case.op
    B, T = shape(case) if case.refuse is None else (case.B, case.T)
    d = dict(transposed=op.transposed, stride=op.u, k=op.k, dilation=op.d, padding=op.padding, B=B, T=T, Tout=op.out_len(T),
             rows=op.M, bias=case.bias, res=case.res, slope_in=case.slope_in, slope_out=case.slope_out)
    if case.refuse is None:
        form, _, tile = op.form(B, T)
        q = tile // (op.u if op.u > 1 else 1)
        Tq = T + op.ntaps - 1 if op.u > 1 else op.out_len(T)
        d.update(form=form, Tq=Tq, q_tile=q, ntaps=op.ntaps, KT=op.KT, halo=op.halo, nchunks=-(-op.cin // 16))
    return d
