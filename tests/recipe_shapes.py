"""The distinct layers of the four vocoder recipes the suite had never run, and the conv launch policy that picks their kernels.

Recipes (oracle/vocoder_oracle.py): bigvgan_large_hp, tfr_hifigan_hp, nsfhifigan_recipe_hp and hifigan_recipe_hp (resblock "2").
Every layer is listed once with the recipes it occurs in: conv_pre, every ConvTranspose1d, every resblock conv (C, k, dilation) and
every conv_post.  `form()` restates conv_run's choice (amphion_amd/csrc/conv_host.hip) so that each case can be sized to reach the
kernel it names; the tests assert the kernel from the launch manifest, so a restatement that drifts from the library fails loudly.
"""
from dataclasses import dataclass

N_MEL = {"bigvgan_large": 100, "tfr": 100, "nsf": 100, "hifigan_rb2": 80}
TAPS = (1, 2, 3, 5, 7, 11)                       # conv_host.hip: ConvTaps
SMALL_GRID_WGS = 384                             # kSmallGridWorkgroups
BLK_MIN_WGS = 512                                # kConvBlkMinWorkgroups
RG_FAST_MAX_BYTES = 3 << 20                      # kConvRgFastMaxWeightBytes
SMALL_MAX_CHUNKS = 16                            # kSmallConvMaxChunks


def recipe_hps():
    from oracle import vocoder_oracle as vo

    return {"bigvgan_large": vo.bigvgan_large_hp(), "tfr": vo.tfr_hifigan_hp(), "nsf": vo.nsfhifigan_recipe_hp(),
            "hifigan_rb2": vo.hifigan_recipe_hp()}


@dataclass(frozen=True)
class Op:
    cin: int
    cout: int
    k: int
    d: int = 1
    u: int = 0                                   # > 0: ConvTranspose1d with stride u
    pad: int = None                              # explicit padding; None: the recipes' (k - u) // 2 / 'same'

    @property
    def transposed(self):
        return self.u > 0

    @property
    def padding(self):
        if self.pad is not None:
            return self.pad
        return (self.k - self.u) // 2 if self.u else (self.k * self.d - self.d) // 2

    @property
    def name(self):
        p = "" if self.pad is None else f"p{self.pad}"
        if self.u:
            return f"convT{self.cin}-{self.cout}u{self.u}k{self.k}{p}"
        return f"conv{self.cin}-{self.cout}k{self.k}d{self.d}{p}"

    def kwargs(self):
        if self.u:
            return dict(transposed=True, stride=self.u, padding=self.padding)
        return dict(dilation=self.d, padding=self.padding)

    def out_len(self, T):
        if self.u:
            return (T - 1) * self.u - 2 * self.padding + self.k
        return T + 2 * self.padding - self.d * (self.k - 1)

    # ---- the GEMM view (conv_host.hip: conv_build) ----
    @property
    def M(self):
        return self.cout * (self.u or 1)

    @property
    def ntaps(self):
        return -(-self.k // self.u) if self.u else self.k

    @property
    def KT(self):
        return next(t for t in TAPS if t >= self.ntaps)

    @property
    def halo(self):
        if self.u > 1:
            return self.KT - 1
        # stride 1: conv_build runs a ConvTranspose1d as the Conv1d with flipped taps and padding k - 1 - p
        pc = self.k - 1 - self.padding if self.u else self.padding
        lo, hi = -pc, -pc + (self.KT - 1) * self.d
        return max(0, -lo) + max(0, hi)

    @property
    def WM(self):
        return 4 if self.M > 64 else 2 if self.M > 32 else 1

    @property
    def group_rows(self):
        return 32 * self.WM

    @property
    def padded_rows(self):
        return -self.M % self.group_rows

    @property
    def K(self):
        return self.cin * self.ntaps

    def form(self, B, T, precision="f16x3"):
        """(kernel id as tests/test_gpu_recipe_shapes.py names it, GEMM rows per launch group, tile width in output columns)"""
        Tq = T + self.ntaps - 1 if self.u > 1 else self.out_len(T)
        if precision == "f32":
            return "conv_mfma_kernel", self.group_rows, None
        WN = 4 // self.WM
        Mg = self.group_rows
        NI = 4
        nchunks = -(-self.cin // 16)
        if B * -(-Tq // (32 * NI * WN)) * -(-self.M // Mg) < SMALL_GRID_WGS:
            NI = 2
        wgs_half = B * -(-Tq // 64) * -(-self.M // Mg)
        blk_kt = self.KT in (2, 3, 7, 11)
        wn = 1 if self.M % 256 == 0 else 2 if (self.M % 128 == 0 and self.KT != 2 and self.KT >= 7) else 0
        if NI == 4 and wn and blk_kt:
            cm = 2 if self.KT == 2 and nchunks % 2 == 0 else 1
            nt1 = (96 if self.halo <= 32 else 0) if self.KT == 2 else (128 if self.halo <= 64 else 0)
            nt = wn * nt1
            if nt and B * -(-Tq // nt) * (self.M // (256 // wn)) >= BLK_MIN_WGS:
                rows = 256 // wn
                wbytes = (-(-self.M // Mg) * Mg) * nchunks * 16 * self.KT * 4
                grid = "2d" if (self.M // rows > 1 and wbytes > RG_FAST_MAX_BYTES) else "1d"    # one row group: grid.y = 1 either way
                return f"conv_blk_kernel/k{self.KT}/wn{wn}/{grid}", rows, nt * (self.u or 1)
        small = (not self.u and self.WM == 4 and self.KT in (1, 3, 5, 7, 11) and self.KT == self.ntaps and nchunks <= SMALL_MAX_CHUNKS
                 and self.halo <= 64)
        if NI == 2 and small and (self.KT <= 5 or wgs_half <= 128):
            return "conv_small_kernel", 128, 32 * (1 if self.halo <= 32 else 2)
        return "conv_f16x3_kernel", Mg, 32 * NI * WN * (self.u or 1)


def recipe_ops():
    """{Op: sorted recipe names} over the four recipes: conv_pre, ups, every resblock conv (c1 at each dilation, c2 at 1 / resblock 2's
    dilated convs) and conv_post"""
    ops = {}
    for rname, hp in recipe_hps().items():
        c0 = hp["upsample_initial_channel"]
        add = lambda op: ops.setdefault(op, set()).add(rname)
        add(Op(N_MEL[rname], c0, 7, 1))
        for i, (u, k) in enumerate(zip(hp["upsample_rates"], hp["upsample_kernel_sizes"])):
            add(Op(c0 // 2 ** i, c0 // 2 ** (i + 1), k, u=u))
            C = c0 // 2 ** (i + 1)
            for kk, ds in zip(hp["resblock_kernel_sizes"], hp["resblock_dilation_sizes"]):
                for d in ds:
                    add(Op(C, C, kk, d))
                if hp["resblock"] == "1":
                    add(Op(C, C, kk, 1))
        add(Op(c0 // 2 ** len(hp["upsample_rates"]), 1, 7, 1))
    return {op: sorted(r) for op, r in ops.items()}
