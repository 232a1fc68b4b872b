// Device building blocks of the f16x3 kernels that contract host-packed A fragments, read from L2, against a B operand staged in LDS
// over its whole K extent (pw_f16x3.hip per K step; dsconv_f16x3.hip per K step with its own three-tap A pack; dw_layer_f16x3.hip and
// codec_unit_f16x3.hip at once, twice, around a seam; tconv_f16x3.hip at once, one GEMM, both taps one column apart in the same window):
//   A  [row block][k16][plane hi | lo][lane] x 16 B (amp_host.h: pack_a_f16x3 with taps = 1): a wave reads the fragment pair of
//      k-extent k of row block mb at wp[(mb * k16 + k) * 128 + lane] and + 64;
//   B  [plane hi | lo][channel octet][column][8 x f16], S columns wide: lane (hi, l31) reads the fragment of k-extent k, column c at
//      smem[(2 k + hi) * S + c] and + plane.
// Two-GEMM kernels: waves 2 x 2, wave (wm, wn) owns columns 32 wn .. 32 wn + 31 and row blocks wm, wm + 2, ..; GEMM 1's accumulators pass a
// seam function in registers, go x16 / split to the FRONT of the same LDS (after a barrier) and are GEMM 2's B operand, TN columns wide.
#pragma once
#include "f16x3_device.h"

namespace amp {

// the hi / lo pair of one staged quad (or any uint2 slot) of a B operand; plane2 = uint2 per plane
__device__ __forceinline__ void bplane_store(uint2* dst, int plane2, int idx, uint2 h, uint2 l) {
    dst[idx] = h;
    dst[plane2 + idx] = l;
}

// both planes of one B fragment; plane = uint4 per plane
__device__ __forceinline__ void bfrag_load(const uint4* smem, int plane, int off, Frag& bh, Frag& bl) {
    bh.u = smem[off];
    bl.u = smem[plane + off];
}

// the A fragment pairs of MI row blocks at one k-extent; wa points at (first row block, that k-extent, this lane), mbs = uint4 per row block
template <int MI>
__device__ __forceinline__ void afrag_load(Frag* ah, Frag* al, const uint4* wa, size_t mbs) {
#pragma unroll
    for (int i = 0; i < MI; ++i) {
        ah[i].u = wa[i * mbs];
        al[i].u = wa[i * mbs + 64];
    }
}

// Where the packed A of a wave's MI row blocks (mbs uint4 apart) lies: wa points at (first row block, k-extent 0, this lane).
struct APack {
    const uint4* wa;
    size_t mbs;
    int k16;
};

// acc[i][0] += A[row block i][k0 .. k0 + n) * B, B being n k-extents of an operand `stride` columns wide read from ITS k-extent 0 at
// lane offset rd = hi * stride + column.  One accumulator tile per row block; MI = 2 is one B fragment under two A streams (DiffWave's
// gate and filter rows), swept as mfma3_tiles does: hh of both, hl of both, lh of both.
// AHEAD: ah / al hold extent k0 on entry (afrag_load) and the loads of extent k + 1 fly under the MFMAs of extent k (the last extent
// re-reads itself: no pad entries, no branch) -- GEMM 1, whose K is long.  A conv tap is one call: rd moves on by tap * d over the same
// staged channels, k0 by the channels' extents, and the caller's ah / al carry the look-ahead across the calls.
// !AHEAD: extent k is read in step k -- GEMM 2, whose K = C is 2 .. 12 extents (ah / al are scratch then).  The two forms stay one text
// with a flag: split in two, GEMM 1 is 4 % slower on the DiffWave sampler (profiles/wholek_refactor_ab_15dfbb2.txt).
template <int MI, bool AHEAD>
__device__ __forceinline__ void gemm_wholek(f32x16 (*acc)[1], Frag* ah, Frag* al, const APack& A, int k0, int n, const uint4* smem, int plane,
                                            int stride, int rd) {
    for (int kc = 0; kc < n; ++kc) {
        const int k = k0 + kc;
        Frag nh[MI], nl[MI], bh, bl;
        if (AHEAD) {
            const int kn = k + 1 < A.k16 ? k + 1 : k;
            afrag_load<MI>(nh, nl, A.wa + kn * 128, A.mbs);
        } else {
            afrag_load<MI>(ah, al, A.wa + k * 128, A.mbs);
        }
        bfrag_load(smem, plane, 2 * kc * stride + rd, bh, bl);
        mfma3_tiles<MI, 1>(acc, ah, al, &bh, &bl);
        if (AHEAD) {
#pragma unroll
            for (int i = 0; i < MI; ++i) {
                ah[i] = nh[i];
                al[i] = nl[i];
            }
        }
    }
}

__device__ __forceinline__ void acc_zero(f32x16& acc) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
}

// The seam: z[pi][r] is GEMM 1's output (after the seam function) of row block p = wm + 2 pi, register r.  Registers 4j .. 4j + 3 of a
// lane are channels 32 p + 8 j + 4 hi + 0 .. 3 of column `col` = 32 wn + l31, the half `hi` of channel octet 4 p + j.  range_max: the caller's
// running maximum for the range flag, or nullptr where the seam function bounds |z| (DiffWave: |sigmoid * tanh| <= 1); snake does not.
template <int NPW>
__device__ __forceinline__ void seam_store(const float (*z)[16], uint2* dst, int plane2, int TN, int wm, int col, int hi, int NP, float* range_max) {
#pragma unroll
    for (int pi = 0; pi < NPW; ++pi) {
        const int p = wm + 2 * pi;
        if (p >= NP) break;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            uint2 sh, sl;
            if (range_max) {
                stage4_f16(z[pi][4 * j], z[pi][4 * j + 1], z[pi][4 * j + 2], z[pi][4 * j + 3], 16.f, 16.f, *range_max, sh, sl);
            } else {
                const amp_f32x2 v01 = {z[pi][4 * j] * 16.f, z[pi][4 * j + 1] * 16.f};
                const amp_f32x2 v23 = {z[pi][4 * j + 2] * 16.f, z[pi][4 * j + 3] * 16.f};
                split4_f16(v01, v23, sh, sl);
            }
            bplane_store(dst, plane2, bplane_idx(2 * (p * 4 + j) + hi, col, TN), sh, sl);
        }
    }
}

}  // namespace amp
