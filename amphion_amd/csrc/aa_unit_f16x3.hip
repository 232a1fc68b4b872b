// The residual unit of FACodec (models/codec/ns3_codec/facodec.py: ResidualUnit with Activation1d(SnakeBeta) in place of Snake1d) in one launch:
//     y = x + conv1x1( A2( conv7_dil( A1(x) ) ) ),      A = down2( snake( up2(.) ) ), 12 taps each way (act1d_math.h, small_kernels.hip: act1d)
// as the two GEMMs around a seam of wholek_f16x3.h -- the sibling of codec_unit_f16x3.hip, whose staging and seam are element-wise.  Here both are
// FIRs along time with an 11-column reach (y[t] depends on x[t - 5 .. t + 5]), so:
//   * one workgroup owns AA_TN = 54 output columns of one item and all C rows; GEMM 1 runs over AA_N1 = 64 = 54 + 2 * 5 columns (t = q0 - 5 + c),
//     from a staged A1(x) window of W = 64 + 6 d columns (t = q0 - 5 - 3 d + w);
//   * an activation runs in rounds of channels through an fp32 row buffer in LDS: every thread forms runs of four Snake PAIRS (s[2j - 1], s[2j]
//     share their six taps of the input, as in act1d_kernel) -> barrier -> every thread filters four channels of one column down and splits them
//     into the operand planes.  Per element the operation order is act1d_kernel's;
//   * GEMM 1's accumulators (+ bias) stay in registers until every wave has left the staged operand, then pass one 32-row block at a time through
//     an fp32 tile in LDS, where A2 reads them along time.
// Two padding rules meet here.  The conv pads ITS input with zeros: a staged column outside [0, T) is selected to 0 after the activation.  The
// activation pads by replication at the ITEM's ends: every read of x or of conv 1's output z is at clamp(t, 0, T - 1) and every read of a Snake
// value at clamp(n, 0, 2 T - 1), so a halo column of GEMM 1 outside [0, T) is computed and never read.  T < 6 is the same text with every index
// clamped.  Every output has one owner, the summation order is fixed, no atomics except the range flag, which both staged operands feed.
#include "act1d_math.h"
#include "wholek_f16x3.h"

namespace amp {

constexpr int AA_CH1 = 16;              // channels per round of A1
constexpr int AA_ZS = 72;               // row stride of the fp32 tile of conv 1's output (64 columns; 72: the two lane halves land 32 banks apart)
constexpr int AA_SROW2 = 2 * AA_TN + 10;

// Snake values of `nch` channels into sbuf[ch * srow + i], i = n - n0 < 2 * npairs, n0 = 2 * j_first - 1: pair p is (s[2j - 1], s[2j]), j = j_first + p,
//     u[n] = sum_k in(j + 2 - k) * fu2[par + 2 k]   (par = 0 for n = 2j - 1, 1 for n = 2j),   s = u + invb * sin^2(a u)
// -- act1d_kernel's chains.  in(ch, t) returns the input at clamp(t, 0, T - 1).
template <class In>
__device__ __forceinline__ void aa_up_snake(In in, float* sbuf, int srow, int nch, int npairs, int j_first, const float (&fu2)[12], const float* a_,
                                            const float* invb_, int tid) {
    const int runs = (npairs + 3) >> 2;
    for (int idx = tid; idx < nch * runs; idx += 256) {
        const int ch = idx / runs;
        const int p0 = (idx - ch * runs) * 4;
        const int j0 = j_first + p0;
        float xv[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) xv[i] = in(ch, j0 - 3 + i);
        const float al = a_[ch], ib = invb_[ch];
        float* row = sbuf + ch * srow + 2 * p0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (p0 + q >= npairs) break;
            f32x2 u = pk_splat(0.f);
#pragma unroll
            for (int k = 0; k < 6; ++k) u = pk_fma(pk_splat(xv[q + 5 - k]), (f32x2){fu2[2 * k], fu2[2 * k + 1]}, u);
            const f32x2 xa = u * al;
            const f32x2 s2 = {snake_sin2(xa.x), snake_sin2(xa.y)};
            const f32x2 s = pk_fma(pk_splat(ib), s2, u);
            *reinterpret_cast<float2*>(row + 2 * q) = make_float2(s.x, s.y);
        }
    }
}

// y[t] = sum_j fd[j] * s[clamp(2 t + j - 5, 0, 2 T - 1)] from a row of Snake values: b = the buffer index of tap 0 (even), [lo, hi] = the buffer
// indices of n = 0 and n = 2 T - 1.  Two chains (even taps, odd taps) added at the end, as act1d_kernel does.
__device__ __forceinline__ float aa_down(const float* srow, int b, int lo, int hi, const float (&fd)[12]) {
    f32x2 acc = pk_splat(0.f);
    if (b >= lo && b + 11 <= hi) {
#pragma unroll
        for (int m = 0; m < 6; ++m) {
            const float2 v = *reinterpret_cast<const float2*>(srow + b + 2 * m);
            acc = pk_fma((f32x2){fd[2 * m], fd[2 * m + 1]}, (f32x2){v.x, v.y}, acc);
        }
    } else {
#pragma unroll
        for (int m = 0; m < 6; ++m) {
            int i0 = b + 2 * m, i1 = b + 2 * m + 1;
            i0 = i0 < lo ? lo : (i0 > hi ? hi : i0);
            i1 = i1 < lo ? lo : (i1 > hi ? hi : i1);
            acc = pk_fma((f32x2){fd[2 * m], fd[2 * m + 1]}, (f32x2){srow[i0], srow[i1]}, acc);
        }
    }
    return acc.x + acc.y;
}

template <int NPW>   // row blocks per wave: ceil(C / 64)
__global__ __launch_bounds__(256) void aa_unit_f16x3_kernel(const AaUnitArgs a) {
    constexpr int TN = AA_TN, N1 = AA_N1;
    // GEMM 1: [2 planes][C / 8 octets][W] operand, then [AA_CH1][2 W + 10] Snake values.  After it: [2][C / 8][64] seam operand, the fp32 tile
    // [32][AA_ZS], [32][AA_SROW2] Snake values.
    extern __shared__ __attribute__((aligned(16))) uint4 aa_smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int hi = lane >> 5, l31 = lane & 31;
    const int item = blockIdx.x / a.tiles_per_item;
    const int q0 = (blockIdx.x - item * a.tiles_per_item) * TN;
    const int C = a.C, T = a.T, d = a.d;
    const int NP = C >> 5;
    const int W = N1 + 6 * d;                 // staged columns: t = ta + w
    const int ta = q0 - 5 - 3 * d;
    const int NO = C >> 3;                    // channel octets
    const int PLANE = NO * W;                 // uint4 per plane

    const float* xb = a.x + (size_t)item * C * T;
    float fu2[12], fd[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) { fu2[k] = 2.f * a.filt[k]; fd[k] = a.filt[12 + k]; }

    // ---- stage A1(x) ----
    float range_max = 0.f;
    {
        float* sbuf = reinterpret_cast<float*>(aa_smem + 2 * PLANE);
        const int srow = 2 * W + 10;
        const int n0 = 2 * ta - 5;            // n of buffer index 0
        const int lo = -n0, shi = 2 * T - 1 - n0;
        uint2* dst = reinterpret_cast<uint2*>(aa_smem);
        for (int c0 = 0; c0 < C; c0 += AA_CH1) {
            const float* xc = xb + (size_t)c0 * T;
            aa_up_snake([&](int ch, int t) { t = t < 0 ? 0 : (t > T - 1 ? T - 1 : t); return xc[(size_t)ch * T + t]; }, sbuf, srow, AA_CH1, W + 5, ta - 2, fu2,
                        a.a1 + c0, a.invb1 + c0, tid);
            __syncthreads();
            for (int idx = tid; idx < (AA_CH1 / 4) * W; idx += 256) {
                const int ql = idx / W;
                const int w = idx - ql * W;
                const int t = ta + w;
                float v[4] = {0.f, 0.f, 0.f, 0.f};
                if (t >= 0 && t < T) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = aa_down(sbuf + (4 * ql + e) * srow, 2 * w, lo, shi, fd);
                }
                uint2 fh, fl;
                stage4_f16(v[0], v[1], v[2], v[3], 16.f, 16.f, range_max, fh, fl);
                bplane_store(dst, 2 * PLANE, bplane_idx((c0 >> 2) + ql, w, W), fh, fl);
            }
            __syncthreads();
        }
    }

    // ---- GEMM 1 (k = 7, dilation d) + bias, kept in registers until every wave has left the staged operand ----
    const int KC = C >> 4;                    // 16-channel chunks per tap
    const int K16 = 7 * KC;
    float z[NPW][16];
    const int col = wn * 32 + l31;
#pragma unroll
    for (int pi = 0; pi < NPW; ++pi) {
        const int p = wm + 2 * pi;
        if (p >= NP) break;
        f32x16 acc[1][1];
        acc_zero(acc[0][0]);
        const APack A{a.wp1 + (size_t)p * K16 * 128 + lane, 0, K16};
        Frag ah, al;
        afrag_load<1>(&ah, &al, A.wa, 0);
        for (int tap = 0; tap < 7; ++tap) gemm_wholek<1, true>(acc, &ah, &al, A, tap * KC, KC, aa_smem, PLANE, W, hi * W + col + tap * d);
#pragma unroll
        for (int r = 0; r < 16; ++r) z[pi][r] = acc[0][0][r] * a.inv1 + a.bias1[acc_row(r, hi, p * 32)];
    }
    __syncthreads();

    // ---- the seam: A2 along time, one 32-row block at a time ----
    const int PLANE2 = NO * N1;
    {
        float* zbuf = reinterpret_cast<float*>(aa_smem + 2 * PLANE2);
        float* sbuf = zbuf + 32 * AA_ZS;
        const int n0 = 2 * q0 - 5;
        const int lo = -n0, shi = 2 * T - 1 - n0;
        const int zoff = q0 - 5;              // t of the tile's column 0
        uint2* dst = reinterpret_cast<uint2*>(aa_smem);
#pragma unroll
        for (int pi = 0; pi < NPW; ++pi) {
#pragma unroll
            for (int par = 0; par < 2; ++par) {
                const int p = 2 * pi + par;
                if (p >= NP) break;
                if (wm == par) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) zbuf[acc_row(r, hi) * AA_ZS + col] = z[pi][r];
                }
                __syncthreads();
                aa_up_snake([&](int ch, int t) { t = t < 0 ? 0 : (t > T - 1 ? T - 1 : t); return zbuf[ch * AA_ZS + (t - zoff)]; }, sbuf, AA_SROW2, 32, TN + 5,
                            q0 - 2, fu2, a.a2 + p * 32, a.invb2 + p * 32, tid);
                __syncthreads();
                for (int idx = tid; idx < 8 * N1; idx += 256) {
                    const int ql = idx >> 6;
                    const int c = idx & 63;
                    float v[4] = {0.f, 0.f, 0.f, 0.f};
                    if (c < TN && q0 + c < T) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = aa_down(sbuf + (4 * ql + e) * AA_SROW2, 2 * c, lo, shi, fd);
                    }
                    uint2 sh, sl;
                    stage4_f16(v[0], v[1], v[2], v[3], 16.f, 16.f, range_max, sh, sl);
                    bplane_store(dst, 2 * PLANE2, bplane_idx(p * 8 + ql, c, N1), sh, sl);
                }
            }
        }
    }
    raise_range(a.range_flag, range_max, lane);
    __syncthreads();

    // ---- GEMM 2 (1 x 1) + bias + residual ----
    const int q = q0 + col;
    for (int rb = wm; rb < NP; rb += 2) {
        f32x16 acc[1][1];
        acc_zero(acc[0][0]);
        Frag ah, al;
        gemm_wholek<1, false>(acc, &ah, &al, APack{a.wp2 + (size_t)rb * KC * 128 + lane, 0, KC}, 0, KC, aa_smem, PLANE2, N1, hi * N1 + col);
        if (col >= TN || q >= T) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = acc_row(r, hi, rb * 32);
            const size_t o = ((size_t)item * C + m) * T + q;
            a.y[o] = a.x[o] + (acc[0][0][r] * a.inv2 + a.bias2[m]);
        }
    }
}

size_t aa_unit_lds_bytes(int C, int d) {
    const size_t W = AA_N1 + 6 * d;
    const size_t stage = (size_t)2 * (C / 8) * W * sizeof(uint4) + (size_t)AA_CH1 * (2 * W + 10) * sizeof(float);
    const size_t seam = (size_t)2 * (C / 8) * AA_N1 * sizeof(uint4) + (size_t)32 * (AA_ZS + AA_SROW2) * sizeof(float);
    return stage > seam ? stage : seam;
}

hipError_t launch_aa_unit(AaUnitArgs a, int B, hipStream_t stream) {
    a.tiles_per_item = (a.T + AA_TN - 1) / AA_TN;
    const unsigned grid = (unsigned)((size_t)B * a.tiles_per_item);
    const size_t lds = aa_unit_lds_bytes(a.C, a.d);
    const double cols = (double)B * a.T;
    const int npw = (a.C + 63) / 64;
    note_kernel("aa_unit_f16x3_kernel", npw);
    note_work(grid, (2.0 * 7 * a.C * a.C + 2.0 * a.C * a.C) * cols / 1e9, 4.0 * cols * 2 * a.C / 1e6, "aa unit C=%d d=%d T=%d B=%d", a.C, a.d, a.T, B);
    return npw == 1 ? launch_dynamic_lds<&aa_unit_f16x3_kernel<1>>(grid, lds, stream, a)
                    : launch_dynamic_lds<&aa_unit_f16x3_kernel<2>>(grid, lds, stream, a);
}

}  // namespace amp
