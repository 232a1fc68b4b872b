// The residual unit of the Amphion codec encoder in one launch (models/codec/amphion_codec/codec.py:60-76, Snake :34-39):
//     y = x + conv1x1( snake_2( conv7_dil( snake_1(x) ) ) ),      snake(v) = v + (alpha + 1e-9)^-1 sin^2(alpha v)
// as the two GEMMs around a seam of wholek_f16x3.h (layouts, wave grid, arithmetic: there).  GEMM 1 is the k = 7 dilated conv as an implicit
// GEMM with K = 7 C (tap-major): snake_1(x) is evaluated ONCE per staged element over the tile's window of 64 + 6 d columns; tap j is the same
// rows read j d columns further on.  The conv pads ITS input: a staged column outside [0, T) is 0 after the activation (a select, so nothing in
// the padding can leak).  The seam function is bias + snake_2; GEMM 2 (K = C) is the 1 x 1 conv.  One workgroup owns 64 output columns of one
// item and all C rows: no atomics except the range flag, fixed summation order, a batch row never depends on the batch.  Both staged operands
// feed the range flag (snake is unbounded).
#include "act1d_math.h"
#include "wholek_f16x3.h"

namespace amp {

__device__ __forceinline__ float codec_snake(float v, float al, float invb) { return fmaf(invb, snake_sin2(v * al), v); }

template <int NPW>   // row blocks per wave: ceil(C / 64)
__global__ __launch_bounds__(256) void codec_unit_f16x3_kernel(const CodecUnitArgs a) {
    constexpr int TN = CU_TN;
    extern __shared__ __attribute__((aligned(16))) uint4 cu_smem[];   // [2 planes][C / 8 octets][W]; the seam: [2][C / 8][TN]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int hi = lane >> 5, l31 = lane & 31;
    const int item = blockIdx.x / a.tiles_per_item;
    const int q0 = (blockIdx.x - item * a.tiles_per_item) * TN;
    const int C = a.C, T = a.T, d = a.d;
    const int NP = C >> 5;
    const int W = TN + 6 * d;                 // staged columns: t = q0 - 3 d + w
    const int NO = C >> 3;                    // channel octets
    const int PLANE = NO * W;                 // uint4 per plane

    const float* xb = a.x + (size_t)item * C * T;

    // ---- stage snake_1(x): item idx = quad of 4 channels x one column ----
    float range_max = 0.f;
    {
        uint2* dst = reinterpret_cast<uint2*>(cu_smem);
        const int total = (C >> 2) * W;
        for (int idx = tid; idx < total; idx += 256) {
            const int qd = idx / W;
            const int w = idx - qd * W;
            const int c0 = qd * 4;
            const int t = q0 - 3 * d + w;
            const bool ok = t >= 0 && t < T;
            const int tc = t < 0 ? 0 : (t > T - 1 ? T - 1 : t);
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float xv = xb[(size_t)(c0 + e) * T + tc];
                AMP_OPAQUE(xv);
                const float s = codec_snake(xv, a.alpha1[c0 + e], a.invb1[c0 + e]);
                v[e] = ok ? s : 0.f;
            }
            uint2 fh, fl;
            stage4_f16(v[0], v[1], v[2], v[3], 16.f, 16.f, range_max, fh, fl);
            bplane_store(dst, 2 * PLANE, bplane_idx(qd, w, W), fh, fl);
        }
    }
    __syncthreads();

    // ---- GEMM 1 (k = 7, dilation d) + bias + snake_2, kept in registers until every wave has left the staged operand ----
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
        for (int tap = 0; tap < 7; ++tap) gemm_wholek<1, true>(acc, &ah, &al, A, tap * KC, KC, cu_smem, PLANE, W, hi * W + col + tap * d);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = acc_row(r, hi, p * 32);
            const float v = acc[0][0][r] * a.inv1 + a.bias1[m];
            z[pi][r] = codec_snake(v, a.alpha2[m], a.invb2[m]);
        }
    }
    __syncthreads();

    // ---- seam ----
    const int PLANE2 = NO * TN;
    seam_store<NPW>(z, reinterpret_cast<uint2*>(cu_smem), 2 * PLANE2, TN, wm, col, hi, NP, &range_max);
    raise_range(a.range_flag, range_max, lane);
    __syncthreads();

    // ---- GEMM 2 (1 x 1) + bias + residual ----
    const int q = q0 + col;
    for (int rb = wm; rb < NP; rb += 2) {
        f32x16 acc[1][1];
        acc_zero(acc[0][0]);
        Frag ah, al;
        gemm_wholek<1, false>(acc, &ah, &al, APack{a.wp2 + (size_t)rb * KC * 128 + lane, 0, KC}, 0, KC, cu_smem, PLANE2, TN, hi * TN + col);
        if (q >= T) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = acc_row(r, hi, rb * 32);
            const size_t o = ((size_t)item * C + m) * T + q;
            a.y[o] = a.x[o] + (acc[0][0][r] * a.inv2 + a.bias2[m]);
        }
    }
}

size_t codec_unit_lds_bytes(int C, int d) { return (size_t)2 * (C / 8) * (CU_TN + 6 * d) * sizeof(uint4); }

hipError_t launch_codec_unit(CodecUnitArgs a, int B, hipStream_t stream) {
    a.tiles_per_item = (a.T + CU_TN - 1) / CU_TN;
    const unsigned grid = (unsigned)((size_t)B * a.tiles_per_item);
    const size_t lds = codec_unit_lds_bytes(a.C, a.d);
    const double cols = (double)B * a.T;
    const int npw = (a.C + 63) / 64;
    note_kernel("codec_unit_f16x3_kernel", npw);
    note_work(grid, (2.0 * 7 * a.C * a.C + 2.0 * a.C * a.C) * cols / 1e9, 4.0 * cols * 2 * a.C / 1e6, "codec unit C=%d d=%d T=%d B=%d", a.C, a.d, a.T, B);
    return npw == 1 ? launch_dynamic_lds<&codec_unit_f16x3_kernel<1>>(grid, lds, stream, a)
         : npw == 2 ? launch_dynamic_lds<&codec_unit_f16x3_kernel<2>>(grid, lds, stream, a)
                    : launch_dynamic_lds<&codec_unit_f16x3_kernel<3>>(grid, lds, stream, a);
}

}  // namespace amp
