// The residual unit of the Amphion codec encoder in one launch (models/codec/amphion_codec/codec.py:60-76, Snake :34-39):
//     y = x + conv1x1( snake_2( conv7_dil( snake_1(x) ) ) ),      snake(v) = v + (alpha + 1e-9)^-1 sin^2(alpha v)
// as two GEMMs around a seam held in LDS, the structure of dw_layer_f16x3.hip.  GEMM 1 is the k = 7 dilated conv as an implicit GEMM with
// K = 7 C (tap-major): snake_1(x) is evaluated ONCE per staged element over the tile's window of 64 + 6 d columns ([plane][channel octet][column]
// [8 x f16]); tap j is the same rows read 3 j .. columns further on, one ds_read_b128 per B fragment.  The conv pads ITS input: a staged column
// outside [0, T) is 0 after the activation (a select, so nothing in the padding can leak).  The seam applies bias and snake_2 to GEMM 1's
// accumulators in registers, x16 / splits them and writes the B operand of GEMM 2 (K = C) over the front of the same LDS.  One workgroup owns 64
// output columns of one item and all C rows: no atomics except the range flag, fixed summation order, a batch row never depends on the batch.
//
// f16x3 arithmetic as everywhere (f16x3_device.h): weights pre-split on the host after a per-matrix 2^s, activations x16 and split while staged,
// hh + hl + lh MFMA terms into f32.  Both staged operands feed the range flag.  Waves are 2 x 2: wave (wm, wn) owns columns 32 wn .. 32 wn + 31
// and the row blocks wm, wm + 2, .. of both GEMMs.
#include "act1d_math.h"
#include "f16x3_device.h"

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
            const int o2 = (((qd >> 1) * W + w) << 1) + (qd & 1);
            dst[o2] = fh;
            dst[2 * PLANE + o2] = fl;
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
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        const uint4* wp = a.wp1 + (size_t)p * K16 * 128 + lane;
        Frag wh, wl;
        wh.u = wp[0];
        wl.u = wp[64];
        int k = 0;
        for (int tap = 0; tap < 7; ++tap) {
            const int rd = hi * W + col + tap * d;
            for (int kc = 0; kc < KC; ++kc, ++k) {
                const int kn = k + 1 < K16 ? k + 1 : k;       // the next A fragment flies under this step's MFMAs
                Frag nwh, nwl, bh, bl;
                nwh.u = wp[kn * 128];
                nwl.u = wp[kn * 128 + 64];
                bh.u = cu_smem[2 * kc * W + rd];
                bl.u = cu_smem[PLANE + 2 * kc * W + rd];
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh.h, bh.h, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh.h, bl.h, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl.h, bh.h, acc, 0, 0, 0);
                wh = nwh;
                wl = nwl;
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = p * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
            const float v = acc[r] * a.inv1 + a.bias1[m];
            z[pi][r] = codec_snake(v, a.alpha2[m], a.invb2[m]);
        }
    }
    __syncthreads();

    // ---- seam: registers 4j .. 4j + 3 of a lane are channels 32 p + 8 j + 4 hi + 0 .. 3 of column 32 wn + l31 ----
    const int PLANE2 = NO * TN;
    {
        uint2* dst = reinterpret_cast<uint2*>(cu_smem);
#pragma unroll
        for (int pi = 0; pi < NPW; ++pi) {
            const int p = wm + 2 * pi;
            if (p >= NP) break;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                uint2 sh, sl;
                stage4_f16(z[pi][4 * j], z[pi][4 * j + 1], z[pi][4 * j + 2], z[pi][4 * j + 3], 16.f, 16.f, range_max, sh, sl);
                const int o2 = (((p * 4 + j) * TN + col) << 1) + hi;
                dst[o2] = sh;
                dst[2 * PLANE2 + o2] = sl;
            }
        }
    }
    if (a.range_flag && __any(range_max > 65504.f) && lane == 0) atomicOr(a.range_flag, 1u);
    __syncthreads();

    // ---- GEMM 2 (1 x 1) + bias + residual ----
    const int q = q0 + col;
    for (int rb = wm; rb < NP; rb += 2) {
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        const uint4* w2 = a.wp2 + (size_t)rb * KC * 128 + lane;
        const int rd = hi * TN + col;
        for (int k = 0; k < KC; ++k) {
            Frag wh, wl, bh, bl;
            wh.u = w2[k * 128];
            wl.u = w2[k * 128 + 64];
            bh.u = cu_smem[2 * k * TN + rd];
            bl.u = cu_smem[PLANE2 + 2 * k * TN + rd];
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh.h, bh.h, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh.h, bl.h, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl.h, bh.h, acc, 0, 0, 0);
        }
        if (q >= T) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = rb * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
            const size_t o = ((size_t)item * C + m) * T + q;
            a.y[o] = a.x[o] + (acc[r] * a.inv2 + a.bias2[m]);
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
    if (npw == 1) {
        if (hipError_t e = ensure_dynamic_lds<&codec_unit_f16x3_kernel<1>>(lds); e != hipSuccess) return e;
        hipLaunchKernelGGL(codec_unit_f16x3_kernel<1>, dim3(grid), dim3(256), lds, stream, a);
    } else if (npw == 2) {
        if (hipError_t e = ensure_dynamic_lds<&codec_unit_f16x3_kernel<2>>(lds); e != hipSuccess) return e;
        hipLaunchKernelGGL(codec_unit_f16x3_kernel<2>, dim3(grid), dim3(256), lds, stream, a);
    } else {
        if (hipError_t e = ensure_dynamic_lds<&codec_unit_f16x3_kernel<3>>(lds); e != hipSuccess) return e;
        hipLaunchKernelGGL(codec_unit_f16x3_kernel<3>, dim3(grid), dim3(256), lds, stream, a);
    }
    return hipGetLastError();
}

}  // namespace amp
