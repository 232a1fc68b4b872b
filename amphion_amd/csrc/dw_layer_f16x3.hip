// One DiffWave residual layer in one launch (models/vocoders/diffusion/diffwave/diffwave.py:96-124, ResidualBlock):
//     y    = x + dconst[c]                                   (diffusion_projection(e): a per-channel constant)
//     a    = dilated_conv(y) + conditioner_projection(cond)  (k = 3, dilation d, ZERO padding of y; 1 x 1 over n_mel; both biases)
//     z    = sigmoid(a[:C]) * tanh(a[C:])                    (first half gate, second half filter)
//     r    = output_projection(z)                            (C -> 2C, k = 1)
//     x_out = (x + r[:C]) / sqrt(2),   skip_out = skip_in + r[C:]
// as the two GEMMs around a seam of wholek_f16x3.h (layouts, wave grid, arithmetic: there).  GEMM 1 has K = 3C + n_mel: the three taps are
// three SEPARATELY staged column tiles of x at t - d, t, t + d (the dilation never enters a halo: d = 512 costs what d = 1 costs), the
// conditioner rows follow as further K.  The gated product is the B operand of GEMM 2; re-using the front of the same LDS keeps two
// workgroups per CU at the recipe width.  One workgroup owns 64 output columns of one item and all 2C rows: no atomics (except the
// range flag), fixed summation order, a batch row never depends on what it is batched with.  In GEMM 1 a wave contracts the gate row
// block p AND its filter row block p + C / 32 for p = wm, wm + 2, .. (so sigmoid * tanh is formed in registers); in GEMM 2 the row blocks
// wm, wm + 2, .. of the 2C output rows.
//
// dw_layer_f32_kernel is the exact-fp32 form of the same layer (AMP_PRECISION_F32, and the repeat after a range report): the same
// per-tap staging, fp32 in LDS, one fmaf chain per output on the vector ALU.  It is not meant to be fast.
#include "wholek_f16x3.h"

namespace amp {

template <int NPW>   // gate / filter row-block pairs per wave: ceil(C / 64)
__global__ __launch_bounds__(256, 2) void dw_layer_f16x3_kernel(const DwLayerArgs a) {
    constexpr int TN = DW_TN;
    extern __shared__ __attribute__((aligned(16))) uint4 dw_smem[];   // [2 planes][K16 * 2 octets][TN]; the seam: [2][C / 8][TN]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int hi = lane >> 5, l31 = lane & 31;
    const int item = blockIdx.x / a.tiles_per_item;
    const int q0 = (blockIdx.x - item * a.tiles_per_item) * TN;
    const int C = a.C, L = a.L, d = a.d, K16 = a.K16;
    const int NP = C >> 5;
    const int PLANE = K16 * 2 * TN;       // uint4 per plane of the staged operand
    const int K3 = 3 * C;

    const float* xb = a.x + (size_t)item * C * L;
    const float* cb = a.cond + (size_t)item * a.n_mel * L;
    const float* dc = a.dconst + (size_t)item * a.dconst_bs;

    // ---- stage: quad qd = 4 channels of K x column `lane`; K index = tap * C + c, then 3C + mel channel ----
    float range_max = 0.f;
    {
        uint2* dst = reinterpret_cast<uint2*>(dw_smem);
        const int nit = K16;              // (4 K16 quads) / (4 waves)
        for (int it = 0; it < nit; ++it) {
            const int qd = it * 4 + wave;
            const int k0 = qd * 4;
            float v[4];
            if (k0 < K3) {
                const int tap = k0 / C;
                const int c0 = k0 - tap * C;
                const int t = q0 + lane + (tap - 1) * d;
                const bool ok = t >= 0 && t < L;
                const int tc = t < 0 ? 0 : (t > L - 1 ? L - 1 : t);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float xv = xb[(size_t)(c0 + e) * L + tc];
                    AMP_OPAQUE(xv);
                    v[e] = ok ? xv + dc[c0 + e] : 0.f;      // the conv pads y, not x: a tap outside [0, L) contributes 0
                }
            } else {
                const int j0 = k0 - K3;
                const int t = q0 + lane;
                const bool ok = t < L;
                const int tc = ok ? t : L - 1;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int j = j0 + e;
                    float cv = cb[(size_t)(j < a.n_mel ? j : a.n_mel - 1) * L + tc];
                    AMP_OPAQUE(cv);
                    v[e] = (ok && j < a.n_mel) ? cv : 0.f;
                }
            }
            uint2 fh, fl;
            stage4_f16(v[0], v[1], v[2], v[3], 16.f, 16.f, range_max, fh, fl);
            bplane_store(dst, 2 * PLANE, bplane_idx(qd, lane, TN), fh, fl);
        }
    }
    raise_range(a.range_flag, range_max, lane);
    __syncthreads();

    // ---- GEMM 1 + gate: z = sigmoid(gate) * tanh(filter), kept in registers until every wave has left the staged operand ----
    float z[NPW][16];
    const int rd0 = hi * TN + wn * 32 + l31;
#pragma unroll
    for (int pi = 0; pi < NPW; ++pi) {
        const int p = wm + 2 * pi;
        if (p >= NP) break;
        f32x16 acc[2][1];                  // gate, filter
        acc_zero(acc[0][0]);
        acc_zero(acc[1][0]);
        const APack A{a.wp1 + (size_t)p * K16 * 128 + lane, (size_t)NP * K16 * 128, K16};
        Frag ah[2], al[2];
        afrag_load<2>(ah, al, A.wa, A.mbs);
        gemm_wholek<2, true>(acc, ah, al, A, 0, K16, dw_smem, PLANE, TN, rd0);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = acc_row(r, hi, p * 32);
            const float g = acc[0][0][r] * a.inv1 + a.bias1[m];
            const float f = acc[1][0][r] * a.inv1 + a.bias1[C + m];
            z[pi][r] = (1.f / (1.f + expf(-g))) * tanhf(f);
        }
    }
    __syncthreads();

    // ---- seam: |z| <= 1, no range report ----
    const int PLANE2 = (C >> 3) * TN;
    seam_store<NPW>(z, reinterpret_cast<uint2*>(dw_smem), 2 * PLANE2, TN, wm, wn * 32 + l31, hi, NP, nullptr);
    __syncthreads();

    // ---- GEMM 2 + epilogue: rows [0, C) the residual, rows [C, 2C) the skip ----
    const int KC = C >> 4;
    const float sqrt2 = 1.41421356237309504880f;
    for (int rb = wm; rb < 2 * NP; rb += 2) {
        f32x16 acc[1][1];
        acc_zero(acc[0][0]);
        Frag ah, al;
        gemm_wholek<1, false>(acc, &ah, &al, APack{a.wp2 + (size_t)rb * KC * 128 + lane, 0, KC}, 0, KC, dw_smem, PLANE2, TN, rd0);
        const int q = q0 + wn * 32 + l31;
        if (q >= L) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = acc_row(r, hi, rb * 32);
            const float v = acc[0][0][r] * a.inv2 + a.bias2[m];
            if (rb < NP) {
                const size_t o = ((size_t)item * C + m) * L + q;
                a.x_out[o] = (a.x[o] + v) / sqrt2;
            } else {
                const size_t o = ((size_t)item * C + (m - C)) * L + q;
                a.skip_out[o] = a.skip_in ? v + a.skip_in[o] : v;
            }
        }
    }
}

// exact fp32: thread (column = tid & 63, group = tid >> 6); the group index is wave-uniform, so the weights are scalar loads
__global__ __launch_bounds__(256) void dw_layer_f32_kernel(const DwLayerArgs a) {
    constexpr int TN = DW_TN;
    extern __shared__ __attribute__((aligned(16))) float dw_smem_f[];   // [K][TN] staged operand, then [C][TN] gated product
    const int tid = threadIdx.x;
    const int col = tid & 63;
    const int grp = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int item = blockIdx.x / a.tiles_per_item;
    const int q0 = (blockIdx.x - item * a.tiles_per_item) * TN;
    const int C = a.C, L = a.L, d = a.d;
    const int K3 = 3 * C, K = K3 + a.n_mel;
    float* S = dw_smem_f;
    float* Z = dw_smem_f + (size_t)K * TN;
    const float* xb = a.x + (size_t)item * C * L;
    const float* cb = a.cond + (size_t)item * a.n_mel * L;
    const float* dc = a.dconst + (size_t)item * a.dconst_bs;

    for (int k = grp; k < K; k += 4) {
        float v;
        if (k < K3) {
            const int tap = k / C;
            const int c = k - tap * C;
            const int t = q0 + col + (tap - 1) * d;
            v = (t >= 0 && t < L) ? xb[(size_t)c * L + t] + dc[c] : 0.f;
        } else {
            const int t = q0 + col;
            v = t < L ? cb[(size_t)(k - K3) * L + t] : 0.f;
        }
        S[k * TN + col] = v;
    }
    __syncthreads();
    for (int c = grp; c < C; c += 4) {
        const float* wg = a.w1f + (size_t)c * K;
        const float* wf = a.w1f + (size_t)(C + c) * K;
        float g = 0.f, f = 0.f;
        for (int k = 0; k < K; ++k) {
            const float s = S[k * TN + col];
            g = fmaf(wg[k], s, g);
            f = fmaf(wf[k], s, f);
        }
        g += a.bias1[c];
        f += a.bias1[C + c];
        Z[c * TN + col] = (1.f / (1.f + expf(-g))) * tanhf(f);
    }
    __syncthreads();
    const int q = q0 + col;
    const float sqrt2 = 1.41421356237309504880f;
    for (int m = grp; m < 2 * C; m += 4) {
        const float* w = a.w2f + (size_t)m * C;
        float v = 0.f;
        for (int c = 0; c < C; ++c) v = fmaf(w[c], Z[c * TN + col], v);
        v += a.bias2[m];
        if (q >= L) continue;
        if (m < C) {
            const size_t o = ((size_t)item * C + m) * L + q;
            a.x_out[o] = (a.x[o] + v) / sqrt2;
        } else {
            const size_t o = ((size_t)item * C + (m - C)) * L + q;
            a.skip_out[o] = a.skip_in ? v + a.skip_in[o] : v;
        }
    }
}

size_t dw_layer_lds_bytes(int C, int n_mel, bool f32) {
    const int K = 3 * C + n_mel;
    if (f32) return (size_t)(K + C) * DW_TN * sizeof(float);
    const int K16 = (K + 15) / 16;
    return (size_t)2 * K16 * 2 * DW_TN * sizeof(uint4);
}

hipError_t launch_dw_layer(DwLayerArgs a, int B, bool f32, hipStream_t stream) {
    a.tiles_per_item = (a.L + DW_TN - 1) / DW_TN;
    const unsigned grid = (unsigned)((size_t)B * a.tiles_per_item);
    const size_t lds = dw_layer_lds_bytes(a.C, a.n_mel, f32);
    const double samples = (double)B * a.L;
    const double gf = (2.0 * (3 * a.C + a.n_mel) * 2 * a.C + 2.0 * a.C * 2 * a.C) * samples / 1e9;
    const double mb = 4.0 * samples * (a.C + a.n_mel + a.C + a.C + (a.skip_in ? a.C : 0)) / 1e6;
    if (f32) {
        if (hipError_t e = ensure_dynamic_lds<&dw_layer_f32_kernel>(lds); e != hipSuccess) return e;
        note_kernel("dw_layer_f32_kernel");
        note_work(grid, gf, mb, "diffwave layer C=%d n_mel=%d d=%d L=%d B=%d", a.C, a.n_mel, a.d, a.L, B);
        hipLaunchKernelGGL(dw_layer_f32_kernel, dim3(grid), dim3(256), lds, stream, a);
        return hipGetLastError();
    }
    a.K16 = (3 * a.C + a.n_mel + 15) / 16;
    const int npw = (a.C + 63) / 64;
    note_kernel("dw_layer_f16x3_kernel", npw);
    note_work(grid, gf, mb, "diffwave layer C=%d n_mel=%d d=%d L=%d B=%d", a.C, a.n_mel, a.d, a.L, B);
    return npw == 1 ? launch_dynamic_lds<&dw_layer_f16x3_kernel<1>>(grid, lds, stream, a)
                    : launch_dynamic_lds<&dw_layer_f16x3_kernel<2>>(grid, lds, stream, a);
}

}  // namespace amp
