// The up-sampling step of the DAC-style decoder blocks in one launch (models/codec/amphion_codec/codec.py:146-165, DualCodec's
// model_codec/dac_model.py:129-146):   y = ConvTranspose1d(cin, cout, k = 2 s, stride s, padding p, output_padding op)( snake(x) ).
// Polyphase: with u = t + p, q = u div s, r = u mod s
//     y[o, t] = b[o] + sum_c  w[c, o, r] a(x[c, q])  +  w[c, o, r + s] a(x[c, q - 1]),
// a GEMM with M = cout s rows m = o s + r, K = 2 cin (tap-major) and one column per q, on the blocks of wholek_f16x3.h (layouts, wave grid,
// arithmetic: there).  A workgroup owns TC_TN = 64 consecutive q of one item and ALL rows: it stages ONE window of 65 columns (q - 1 .. q + 63)
// over the whole cin -- snake is evaluated once per staged element; a column outside [0, T) is 0 AFTER the activation (a select) -- and both taps
// read that window one column apart.  M exceeds what a wave's accumulators hold (1536 rows at 192 x 8): wave (wm, wn) sweeps its row blocks
// wm, wm + 2, .. in groups of 4, then 2, then 1 over the same staged B, the A fragments streamed from L2.  Row order m = o s + r: the four
// consecutive rows a lane holds per register quad are consecutive output samples of one channel for s % 4 == 0 (two and two for even s), and
// the next lane's run follows at + s: per-lane vector stores, contiguous across lanes, as wide as the address is aligned.  One owner per output
// sample, fixed summation order, no atomics except the range flag (the staged activations feed it: snake is unbounded).
#include "act1d_math.h"
#include "wholek_f16x3.h"

namespace amp {

struct TcTile {
    const uint4* smem;
    int plane, KC, K16, rd0;   // rd0: lane offset of tap 1 (x[q - 1]) in the staged window; tap 0 reads one column further on
    int item, q, hi, lane;
};

// the four registers 4 j .. 4 j + 3 of one accumulator tile: rows m0 .. m0 + 3 of column t.q
__device__ __forceinline__ void tconv_store4(const TconvArgs& a, const TcTile& t, int m0, float v0, float v1, float v2, float v3) {
    if (m0 >= a.M) return;
    const int s = a.s, Tout = a.Tout;
    const int tb = t.q * s - a.p;
    int o = m0 / s, r = m0 - o * s;
    float* yrow = a.y + ((size_t)t.item * a.cout + o) * Tout;
    if ((s & 3) == 0) {
        // rows m0 .. m0 + 3 are samples t0 .. t0 + 3 of channel o (r % 4 == 0, r + 3 < s; M % 4 == 0)
        const float b = a.bias[o];
        v0 = v0 * a.inv + b; v1 = v1 * a.inv + b; v2 = v2 * a.inv + b; v3 = v3 * a.inv + b;
        const int t0 = tb + r;
        float* d = yrow + t0;
        if (t0 >= 0 && t0 + 3 < Tout) {
            const unsigned long long ad = (unsigned long long)d;
            if ((ad & 15) == 0) {
                *reinterpret_cast<float4*>(d) = make_float4(v0, v1, v2, v3);
            } else if ((ad & 7) == 0) {
                *reinterpret_cast<float2*>(d) = make_float2(v0, v1);
                *reinterpret_cast<float2*>(d + 2) = make_float2(v2, v3);
            } else {
                d[0] = v0; d[1] = v1; d[2] = v2; d[3] = v3;
            }
        } else {
            if (t0 >= 0 && t0 < Tout) d[0] = v0;
            if (t0 + 1 >= 0 && t0 + 1 < Tout) d[1] = v1;
            if (t0 + 2 >= 0 && t0 + 2 < Tout) d[2] = v2;
            if (t0 + 3 >= 0 && t0 + 3 < Tout) d[3] = v3;
        }
        return;
    }
    const float v[4] = {v0, v1, v2, v3};
    if ((s & 1) == 0) {
        // even s: rows (m0, m0 + 1) and (m0 + 2, m0 + 3) are two consecutive samples each (r even, r + 1 < s; M even)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (m0 + 2 * h < a.M) {
                const float b = a.bias[o];
                const float w0 = v[2 * h] * a.inv + b, w1 = v[2 * h + 1] * a.inv + b;
                const int t0 = tb + r;
                float* d = yrow + t0;
                if (t0 >= 0 && t0 + 1 < Tout && (((unsigned long long)d) & 7) == 0) {
                    *reinterpret_cast<float2*>(d) = make_float2(w0, w1);
                } else {
                    if (t0 >= 0 && t0 < Tout) d[0] = w0;
                    if (t0 + 1 >= 0 && t0 + 1 < Tout) d[1] = w1;
                }
            }
            r += 2;
            if (r >= s) { r = 0; ++o; yrow += Tout; }
        }
        return;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (m0 + e < a.M) {
            const int t1 = tb + r;
            if (t1 >= 0 && t1 < Tout) yrow[t1] = v[e] * a.inv + a.bias[o];
        }
        if (++r >= s) { r = 0; ++o; yrow += Tout; }
    }
}

// MI row blocks rb0, rb0 + 2, .. of this wave over the staged window: both taps, then the store
template <int MI>
__device__ __forceinline__ void tconv_rows(const TconvArgs& a, const TcTile& t, int rb0) {
    f32x16 acc[MI][1];
#pragma unroll
    for (int i = 0; i < MI; ++i) acc_zero(acc[i][0]);
    const APack A{a.wp + (size_t)rb0 * t.K16 * 128 + t.lane, (size_t)2 * t.K16 * 128, t.K16};
    Frag ah[MI], al[MI];
    afrag_load<MI>(ah, al, A.wa, A.mbs);
    gemm_wholek<MI, true>(acc, ah, al, A, 0, t.KC, t.smem, t.plane, TC_TN + 1, t.rd0 + 1);
    gemm_wholek<MI, true>(acc, ah, al, A, t.KC, t.KC, t.smem, t.plane, TC_TN + 1, t.rd0);
#pragma unroll
    for (int i = 0; i < MI; ++i) {
        const int mb = (rb0 + 2 * i) * 32 + 4 * t.hi;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            tconv_store4(a, t, mb + 8 * j, acc[i][0][4 * j], acc[i][0][4 * j + 1], acc[i][0][4 * j + 2], acc[i][0][4 * j + 3]);
    }
}

__global__ __launch_bounds__(256) void tconv_f16x3_kernel(const TconvArgs a) {
    constexpr int TN = TC_TN, W = TN + 1;
    extern __shared__ __attribute__((aligned(16))) uint4 tc_smem[];   // [2 planes][cin / 8 octets][W], then alpha [cin] | 1 / (alpha + 1e-9) [cin]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int hi = lane >> 5, l31 = lane & 31;
    const int item = blockIdx.x / a.tiles_per_item;
    const int q0 = a.q_first + (blockIdx.x - item * a.tiles_per_item) * TN;
    const int cin = a.cin, T = a.T;
    const int NO = cin >> 3;                  // channel octets
    const int PLANE = NO * W;                 // uint4 per plane

    float* act = reinterpret_cast<float*>(tc_smem + 2 * PLANE);
    const bool snake = a.alpha != nullptr;
    if (snake) {
        for (int c = tid; c < cin; c += 256) {
            const float al = a.alpha[c];
            act[c] = al;
            act[cin + c] = 1.0f / (al + 0.000000001f);
        }
        __syncthreads();
    }

    // ---- stage a(x) over columns q0 - 1 .. q0 + 63: item idx = quad of 4 channels x one column ----
    const float* xb = a.x + (size_t)item * cin * T;
    float range_max = 0.f;
    {
        uint2* dst = reinterpret_cast<uint2*>(tc_smem);
        const int total = (cin >> 2) * W;
        for (int idx = tid; idx < total; idx += 256) {
            const int qd = idx / W;
            const int w = idx - qd * W;
            const int c0 = qd * 4;
            const int q = q0 - 1 + w;
            const bool ok = q >= 0 && q < T;
            const int qc = q < 0 ? 0 : (q > T - 1 ? T - 1 : q);
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float xv = xb[(size_t)(c0 + e) * T + qc];
                AMP_OPAQUE(xv);
                if (snake) xv = fmaf(act[cin + c0 + e], snake_sin2(xv * act[c0 + e]), xv);
                v[e] = ok ? xv : 0.f;
            }
            uint2 fh, fl;
            stage4_f16(v[0], v[1], v[2], v[3], 16.f, 16.f, range_max, fh, fl);
            bplane_store(dst, 2 * PLANE, bplane_idx(qd, w, W), fh, fl);
        }
    }
    raise_range(a.range_flag, range_max, lane);
    __syncthreads();

    // ---- the row sweep: this wave's row blocks wm, wm + 2, .. in groups of 4, 2, 1 ----
    const int col = wn * 32 + l31;
    TcTile t;
    t.smem = tc_smem; t.plane = PLANE; t.KC = cin >> 4; t.K16 = 2 * t.KC; t.rd0 = hi * W + col;
    t.item = item; t.q = q0 + col; t.hi = hi; t.lane = lane;
    int rb = wm;
    for (; rb + 6 < a.NRB; rb += 8) tconv_rows<4>(a, t, rb);
    if (rb + 2 < a.NRB) { tconv_rows<2>(a, t, rb); rb += 4; }
    if (rb < a.NRB) tconv_rows<1>(a, t, rb);
}

size_t tconv_lds_bytes(int cin) { return (size_t)2 * (cin / 8) * (TC_TN + 1) * sizeof(uint4) + (size_t)2 * cin * sizeof(float); }

hipError_t launch_tconv(TconvArgs a, int B, hipStream_t stream) {
    const int q_last = (a.Tout - 1 + a.p) / a.s;
    const int nq = q_last - a.q_first + 1;
    a.tiles_per_item = (nq + TC_TN - 1) / TC_TN;
    const unsigned grid = (unsigned)((size_t)B * a.tiles_per_item);
    note_kernel("tconv_f16x3_kernel");
    note_work(grid, 2.0 * a.M * 2.0 * a.cin * (double)nq * B / 1e9, 4.0 * B * ((double)a.cin * a.T + (double)a.cout * a.Tout) / 1e6,
              "snake + ConvT %d->%d k=%d s=%d T=%d->%d B=%d", a.cin, a.cout, 2 * a.s, a.s, a.T, a.Tout, B);
    return launch_dynamic_lds<&tconv_f16x3_kernel>(grid, tconv_lds_bytes(a.cin), stream, a);
}

}  // namespace amp
