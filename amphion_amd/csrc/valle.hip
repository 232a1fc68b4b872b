// The kernels of VALL-E's decoder (models/tts/valle/valle.py: a pre-norm LayerNorm / ReLU transformer over [text | audio]) that the tree did not
// have; the prefix-LM prefill attention is an instantiation of llama_nar.hip's kernel (amp_prefix_attention):
//     amp_pw_forward_vec_ln    an amp_pw Linear at T = 1 (B <= 8) with the LayerNorm of its input folded into the staging of x and a ReLU or
//                              residual epilogue: LN -> q | k | v, LN -> linear1 -> ReLU, LN -> predict layer of a decode step in one launch pair
//     amp_embed_pos            token embedding plus the sinusoidal position row from a running position, channel-first
// Plain fp32 on the vector pipe.  Deterministic: every sum runs in an order fixed by the shape alone, no atomics on data (amp_embed_pos ORs
// its bad-id flag), no workgroup waits for another.
#include <hip/hip_runtime.h>

#include "amp_host.h"
#include "amphion_hip.h"

namespace amp {

// ---- amp_pw_forward_vec_ln ------------------------------------------------------------------------------------------------------------
// llama_ar.hip's pw_vec_kernel (the same packed weights, grid, K slices, workspace layout and order of every sum: with ln_gamma = NULL and no
// ReLU the bits are amp_pw_forward_vec's) with one more stage in front.  Every workgroup forms the statistics of the WHOLE row of each item
// itself -- thread t takes channels t, t + 256, ... in ascending order (the first PL_XR of them stay in registers for the second pass), a wave
// butterfly, the four waves in order through LDS; the mean first, then the biased variance about it -- and then stages its own K slice as
// (x - mean) * rstd * gamma + beta.  A row is 4 KB at 1024 channels and comes from L2 after the first workgroup; what it buys is the
// norm's own launch at T = 1 and the round trip of its output.  Every workgroup runs the same instructions on the same values in the same
// order, so all of them hold the same bits.
constexpr int PL_XS = 1024;      // channels of x a workgroup stages per item (pw_vec_kernel's PV_XS)
constexpr int PL_MAXB = 8;
constexpr int PL_MAX_CIN = 4096; // the LN form: 16 channels per thread
constexpr int PL_XR = 4;         // channels per thread and item kept in registers between the two passes

struct PwVecLnArgs {
    const void* wp;
    const float* x;       // [B, Cin], items xbs apart
    long long xbs;
    const float* lg;      // LayerNorm weight [Cin] or nullptr (no norm)
    const float* lb;      // LayerNorm bias [Cin]
    float eps;
    float* ws;            // [ksplit][B][rows_pad]
    int Cin, B, units, per_slice, rows_pad;
};

__device__ __forceinline__ float pl_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <int F32, int NB>
__global__ __launch_bounds__(256) void pw_vec_ln_kernel(PwVecLnArgs a) {
    constexpr int CU = F32 ? 8 : 16;                       // channels per unit
    __shared__ __attribute__((aligned(16))) float xs[NB][PL_XS];
    __shared__ float red[4][NB][32];
    __shared__ float stat[2][4][NB];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, hi = lane >> 5;
    const int mb = blockIdx.x, ks = blockIdx.y;
    const int u0 = ks * a.per_slice;
    const int u1 = u0 + a.per_slice < a.units ? u0 + a.per_slice : a.units;
    const int nch = (u1 - u0) * CU;                        // <= PL_XS (host)
    const int Cin = a.Cin;
    float mean[NB], rstd[NB];
    if (a.lg) {                                            // uniform over the grid
        float xr[NB][PL_XR];
        // items beyond B read item B - 1 again: in bounds, and never staged
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const float* xb = a.x + (size_t)(b < a.B ? b : a.B - 1) * (size_t)a.xbs;
            float s = 0.f;
#pragma unroll
            for (int i = 0; i < PL_XR; ++i) {
                const int ch = tid + 256 * i;
                xr[b][i] = ch < Cin ? xb[ch] : 0.f;
                s += xr[b][i];
            }
            for (int ch = tid + 256 * PL_XR; ch < Cin; ch += 256) s += xb[ch];
            s = pl_wave_sum(s);
            if (lane == 0) stat[0][w][b] = s;
        }
        __syncthreads();
#pragma unroll
        for (int b = 0; b < NB; ++b) mean[b] = (((stat[0][0][b] + stat[0][1][b]) + stat[0][2][b]) + stat[0][3][b]) / (float)Cin;
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const float* xb = a.x + (size_t)(b < a.B ? b : a.B - 1) * (size_t)a.xbs;
            float s = 0.f;
#pragma unroll
            for (int i = 0; i < PL_XR; ++i) {
                const float d = tid + 256 * i < Cin ? xr[b][i] - mean[b] : 0.f;
                s = fmaf(d, d, s);
            }
            for (int ch = tid + 256 * PL_XR; ch < Cin; ch += 256) {
                const float d = xb[ch] - mean[b];
                s = fmaf(d, d, s);
            }
            s = pl_wave_sum(s);
            if (lane == 0) stat[1][w][b] = s;
        }
        __syncthreads();
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const float var = (((stat[1][0][b] + stat[1][1][b]) + stat[1][2][b]) + stat[1][3][b]) / (float)Cin;
            rstd[b] = 1.0f / sqrtf(var + a.eps);
        }
        for (int idx = tid; idx < NB * nch; idx += 256) {
            const int b = idx / nch, cl = idx - b * nch, ch = u0 * CU + cl;
            float v = 0.f;
            if (b < a.B && ch < Cin) {
                float mu = 0.f, rs = 0.f;                  // (static indices only: mean / rstd stay in registers)
#pragma unroll
                for (int k = 0; k < NB; ++k) { mu = k == b ? mean[k] : mu; rs = k == b ? rstd[k] : rs; }
                v = (a.x[(size_t)b * (size_t)a.xbs + ch] - mu) * rs * a.lg[ch] + a.lb[ch];
            }
            xs[b][cl] = v;
        }
    } else {
        for (int idx = tid; idx < NB * nch; idx += 256) {
            const int b = idx / nch, cl = idx - b * nch, ch = u0 * CU + cl;
            xs[b][cl] = (b < a.B && ch < Cin) ? a.x[(size_t)b * (size_t)a.xbs + ch] : 0.f;
        }
    }
    __syncthreads();
    float acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = 0.f;
    if (F32) {
        const float4* wp = reinterpret_cast<const float4*>(a.wp) + (size_t)mb * a.units * 64 + lane;
#pragma unroll 4
        for (int u = u0 + w; u < u1; u += 4) {
            const float4 wv = wp[(size_t)u * 64];
            const int xo = (u - u0) * 8 + hi;
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                acc[b] = fmaf(wv.x, xs[b][xo], acc[b]);
                acc[b] = fmaf(wv.y, xs[b][xo + 2], acc[b]);
                acc[b] = fmaf(wv.z, xs[b][xo + 4], acc[b]);
                acc[b] = fmaf(wv.w, xs[b][xo + 6], acc[b]);
            }
        }
    } else {
        const uint4* wp = reinterpret_cast<const uint4*>(a.wp) + (size_t)mb * a.units * 128 + lane;
#pragma unroll 4
        for (int u = u0 + w; u < u1; u += 4) {
            union { uint4 q; _Float16 h[8]; } vh, vl;
            vh.q = wp[(size_t)u * 128];
            vl.q = wp[(size_t)u * 128 + 64];
            float wv[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) wv[e] = (float)vh.h[e] + (float)vl.h[e];
            const int xo = (u - u0) * 16 + 8 * hi;
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const float4 x0 = *reinterpret_cast<const float4*>(&xs[b][xo]), x1 = *reinterpret_cast<const float4*>(&xs[b][xo + 4]);
                acc[b] = fmaf(wv[0], x0.x, acc[b]);
                acc[b] = fmaf(wv[1], x0.y, acc[b]);
                acc[b] = fmaf(wv[2], x0.z, acc[b]);
                acc[b] = fmaf(wv[3], x0.w, acc[b]);
                acc[b] = fmaf(wv[4], x1.x, acc[b]);
                acc[b] = fmaf(wv[5], x1.y, acc[b]);
                acc[b] = fmaf(wv[6], x1.z, acc[b]);
                acc[b] = fmaf(wv[7], x1.w, acc[b]);
            }
        }
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const float t = acc[b] + __shfl_xor(acc[b], 32);
        if (hi == 0) red[w][b][lane] = t;
    }
    __syncthreads();
    if (tid < NB * 32) {
        const int b = tid >> 5, r = tid & 31;
        if (b < a.B) a.ws[((size_t)ks * a.B + b) * a.rows_pad + mb * 32 + r] = ((red[0][b][r] + red[1][b][r]) + red[2][b][r]) + red[3][b][r];
    }
}

// the K slices in ascending order, then scale, bias and ReLU or the residual epilogue
__global__ __launch_bounds__(256) void pw_vec_ln_epilogue_kernel(const float* __restrict__ ws, int ksplit, int B, int rows_pad, int Cout, float scale,
                                                                 const float* __restrict__ bias, const float* __restrict__ gamma, const float* res,
                                                                 int relu, float* y) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= B * Cout) return;
    const int b = idx / Cout, row = idx - b * Cout;
    float s = 0.f;
    for (int ks = 0; ks < ksplit; ++ks) s += ws[((size_t)ks * B + b) * rows_pad + row];
    float v = s * scale + bias[row];
    if (res) v = res[idx] + gamma[row] * v;
    if (relu) v = __builtin_fmaxf(v, 0.f);
    y[idx] = v;
}

// amp_pw_forward_vec's plan (llama_ar.hip: pw_vec_ksplit / pw_vec_plan), restated because that unit keeps its own: K slices so that the
// staged x fits (PL_XS channels) and the grid has at least 256 workgroups, at least one unit per wave, no empty slice
struct PwVecLnPlan {
    int f32, units, cu, row_blocks, ksplit, per_slice;
    const void* wp;
    const float* bias;
    float scale;
};

static int pw_vec_ln_plan(const amp_pw* p, PwVecLnPlan* out) {
    PwVecLnPlan pl{};
    pl.f32 = p->precision == PREC_F32;
    pl.row_blocks = (p->cout + 31) / 32;
    if (pl.f32) {
        if (!p->conv || p->conv->KT != 1 || p->conv->precision != PREC_F32) { set_error("amp_pw_forward_vec_ln: the handle's exact-fp32 conv is not a one-tap pack"); return AMP_ERR_UNSUPPORTED; }
        pl.units = p->conv->nchunks; pl.cu = KC;
        pl.wp = p->conv->wp_dev; pl.bias = p->conv->bias_dev; pl.scale = 1.f;
    } else {
        pl.units = p->nsteps * 4; pl.cu = KC16;
        pl.wp = p->wp_dev; pl.bias = p->bias_dev; pl.scale = 16.f * p->inv_scale;     // 1 / 2^s: the staged x carries no x16 here
    }
    const int fit = (pl.units * pl.cu + PL_XS - 1) / PL_XS;
    int want = (256 + pl.row_blocks - 1) / pl.row_blocks;
    const int most = pl.units / 4 > 1 ? pl.units / 4 : 1;
    if (want > most) want = most;
    pl.ksplit = want > fit ? want : fit;
    pl.per_slice = (pl.units + pl.ksplit - 1) / pl.ksplit;
    pl.ksplit = (pl.units + pl.per_slice - 1) / pl.per_slice;
    *out = pl;
    return AMP_OK;
}

template <int F32>
static void pw_vec_ln_launch(const PwVecLnArgs& a, int nb, dim3 grid, hipStream_t st) {
    if (nb <= 1) hipLaunchKernelGGL((pw_vec_ln_kernel<F32, 1>), grid, dim3(256), 0, st, a);
    else if (nb <= 2) hipLaunchKernelGGL((pw_vec_ln_kernel<F32, 2>), grid, dim3(256), 0, st, a);
    else if (nb <= 4) hipLaunchKernelGGL((pw_vec_ln_kernel<F32, 4>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((pw_vec_ln_kernel<F32, 8>), grid, dim3(256), 0, st, a);
}

// ---- amp_embed_pos ----------------------------------------------------------------------------------------------------------------------
// amp_embed_sum_c's workgroup: 32 frames x 64 channels through an LDS tile, so the table and position rows are read as 256-B segments along D and
// y is stored along T.  The product by x_scale, the product by alpha and the add are three roundings, as torch's `x * x_scale + alpha * pe`.
constexpr int EP_TT = 32, EP_DT = 64;
struct EmbedPosArgs {
    const long long* tokens;   // [B, T]
    const float* weight;       // [rows, D]
    const float* pe;           // [pe_rows, D]
    const float* alpha;        // one value on the device
    float* y;                  // [B, D, T]
    unsigned* flag;
    int rows, D, T, pos0;
    float x_scale;
};

__global__ __launch_bounds__(256) void embed_pos_kernel(const EmbedPosArgs a) {
    __shared__ float tile[EP_TT][EP_DT + 1];
    __shared__ int code[EP_TT];
    const int tid = threadIdx.x;
    const int t0 = blockIdx.x * EP_TT, d0 = blockIdx.y * EP_DT, b = blockIdx.z;
    const int D = a.D, T = a.T;
    if (tid < EP_TT) {
        long long c = t0 + tid < T ? a.tokens[(size_t)b * T + t0 + tid] : 0;
        if (c < 0 || c >= a.rows) { atomicOr(a.flag, 1u); c = 0; }
        code[tid] = (int)c;
    }
    __syncthreads();
    const float alpha = a.alpha[0];
    const int dx = tid & (EP_DT - 1), fy = tid / EP_DT;          // the row-major side: channel dx, frames fy, fy + 4, ..
    if (d0 + dx < D) {
        for (int f = fy; f < EP_TT && t0 + f < T; f += 256 / EP_DT) {
            const float e = __fmul_rn(a.weight[(size_t)code[f] * D + d0 + dx], a.x_scale);
            const float p = __fmul_rn(alpha, a.pe[(size_t)(a.pos0 + t0 + f) * D + d0 + dx]);
            tile[f][dx] = __fadd_rn(e, p);
        }
    }
    __syncthreads();
    const int tx = tid & (EP_TT - 1), dy = tid / EP_TT;          // the time-major side: frame tx, channels dy, dy + 8, ..
    if (t0 + tx < T) {
        const size_t obase = ((size_t)b * D + d0) * T + t0 + tx;
        for (int d = dy; d < EP_DT && d0 + d < D; d += 256 / EP_TT) a.y[obase + (size_t)d * T] = tile[tx][d];
    }
}

static bool overlaps(const void* p, size_t pn, const void* q, size_t qn) {
    const char* a = reinterpret_cast<const char*>(p);
    const char* b = reinterpret_cast<const char*>(q);
    return pn && qn && a < b + qn && b < a + pn;
}

}  // namespace amp

using namespace amp;

extern "C" {

size_t amp_pw_forward_vec_ln_workspace_bytes(const amp_pw* p, int B) {
    PwVecLnPlan pl;
    if (!p || B < 1 || B > PL_MAXB || pw_vec_ln_plan(p, &pl) != AMP_OK) return 0;
    return (size_t)pl.ksplit * B * (size_t)(pl.row_blocks * 32) * sizeof(float);
}

int amp_pw_forward_vec_ln(const amp_pw* p, const float* x_dev, long long x_batch_stride, int B, const float* ln_gamma_dev, const float* ln_beta_dev,
                          float eps, int relu, const float* gamma_dev, const float* res_dev, float* y_dev, float* workspace_dev,
                          size_t workspace_bytes, void* stream) {
    if (!p || !x_dev || !y_dev || !workspace_dev) { set_error("amp_pw_forward_vec_ln: null argument"); return AMP_ERR_INVALID; }
    if (B < 1 || B > PL_MAXB) { set_error("amp_pw_forward_vec_ln: B=%d is outside [1, %d]", B, PL_MAXB); return AMP_ERR_INVALID; }
    if ((ln_gamma_dev == nullptr) != (ln_beta_dev == nullptr)) { set_error("amp_pw_forward_vec_ln: ln_gamma and ln_beta come together"); return AMP_ERR_INVALID; }
    if (ln_gamma_dev && p->cin > PL_MAX_CIN) { set_error("amp_pw_forward_vec_ln: the LayerNorm form covers cin <= %d, got %d", PL_MAX_CIN, p->cin); return AMP_ERR_INVALID; }
    if (ln_gamma_dev && (!(eps >= 0.f) || !(eps < 1e30f))) { set_error("amp_pw_forward_vec_ln: eps=%g", (double)eps); return AMP_ERR_INVALID; }
    if ((res_dev == nullptr) != (gamma_dev == nullptr)) { set_error("amp_pw_forward_vec_ln: the residual epilogue needs gamma and res"); return AMP_ERR_INVALID; }
    if (res_dev && relu) { set_error("amp_pw_forward_vec_ln: relu beside the residual epilogue"); return AMP_ERR_INVALID; }
    if (x_batch_stride == 0) x_batch_stride = p->cin;
    if (x_batch_stride < p->cin) { set_error("amp_pw_forward_vec_ln: batch stride %lld < cin", x_batch_stride); return AMP_ERR_INVALID; }
    PwVecLnPlan pl;
    AMP_RC(pw_vec_ln_plan(p, &pl));
    const int rows_pad = pl.row_blocks * 32;
    const size_t need = (size_t)pl.ksplit * B * (size_t)rows_pad * sizeof(float);
    if (workspace_bytes < need) {
        set_error("amp_pw_forward_vec_ln: workspace of %zu bytes, %zu needed (amp_pw_forward_vec_ln_workspace_bytes)", workspace_bytes, need);
        return AMP_ERR_INVALID;
    }
    const size_t xspan = ((size_t)(B - 1) * (size_t)x_batch_stride + (size_t)p->cin) * sizeof(float), ybytes = (size_t)B * p->cout * sizeof(float);
    if (overlaps(y_dev, ybytes, x_dev, xspan) || overlaps(workspace_dev, need, x_dev, xspan) || overlaps(workspace_dev, need, y_dev, ybytes)) {
        set_error("amp_pw_forward_vec_ln: x, y and the workspace must not overlap");
        return AMP_ERR_INVALID;
    }
    if (res_dev && res_dev != y_dev && overlaps(res_dev, ybytes, y_dev, ybytes)) {
        set_error("amp_pw_forward_vec_ln: res must be y or not overlap it");
        return AMP_ERR_INVALID;
    }
    PwVecLnArgs a{};
    a.wp = pl.wp; a.x = x_dev; a.xbs = x_batch_stride; a.ws = workspace_dev;
    a.lg = ln_gamma_dev; a.lb = ln_beta_dev; a.eps = eps;
    a.Cin = p->cin; a.B = B; a.units = pl.units; a.per_slice = pl.per_slice; a.rows_pad = rows_pad;
    const dim3 grid((unsigned)pl.row_blocks, (unsigned)pl.ksplit);
    hipStream_t st = (hipStream_t)stream;
    note_kernel("pw_vec_ln_kernel", pl.f32, B);
    note_work((unsigned long long)grid.x * grid.y, 2.0 * (double)p->cout * p->cin * B / 1e9, 4.0 * (double)rows_pad * pl.units * pl.cu / 1e6,
              "pw vec ln %d->%d ln=%d relu=%d res=%d B=%d grid=%ux%u", p->cin, p->cout, ln_gamma_dev ? 1 : 0, relu ? 1 : 0, res_dev ? 1 : 0, B, grid.x, grid.y);
    if (pl.f32) pw_vec_ln_launch<1>(a, B, grid, st);
    else pw_vec_ln_launch<0>(a, B, grid, st);
    AMP_HIP(hipGetLastError());
    const unsigned nb = (unsigned)((B * p->cout + 255) / 256);
    note_kernel("pw_vec_ln_epilogue_kernel");
    note_work(nb, 0.0, 4.0 * (double)B * p->cout * (pl.ksplit + 2) / 1e6, "pw vec ln epilogue C=%d B=%d slices=%d", p->cout, B, pl.ksplit);
    hipLaunchKernelGGL(pw_vec_ln_epilogue_kernel, dim3(nb), dim3(256), 0, st, workspace_dev, pl.ksplit, B, rows_pad, p->cout, pl.scale, pl.bias, gamma_dev,
                       res_dev, relu ? 1 : 0, y_dev);
    AMP_HIP(hipGetLastError());
    return AMP_OK;
}

int amp_embed_pos(const long long* tokens_dev, const float* weight_dev, int rows, int D, const float* pe_dev, int pe_rows, int pos0, float x_scale,
                  const float* alpha_dev, int B, int T, float* y_dev, unsigned* flag_dev, void* stream) {
    if (!tokens_dev || !weight_dev || !pe_dev || !alpha_dev || !y_dev || !flag_dev) { set_error("amp_embed_pos: null argument"); return AMP_ERR_INVALID; }
    if (rows < 1 || D < 1 || B < 1 || T < 1 || pe_rows < 1) { set_error("amp_embed_pos: rows=%d D=%d B=%d T=%d pe_rows=%d", rows, D, B, T, pe_rows); return AMP_ERR_INVALID; }
    if (pos0 < 0 || (long long)pos0 + T > pe_rows) {
        set_error("amp_embed_pos: positions [%d, %lld) are beyond a table of %d rows", pos0, (long long)pos0 + T, pe_rows);
        return AMP_ERR_INVALID;
    }
    const int gd = (D + EP_DT - 1) / EP_DT;
    if (B > 65535 || gd > 65535) { set_error("amp_embed_pos: B=%d D=%d is beyond the grid", B, D); return AMP_ERR_UNSUPPORTED; }
    EmbedPosArgs a{};
    a.tokens = tokens_dev; a.weight = weight_dev; a.pe = pe_dev; a.alpha = alpha_dev; a.y = y_dev; a.flag = flag_dev;
    a.rows = rows; a.D = D; a.T = T; a.pos0 = pos0; a.x_scale = x_scale;
    const dim3 grid((unsigned)((T + EP_TT - 1) / EP_TT), (unsigned)gd, (unsigned)B);
    note_kernel("embed_pos_kernel");
    note_work((unsigned long long)grid.x * grid.y * grid.z, 0.0, 12.0 * (double)B * D * T / 1e6, "embed + position D=%d T=%d pos0=%d B=%d", D, T, pos0, B);
    hipLaunchKernelGGL(embed_pos_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
    AMP_HIP(hipGetLastError());
    return AMP_OK;
}

}  // extern "C"
