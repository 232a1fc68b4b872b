// An amp_pw Linear at T = 1 (B <= 8) as a weight-streaming matrix-vector product: the Linears of a decode step (Vevo's autoregressive
// transformer, VALL-E), one kernel body under two entry points:
//     amp_pw_forward_vec       y = W x + b, or res + gamma * (W x + b)
//     amp_pw_forward_vec_ln    the same with the LayerNorm of x folded into the staging of x and a ReLU or residual epilogue: LN -> q | k | v,
//                              LN -> linear1 -> ReLU, LN -> predict layer of a decode step in one launch pair; with ln_gamma = NULL there
//                              is no norm and it launches amp_pw_forward_vec's kernel
// Plain fp32 on the vector pipe.  Deterministic: every sum runs in an order fixed by the shape alone, no atomics, no workgroup waits for
// another.
#include <hip/hip_runtime.h>

#include "amp_host.h"
#include "amphion_hip.h"

namespace amp {

// The handle's packed weights are MFMA A fragments: per 32-row block and K unit one 16-byte entry per lane (amp_host.h: pack_a_f16x3 --
// a hi and a lo plane, lane l = row l & 31, channels 16 u + 8 (l >> 5) + 0 .. 7; conv_host.hip's exact-fp32 pack -- one plane of floats,
// channels 8 u + 2 p + (l >> 5)).  Workgroup (mb, ks) of four waves streams the units [u0, u1) of row block mb, wave w the units
// u0 + w, u0 + w + 4, ...: a wave's load of an entry is 1 KiB contiguous, every weight is read once, by one lane.  The weight is hi + lo
// (exact in fp32: the two halves of one fp32 value) or the fp32 weight itself, the product an fp32 fma against the x of up to NB items,
// staged once per workgroup in LDS (zeros beyond Cin and beyond B).  Lanes l and l ^ 32 share a row: one exchange, then the four waves in
// order through LDS, and the slice's partial sums go to the workspace [ks][b][row].  pw_vec_epilogue_kernel adds the K slices in ascending
// order and applies scale, bias and the ReLU or residual epilogue.  The K slices give every Linear of the recipes more workgroups than CUs
// (pw_vec_plan); the order of every sum is fixed by the shape alone.
//
// LN: one more stage in front.  Every workgroup forms the statistics of the WHOLE row of each item itself -- thread t takes channels t,
// t + 256, ... in ascending order (the first PV_XR of them stay in registers for the second pass), a wave butterfly, the four waves in
// order through LDS; the mean first, then the biased variance about it -- and then stages its own K slice as
// (x - mean) * rstd * gamma + beta.  A row is 4 KB at 1024 channels and comes from L2 after the first workgroup; what it buys is the
// norm's own launch at T = 1 and the round trip of its output.  Every workgroup runs the same instructions on the same values in the same
// order, so all of them hold the same bits.
constexpr int PV_XS = 1024;      // channels of x a workgroup stages per item
constexpr int PV_MAXB = 8;
constexpr int PV_MAX_CIN = 4096; // the LN form: 16 channels per thread
constexpr int PV_XR = 4;         // the LN form: channels per thread and item kept in registers between the two passes

struct PwVecArgs {
    const void* wp;
    const float* x;       // [B, Cin], items xbs apart
    long long xbs;
    float* ws;            // [ksplit][B][rows_pad]
    int Cin, B, units, per_slice, rows_pad;
    // read by the LN form alone
    const float* lg;      // LayerNorm weight [Cin]
    const float* lb;      // LayerNorm bias [Cin]
    float eps;
};

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <int F32, int NB, bool LN>
__device__ __forceinline__ void pw_vec_body(const PwVecArgs& a) {
    constexpr int CU = F32 ? 8 : 16;                       // channels per unit
    __shared__ __attribute__((aligned(16))) float xs[NB][PV_XS];
    __shared__ float red[4][NB][32];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, hi = lane >> 5;
    const int mb = blockIdx.x, ks = blockIdx.y;
    const int u0 = ks * a.per_slice;
    const int u1 = u0 + a.per_slice < a.units ? u0 + a.per_slice : a.units;
    const int nch = (u1 - u0) * CU;                        // <= PV_XS (host)
    const int Cin = a.Cin;
    if constexpr (LN) {
        __shared__ float stat[2][4][NB];
        float mean[NB], rstd[NB];
        float xr[NB][PV_XR];
        // items beyond B read item B - 1 again: in bounds, and never staged
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const float* xb = a.x + (size_t)(b < a.B ? b : a.B - 1) * (size_t)a.xbs;
            float s = 0.f;
#pragma unroll
            for (int i = 0; i < PV_XR; ++i) {
                const int ch = tid + 256 * i;
                xr[b][i] = ch < Cin ? xb[ch] : 0.f;
                s += xr[b][i];
            }
            for (int ch = tid + 256 * PV_XR; ch < Cin; ch += 256) s += xb[ch];
            s = wave_sum(s);
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
            for (int i = 0; i < PV_XR; ++i) {
                const float d = tid + 256 * i < Cin ? xr[b][i] - mean[b] : 0.f;
                s = fmaf(d, d, s);
            }
            for (int ch = tid + 256 * PV_XR; ch < Cin; ch += 256) {
                const float d = xb[ch] - mean[b];
                s = fmaf(d, d, s);
            }
            s = wave_sum(s);
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

template <int F32, int NB>
__global__ __launch_bounds__(256) void pw_vec_kernel(PwVecArgs a) { pw_vec_body<F32, NB, false>(a); }

template <int F32, int NB>
__global__ __launch_bounds__(256) void pw_vec_ln_kernel(PwVecArgs a) { pw_vec_body<F32, NB, true>(a); }

// the K slices in ascending order, then scale, bias and ReLU or the residual epilogue.  RELU is a template argument, not a launch argument: with
// a run-time flag the no-ReLU launches of a decode step measured 0.2 - 0.3 us longer per Linear than the epilogue they had before
template <bool RELU>
__global__ __launch_bounds__(256) void pw_vec_epilogue_kernel(const float* __restrict__ ws, int ksplit, int B, int rows_pad, int Cout, float scale,
                                                              const float* __restrict__ bias, const float* __restrict__ gamma, const float* res,
                                                              float* y) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= B * Cout) return;
    const int b = idx / Cout, row = idx - b * Cout;
    float s = 0.f;
    for (int ks = 0; ks < ksplit; ++ks) s += ws[((size_t)ks * B + b) * rows_pad + row];
    float v = s * scale + bias[row];
    if (res) v = res[idx] + gamma[row] * v;
    if (RELU) v = __builtin_fmaxf(v, 0.f);
    y[idx] = v;
}

struct PwVecPlan {
    int f32, units, cu, row_blocks, ksplit, per_slice;
    const void* wp;
    const float* bias;
    float scale;
};

// K slices: enough that the staged x fits (PV_XS channels) and that the grid has at least 256 workgroups, at least one unit per wave, no
// empty slice
static int pw_vec_plan(const char* who, const amp_pw* p, PwVecPlan* out) {
    PwVecPlan pl{};
    pl.f32 = p->precision == PREC_F32;
    pl.row_blocks = (p->cout + 31) / 32;
    if (pl.f32) {
        if (!p->conv || p->conv->KT != 1 || p->conv->precision != PREC_F32) { set_error("%s: the handle's exact-fp32 conv is not a one-tap pack", who); return AMP_ERR_UNSUPPORTED; }
        pl.units = p->conv->nchunks; pl.cu = KC;
        pl.wp = p->conv->wp_dev; pl.bias = p->conv->bias_dev; pl.scale = 1.f;
    } else {
        pl.units = p->nsteps * 4; pl.cu = KC16;
        pl.wp = p->wp_dev; pl.bias = p->bias_dev; pl.scale = 16.f * p->inv_scale;     // 1 / 2^s: the staged x carries no x16 here
    }
    const int fit = (pl.units * pl.cu + PV_XS - 1) / PV_XS;
    int want = (256 + pl.row_blocks - 1) / pl.row_blocks;
    const int most = pl.units / 4 > 1 ? pl.units / 4 : 1;
    if (want > most) want = most;
    pl.ksplit = want > fit ? want : fit;
    pl.per_slice = (pl.units + pl.ksplit - 1) / pl.ksplit;
    pl.ksplit = (pl.units + pl.per_slice - 1) / pl.per_slice;
    *out = pl;
    return AMP_OK;
}

static size_t pw_vec_workspace_bytes(const char* who, const amp_pw* p, int B) {
    PwVecPlan pl;
    if (!p || B < 1 || B > PV_MAXB || pw_vec_plan(who, p, &pl) != AMP_OK) return 0;
    return (size_t)pl.ksplit * B * (size_t)(pl.row_blocks * 32) * sizeof(float);
}

template <int F32, bool LN>
static void pw_vec_launch_nb(const PwVecArgs& a, dim3 grid, hipStream_t st) {
    auto k = pw_vec_kernel<F32, 1>;
    if (a.B <= 1) k = LN ? pw_vec_ln_kernel<F32, 1> : pw_vec_kernel<F32, 1>;
    else if (a.B <= 2) k = LN ? pw_vec_ln_kernel<F32, 2> : pw_vec_kernel<F32, 2>;
    else if (a.B <= 4) k = LN ? pw_vec_ln_kernel<F32, 4> : pw_vec_kernel<F32, 4>;
    else k = LN ? pw_vec_ln_kernel<F32, 8> : pw_vec_kernel<F32, 8>;
    hipLaunchKernelGGL(k, grid, dim3(256), 0, st, a);
}

static void pw_vec_launch(int f32, const PwVecArgs& a, dim3 grid, hipStream_t st) {
    if (a.lg) f32 ? pw_vec_launch_nb<1, true>(a, grid, st) : pw_vec_launch_nb<0, true>(a, grid, st);
    else f32 ? pw_vec_launch_nb<1, false>(a, grid, st) : pw_vec_launch_nb<0, false>(a, grid, st);
}

// the first two checks of both entries, ahead of their own (`who` names the entry in every refusal)
static int pw_vec_check_args(const char* who, const amp_pw* p, const float* x_dev, const float* y_dev, const float* workspace_dev, int B) {
    if (!p || !x_dev || !y_dev || !workspace_dev) { set_error("%s: null argument", who); return AMP_ERR_INVALID; }
    if (B < 1 || B > PV_MAXB) { set_error("%s: B=%d is outside [1, %d]", who, B, PV_MAXB); return AMP_ERR_INVALID; }
    return AMP_OK;
}

// What both entries do behind pw_vec_check_args and their own argument checks (`ln_entry` picks the entry's profile labels): the checks on
// strides, workspace and overlap, the plan and the two launches.  lg = NULL: no norm; res = NULL: no residual.
static int pw_vec_forward(const char* who, bool ln_entry, const amp_pw* p, const float* x_dev, long long x_batch_stride, int B, const float* lg,
                          const float* lb, float eps, int relu, const float* gamma_dev, const float* res_dev, float* y_dev, float* workspace_dev,
                          size_t workspace_bytes, hipStream_t st) {
    if (x_batch_stride == 0) x_batch_stride = p->cin;
    if (x_batch_stride < p->cin) { set_error("%s: batch stride %lld < cin", who, x_batch_stride); return AMP_ERR_INVALID; }
    PwVecPlan pl;
    AMP_RC(pw_vec_plan(who, p, &pl));
    const int rows_pad = pl.row_blocks * 32;
    const size_t need = (size_t)pl.ksplit * B * (size_t)rows_pad * sizeof(float);
    if (workspace_bytes < need) {
        set_error("%s: workspace of %zu bytes, %zu needed (%s_workspace_bytes)", who, workspace_bytes, need, who);
        return AMP_ERR_INVALID;
    }
    const size_t xspan = ((size_t)(B - 1) * (size_t)x_batch_stride + (size_t)p->cin) * sizeof(float), ybytes = (size_t)B * p->cout * sizeof(float);
    if (ranges_overlap(y_dev, ybytes, x_dev, xspan) || ranges_overlap(workspace_dev, need, x_dev, xspan) || ranges_overlap(workspace_dev, need, y_dev, ybytes)) {
        set_error("%s: x, y and the workspace must not overlap", who);
        return AMP_ERR_INVALID;
    }
    if (res_dev && res_dev != y_dev && ranges_overlap(res_dev, ybytes, y_dev, ybytes)) {
        set_error("%s: res must be y or not overlap it", who);
        return AMP_ERR_INVALID;
    }
    PwVecArgs a{};
    a.wp = pl.wp; a.x = x_dev; a.xbs = x_batch_stride; a.ws = workspace_dev;
    a.Cin = p->cin; a.B = B; a.units = pl.units; a.per_slice = pl.per_slice; a.rows_pad = rows_pad;
    a.lg = lg; a.lb = lb; a.eps = eps;
    const dim3 grid((unsigned)pl.row_blocks, (unsigned)pl.ksplit);
    const double gflop = 2.0 * (double)p->cout * p->cin * B / 1e9, mb = 4.0 * (double)rows_pad * pl.units * pl.cu / 1e6;
    if (ln_entry) {
        note_kernel("pw_vec_ln_kernel", pl.f32, B);
        note_work((unsigned long long)grid.x * grid.y, gflop, mb, "pw vec ln %d->%d ln=%d relu=%d res=%d B=%d grid=%ux%u", p->cin, p->cout, lg ? 1 : 0,
                  relu ? 1 : 0, res_dev ? 1 : 0, B, grid.x, grid.y);
    } else {
        note_kernel("pw_vec_kernel", pl.f32, B);
        note_work((unsigned long long)grid.x * grid.y, gflop, mb, "pw vec %d->%d epi=%d B=%d grid=%ux%u", p->cin, p->cout,
                  res_dev ? AMP_PW_SCALE_RES : AMP_PW_BIAS, B, grid.x, grid.y);
    }
    pw_vec_launch(pl.f32, a, grid, st);
    AMP_HIP(hipGetLastError());
    const unsigned nb = (unsigned)((B * p->cout + 255) / 256);
    note_kernel(ln_entry ? "pw_vec_ln_epilogue_kernel" : "pw_vec_epilogue_kernel");
    note_work(nb, 0.0, 4.0 * (double)B * p->cout * (pl.ksplit + 2) / 1e6, ln_entry ? "pw vec ln epilogue C=%d B=%d slices=%d" : "pw vec epilogue C=%d B=%d slices=%d",
              p->cout, B, pl.ksplit);
    hipLaunchKernelGGL(relu ? pw_vec_epilogue_kernel<true> : pw_vec_epilogue_kernel<false>, dim3(nb), dim3(256), 0, st, workspace_dev, pl.ksplit, B,
                       rows_pad, p->cout, pl.scale, pl.bias, gamma_dev, res_dev, y_dev);
    AMP_HIP(hipGetLastError());
    return AMP_OK;
}

}  // namespace amp

using namespace amp;

extern "C" {

size_t amp_pw_forward_vec_workspace_bytes(const amp_pw* p, int B) { return pw_vec_workspace_bytes("amp_pw_forward_vec", p, B); }

size_t amp_pw_forward_vec_ln_workspace_bytes(const amp_pw* p, int B) { return pw_vec_workspace_bytes("amp_pw_forward_vec_ln", p, B); }

int amp_pw_forward_vec(const amp_pw* p, const float* x_dev, long long x_batch_stride, int B, int epilogue, const float* gamma_dev,
                       const float* res_dev, float* y_dev, float* workspace_dev, size_t workspace_bytes, void* stream) {
    const char* who = "amp_pw_forward_vec";
    AMP_RC(pw_vec_check_args(who, p, x_dev, y_dev, workspace_dev, B));
    if (epilogue != AMP_PW_BIAS && epilogue != AMP_PW_SCALE_RES) { set_error("%s: epilogue %d (AMP_PW_BIAS or AMP_PW_SCALE_RES)", who, epilogue); return AMP_ERR_INVALID; }
    if (epilogue == AMP_PW_SCALE_RES && (!gamma_dev || !res_dev)) { set_error("%s: AMP_PW_SCALE_RES needs gamma and res", who); return AMP_ERR_INVALID; }
    const bool sr = epilogue == AMP_PW_SCALE_RES;
    return pw_vec_forward(who, false, p, x_dev, x_batch_stride, B, nullptr, nullptr, 0.f, 0, sr ? gamma_dev : nullptr, sr ? res_dev : nullptr, y_dev,
                          workspace_dev, workspace_bytes, (hipStream_t)stream);
}

int amp_pw_forward_vec_ln(const amp_pw* p, const float* x_dev, long long x_batch_stride, int B, const float* ln_gamma_dev, const float* ln_beta_dev,
                          float eps, int relu, const float* gamma_dev, const float* res_dev, float* y_dev, float* workspace_dev,
                          size_t workspace_bytes, void* stream) {
    const char* who = "amp_pw_forward_vec_ln";
    AMP_RC(pw_vec_check_args(who, p, x_dev, y_dev, workspace_dev, B));
    if ((ln_gamma_dev == nullptr) != (ln_beta_dev == nullptr)) { set_error("%s: ln_gamma and ln_beta come together", who); return AMP_ERR_INVALID; }
    if (ln_gamma_dev && p->cin > PV_MAX_CIN) { set_error("%s: the LayerNorm form covers cin <= %d, got %d", who, PV_MAX_CIN, p->cin); return AMP_ERR_INVALID; }
    if (ln_gamma_dev && (!(eps >= 0.f) || !(eps < 1e30f))) { set_error("%s: eps=%g", who, (double)eps); return AMP_ERR_INVALID; }
    if ((res_dev == nullptr) != (gamma_dev == nullptr)) { set_error("%s: the residual epilogue needs gamma and res", who); return AMP_ERR_INVALID; }
    if (res_dev && relu) { set_error("%s: relu beside the residual epilogue", who); return AMP_ERR_INVALID; }
    return pw_vec_forward(who, true, p, x_dev, x_batch_stride, B, ln_gamma_dev, ln_beta_dev, eps, relu, gamma_dev, res_dev, y_dev, workspace_dev,
                          workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"
