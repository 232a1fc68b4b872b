// The frame-rate kernels of FastSpeech2 / JETS inference (models/tts/fastspeech2/fs2.py, models/tts/jets/jets.py) that the conv family,
// the pointwise GEMM, amp_layer_norm_c and amp_expand_path do not cover:
//     amp_fs2_durations        VarianceAdaptor's clamp(round(exp(log_d) - 1) * d_control, min = 0), its truncated running sum and the mel lengths
//     amp_bucketize_embed_add  x += embedding(bucketize(prediction * control, bins)) and the scaled prediction, one launch
//     amp_layer_norm_c_head    VariancePredictor's tail: layer_norm_2 -> Linear(C, 1) -> masked_fill, the normalised tensor never written
// (amp_mh_attention, the FFT block's attention, is the no-rotation form of llama_nar.hip's kernel.)
// Everything is channel-first [B, C, T] fp32, plain fp32 arithmetic.  Deterministic: no atomics, every reduction in a fixed order.
#include <hip/hip_runtime.h>

#include "amp_host.h"
#include "amphion_hip.h"
#include "gelu_erf.h"

namespace amp {

// ---- amp_fs2_durations -------------------------------------------------------------------------------------------------------------
// One workgroup per item walks its T columns in chunks of 256: thread i of a chunk forms d = max(rint(expf(x) - 1) * d_control, 0) (rintf is
// round-half-even, torch.round's rule; NaN stays NaN as under torch.clamp) and n = (int)d as LengthRegulator.expand truncates it
// (`max(int(expand_size), 0)`; saturated at 2^24 per token, NaN counts 0), the chunk's inclusive scan of n goes through LDS (integer adds:
// any order gives the same sum; this one is fixed anyway) on top of the carry of the chunks before, saturated at INT_MAX.
constexpr int FD_N = 256;
__global__ __launch_bounds__(FD_N) void fs2_durations_kernel(const float* __restrict__ logd, float d_control, float* __restrict__ d_rounded,
                                                             int* __restrict__ cum, int* __restrict__ mel_len, int T) {
    __shared__ long long scan[2][FD_N];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* xb = logd + (size_t)b * T;
    long long carry = 0;
    for (int t0 = 0; t0 < T; t0 += FD_N) {
        const int t = t0 + tid;
        long long n = 0;
        if (t < T) {
            const float r = rintf(expf(xb[t]) - 1.0f) * d_control;
            const float d = r < 0.f ? 0.f : r;             // (-0 stays -0, NaN stays NaN)
            d_rounded[(size_t)b * T + t] = d;
            n = d >= 16777216.f ? 16777216ll : (d >= 1.f ? (long long)(int)d : 0ll);
        }
        int cur = 0;
        scan[0][tid] = n;
        __syncthreads();
#pragma unroll
        for (int step = 1; step < FD_N; step <<= 1) {
            const long long v = scan[cur][tid] + (tid >= step ? scan[cur][tid - step] : 0ll);
            scan[cur ^ 1][tid] = v;
            cur ^= 1;
            __syncthreads();
        }
        const long long run = carry + scan[cur][tid];
        if (t < T) cum[(size_t)b * T + t] = run > 2147483647ll ? 2147483647 : (int)run;
        carry += scan[cur][FD_N - 1];
        __syncthreads();                                   // the next chunk overwrites scan[0]
    }
    if (tid == 0) mel_len[b] = carry > 2147483647ll ? 2147483647 : (int)carry;
}

// ---- amp_bucketize_embed_add -------------------------------------------------------------------------------------------------------
// amp_embed_sum_c's workgroup: 32 frames x 64 channels through an LDS tile, so the table rows are gathered as 256-B segments and x / y move as
// 128-B time segments.  The index of frame t is the number of boundaries < v, v = pred * control (one fp32 multiply): the first position whose
// boundary is >= v, found by bisection with torch's own comparison, !(bins[mid] >= v) -> right, under which a NaN goes past every boundary.
constexpr int BE_TT = 32, BE_DT = 64;
__global__ __launch_bounds__(256) void bucketize_embed_add_kernel(const float* __restrict__ pred, float control, const float* __restrict__ bins,
                                                                  int n_bounds, const float* __restrict__ table, const float* x, float* y,
                                                                  float* __restrict__ pred_out, int D, int T) {
    __shared__ float tile[BE_TT][BE_DT + 1];
    __shared__ int code[BE_TT];
    const int tid = threadIdx.x;
    const int t0 = blockIdx.x * BE_TT, d0 = blockIdx.y * BE_DT, b = blockIdx.z;
    if (tid < BE_TT) {
        int idx = 0;
        if (t0 + tid < T) {
            const float v = fp_opaque(pred[(size_t)b * T + t0 + tid] * control);
            if (blockIdx.y == 0) pred_out[(size_t)b * T + t0 + tid] = v;
            int lo = 0, hi = n_bounds;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (!(bins[mid] >= v)) lo = mid + 1; else hi = mid;
            }
            idx = lo;
        }
        code[tid] = idx;
    }
    const int tx = tid & (BE_TT - 1), dy = tid / BE_TT;          // the time-major side: frame tx, channels dy, dy + 8, ..
    const size_t obase = ((size_t)b * D + d0) * T + t0 + tx;
    if (t0 + tx < T) {
        for (int d = dy; d < BE_DT && d0 + d < D; d += 256 / BE_TT) tile[tx][d] = x[obase + (size_t)d * T];
    }
    __syncthreads();
    const int dx = tid & (BE_DT - 1), fy = tid / BE_DT;          // the row-major side: channel dx, frames fy, fy + 4, ..
    if (d0 + dx < D) {
        for (int f = fy; f < BE_TT && t0 + f < T; f += 256 / BE_DT) tile[f][dx] = tile[f][dx] + table[(size_t)code[f] * D + d0 + dx];
    }
    __syncthreads();
    if (t0 + tx < T) {
        for (int d = dy; d < BE_DT && d0 + d < D; d += 256 / BE_TT) y[obase + (size_t)d * T] = tile[tx][d];
    }
}

// ---- amp_layer_norm_c_head ---------------------------------------------------------------------------------------------------------
// amp_layer_norm_c's workgroup (32 time columns x 8 channel groups, thread (tx, g) holds channels g, g + 8, ... of column tx, 32 of them in
// registers and the rest re-read), its two passes (mean, then the biased variance of the centred values) and its LDS reductions in the same
// fixed order; the affine is the same (v - mu) * rstd, then fma(., gamma, beta).  What follows is a third reduction of the same shape over
// w[c] * LN(x)[c] in place of the store: thread partials by fma in ascending channel order, the eight groups added in order, + b0.
constexpr int LH_TT = 32, LH_G = 8, LH_NC = 32;
__global__ __launch_bounds__(256) void layer_norm_c_head_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                                const float* __restrict__ beta, const float* __restrict__ w, float b0,
                                                                const int* __restrict__ lens, float* __restrict__ y, int C, int T, float eps) {
    __shared__ float red[LH_G][LH_TT + 1];
    const int tx = threadIdx.x & (LH_TT - 1), g = threadIdx.x / LH_TT;
    const int t = blockIdx.x * LH_TT + tx;
    const int b = blockIdx.y;
    const bool ok = t < T;
    const int len = lens ? lens[b] : T;
    if (blockIdx.x * LH_TT >= len) {                     // block-uniform: a tile beyond the item's end is zeros
        if (ok && g == 0) y[(size_t)b * T + t] = 0.f;
        return;
    }
    const float* xb = x + (size_t)b * C * T + (ok ? t : 0);
    auto reduce = [&](float part) {                      // sum over the 8 channel groups of column tx, same order in every thread
        red[g][tx] = part;
        __syncthreads();
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < LH_G; ++k) s += red[k][tx];
        __syncthreads();
        return s;
    };
    float v[LH_NC], gr[LH_NC], br[LH_NC], wr[LH_NC];
#pragma unroll
    for (int i = 0; i < LH_NC; ++i) {                    // unconditional loads (clamped channel), the select applied afterwards
        const int c = g + LH_G * i;
        const int cc = c < C ? c : C - 1;
        v[i] = xb[(size_t)cc * T];
        gr[i] = gamma[cc]; br[i] = beta[cc]; wr[i] = w[cc];
    }
    float part = 0.f;
#pragma unroll
    for (int i = 0; i < LH_NC; ++i) {
        v[i] = (ok && g + LH_G * i < C) ? v[i] : 0.f;
        part += v[i];
    }
    for (int c = g + LH_G * LH_NC; c < C; c += LH_G) part += ok ? xb[(size_t)c * T] : 0.f;
    const float mu = reduce(part) / (float)C;
    part = 0.f;
#pragma unroll
    for (int i = 0; i < LH_NC; ++i) {
        const float d = g + LH_G * i < C ? v[i] - mu : 0.f;
        part = fmaf(d, d, part);
    }
    for (int c = g + LH_G * LH_NC; c < C; c += LH_G) {
        const float d = (ok ? xb[(size_t)c * T] : 0.f) - mu;
        part = fmaf(d, d, part);
    }
    const float rstd = 1.0f / sqrtf(reduce(part) / (float)C + eps);
    auto affine = [&](float xv, float ga, float be) {
#pragma clang fp contract(off)
        const float u = fp_opaque((xv - mu) * rstd);
        return fp_opaque(fmaf(u, ga, be));
    };
    part = 0.f;
#pragma unroll
    for (int i = 0; i < LH_NC; ++i)
        if (g + LH_G * i < C) part = fmaf(wr[i], affine(v[i], gr[i], br[i]), part);
    for (int c = g + LH_G * LH_NC; c < C; c += LH_G) part = fmaf(w[c], affine(ok ? xb[(size_t)c * T] : 0.f, gamma[c], beta[c]), part);
    const float s = reduce(part) + b0;
    if (ok && g == 0) y[(size_t)b * T + t] = t < len ? s : 0.f;
}

}  // namespace amp

using namespace amp;

extern "C" {

int amp_fs2_durations(const float* log_d_dev, int B, int T, float d_control, float* d_rounded_dev, int* cum_dev, int* mel_len_dev, void* stream) {
    if (!log_d_dev || !d_rounded_dev || !cum_dev || !mel_len_dev) { set_error("amp_fs2_durations: null argument"); return AMP_ERR_INVALID; }
    if (B < 1 || T < 1) { set_error("amp_fs2_durations: B=%d T=%d", B, T); return AMP_ERR_INVALID; }
    if (!(d_control > 0.f) || !(d_control < 1e30f)) { set_error("amp_fs2_durations: d_control=%g", (double)d_control); return AMP_ERR_INVALID; }
    if (log_d_dev == d_rounded_dev) { set_error("amp_fs2_durations: d_rounded must not alias log_d"); return AMP_ERR_INVALID; }
    note_kernel("fs2_durations_kernel");
    note_work((unsigned long long)B, 0.0, 12.0 * (double)B * T / 1e6, "fs2 durations B=%d T=%d", B, T);
    hipLaunchKernelGGL(fs2_durations_kernel, dim3((unsigned)B), dim3(FD_N), 0, (hipStream_t)stream, log_d_dev, d_control, d_rounded_dev, cum_dev,
                       mel_len_dev, T);
    AMP_HIP(hipGetLastError());
    return AMP_OK;
}

int amp_bucketize_embed_add(const float* pred_dev, float control, const float* bins_dev, int n_bounds, const float* table_dev, int n_rows,
                            const float* x_dev, int B, int D, int T, float* y_dev, float* pred_out_dev, void* stream) {
    if (!pred_dev || !bins_dev || !table_dev || !x_dev || !y_dev || !pred_out_dev) { set_error("amp_bucketize_embed_add: null argument"); return AMP_ERR_INVALID; }
    if (B < 1 || D < 1 || T < 1) { set_error("amp_bucketize_embed_add: B=%d D=%d T=%d", B, D, T); return AMP_ERR_INVALID; }
    if (n_bounds < 1 || n_rows < n_bounds + 1) {
        set_error("amp_bucketize_embed_add: %d boundaries need a table of at least %d rows (got %d)", n_bounds, n_bounds + 1, n_rows);
        return AMP_ERR_INVALID;
    }
    if (!(control == control)) { set_error("amp_bucketize_embed_add: control is NaN"); return AMP_ERR_INVALID; }
    if (pred_out_dev == pred_dev) { set_error("amp_bucketize_embed_add: pred_out must not alias pred"); return AMP_ERR_INVALID; }
    const unsigned dblocks = (unsigned)((D + BE_DT - 1) / BE_DT);
    if (B > 65535 || dblocks > 65535) { set_error("amp_bucketize_embed_add: B=%d D=%d is beyond the grid", B, D); return AMP_ERR_UNSUPPORTED; }
    const dim3 grid((unsigned)((T + BE_TT - 1) / BE_TT), dblocks, (unsigned)B);
    note_kernel("bucketize_embed_add_kernel");
    note_work((unsigned long long)grid.x * grid.y * grid.z, 0.0, 8.0 * (double)B * D * T / 1e6, "bucketize embed add D=%d T=%d B=%d bins=%d", D, T, B,
              n_bounds + 1);
    hipLaunchKernelGGL(bucketize_embed_add_kernel, grid, dim3(256), 0, (hipStream_t)stream, pred_dev, control, bins_dev, n_bounds, table_dev, x_dev,
                       y_dev, pred_out_dev, D, T);
    AMP_HIP(hipGetLastError());
    return AMP_OK;
}

int amp_layer_norm_c_head(const float* x_dev, const float* gamma_dev, const float* beta_dev, const float* w_dev, float b0, const int* lens_dev, int B,
                          int C, int T, float eps, float* y_dev, void* stream) {
    if (!x_dev || !gamma_dev || !beta_dev || !w_dev || !y_dev) { set_error("amp_layer_norm_c_head: null argument"); return AMP_ERR_INVALID; }
    if (B < 1 || C < 1 || T < 1 || B > 65535 || !(eps >= 0.f)) { set_error("amp_layer_norm_c_head: B=%d C=%d T=%d eps=%g", B, C, T, (double)eps); return AMP_ERR_INVALID; }
    const dim3 grid((unsigned)((T + LH_TT - 1) / LH_TT), (unsigned)B);
    note_kernel("layer_norm_c_head_kernel");
    note_work((unsigned long long)grid.x * grid.y, 0.0, 4.0 * (double)B * C * T / 1e6, "layer norm + head C=%d T=%d B=%d", C, T, B);
    hipLaunchKernelGGL(layer_norm_c_head_kernel, grid, dim3(256), 0, (hipStream_t)stream, x_dev, gamma_dev, beta_dev, w_dev, b0, lens_dev, y_dev, C, T,
                       eps);
    AMP_HIP(hipGetLastError());
    return AMP_OK;
}

}  // extern "C"
