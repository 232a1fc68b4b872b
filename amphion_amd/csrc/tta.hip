// The element-wise and reduction launches of AudioLDM's UNet and of the AutoencoderKL decoder that are not a GEMM:
//     amp_group_norm_stats   GroupNorm(32)'s mean | rstd [B, 32, 2] of a channel-first x [B, C, T] (the conv reads them: conv2d_f16x3.hip's norm on load)
//     amp_group_norm         the apply with an optional SiLU, where no 3 x 3 conv follows (SpatialTransformer.norm -> proj_in)
//     amp_geglu              GEGLU on the stacked value | gate GEMM output
// Plain fp32 element-wise arithmetic; the statistics are summed in fp64.  Deterministic: fixed summation order, no atomics.
#include <hip/hip_runtime.h>

#include "amp_host.h"
#include "amphion_hip.h"
#include "gelu_erf.h"

namespace amp {

constexpr int GN_GROUPS = 32;
constexpr int GN_THREADS = 512;

// thread-strided partial sums, then a tree over LDS: the order depends on n alone
__device__ __forceinline__ double gn_block_sum(double v, double* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int s = GN_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// One workgroup per (item, group): the group's (C / 32) T elements are contiguous.  Two passes, the second centred, so |mean| >> std costs
// nothing; fp64 sums, so the result is the fp32 rounding of the exact statistics for every n this library meets.
__global__ __launch_bounds__(GN_THREADS) void group_norm_stats_kernel(const float* __restrict__ x, float* __restrict__ mr, size_t n, float eps) {
    __shared__ double red[GN_THREADS];
    const float* xg = x + (size_t)blockIdx.x * n;
    double s0 = 0.0, s1 = 0.0;
    size_t i = threadIdx.x;
    for (; i + GN_THREADS < n; i += 2 * GN_THREADS) {
        s0 += (double)xg[i];
        s1 += (double)xg[i + GN_THREADS];
    }
    if (i < n) s0 += (double)xg[i];
    const double mean = gn_block_sum(s0 + s1, red) / (double)n;
    double q0 = 0.0, q1 = 0.0;
    i = threadIdx.x;
    for (; i + GN_THREADS < n; i += 2 * GN_THREADS) {
        const double d0 = (double)xg[i] - mean, d1 = (double)xg[i + GN_THREADS] - mean;
        q0 += d0 * d0;
        q1 += d1 * d1;
    }
    if (i < n) {
        const double d0 = (double)xg[i] - mean;
        q0 += d0 * d0;
    }
    const double var = gn_block_sum(q0 + q1, red) / (double)n;      // biased, as torch's
    if (threadIdx.x == 0) {
        mr[2 * (size_t)blockIdx.x] = (float)mean;
        mr[2 * (size_t)blockIdx.x + 1] = (float)(1.0 / sqrt(var + (double)eps));
    }
}

__device__ __forceinline__ float tta_silu(float v) { return v / (1.0f + expf(-v)); }

__global__ __launch_bounds__(256) void group_norm_apply_kernel(const float* x, const float* __restrict__ mr, const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, float* y, int C, int T, int silu) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const int c = blockIdx.y, b = blockIdx.z;
    const float* m = mr + 2 * ((size_t)b * GN_GROUPS + c / (C / GN_GROUPS));
    const size_t o = ((size_t)b * C + c) * T + t;
    const float v = (x[o] - m[0]) * m[1] * gamma[c] + beta[c];
    y[o] = silu ? tta_silu(v) : v;
}

// u [B, 2F, T]: item blockIdx.y, n = F * T elements of value followed by n of gate.  vec: n % 4 == 0 and both bases 16-byte aligned.
__global__ __launch_bounds__(256) void geglu_kernel(const float* __restrict__ u, float* __restrict__ y, size_t n, int vec) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const float* a = u + (size_t)blockIdx.y * 2 * n;
    const float* g = a + n;
    float* yb = y + (size_t)blockIdx.y * n;
    if (vec) {
        if (i < (n >> 2)) {
            const float4 p = reinterpret_cast<const float4*>(a)[i], q = reinterpret_cast<const float4*>(g)[i];
            reinterpret_cast<float4*>(yb)[i] = make_float4(p.x * gelu_erf(q.x), p.y * gelu_erf(q.y), p.z * gelu_erf(q.z), p.w * gelu_erf(q.w));
        }
    } else if (i < n) {
        yb[i] = a[i] * gelu_erf(g[i]);
    }
}

}  // namespace amp

using namespace amp;

extern "C" {

int amp_group_norm_stats(const float* x_dev, int B, int C, int T, float eps, float* mean_rstd_dev, void* stream) {
    if (!x_dev || !mean_rstd_dev || B < 1 || C < 1 || T < 1 || !(eps >= 0.f) || !(eps < 1e30f)) {
        set_error("amp_group_norm_stats: bad argument (B=%d C=%d T=%d eps=%g)", B, C, T, (double)eps);
        return AMP_ERR_INVALID;
    }
    if (C % GN_GROUPS) { set_error("amp_group_norm_stats: C=%d is not a multiple of 32", C); return AMP_ERR_UNSUPPORTED; }
    if ((long long)B * GN_GROUPS > 0x7fffffffll) { set_error("amp_group_norm_stats: B=%d is beyond the grid", B); return AMP_ERR_UNSUPPORTED; }
    const size_t n = (size_t)(C / GN_GROUPS) * T;
    if (ranges_overlap(x_dev, (size_t)B * C * T * sizeof(float), mean_rstd_dev, (size_t)B * GN_GROUPS * 2 * sizeof(float))) {
        set_error("amp_group_norm_stats: mean_rstd overlaps x");
        return AMP_ERR_INVALID;
    }
    note_kernel("group_norm_stats_kernel");
    note_work((unsigned long long)B * GN_GROUPS, 0.0, 8.0 * (double)B * C * T / 1e6, "group norm stats C=%d T=%d B=%d", C, T, B);
    hipLaunchKernelGGL(group_norm_stats_kernel, dim3((unsigned)(B * GN_GROUPS)), dim3(GN_THREADS), 0, (hipStream_t)stream, x_dev, mean_rstd_dev, n, eps);
    AMP_HIP(hipGetLastError());
    return AMP_OK;
}

int amp_group_norm(const float* x_dev, const float* mean_rstd_dev, const float* gamma_dev, const float* beta_dev, int B, int C, int T, int silu,
                   float* y_dev, void* stream) {
    if (!x_dev || !mean_rstd_dev || !gamma_dev || !beta_dev || !y_dev || B < 1 || C < 1 || T < 1) {
        set_error("amp_group_norm: bad argument (B=%d C=%d T=%d)", B, C, T);
        return AMP_ERR_INVALID;
    }
    if (C % GN_GROUPS) { set_error("amp_group_norm: C=%d is not a multiple of 32", C); return AMP_ERR_UNSUPPORTED; }
    if (C > 65535 || B > 65535) { set_error("amp_group_norm: C=%d or B=%d is beyond the grid (65535)", C, B); return AMP_ERR_UNSUPPORTED; }
    const size_t bytes = (size_t)B * C * T * sizeof(float);
    if (y_dev != x_dev && ranges_overlap(x_dev, bytes, y_dev, bytes)) { set_error("amp_group_norm: y must be x or not overlap it"); return AMP_ERR_INVALID; }
    const dim3 grid((unsigned)((T + 255) / 256), (unsigned)C, (unsigned)B);
    note_kernel("group_norm_apply_kernel");
    note_work((unsigned long long)grid.x * grid.y * grid.z, 0.0, 8.0 * (double)B * C * T / 1e6, "group norm apply C=%d T=%d B=%d silu=%d", C, T, B, silu ? 1 : 0);
    hipLaunchKernelGGL(group_norm_apply_kernel, grid, dim3(256), 0, (hipStream_t)stream, x_dev, mean_rstd_dev, gamma_dev, beta_dev, y_dev, C, T, silu ? 1 : 0);
    AMP_HIP(hipGetLastError());
    return AMP_OK;
}

int amp_geglu(const float* u_dev, int B, int F, int T, float* y_dev, void* stream) {
    if (!u_dev || !y_dev || B < 1 || F < 1 || T < 1 || B > 65535) { set_error("amp_geglu: bad argument (B=%d F=%d T=%d)", B, F, T); return AMP_ERR_INVALID; }
    const size_t n = (size_t)F * T;
    if (ranges_overlap(u_dev, 2 * (size_t)B * n * sizeof(float), y_dev, (size_t)B * n * sizeof(float))) { set_error("amp_geglu: y must not overlap u"); return AMP_ERR_INVALID; }
    const int vec = (n & 3) == 0 && ((reinterpret_cast<uintptr_t>(u_dev) | reinterpret_cast<uintptr_t>(y_dev)) & 15) == 0 ? 1 : 0;
    const size_t threads = vec ? n >> 2 : n;
    const size_t blocks = (threads + 255) / 256;
    if (blocks > 0x7fffffffull) { set_error("amp_geglu: F*T=%zu is beyond the grid", n); return AMP_ERR_UNSUPPORTED; }
    note_kernel("geglu_kernel");
    note_work((unsigned long long)blocks * B, 0.0, 12.0 * (double)B * n / 1e6, "geglu F=%d T=%d B=%d", F, T, B);
    hipLaunchKernelGGL(geglu_kernel, dim3((unsigned)blocks, (unsigned)B), dim3(256), 0, (hipStream_t)stream, u_dev, y_dev, n, vec);
    AMP_HIP(hipGetLastError());
    return AMP_OK;
}

}  // extern "C"
