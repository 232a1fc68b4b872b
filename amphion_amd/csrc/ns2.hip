// The element-wise part of NaturalSpeech2's ODE solver (models/tts/naturalspeech2/diffusion.py:72-102) that is not the WaveNet:
//     amp_ns2_ode_step    the tail of Diffusion.cal_dxt and the update `xt - dxt` in one launch (about ten element-wise launches of the reference)
// The WaveNet's residual layer is ns2_layer_f16x3.hip, its attention llama_nar.hip's amp_cross_attention.  Plain fp32, deterministic.
#include <hip/hip_runtime.h>

#include "amp_host.h"
#include "amphion_hip.h"

namespace amp {

// cal_dxt's order of operations, one rounding each (nothing contracts: the products feed subtractions and a divide through named values):
//     mean  = x0 * e                      e     = exp(-0.5 * cum_beta / sigma^2)
//     noise = x_eval - mean
//     logp  = -noise / (var + 1e-8)       var   = sigma^2 * (1 - exp(-cum_beta / sigma^2))
//     dxt   = (-0.5 * hb) * (logp + x_eval * is2)      hb = h * beta_t, is2 = 1 / sigma^2
//     out   = x_base - dxt                (mid: 0.5 * (out + x_base), the midpoint solver's x_mid)
__device__ __forceinline__ float ode_step_f(float xe, float x0, float xb, float e, float den, float coef, float is2, int mid) {
    const float mean = __fmul_rn(x0, e);
    const float noise = xe - mean;
    const float logp = -noise / den;
    const float dxt = __fmul_rn(coef, logp + __fmul_rn(xe, is2));
    const float o = xb - dxt;
    return mid ? 0.5f * (o + xb) : o;
}

// amp_gelu's shape: vec = every base 16-byte aligned -- threads [0, n / 4) take quads, the next n % 4 threads the tail
__global__ __launch_bounds__(256) void ns2_ode_step_kernel(const float* xe, const float* x0, const float* xb, float* out, size_t n, float e, float den,
                                                           float coef, float is2, int mid, int vec) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (vec) {
        const size_t nq = n >> 2;
        if (i < nq) {
            const float4 a = reinterpret_cast<const float4*>(xe)[i], b = reinterpret_cast<const float4*>(x0)[i], c = reinterpret_cast<const float4*>(xb)[i];
            reinterpret_cast<float4*>(out)[i] = make_float4(ode_step_f(a.x, b.x, c.x, e, den, coef, is2, mid), ode_step_f(a.y, b.y, c.y, e, den, coef, is2, mid),
                                                            ode_step_f(a.z, b.z, c.z, e, den, coef, is2, mid), ode_step_f(a.w, b.w, c.w, e, den, coef, is2, mid));
        } else {
            const size_t k = 4 * nq + (i - nq);
            if (k < n) out[k] = ode_step_f(xe[k], x0[k], xb[k], e, den, coef, is2, mid);
        }
    } else if (i < n) {
        out[i] = ode_step_f(xe[i], x0[i], xb[i], e, den, coef, is2, mid);
    }
}

}  // namespace amp

using namespace amp;

extern "C" {

int amp_ns2_ode_step(const float* x_eval_dev, const float* x0_pred_dev, const float* x_base_dev, long long n, float mean_scale, float variance,
                     float h_beta, float inv_sigma2, int midpoint_half, float* out_dev, void* stream) {
    if (!x_eval_dev || !x0_pred_dev || !x_base_dev || !out_dev || n <= 0) { set_error("amp_ns2_ode_step: bad argument (n=%lld)", n); return AMP_ERR_INVALID; }
    if (!(mean_scale == mean_scale) || !(variance == variance) || !(h_beta == h_beta) || !(inv_sigma2 == inv_sigma2)) {
        set_error("amp_ns2_ode_step: a NaN scalar");
        return AMP_ERR_INVALID;
    }
    const size_t bytes = (size_t)n * sizeof(float);
    for (const float* p : {x_eval_dev, x0_pred_dev, x_base_dev}) {
        const char* a = (const char*)p;
        const char* o = (const char*)out_dev;
        if (p != out_dev && a < o + bytes && o < a + bytes) { set_error("amp_ns2_ode_step: out must be an input or not overlap it"); return AMP_ERR_INVALID; }
    }
    const int vec = ((reinterpret_cast<uintptr_t>(x_eval_dev) | reinterpret_cast<uintptr_t>(x0_pred_dev) | reinterpret_cast<uintptr_t>(x_base_dev) |
                      reinterpret_cast<uintptr_t>(out_dev)) & 15) == 0 ? 1 : 0;
    const long long threads = vec ? (n >> 2) + (n & 3) : n;
    const long long blocks = (threads + 255) / 256;
    if (blocks > 0x7fffffffll) { set_error("amp_ns2_ode_step: n=%lld is beyond the grid", n); return AMP_ERR_UNSUPPORTED; }
    note_kernel("ns2_ode_step_kernel");
    note_work((unsigned long long)blocks, 0.0, 16.0 * (double)n / 1e6, "ns2 ode step n=%lld mid=%d", n, midpoint_half ? 1 : 0);
    hipLaunchKernelGGL(ns2_ode_step_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x_eval_dev, x0_pred_dev, x_base_dev, out_dev, (size_t)n,
                       mean_scale, variance + 1e-8f, -0.5f * h_beta, inv_sigma2, midpoint_half ? 1 : 0, vec);
    AMP_HIP(hipGetLastError());
    return AMP_OK;
}

}  // extern "C"
