// The feature preparation in front of DualCodec's semantic branch (infer/dualcodec/inference_with_semantic.py:155-164,232): the w2v-BERT
// hidden states [B, T, C] (time-major) are normalised per channel, transposed to channel-first and average-pooled over `factor` frames:
//     out[b, c, u] = (1 / f) * sum_{k < f} (hidden[b, u f + k, c] - mean[c]) / std[c]          u < floor(T / f)
// Plain fp32 in this order: subtract, divide, the f terms summed in ascending time order starting from the first term, then times 1 / f
// (f = 1: the product is exact).  mean or std NULL skips that step.  The tail frames T - (T mod f) .. T - 1 are never read.
//
// One workgroup of 256 threads owns 64 channels x 32 output frames and transposes through LDS: the load walks channels fastest (256-B rows
// of the time-major input), the store walks output frames fastest (128-B rows of the channel-first output).
#include "amp_host.h"

namespace amp {

constexpr int SP_TC = 64, SP_TT = 32;

__global__ __launch_bounds__(256) void semantic_prepare_kernel(const float* __restrict__ hidden, const float* __restrict__ mean,
                                                               const float* __restrict__ stdv, float* __restrict__ out, int T, int C, int To,
                                                               int f, float inv_f) {
    __shared__ float tile[SP_TC][SP_TT + 1];
    const int tid = threadIdx.x;
    const int c0 = blockIdx.y * SP_TC, u0 = blockIdx.x * SP_TT;
    const int b = blockIdx.z;
    {
        const int cl = tid & (SP_TC - 1), g = tid / SP_TC;       // 4 frame groups
        const int c = c0 + cl;
        const bool cok = c < C;
        const float m = (mean && cok) ? mean[c] : 0.f;
        const float s = (stdv && cok) ? stdv[c] : 1.f;
        const float* hb = hidden + (size_t)b * T * C + (cok ? c : 0);
        for (int ul = g; ul < SP_TT; ul += 256 / SP_TC) {
            const int u = u0 + ul;
            float acc = 0.f;
            if (cok && u < To) {
                for (int k = 0; k < f; ++k) {
                    float v = hb[((size_t)u * f + k) * C];
                    if (mean) v -= m;
                    if (stdv) v /= s;
                    acc = k ? acc + v : v;
                }
                acc *= inv_f;
            }
            tile[cl][ul] = acc;
        }
    }
    __syncthreads();
    {
        const int ul = tid & (SP_TT - 1), g = tid / SP_TT;       // 8 channel groups
        const int u = u0 + ul;
        if (u < To) {
            float* ob = out + (size_t)b * C * To + u;
            for (int cl = g; cl < SP_TC; cl += 256 / SP_TT) {
                const int c = c0 + cl;
                if (c < C) ob[(size_t)c * To] = tile[cl][ul];
            }
        }
    }
}

}  // namespace amp

using namespace amp;

extern "C" {

int amp_semantic_prepare(const float* hidden_dev, const float* mean_dev, const float* std_dev, int B, int T, int C, int factor, float* out_dev,
                         void* stream) {
    if (!hidden_dev || !out_dev) { set_error("amp_semantic_prepare: null argument"); return AMP_ERR_INVALID; }
    if (B <= 0 || T <= 0 || C <= 0 || factor < 1) { set_error("amp_semantic_prepare: B=%d T=%d C=%d factor=%d", B, T, C, factor); return AMP_ERR_INVALID; }
    if (T < factor) { set_error("amp_semantic_prepare: T=%d is shorter than one pooling window (factor %d)", T, factor); return AMP_ERR_INVALID; }
    if (hidden_dev == out_dev) { set_error("amp_semantic_prepare: out must not alias hidden"); return AMP_ERR_INVALID; }
    const int To = T / factor;
    const long long gy = (C + SP_TC - 1) / SP_TC;
    if (B > 65535 || gy > 65535) { set_error("amp_semantic_prepare: B=%d C=%d is beyond the grid", B, C); return AMP_ERR_UNSUPPORTED; }
    const dim3 grid((To + SP_TT - 1) / SP_TT, (unsigned)gy, B);
    const double n = (double)B * To * C;
    note_kernel("semantic_prepare_kernel");
    note_work((unsigned long long)grid.x * grid.y * grid.z, n * factor * 3.0 / 1e9, n * (factor + 1) * 4.0 / 1e6,
              "semantic prepare C=%d T=%d f=%d B=%d", C, T, factor, B);
    hipLaunchKernelGGL(semantic_prepare_kernel, grid, dim3(256), 0, (hipStream_t)stream, hidden_dev, mean_dev, std_dev, out_dev, T, C, To, factor,
                       1.0f / (float)factor);
    AMP_HIP(hipGetLastError());
    return AMP_OK;
}

}  // extern "C"
