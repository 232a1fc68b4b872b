// The kernels of VALL-E's decoder (models/tts/valle/valle.py: a pre-norm LayerNorm / ReLU transformer over [text | audio]) that the tree did not
// have.  The prefix-LM prefill attention is an instantiation of llama_nar.hip's kernel (amp_prefix_attention) and the Linears of a decode
// step, with the LayerNorm in front of them folded in, are pw_vec.hip's (amp_pw_forward_vec_ln); what is left here:
//     amp_embed_pos            token embedding plus the sinusoidal position row from a running position, channel-first
// Plain fp32 on the vector pipe.  Deterministic: no sums, no atomics on data (amp_embed_pos ORs its bad-id flag), no workgroup waits for
// another.
#include <hip/hip_runtime.h>

#include "amp_host.h"
#include "amphion_hip.h"

namespace amp {

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

}  // namespace amp

using namespace amp;

extern "C" {

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
