// Residual vector quantizer with full-width Euclidean codebooks in eval mode: SpeechTokenizer's ResidualVectorQuantization
// (models/codec/speechtokenizer/modules/quantization/core_vq.py:180-236,331-388).  No projections: the codebook dimension IS the latent's
// (D <= 1024), K <= 4096 rows, N <= 32 levels.  amp_evq_encode = ResidualVectorQuantization.forward / .encode (codes, the sum of the levels'
// rows, every level's rows) in ONE launch for all levels; amp_evq_decode = .decode.
//
// Everything here decides or reproduces INTEGERS, so it is plain fp32 on the vector ALU, as csrc/fvq.hip is.  A workgroup of 256 threads owns
// EVQ_TF = 16 frames of one item and keeps their residual [16][D] and the running sum [16][D] in LDS across all levels: z is read once and the
// sum written once, whatever N is, and a codebook is streamed once per 16 frames, not once per frame.  Per level, in the reference's order:
//   dist = -((sum x^2 - (2 x) . e_k) + sum e_k^2)   core_vq.py:182-186; the doubling is exact, x . e_k is one fmaf chain over D in ascending
//                                                   order, sum e_k^2 is formed once at create time
//   code = lowest k of the largest dist             dist.max(-1).indices: a thread scans its k ascending with a strict <, ties between threads go
//                                                   to the lower index (the comparison runs on the un-negated value: the negation is exact)
//   residual -= embed[code];  sum += embed[code]
// The distances are register-tiled: a thread owns 4 frames x 4 codebook rows (thread = frame group + 4 * row group), so eight 16-byte loads --
// four rows from global memory, four frames' residual from LDS -- feed sixty-four fmaf; the four frame groups of a row group read a row as one
// broadcast request.  LDS rows are padded by 4 floats: the frames' 16-byte reads fall into different bank groups.  Codebook rows are zero-padded
// to a multiple of 4 floats; a padded term is fmaf(0, 0, acc) = acc, bit for bit.
// With st > 0 the walk starts level st from the WHOLE input, as ResidualVectorQuantization.encode does (core_vq.py:370-378): restated, not repaired.
#include <string.h>

#include <memory>

#include "amp_host.h"

namespace amp {

constexpr int EVQ_TF = 16;

struct EvqArgs {
    const float* z;          // [B, D, T]
    long long* codes;        // [n, B, T]
    float* zq;               // [B, D, T] or nullptr
    float* allq;             // [n, B, D, T] or nullptr
    const float* cb;         // [N][K][DP]
    const float* cn2;        // [N][K]
    int B, D, DP, K, T, st, n;
    int tiles_per_item;
};

__global__ __launch_bounds__(256) void evq_encode_kernel(const EvqArgs a) {
    extern __shared__ __attribute__((aligned(16))) float evq_smem[];
    const int D = a.D, DP = a.DP, K = a.K, T = a.T;
    const int RS = DP + 4;                     // row stride of R and Q
    float* R = evq_smem;                       // [TF][RS] residual
    float* Q = R + EVQ_TF * RS;                // [TF][RS] sum of the levels' rows
    float* X2 = Q + EVQ_TF * RS;               // [TF]
    float* BD = X2 + EVQ_TF;                   // [4][TF]
    int* BI = reinterpret_cast<int*>(BD + 4 * EVQ_TF);   // [4][TF]
    int* CODE = BI + 4 * EVQ_TF;               // [TF]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int f = tid & 15;
    const int part16 = tid >> 4;
    const int item = blockIdx.x / a.tiles_per_item;
    const int t0 = (blockIdx.x - item * a.tiles_per_item) * EVQ_TF;
    const int t = t0 + f;
    const bool tok = t < T;
    const float* zb = a.z + (size_t)item * D * T;

    for (int c = part16; c < DP; c += 16) {
        R[f * RS + c] = (tok && c < D) ? zb[(size_t)c * T + t] : 0.f;
        Q[f * RS + c] = 0.f;
    }
    __syncthreads();

    for (int l = 0; l < a.n; ++l) {
        const float* cb = a.cb + (size_t)(a.st + l) * K * DP;
        const float* cn2 = a.cn2 + (size_t)(a.st + l) * K;
        if (tid < EVQ_TF) {
            float s = 0.f;
            for (int c = 0; c < D; ++c) s = fmaf(R[tid * RS + c], R[tid * RS + c], s);
            X2[tid] = s;
        }
        __syncthreads();
        {
            // thread tile: 4 frames x 4 rows, so that eight 16-byte loads (four rows, four frames) feed sixty-four fmaf
            const int fg = tid & 3;                    // frames 4 fg .. 4 fg + 3
            const int kp = tid >> 2;                   // rows 4 kp + 256 pass + 0 .. 3, ascending within the thread
            const float4* r4[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) r4[i] = reinterpret_cast<const float4*>(R + (4 * fg + i) * RS);
            float best[4];
            int bi[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) { best[i] = __builtin_inff(); bi[i] = 0; }
            for (int k0 = kp * 4; k0 < K; k0 += 256) {
                const float4* row[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) row[u] = reinterpret_cast<const float4*>(cb + (size_t)(k0 + u < K ? k0 + u : K - 1) * DP);
                float dot[4][4];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int u = 0; u < 4; ++u) dot[i][u] = 0.f;
                for (int c4 = 0; c4 < DP / 4; ++c4) {
                    float4 e[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) e[u] = row[u][c4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        float4 x = r4[i][c4];
                        x.x *= 2.f; x.y *= 2.f; x.z *= 2.f; x.w *= 2.f;
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            float s = dot[i][u];
                            s = fmaf(x.x, e[u].x, s);
                            s = fmaf(x.y, e[u].y, s);
                            s = fmaf(x.z, e[u].z, s);
                            s = fmaf(x.w, e[u].w, s);
                            dot[i][u] = s;
                        }
                    }
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float x2 = X2[4 * fg + i];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        if (k0 + u < K) {
                            const float dist = (x2 - dot[i][u]) + cn2[k0 + u];
                            if (dist < best[i]) { best[i] = dist; bi[i] = k0 + u; }
                        }
                    }
                }
            }
            // the sixteen row groups of a wave, then the four waves: smaller distance wins, equal distances go to the lower index
#pragma unroll
            for (int o = 4; o <= 32; o <<= 1) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float ob = __shfl_xor(best[i], o, 64);
                    const int oi = __shfl_xor(bi[i], o, 64);
                    if (ob < best[i] || (ob == best[i] && oi < bi[i])) { best[i] = ob; bi[i] = oi; }
                }
            }
            if (lane < 4) {
#pragma unroll
                for (int i = 0; i < 4; ++i) { BD[wave * EVQ_TF + 4 * fg + i] = best[i]; BI[wave * EVQ_TF + 4 * fg + i] = bi[i]; }
            }
        }
        __syncthreads();
        if (tid < EVQ_TF) {
            float best = BD[tid];
            int bi = BI[tid];
            for (int w = 1; w < 4; ++w) {
                const float ob = BD[w * EVQ_TF + tid];
                const int oi = BI[w * EVQ_TF + tid];
                if (ob < best || (ob == best && oi < bi)) { best = ob; bi = oi; }
            }
            CODE[tid] = bi;
            if (t0 + tid < T) a.codes[((size_t)l * a.B + item) * T + t0 + tid] = bi;
        }
        __syncthreads();
        {
            const float* er = cb + (size_t)CODE[f] * DP;
            for (int c = part16; c < D; c += 16) {
                const float s = er[c];
                R[f * RS + c] -= s;
                Q[f * RS + c] += s;
                if (a.allq && tok) a.allq[(((size_t)l * a.B + item) * D + c) * T + t] = s;
            }
        }
        __syncthreads();
    }
    if (a.zq && tok) {
        float* qb = a.zq + (size_t)item * D * T;
        for (int c = part16; c < D; c += 16) qb[(size_t)c * T + t] = Q[f * RS + c];
    }
}

struct EvqDecArgs {
    const long long* codes;  // [n, B, T]
    float* out;              // [B, D, T]
    const float* cb;         // [N][K][DP]
    unsigned* flag;
    int B, D, DP, K, T, st, n;
    int tiles_per_item;
};

// decode: out = 0 + embed[st][codes[0]] + embed[st + 1][codes[1]] + .., the levels added in order.  A thread owns channels c = tid + 256 i (the
// row reads of a wave are contiguous) and walks the tile's 16 frames.  An index outside [0, K) raises the flag and reads row 0 instead.
__global__ __launch_bounds__(256) void evq_decode_kernel(const EvqDecArgs a) {
    extern __shared__ __attribute__((aligned(16))) float evq_dec_smem[];
    int* CODE = reinterpret_cast<int*>(evq_dec_smem);            // [n][TF]
    const int D = a.D, T = a.T, n = a.n;
    const int tid = threadIdx.x;
    const int item = blockIdx.x / a.tiles_per_item;
    const int t0 = (blockIdx.x - item * a.tiles_per_item) * EVQ_TF;
    for (int i = tid; i < n * EVQ_TF; i += 256) {
        const int l = i / EVQ_TF, ff = i - l * EVQ_TF;
        long long c = (t0 + ff < T) ? a.codes[((size_t)l * a.B + item) * T + t0 + ff] : 0;
        if (c < 0 || c >= a.K) { atomicOr(a.flag, 1u); c = 0; }
        CODE[i] = (int)c;
    }
    __syncthreads();
    float* ob = a.out + (size_t)item * D * T;
    const int nf = (T - t0) < EVQ_TF ? (T - t0) : EVQ_TF;
    for (int c = tid; c < D; c += 256) {
        for (int ff = 0; ff < nf; ++ff) {
            float acc = 0.f;
            for (int l = 0; l < n; ++l) acc += a.cb[((size_t)(a.st + l) * a.K + CODE[l * EVQ_TF + ff]) * a.DP + c];
            ob[(size_t)c * T + t0 + ff] = acc;
        }
    }
}

}  // namespace amp

using namespace amp;

struct amp_evq {
    int D = 0, DP = 0, K = 0, N = 0;
    float *cb = nullptr, *cn2 = nullptr;
    unsigned* flag = nullptr;
    DeviceAllocs dev;
};

static size_t evq_lds_bytes(int DP) { return ((size_t)2 * EVQ_TF * (DP + 4) + EVQ_TF * 10) * sizeof(float); }

extern "C" {

int amp_evq_create(int dim, int codebook_size, int num_quantizers, const float* const* codebook_host, amp_evq** out) {
    if (!codebook_host || !out) { set_error("amp_evq_create: null argument"); return AMP_ERR_INVALID; }
    const int D = dim, K = codebook_size, N = num_quantizers;
    if (D < 1 || K < 1 || N < 1) { set_error("amp_evq_create: D=%d K=%d N=%d", D, K, N); return AMP_ERR_INVALID; }
    if (D > 1024 || K > 4096 || N > 32) {
        set_error("amp_evq_create: D=%d K=%d N=%d is outside the kernel (D <= 1024, K <= 4096, N <= 32)", D, K, N);
        return AMP_ERR_UNSUPPORTED;
    }
    auto h = std::make_unique<amp_evq>();
    h->D = D; h->K = K; h->N = N;
    const int DP = (D + 3) & ~3;
    h->DP = DP;
    std::vector<float> cb((size_t)N * K * DP, 0.f), cn2((size_t)N * K, 0.f);
    for (int l = 0; l < N; ++l) {
        if (!codebook_host[l]) { set_error("amp_evq_create: null codebook at level %d", l); return AMP_ERR_INVALID; }
        for (int k = 0; k < K; ++k) {
            const float* r = codebook_host[l] + (size_t)k * D;
            float* row = &cb[((size_t)l * K + k) * DP];
            float s = 0.f;
            for (int j = 0; j < D; ++j) {
                if (!(fabsf(r[j]) < 1e30f)) { set_error("amp_evq_create: non-finite codebook entry (level %d)", l); return AMP_ERR_INVALID; }
                row[j] = r[j];
                s = fmaf(r[j], r[j], s);
            }
            cn2[(size_t)l * K + k] = s;
        }
    }
    // every refusal above is the host's alone: the arguments are judged the same with or without a device
    if (amp_device_count() <= 0) { set_error("amp_evq_create: no HIP device visible (the HIP path has no CPU fallback)"); return AMP_ERR_HIP; }
    AMP_RC(h->dev.upload(cb, &h->cb));
    AMP_RC(h->dev.upload(cn2, &h->cn2));
    const std::vector<float> zero(1, 0.f);
    AMP_RC(h->dev.upload(zero, &h->flag));
    *out = h.release();
    return AMP_OK;
}

void amp_evq_destroy(amp_evq* h) { delete h; }

static int evq_check_shape(const amp_evq* h, int st, int n_q, int B, int T, const char* who) {
    if (!h) { set_error("%s: null handle", who); return AMP_ERR_INVALID; }
    if (B <= 0 || T <= 0) { set_error("%s: B=%d T=%d", who, B, T); return AMP_ERR_INVALID; }
    if (st < 0 || n_q <= st || n_q > h->N) { set_error("%s: levels [%d, %d) of %d", who, st, n_q, h->N); return AMP_ERR_INVALID; }
    if ((long long)B * ((T + EVQ_TF - 1) / EVQ_TF) > 0x7fffffffll) { set_error("%s: B=%d x T=%d is beyond the grid", who, B, T); return AMP_ERR_UNSUPPORTED; }
    return AMP_OK;
}

int amp_evq_encode(const amp_evq* h, const float* z_dev, int B, int T, int st, int n_q, long long* codes_dev, float* zq_dev, float* all_zq_dev,
                   void* stream) {
    AMP_RC(evq_check_shape(h, st, n_q, B, T, "amp_evq_encode"));
    if (!z_dev || !codes_dev) { set_error("amp_evq_encode: null argument"); return AMP_ERR_INVALID; }
    if (z_dev == zq_dev) { set_error("amp_evq_encode: z and zq must not alias"); return AMP_ERR_INVALID; }
    EvqArgs a{};
    a.z = z_dev; a.codes = codes_dev; a.zq = zq_dev; a.allq = all_zq_dev; a.cb = h->cb; a.cn2 = h->cn2;
    a.B = B; a.D = h->D; a.DP = h->DP; a.K = h->K; a.T = T; a.st = st; a.n = n_q - st;
    a.tiles_per_item = (T + EVQ_TF - 1) / EVQ_TF;
    const unsigned grid = (unsigned)((size_t)B * a.tiles_per_item);
    const size_t lds = evq_lds_bytes(h->DP);
    const double frames = (double)B * T;
    note_kernel("evq_encode_kernel");
    note_work(grid, frames * a.n * 2.0 * h->K * h->D / 1e9,
              (frames * h->D * 4.0 * (1 + (zq_dev ? 1 : 0) + (all_zq_dev ? a.n : 0)) + frames * a.n * 8.0) / 1e6, "evq encode D=%d K=%d levels=%d..%d T=%d B=%d",
              h->D, h->K, st, n_q, T, B);
    AMP_HIP(ensure_dynamic_lds<&evq_encode_kernel>(lds));
    hipLaunchKernelGGL(evq_encode_kernel, dim3(grid), dim3(256), lds, (hipStream_t)stream, a);
    AMP_HIP(hipGetLastError());
    return AMP_OK;
}

int amp_evq_decode(const amp_evq* h, const long long* codes_dev, int n, int st, int B, int T, float* out_dev, void* stream) {
    AMP_RC(evq_check_shape(h, st, st + n, B, T, "amp_evq_decode"));
    if (!codes_dev || !out_dev) { set_error("amp_evq_decode: null argument"); return AMP_ERR_INVALID; }
    EvqDecArgs a{};
    a.codes = codes_dev; a.out = out_dev; a.cb = h->cb; a.flag = h->flag;
    a.B = B; a.D = h->D; a.DP = h->DP; a.K = h->K; a.T = T; a.st = st; a.n = n;
    a.tiles_per_item = (T + EVQ_TF - 1) / EVQ_TF;
    const unsigned grid = (unsigned)((size_t)B * a.tiles_per_item);
    const double frames = (double)B * T;
    note_kernel("evq_decode_kernel");
    note_work(grid, 0.0, (frames * h->D * 4.0 * (1 + n) + frames * n * 8.0) / 1e6, "evq decode D=%d K=%d levels=%d..%d T=%d B=%d", h->D, h->K, st, st + n, T, B);
    hipLaunchKernelGGL(evq_decode_kernel, dim3(grid), dim3(256), (size_t)n * EVQ_TF * sizeof(int), (hipStream_t)stream, a);
    AMP_HIP(hipGetLastError());
    return AMP_OK;
}

int amp_evq_check(amp_evq* h, void* stream) {
    if (!h) { set_error("amp_evq_check: null handle"); return AMP_ERR_INVALID; }
    unsigned v = 0;
    hipStream_t st = (hipStream_t)stream;
    AMP_HIP(hipMemcpyAsync(&v, h->flag, sizeof(v), hipMemcpyDeviceToHost, st));
    AMP_HIP(hipStreamSynchronize(st));
    if (v) {
        AMP_HIP(hipMemsetAsync(h->flag, 0, sizeof(v), st));
        AMP_HIP(hipStreamSynchronize(st));
        set_error("amp_evq_decode: a code index outside [0, %d) was given since the last check (the output of that call used row 0 in its place)", h->K);
        return AMP_ERR_INVALID;
    }
    return AMP_OK;
}

}  // extern "C"
