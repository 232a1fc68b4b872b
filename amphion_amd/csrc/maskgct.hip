// The decoding step's sampler of MaskGCT (models/tts/maskgct/maskgct_t2s.py:14-32, 319-337; maskgct_s2a.py the same):
//     amp_mask_sample   top-k filter of the logits, Gumbel-sampled id per frame, softmax probability of that id -- one launch
// The logits are the pointwise GEMM's output, channel-first [B, V, T], read in place; the noise is the reference's own [B, T, V] tensor.
// Plain fp32 with accurate expf / logf and a correctly rounded divide.  Deterministic: no atomics, every reduction in a fixed order.
//
// A wave owns R rows (b, t) in registers, NV = ceil(V / 64) values per lane and row (lane holds v = 64 i + lane), as ORDER-PRESERVING
// INTEGER IMAGES of the floats: key(x) = bits ^ 0x80000000 for x >= 0, ~bits for x < 0, so a < b <=> key(a) < key(b) and a value beyond
// V is key 0, below every float.  The workgroup (four waves, TT = 4 R rows) reads [64 G values x TT frames] stages -- TT consecutive floats
// of each channel-first row, 64 bytes at TT = 16 -- and transposes them through padded LDS, the loads of stage s + 1 in flight behind the
// transposition of stage s.  Then per row:
//   1. the k-th largest key by a 32-step bitwise bisection: theta = the largest c with count(key >= c) >= k, one ballot count per register;
//   2. one walk in index order: kept = key > theta, or key == theta and among the first k - count(key > theta) of them (a tie at the k-th
//      value goes to the LOWER index); the sum of exp(l - max) over the kept, the lowest index of the maximum (the greedy id), and -- in
//      groups of 16 registers, the noise loads of a group issued together -- the noisy value l / temp + g of the kept entries alone.
//   3. wave reductions in a fixed butterfly; an equal noisy value goes to the LOWER index.
// No sort, no histogram.  A NaN logit has a key like any other (beyond +inf or below -inf by its sign): the id stays in [0, V), the
// score is NaN.
#include <hip/hip_runtime.h>

#include "amp_host.h"
#include "amphion_hip.h"

namespace amp {

constexpr int MS_MAX_V = 8192;
constexpr int MS_GROUP = 16;      // registers per noise-load group

struct MaskSampleArgs {
    const float* logits;          // [B, V, T], items bstride apart
    long long bstride;
    const float* u;               // [B, T, V] or nullptr (greedy)
    long long* ids;               // [B, T]
    float* score;                 // [B, T]
    int V, T, k;
    float tdiv;                   // max(temperature, 1e-10)
};

__device__ __forceinline__ unsigned ms_key(float x) {
    const unsigned b = __float_as_uint(x + 0.0f);          // -0 -> +0: the two compare equal as floats
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float ms_val(unsigned key) {
    return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
}

template <int NV, int R>
__global__ __launch_bounds__(256) void mask_sample_kernel(MaskSampleArgs a) {
    constexpr int TT = 4 * R;                 // rows of the workgroup
    constexpr int G = 32 / TT;                // 64-value chunks per stage: a thread loads 8 values per stage
    constexpr int SV = 64 * G;                // values per stage
    constexpr int NS = NV / G;                // stages
    constexpr int LS = TT + 1;                // padded row: a wave's 64 reads of one frame fall on distinct banks
    static_assert(NV % G == 0 && NV % MS_GROUP == 0 && SV * TT == 8 * 256, "stage geometry");
    __shared__ unsigned tile[2][SV * LS];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int V = a.V, T = a.T;
    const int b = blockIdx.y, t0 = blockIdx.x * TT;
    const float* __restrict__ lg = a.logits + (size_t)b * (size_t)a.bstride;

    // ---- the rows into registers
    unsigned key[R][NV];
    unsigned pr[8];
    auto load_stage = [&](int s) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int idx = tid + 256 * e, tl = idx % TT, v = s * SV + idx / TT, t = t0 + tl;
            pr[e] = (v < V && t < T) ? ms_key(lg[(size_t)v * T + t]) : 0u;
        }
    };
    load_stage(0);
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        if (s * SV < V) {                     // uniform over the workgroup
            unsigned* tl_ = tile[s & 1];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int idx = tid + 256 * e;
                tl_[(idx / TT) * LS + idx % TT] = pr[e];
            }
            __syncthreads();                  // one barrier a stage: buffer s & 1 was last read before the barrier of stage s - 1
            if (s + 1 < NS && (s + 1) * SV < V) load_stage(s + 1);
#pragma unroll
            for (int g = 0; g < G; ++g)
#pragma unroll
                for (int r = 0; r < R; ++r) key[r][s * G + g] = tl_[(64 * g + lane) * LS + w * R + r];
        } else {
#pragma unroll
            for (int g = 0; g < G; ++g)
#pragma unroll
                for (int r = 0; r < R; ++r) key[r][s * G + g] = 0u;
        }
    }

    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    const bool greedy = a.u == nullptr;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int t = t0 + w * R + r;
        if (t >= T) continue;                 // uniform over the wave; no barrier below
        // ---- 1. theta = the k-th largest key (values beyond V are key 0 and never reach a candidate, which is >= 1)
        unsigned th = 0u;
        for (int bit = 31; bit >= 0; --bit) {
            const unsigned c = th | (1u << bit);
            int cnt = 0;
#pragma unroll
            for (int i = 0; i < NV; ++i) cnt += __popcll(__ballot(key[r][i] >= c));
            if (cnt >= a.k) th = c;
        }
        int above = 0;
        unsigned kmax = 0u;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            above += __popcll(__ballot(key[r][i] > th));
            kmax = key[r][i] > kmax ? key[r][i] : kmax;
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const unsigned other = (unsigned)__shfl_xor((int)kmax, o);
            kmax = other > kmax ? other : kmax;
        }
        const int need = a.k - above;         // >= 1: how many of the keys equal to theta are kept, lowest indices first
        const float mval = ms_val(kmax);

        // ---- 2. one walk in index order
        const float* __restrict__ ub = greedy ? nullptr : a.u + ((size_t)b * T + t) * (size_t)V;
        int eq_seen = 0, gid = 0x7fffffff, bestv = 0x7fffffff;
        float sum = 0.f, besty = -INFINITY, bestl = 0.f;
#pragma unroll
        for (int g0 = 0; g0 < NV; g0 += MS_GROUP) {
            if (64 * g0 >= V) continue;       // uniform
            unsigned keptm = 0u;
            float uu[MS_GROUP];
#pragma unroll
            for (int j = 0; j < MS_GROUP; ++j) {
                const unsigned kk = key[r][g0 + j];
                const int v = 64 * (g0 + j) + lane;
                const bool in = v < V;
                const bool eq = in && kk == th;
                const unsigned long long em = __ballot(eq);
                const int rank = eq_seen + __popcll(em & lt_mask);
                eq_seen += __popcll(em);
                const bool kept = in && (kk > th || (eq && rank < need));
                keptm |= kept ? (1u << j) : 0u;
                if (in && kk == kmax) gid = v < gid ? v : gid;
                uu[j] = 0.5f;
                if (kept && !greedy) uu[j] = ub[v];
            }
#pragma unroll
            for (int j = 0; j < MS_GROUP; ++j) {
                if ((keptm >> j) & 1u) {
                    const float lv = ms_val(key[r][g0 + j]);
                    sum += expf(lv - mval);
                    if (!greedy) {
                        const float gum = -logf(-logf(uu[j] + 1e-10f) + 1e-10f);
                        const float y = lv / a.tdiv + gum;
                        if (y > besty) { besty = y; bestv = 64 * (g0 + j) + lane; bestl = lv; }   // the lane's indices ascend
                    }
                }
            }
        }

        // ---- 3. the wave's sum, greedy id and noisy argmax
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            sum += __shfl_xor(sum, o);
            const int og = __shfl_xor(gid, o);
            gid = og < gid ? og : gid;
            const float oy = __shfl_xor(besty, o), ol = __shfl_xor(bestl, o);
            const int ov = __shfl_xor(bestv, o);
            if (oy > besty || (oy == besty && ov < bestv)) { besty = oy; bestv = ov; bestl = ol; }
        }
        // greedy, or no noisy value compared above -inf (only with non-finite logits): the lowest index of the maximum
        const bool use_g = greedy || bestv >= V;
        const int id = use_g ? gid : bestv;
        const float lid = use_g ? mval : bestl;
        if (lane == 0) {
            a.ids[(size_t)b * T + t] = (long long)(id < V ? id : V - 1);
            a.score[(size_t)b * T + t] = expf(lid - mval) / sum;
        }
    }
}

template <int NV, int R>
static void launch_mask_sample(const MaskSampleArgs& a, int B, hipStream_t st) {
    constexpr int TT = 4 * R;
    const dim3 grid((unsigned)((a.T + TT - 1) / TT), (unsigned)B);
    note_kernel("mask_sample_kernel", NV, R);
    note_work((unsigned long long)grid.x * grid.y, 0.0, (4.0 * (double)B * a.V * a.T + (a.u ? 4.0 * (double)B * a.T * a.k : 0.0) + 12.0 * (double)B * a.T) / 1e6,
              "mask sample V=%d k=%d T=%d B=%d %s", a.V, a.k, a.T, B, a.u ? "gumbel" : "greedy");
    hipLaunchKernelGGL((mask_sample_kernel<NV, R>), grid, dim3(256), 0, st, a);
}

}  // namespace amp

using namespace amp;

extern "C" {

int amp_mask_sample(const float* logits_dev, long long batch_stride, int B, int V, int T, int k, const float* u_dev, float temperature,
                    long long* ids_dev, float* score_dev, void* stream) {
    if (!logits_dev || !ids_dev || !score_dev) { set_error("amp_mask_sample: null argument"); return AMP_ERR_INVALID; }
    if (V < 2 || V > MS_MAX_V) { set_error("amp_mask_sample: V=%d is outside [2, %d]", V, MS_MAX_V); return AMP_ERR_INVALID; }
    if (k < 1 || k > V) { set_error("amp_mask_sample: k=%d is outside [1, V=%d]", k, V); return AMP_ERR_INVALID; }
    if (B < 1 || T < 1 || B > 65535) { set_error("amp_mask_sample: B=%d T=%d (B <= 65535)", B, T); return AMP_ERR_INVALID; }
    if (batch_stride == 0) batch_stride = (long long)V * T;
    if (batch_stride < (long long)V * T) { set_error("amp_mask_sample: batch stride %lld < V*T", batch_stride); return AMP_ERR_INVALID; }
    if (u_dev && !(temperature == temperature)) { set_error("amp_mask_sample: temperature is NaN"); return AMP_ERR_INVALID; }
    const size_t rows = (size_t)B * T;
    const char* in_lo[2] = {reinterpret_cast<const char*>(logits_dev), reinterpret_cast<const char*>(u_dev)};
    const size_t in_bytes[2] = {((size_t)(B - 1) * (size_t)batch_stride + (size_t)V * T) * sizeof(float), u_dev ? rows * V * sizeof(float) : 0};
    const char* out_lo[2] = {reinterpret_cast<const char*>(ids_dev), reinterpret_cast<const char*>(score_dev)};
    const size_t out_bytes[2] = {rows * sizeof(long long), rows * sizeof(float)};
    for (int o = 0; o < 2; ++o)
        for (int i = 0; i < 2; ++i)
            if (in_bytes[i] && out_lo[o] < in_lo[i] + in_bytes[i] && in_lo[i] < out_lo[o] + out_bytes[o]) {
                set_error("amp_mask_sample: ids / score must not overlap logits / u");
                return AMP_ERR_INVALID;
            }
    if (out_lo[0] < out_lo[1] + out_bytes[1] && out_lo[1] < out_lo[0] + out_bytes[0]) {
        set_error("amp_mask_sample: ids and score overlap");
        return AMP_ERR_INVALID;
    }
    MaskSampleArgs a{};
    a.logits = logits_dev; a.bstride = batch_stride;
    a.u = u_dev;
    a.ids = ids_dev; a.score = score_dev;
    a.V = V; a.T = T; a.k = k;
    a.tdiv = fmaxf(temperature, 1e-10f);
    if (V <= 1024) launch_mask_sample<16, 4>(a, B, (hipStream_t)stream);
    else if (V <= 4096) launch_mask_sample<64, 2>(a, B, (hipStream_t)stream);
    else launch_mask_sample<128, 1>(a, B, (hipStream_t)stream);
    AMP_HIP(hipGetLastError());
    return AMP_OK;
}

}  // extern "C"
