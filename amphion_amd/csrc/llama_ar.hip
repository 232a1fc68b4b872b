// The decoding side of Vevo's autoregressive transformer (models/vc/autoregressive_transformer/ar_model.py: a causal LlamaForCausalLM that
// generates one token at a time).  The prefill is amp_rope_attention_causal (llama_nar.hip) over the pointwise GEMM; a decode step has one
// column per item and is made of the launches of this file and of its Linears (pw_vec.hip: amp_pw_forward_vec):
//     amp_kv_append            rope(k) and v of T new columns into the per-layer caches [B, H dk, Lmax]
//     amp_attention_decode     one query per (item, head) over cache columns [0, L): exact fp32, keys split across workgroups
//     amp_ar_sample            HF's processor chain (repetition penalty, EOS suppression, temperature, top-k, top-p) and the draw
// Plain fp32 on the vector pipe with accurate expf and correctly rounded divides.  Deterministic: every reduction runs in a fixed order, no
// atomics on data (the sampler ORs bits of an LDS bitmap of the ids seen so far), no workgroup waits for another.
#include <hip/hip_runtime.h>

#include "amp_host.h"
#include "amphion_hip.h"

namespace amp {

// ---- amp_kv_append --------------------------------------------------------------------------------------------------------------------
// thread = (item, head, channel pair i < dk / 2, column t): HF's rotate-half form on k, bit copies of v
struct KvAppendArgs {
    const float* k;
    const float* v;
    long long bstride;
    const float* cs;      // [>= pos0 + T, dk / 2]
    const float* sn;
    float* kc;            // [B, H dk, Lmax]
    float* vc;
    int H, dk, T, pos0, Lmax;
    size_t n;             // B * H * (dk / 2) * T
};

__global__ __launch_bounds__(256) void kv_append_kernel(KvAppendArgs a) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.n) return;
    const int half = a.dk >> 1;
    const int t = (int)(idx % (size_t)a.T);
    size_t r = idx / (size_t)a.T;
    const int i = (int)(r % (size_t)half);
    r /= (size_t)half;
    const int h = (int)(r % (size_t)a.H), b = (int)(r / (size_t)a.H);
    const size_t src = (size_t)b * (size_t)a.bstride + ((size_t)h * a.dk + i) * a.T + t;
    const size_t dst = (((size_t)b * a.H + h) * a.dk + i) * a.Lmax + a.pos0 + t;
    const size_t hs = (size_t)half * a.T, hd = (size_t)half * a.Lmax;
    const float x1 = a.k[src], x2 = a.k[src + hs];
    const float c = a.cs[(size_t)(a.pos0 + t) * half + i], s = a.sn[(size_t)(a.pos0 + t) * half + i];
    a.kc[dst] = x1 * c - x2 * s;
    a.kc[dst + hd] = x2 * c + x1 * s;
    a.vc[dst] = a.v[src];
    a.vc[dst + hd] = a.v[src + hs];
}

// ---- amp_attention_decode -------------------------------------------------------------------------------------------------------------
// Workgroup (sp, bh) of two waves owns keys [DEC_S sp, DEC_S (sp + 1)) of one (item, head): a thread is ONE key, the contiguous axis of the
// cache, so every channel row is read as whole 256-byte segments.  It forms its key's score over the dk channels (q' = rope(q) is computed
// by the first dk / 2 threads into LDS; the head dimension is a template argument so that a column's loads are issued together), the
// split's maximum and sum, and -- channel by channel, a wave butterfly over the keys and then the two waves in order -- the split's sum of
// p v.  With one split the quotient goes straight to out; with more, (max, sum, O) go to the workspace and decode_combine_kernel rescales
// and adds the splits in ascending order.  A key >= L is never an operand: its loads are redirected to column L - 1 and its terms are
// selected away, whatever the cache holds there.
constexpr int DEC_S = 128;       // keys per workgroup
constexpr int DEC_MAX_DK = 96;

struct DecodeArgs {
    const float* q;       // [B, H dk], items qbs apart
    long long qbs;
    const float* cs;      // the tables' row 0; row L - 1 is read
    const float* sn;
    const float* kc;
    const float* vc;
    float* out;           // [B, H dk]
    float* ws;            // [B H][nsplit][dk + 2]: max, sum, O
    int H, dk, L, Lmax, nsplit;
    float scale;
};

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = __builtin_fmaxf(v, __shfl_xor(v, o));
    return v;
}

template <int DK>
__global__ __launch_bounds__(DEC_S) void attention_decode_kernel(DecodeArgs a) {
    __shared__ float qs[DEC_MAX_DK];
    __shared__ float red[2][DEC_MAX_DK + 2];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int sp = blockIdx.x, bh = blockIdx.y;
    const int b = bh / a.H, h = bh - b * a.H;
    constexpr int dk = DK, half = DK / 2;
    const int L = a.L;
    if (tid < half) {
        const float* qb = a.q + (size_t)b * (size_t)a.qbs + (size_t)h * dk;
        const float x1 = qb[tid], x2 = qb[tid + half];
        const float c = a.cs[(size_t)(L - 1) * half + tid], s = a.sn[(size_t)(L - 1) * half + tid];
        qs[tid] = x1 * c - x2 * s;
        qs[tid + half] = x2 * c + x1 * s;
    }
    __syncthreads();
    const int key = sp * DEC_S + tid;
    const bool valid = key < L;
    const size_t col = (size_t)(valid ? key : L - 1);
    const float* __restrict__ kb = a.kc + (size_t)bh * dk * a.Lmax + col;
    const float* __restrict__ vb = a.vc + (size_t)bh * dk * a.Lmax + col;
    // the thread's K column and then its V column are loaded whole before they are used: DK independent loads in flight, not DK round trips
    float col_[DK];
#pragma unroll
    for (int d = 0; d < DK; ++d) col_[d] = kb[(size_t)d * a.Lmax];
    float dot = 0.f;
#pragma unroll
    for (int d = 0; d < DK; ++d) dot = fmaf(qs[d], col_[d], dot);
#pragma unroll
    for (int d = 0; d < DK; ++d) col_[d] = vb[(size_t)d * a.Lmax];
    const float s = valid ? dot * a.scale : -INFINITY;
    const float wm = wave_max(s);
    if (lane == 0) red[w][0] = wm;
    __syncthreads();
    const float m = __builtin_fmaxf(red[0][0], red[1][0]);      // finite: key DEC_S sp < L is in this split
    __syncthreads();
    const float p = valid ? expf(s - m) : 0.f;
    const float ps = wave_sum(p);
    if (lane == 0) red[w][dk + 1] = ps;
#pragma unroll
    for (int d = 0; d < DK; ++d) {
        const float o = wave_sum(valid ? p * col_[d] : 0.f);
        if (lane == 0) red[w][1 + d] = o;
    }
    __syncthreads();
    const float l = red[0][dk + 1] + red[1][dk + 1];
    if (tid < dk) {
        const float o = red[0][1 + tid] + red[1][1 + tid];
        if (a.nsplit == 1) {
            a.out[(size_t)bh * dk + tid] = o / l;
        } else {
            float* wsp = a.ws + ((size_t)bh * a.nsplit + sp) * (size_t)(dk + 2);
            wsp[2 + tid] = o;
            if (tid == 0) { wsp[0] = m; wsp[1] = l; }
        }
    }
}

// thread d < dk of workgroup bh (two waves): the splits in ascending order
__global__ __launch_bounds__(DEC_S) void decode_combine_kernel(DecodeArgs a) {
    const int bh = blockIdx.x, d = threadIdx.x, dk = a.dk;
    if (d >= dk) return;
    const float* wsp = a.ws + (size_t)bh * a.nsplit * (size_t)(dk + 2);
    float M = -INFINITY;
    for (int sp = 0; sp < a.nsplit; ++sp) M = __builtin_fmaxf(M, wsp[(size_t)sp * (dk + 2)]);
    float l = 0.f, o = 0.f;
    for (int sp = 0; sp < a.nsplit; ++sp) {
        const float* e = wsp + (size_t)sp * (dk + 2);
        const float f = expf(e[0] - M);
        l = fmaf(e[1], f, l);
        o = fmaf(e[2 + d], f, o);
    }
    a.out[(size_t)bh * dk + d] = o / l;
}

// ---- amp_ar_sample --------------------------------------------------------------------------------------------------------------------
// One workgroup of 16 waves per item; thread t holds the values v = 1024 i + t, i < 16, in registers.  In HF's order:
//   1. the ids seen so far set bits of an LDS bitmap (an id counts once however often it occurs, as HF's gather / scatter does); a logit
//      whose bit is set becomes l < 0 ? l p : l / p;
//   2. the EOS logit becomes -inf while the caller says so;  3. l / temperature;
//   4. theta = the k-th largest value by a 32-step bitwise bisection over the order-preserving integer images (maskgct.hip), kept =
//      key >= theta: HF removes l < theta, so every tie at the boundary stays;
//   5. p1 = softmax over the kept; HF removes the ascending-sorted prefix whose cumulative p1 is <= 1 - top_p, that is the values v with
//      mass(l_v) = sum of p1 over {l <= l_v} <= 1 - top_p -- a second bisection finds the largest such key; the maximum always stays;
//   6. p = softmax over what is left, id = argmax p_v / q_v, the lower index on a tie.
// Every workgroup-wide count, sum and argmax is: the thread's registers in ascending i, a wave butterfly, the 16 waves in ascending order.
constexpr int AS_NV = 16, AS_THREADS = 1024, AS_WAVES = 16, AS_MAX_V = AS_NV * AS_THREADS;

struct ArSampleArgs {
    const float* logits;  // [B, V], items bstride apart
    long long bstride;
    const float* q;       // [B, V] Exp(1) noise
    long long* ids;       // [B, cap]: the ids so far in [0, n), the new one goes to [n]
    long long cap;
    int V, n, k, eos;     // eos < 0: not suppressed
    float temperature, penalty, drop;     // drop = 1 - top_p; < 0: top-p disabled
};

__device__ __forceinline__ unsigned as_key(float x) {
    const unsigned b = __float_as_uint(x + 0.0f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__global__ __launch_bounds__(AS_THREADS) void ar_sample_kernel(ArSampleArgs a) {
    __shared__ unsigned seen[AS_MAX_V / 32];
    __shared__ int icnt[2][AS_WAVES];
    __shared__ float fsum[2][AS_WAVES];
    __shared__ float bestr[AS_WAVES];
    __shared__ int bestv[AS_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int V = a.V, b = blockIdx.x;
    const float* __restrict__ lg = a.logits + (size_t)b * (size_t)a.bstride;
    long long* idb = a.ids + (size_t)b * (size_t)a.cap;
    int par = 0;                                           // which of the two exchange buffers the next reduction uses
    auto block_count = [&](int wave_count) {
        if (lane == 0) icnt[par][w] = wave_count;
        __syncthreads();
        int c = 0;
#pragma unroll
        for (int i = 0; i < AS_WAVES; ++i) c += icnt[par][i];
        par ^= 1;
        return c;
    };
    auto block_sum = [&](float part) {
        part = wave_sum(part);
        if (lane == 0) fsum[par][w] = part;
        __syncthreads();
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < AS_WAVES; ++i) s += fsum[par][i];
        par ^= 1;
        return s;
    };

    // ---- 1 - 3
    const bool penal = a.penalty != 1.0f;
    if (penal) {
        for (int i = tid; i < AS_MAX_V / 32; i += AS_THREADS) seen[i] = 0u;
        __syncthreads();
        for (int i = tid; i < a.n; i += AS_THREADS) {
            const long long id = idb[i];
            if (id >= 0 && id < V) atomicOr(&seen[id >> 5], 1u << (id & 31));
        }
        __syncthreads();
    }
    float lv[AS_NV];
    unsigned key[AS_NV];
    unsigned kmax = 0u;
#pragma unroll
    for (int i = 0; i < AS_NV; ++i) {
        const int v = AS_THREADS * i + tid;
        float l = v < V ? lg[v] : -INFINITY;
        if (penal && v < V && ((seen[v >> 5] >> (v & 31)) & 1u)) l = l < 0.f ? l * a.penalty : l / a.penalty;
        if (v == a.eos) l = -INFINITY;
        l = l / a.temperature;
        lv[i] = l;
        key[i] = v < V ? as_key(l) : 0u;                   // beyond V: below every float
        kmax = key[i] > kmax ? key[i] : kmax;
    }

    // ---- 4. theta = the k-th largest key
    const int k = a.k < V ? a.k : V;
    unsigned th = 0u;
    for (int bit = 31; bit >= 0; --bit) {
        const unsigned c = th | (1u << bit);
        int cnt = 0;
#pragma unroll
        for (int i = 0; i < AS_NV; ++i) cnt += __popcll(__ballot(key[i] >= c));
        if (block_count(cnt) >= k) th = c;
    }
    // the workgroup's maximum: the waves' maxima through the count exchange (keys are integers)
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const unsigned other = (unsigned)__shfl_xor((int)kmax, o);
        kmax = other > kmax ? other : kmax;
    }
    if (lane == 0) icnt[par][w] = (int)kmax;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < AS_WAVES; ++i) kmax = (unsigned)icnt[par][i] > kmax ? (unsigned)icnt[par][i] : kmax;
    par ^= 1;
    float mval = 0.f;
    {
        const unsigned kb = (kmax & 0x80000000u) ? (kmax & 0x7fffffffu) : ~kmax;
        mval = __uint_as_float(kb);
    }

    // ---- 5. top-p over the kept
    float e[AS_NV];
    float part = 0.f;
#pragma unroll
    for (int i = 0; i < AS_NV; ++i) {
        const bool kept = AS_THREADS * i + tid < V && key[i] >= th;
        e[i] = kept ? expf(lv[i] - mval) : 0.f;
        part += e[i];
    }
    if (a.drop >= 0.f) {
        const float s1 = block_sum(part);
        float p1[AS_NV];
#pragma unroll
        for (int i = 0; i < AS_NV; ++i) p1[i] = e[i] / s1;
        unsigned cut = 0u;                                 // the largest key c with mass(key <= c) <= drop
        for (int bit = 31; bit >= 0; --bit) {
            const unsigned c = cut | (1u << bit);
            float ms = 0.f;
#pragma unroll
            for (int i = 0; i < AS_NV; ++i) ms += key[i] <= c ? p1[i] : 0.f;
            if (block_sum(ms) <= a.drop) cut = c;
        }
        part = 0.f;
#pragma unroll
        for (int i = 0; i < AS_NV; ++i) {
            if (key[i] <= cut && key[i] != kmax) e[i] = 0.f;
            part += e[i];
        }
    }

    // ---- 6. the draw
    const float s2 = block_sum(part);
    const float* __restrict__ qb = a.q + (size_t)b * (size_t)V;
    float br = -1.f;
    int bv = 0x7fffffff;
#pragma unroll
    for (int i = 0; i < AS_NV; ++i) {
        const int v = AS_THREADS * i + tid;
        if (e[i] > 0.f) {
            const float r = (e[i] / s2) / qb[v];
            if (r > br) { br = r; bv = v; }                // the thread's indices ascend
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const float orr = __shfl_xor(br, o);
        const int ov = __shfl_xor(bv, o);
        if (orr > br || (orr == br && ov < bv)) { br = orr; bv = ov; }
    }
    if (lane == 0) { bestr[w] = br; bestv[w] = bv; }
    __syncthreads();
    if (tid == 0) {
        for (int i = 1; i < AS_WAVES; ++i)
            if (bestr[i] > br || (bestr[i] == br && bestv[i] < bv)) { br = bestr[i]; bv = bestv[i]; }
        // nothing compared above -1 only with non-finite logits or noise: the id still stays in [0, V)
        idb[a.n] = (long long)(bv < V ? bv : V - 1);
    }
}

}  // namespace amp

using namespace amp;

extern "C" {

int amp_kv_append(const float* k_dev, const float* v_dev, long long batch_stride, const float* cos_dev, const float* sin_dev, int B, int H,
                  int dk, int T, int pos0, int Lmax, float* kcache_dev, float* vcache_dev, void* stream) {
    if (!k_dev || !v_dev || !cos_dev || !sin_dev || !kcache_dev || !vcache_dev) { set_error("amp_kv_append: null argument"); return AMP_ERR_INVALID; }
    if (dk != 64 && dk != 96) { set_error("amp_kv_append: head dimension %d is not covered (dk = 64 or 96)", dk); return AMP_ERR_INVALID; }
    if (B < 1 || H < 1 || T < 1 || (long long)B * H > 65535) { set_error("amp_kv_append: B=%d H=%d T=%d (B*H <= 65535)", B, H, T); return AMP_ERR_INVALID; }
    if (pos0 < 0 || Lmax < 1 || (long long)pos0 + T > Lmax) {
        set_error("amp_kv_append: columns [%d, %lld) do not fit a cache of %d", pos0, (long long)pos0 + T, Lmax);
        return AMP_ERR_INVALID;
    }
    if (batch_stride == 0) batch_stride = (long long)H * dk * T;
    if (batch_stride < (long long)H * dk * T) { set_error("amp_kv_append: batch stride %lld < H*dk*T", batch_stride); return AMP_ERR_INVALID; }
    const size_t span = ((size_t)(B - 1) * (size_t)batch_stride + (size_t)H * dk * T) * sizeof(float);
    const size_t cbytes = (size_t)B * H * dk * Lmax * sizeof(float);
    if (ranges_overlap(kcache_dev, cbytes, vcache_dev, cbytes) || ranges_overlap(kcache_dev, cbytes, k_dev, span) || ranges_overlap(kcache_dev, cbytes, v_dev, span) ||
        ranges_overlap(vcache_dev, cbytes, k_dev, span) || ranges_overlap(vcache_dev, cbytes, v_dev, span)) {
        set_error("amp_kv_append: the caches must not overlap each other or k / v");
        return AMP_ERR_INVALID;
    }
    KvAppendArgs a{};
    a.k = k_dev; a.v = v_dev; a.bstride = batch_stride;
    a.cs = cos_dev; a.sn = sin_dev;
    a.kc = kcache_dev; a.vc = vcache_dev;
    a.H = H; a.dk = dk; a.T = T; a.pos0 = pos0; a.Lmax = Lmax;
    a.n = (size_t)B * H * (dk / 2) * T;
    const size_t blocks = (a.n + 255) / 256;
    if (blocks > 0x7fffffffull) { set_error("amp_kv_append: B*H*dk*T is beyond the grid"); return AMP_ERR_UNSUPPORTED; }
    note_kernel("kv_append_kernel");
    note_work((unsigned long long)blocks, 0.0, 16.0 * (double)B * H * dk * T / 1e6, "kv append B=%d H=%d dk=%d T=%d pos0=%d", B, H, dk, T, pos0);
    hipLaunchKernelGGL(kv_append_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    AMP_HIP(hipGetLastError());
    return AMP_OK;
}

int amp_attention_decode_split(void) { return DEC_S; }

size_t amp_attention_decode_workspace_bytes(int B, int H, int dk, int Lmax) {
    if (B < 1 || H < 1 || dk < 1 || Lmax < 1) return 0;
    return (size_t)B * H * (size_t)((Lmax + DEC_S - 1) / DEC_S) * (size_t)(dk + 2) * sizeof(float);
}

int amp_attention_decode(const float* q_dev, long long q_batch_stride, const float* cos_dev, const float* sin_dev, const float* kcache_dev,
                         const float* vcache_dev, int B, int H, int dk, int L, int Lmax, float scale, float* out_dev, float* workspace_dev,
                         size_t workspace_bytes, void* stream) {
    if (!q_dev || !cos_dev || !sin_dev || !kcache_dev || !vcache_dev || !out_dev) { set_error("amp_attention_decode: null argument"); return AMP_ERR_INVALID; }
    if (dk != 64 && dk != 96) { set_error("amp_attention_decode: head dimension %d is not covered (dk = 64 or 96)", dk); return AMP_ERR_INVALID; }
    if (B < 1 || H < 1 || (long long)B * H > 65535) { set_error("amp_attention_decode: B=%d H=%d (B*H <= 65535)", B, H); return AMP_ERR_INVALID; }
    if (Lmax < 1 || L < 1 || L > Lmax) { set_error("amp_attention_decode: L=%d is outside [1, Lmax=%d]", L, Lmax); return AMP_ERR_INVALID; }
    if (!(scale > 0.f) || !(scale < 1e30f)) { set_error("amp_attention_decode: scale=%g", (double)scale); return AMP_ERR_INVALID; }
    if (q_batch_stride == 0) q_batch_stride = (long long)H * dk;
    if (q_batch_stride < (long long)H * dk) { set_error("amp_attention_decode: q batch stride %lld < H*dk", q_batch_stride); return AMP_ERR_INVALID; }
    const int nsplit = (L + DEC_S - 1) / DEC_S;
    const size_t need = nsplit > 1 ? (size_t)B * H * nsplit * (size_t)(dk + 2) * sizeof(float) : 0;
    if (need && (!workspace_dev || workspace_bytes < need)) {
        set_error("amp_attention_decode: workspace of %zu bytes, %zu needed (amp_attention_decode_workspace_bytes)", workspace_bytes, need);
        return AMP_ERR_INVALID;
    }
    const size_t qspan = ((size_t)(B - 1) * (size_t)q_batch_stride + (size_t)H * dk) * sizeof(float);
    const size_t obytes = (size_t)B * H * dk * sizeof(float), cbytes = (size_t)B * H * dk * Lmax * sizeof(float);
    if (ranges_overlap(out_dev, obytes, q_dev, qspan) || ranges_overlap(out_dev, obytes, kcache_dev, cbytes) || ranges_overlap(out_dev, obytes, vcache_dev, cbytes) ||
        ranges_overlap(workspace_dev, need, q_dev, qspan) || ranges_overlap(workspace_dev, need, kcache_dev, cbytes) ||
        ranges_overlap(workspace_dev, need, vcache_dev, cbytes) || ranges_overlap(workspace_dev, need, out_dev, obytes)) {
        set_error("amp_attention_decode: out and the workspace must not overlap q, the caches or each other");
        return AMP_ERR_INVALID;
    }
    DecodeArgs a{};
    a.q = q_dev; a.qbs = q_batch_stride;
    a.cs = cos_dev; a.sn = sin_dev;
    a.kc = kcache_dev; a.vc = vcache_dev;
    a.out = out_dev; a.ws = workspace_dev;
    a.H = H; a.dk = dk; a.L = L; a.Lmax = Lmax; a.nsplit = nsplit;
    a.scale = scale;
    note_kernel("attention_decode_kernel", dk);
    note_work((unsigned long long)nsplit * B * H, 4.0 * (double)B * H * dk * L / 1e9, 8.0 * (double)B * H * dk * L / 1e6,
              "attention decode B=%d H=%d dk=%d L=%d splits=%d", B, H, dk, L, nsplit);
    hipLaunchKernelGGL(dk == 64 ? attention_decode_kernel<64> : attention_decode_kernel<96>, dim3((unsigned)nsplit, (unsigned)(B * H)), dim3(DEC_S), 0,
                       (hipStream_t)stream, a);
    AMP_HIP(hipGetLastError());
    if (nsplit > 1) {
        note_kernel("decode_combine_kernel");
        note_work((unsigned long long)B * H, 0.0, 4.0 * (double)B * H * nsplit * (dk + 2) / 1e6, "attention decode combine splits=%d", nsplit);
        hipLaunchKernelGGL(decode_combine_kernel, dim3((unsigned)(B * H)), dim3(DEC_S), 0, (hipStream_t)stream, a);
        AMP_HIP(hipGetLastError());
    }
    return AMP_OK;
}

int amp_ar_sample(const float* logits_dev, long long batch_stride, int B, int V, const float* q_dev, long long* ids_dev, long long ids_capacity,
                  int n_ids, int eos_id, int suppress_eos, float temperature, int top_k, double top_p, float repetition_penalty, void* stream) {
    if (!logits_dev || !q_dev || !ids_dev) { set_error("amp_ar_sample: null argument"); return AMP_ERR_INVALID; }
    if (V < 2 || V > AS_MAX_V) { set_error("amp_ar_sample: V=%d is outside [2, %d]", V, AS_MAX_V); return AMP_ERR_INVALID; }
    if (B < 1 || B > 65535) { set_error("amp_ar_sample: B=%d is outside [1, 65535]", B); return AMP_ERR_INVALID; }
    if (top_k < 1) { set_error("amp_ar_sample: top_k=%d (>= 1; values beyond V keep every logit)", top_k); return AMP_ERR_INVALID; }
    if (!(top_p > 0.0)) { set_error("amp_ar_sample: top_p=%g (> 0; >= 1 disables the filter)", top_p); return AMP_ERR_INVALID; }
    if (!(temperature > 0.f) || !(temperature < 1e30f)) { set_error("amp_ar_sample: temperature=%g", (double)temperature); return AMP_ERR_INVALID; }
    if (!(repetition_penalty > 0.f) || !(repetition_penalty < 1e30f)) { set_error("amp_ar_sample: repetition_penalty=%g", (double)repetition_penalty); return AMP_ERR_INVALID; }
    if (n_ids < 0 || ids_capacity < 1 || (long long)n_ids >= ids_capacity) {
        set_error("amp_ar_sample: %d ids so far leave no slot in a buffer of %lld", n_ids, ids_capacity);
        return AMP_ERR_INVALID;
    }
    if (suppress_eos && (eos_id < 0 || eos_id >= V)) { set_error("amp_ar_sample: eos_id=%d is outside [0, V=%d)", eos_id, V); return AMP_ERR_INVALID; }
    if (batch_stride == 0) batch_stride = V;
    if (batch_stride < V) { set_error("amp_ar_sample: batch stride %lld < V", batch_stride); return AMP_ERR_INVALID; }
    const size_t lbytes = ((size_t)(B - 1) * (size_t)batch_stride + (size_t)V) * sizeof(float), qbytes = (size_t)B * V * sizeof(float);
    const size_t ibytes = (size_t)B * (size_t)ids_capacity * sizeof(long long);
    if (ranges_overlap(ids_dev, ibytes, logits_dev, lbytes) || ranges_overlap(ids_dev, ibytes, q_dev, qbytes)) {
        set_error("amp_ar_sample: ids must not overlap logits / q");
        return AMP_ERR_INVALID;
    }
    ArSampleArgs a{};
    a.logits = logits_dev; a.bstride = batch_stride; a.q = q_dev;
    a.ids = ids_dev; a.cap = ids_capacity;
    a.V = V; a.n = n_ids; a.k = top_k; a.eos = suppress_eos ? eos_id : -1;
    a.temperature = temperature; a.penalty = repetition_penalty;
    a.drop = top_p >= 1.0 ? -1.f : (float)(1.0 - top_p);
    note_kernel("ar_sample_kernel");
    note_work((unsigned long long)B, 0.0, (8.0 * (double)B * V + 8.0 * (double)B * n_ids) / 1e6, "ar sample V=%d k=%d top_p=%g n=%d B=%d", V, top_k, top_p, n_ids, B);
    hipLaunchKernelGGL(ar_sample_kernel, dim3((unsigned)B), dim3(AS_THREADS), 0, (hipStream_t)stream, a);
    AMP_HIP(hipGetLastError());
    return AMP_OK;
}

}  // extern "C"
