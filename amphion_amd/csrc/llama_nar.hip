// The kernels of the non-autoregressive Llama of Vevo / MaskGCT (models/vc/flow_matching_transformer/llama_nar.py: DiffLlama), the parts
// the pointwise GEMM (pw_f16x3.hip) does not cover:
//     amp_rope_attention        non-causal multi-head self-attention with rotary position embedding and a key mask, one launch
//     amp_rope_attention_causal the same kernel with its compile-time causal flag: the prefill of the autoregressive transformer (llama_ar.hip)
//     amp_mh_attention          the same kernel with its compile-time rotation flag off, head dimension 128: the FFT block of FastSpeech2 / JETS
//     amp_cross_attention       the same, head dimension 64, with query and key extents and batch strides apart: every attention of NaturalSpeech2
//     amp_cross_attention_hd    the same at head dimension 32 (a new instantiation), 64 or 128 (amp_mh_attention's): AudioLDM's spatial transformer
//     amp_prefix_attention      causal without rotation, head dimension 64, with a run-time prefix every query sees: the prefill of VALL-E's AR stage
//     amp_rms_norm_c_adaptive   LlamaAdaptiveRMSNorm (llama_nar.py:32-50) over the channel axis, one weight row per item
//     amp_silu / amp_swiglu     nn.SiLU and LlamaMLP's silu(gate) * up on the stacked gate | up GEMM output
// Everything is channel-first [B, C, T] fp32.  Deterministic: no atomics on data (the attention kernel ORs the op-level range flag).
//
// ---- amp_rope_attention ---------------------------------------------------------------------------------------------------------
// A workgroup of four waves owns 128 queries of one (item, head); a wave owns 32 of them and walks the keys in tiles of 64 with the
// online softmax.  Channel-first suits the TRANSPOSED products (f16x3_device.h for the MFMA layouts):
//     S^T [tk, tq] = K'^T Q'      A = K'^T (row = key, k = channel), B = Q' (k = channel, column = query)
//     O   [d,  tq] = V  P^T       A = V    (row = channel, k = key), B = P^T (k = key, column = query)
// so a lane owns ONE query column in both accumulators: the running maximum, the running sum and the rescale are per-lane scalars
// (the two lanes l and l ^ 32 share a query and hold 16 of every 32 keys each: one cross-lane maximum per tile, one sum at the end).
// The S^T accumulator is the next product's B operand as it stands: registers 8c' .. 8c' + 7 of row block rb are the eight k-slots of
// key chunk c = 2 rb + c', which fixes the order in which V's A fragment takes its keys -- key(hi, j) = 16 c + 8 (j >> 2) + 4 hi + (j & 3),
// two 8-byte reads of V's [channel][key] image.  No P ever goes through LDS.
// Q' = RoPE(q) is split once per wave into registers (a lane loads the channels of its own fragment and their rotate-half partners);
// K' = RoPE(k) and V go global -> registers -> LDS as hi / lo f16 planes, the loads of tile i + 1 issued before the products of tile i.
// Operands are staged after an exact x16 like every f16x3 kernel (|q'|, |k'|, |v| <= 4094, range flag beyond); P in [0, 1] after an
// exact x1024.  A masked key (or one beyond T) is staged as ZERO in K' and V and its score is -inf, so it contributes exactly 0 whatever
// finite value its columns hold.
#include <hip/hip_runtime.h>

#include "amp_host.h"
#include "amphion_hip.h"
#include "f16x3_device.h"

namespace amp {

constexpr int AT_NW = 4;              // waves per workgroup
constexpr int AT_TQ = 32 * AT_NW;     // queries per workgroup
constexpr int AT_TK = 64;             // keys per tile
constexpr int AT_VS = AT_TK + 4;      // V image row stride in f16: 34 dwords, the 32 rows of a fragment read fall on distinct bank pairs
constexpr int AT_MAX_T = 32768;

struct AttnArgs {
    const float* q;
    const float* k;
    const float* v;
    long long qbstride;            // elements between items of q
    long long kvbstride;           // elements between items of k / v (self-attention: both are the stride of the stacked q | k | v tensor)
    const float* cs;               // [T, DK / 2]: rotation only, where Tq == Tk
    const float* sn;
    const unsigned char* mask;     // [B, Tk] or nullptr
    float* out;                    // [B, H * DK, Tq]
    int H, Tq, Tk;                 // queries (rows of q and out are Tq apart) and keys (rows of k and v are Tk apart); equal except for amp_cross_attention
    float c;                       // scale / 256: un-does the two x16 of the staged operands (a power of two at DK = 64 only: one rounding at 96)
    unsigned* range_flag;
    int prefix;                    // CAUSAL && !ROPE only (amp_prefix_attention): keys [0, prefix) are visible to every query
};

// DK = 64 or 96 (with rotation), 32 or 128 (without).  HALF = DK / 2 is the rotate-half distance (16 NP channels: Q' fragment s pairs with s + NP), NF = DK / 16 the k-steps of
// S, ND = DK / 32 the row blocks of O, HO = DK / 16 the channel octets per half: wave w stages octets w, w + 4, ... < HO with their partners
// (at DK = 96 waves 0 and 1 take two octet pairs, waves 2 and 3 one).
// CAUSAL (amp_rope_attention_causal): key j is visible to query i iff j <= i (and the key mask admits it).  The workgroup walks the key
// tiles up to the one that holds its last query; in a tile that reaches beyond the wave's first query the comparison joins the validity
// select below.  A key beyond the query is staged like any other and meets p = exp2(-inf) = 0: it contributes exactly 0.
// CAUSAL && !ROPE (amp_prefix_attention, DK = 64) is the prefix-LM rule: key j is visible to query i iff j < a.prefix || j <= i.  The workgroup
// walks up to the tile of max(its last query, prefix - 1) and the prefix joins the same comparison; prefix = 0 is the causal rule, prefix = T full attention.
// ROPE = false (amp_mh_attention, fastspeech.hip's FFT block): no rotation -- Q' = q and K' = k, cs / sn are never read; the channel pairs
// (i, i + HALF) stay the staging pattern, nothing more.  DK = 128 is built in this form only: its planes (32 KB of K', 34 KB of V) are
// beyond what a static __shared__ array may hold, so they are the launch's dynamic LDS (attn_lds_bytes); DK <= 96 keeps the static arrays.
template <int DK>
constexpr size_t attn_lds_bytes() { return 2 * (size_t)(DK / 8) * AT_TK * sizeof(uint4) + 2 * (size_t)DK * AT_VS * sizeof(_Float16); }

template <int DK, bool CAUSAL, bool ROPE = true>
__global__ __launch_bounds__(64 * AT_NW) void rope_attention_kernel(AttnArgs a) {
    constexpr int AT_DK = DK, HALF = DK / 2, NP = DK / 32, NF = DK / 16, ND = DK / 32, HO = DK / 16, NKO = (HO + AT_NW - 1) / AT_NW;
    constexpr int KPL = (DK / 8) * AT_TK, VPL = AT_DK * AT_VS;
    static_assert(DK % 32 == 0 && DK <= 128, "head dimension");
    uint4 (*kpl)[KPL];                                                        // [plane][channel octet][key] x 8 f16
    _Float16 (*vpl)[VPL];                                                     // [plane][channel][key]
    if constexpr (DK <= 96) {
        __shared__ uint4 kpl_s[2][KPL];
        __shared__ __attribute__((aligned(16))) _Float16 vpl_s[2][VPL];
        kpl = kpl_s; vpl = vpl_s;
    } else {
        extern __shared__ uint4 attn_dyn[];
        kpl = reinterpret_cast<uint4 (*)[KPL]>(attn_dyn);
        vpl = reinterpret_cast<_Float16 (*)[VPL]>(attn_dyn + 2 * KPL);
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, l31 = lane & 31, hi = lane >> 5;
    const int b = blockIdx.y / a.H, h = blockIdx.y - b * a.H;
    const int Tq = a.Tq, T = a.Tk;
    const size_t khead = (size_t)b * (size_t)a.kvbstride + (size_t)h * AT_DK * T;
    const float* __restrict__ qb = a.q + (size_t)b * (size_t)a.qbstride + (size_t)h * AT_DK * Tq;
    const float* __restrict__ kb = a.k + khead;
    const float* __restrict__ vb = a.v + khead;
    const unsigned char* __restrict__ mk = a.mask ? a.mask + (size_t)b * T : nullptr;
    float range_max = 0.f;

    // ---- Q' fragments: lane (l31, hi) holds channels 16 s + 8 hi + j of query l31; channel i < HALF and its partner i + HALF are s and s + NP
    const int tq = blockIdx.x * AT_TQ + 32 * w + l31;
    const int tqc = tq < Tq ? tq : Tq - 1;
    Frag qh[NF], ql[NF];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int i = 16 * p + 8 * hi + j;
            const float x1 = qb[(size_t)i * Tq + tqc], x2 = qb[(size_t)(i + HALF) * Tq + tqc];
            float r1, r2;
            if constexpr (ROPE) {
                const float c = a.cs[(size_t)tqc * HALF + i], s = a.sn[(size_t)tqc * HALF + i];
                r1 = (x1 * c - x2 * s) * 16.f; r2 = (x2 * c + x1 * s) * 16.f;
            } else {
                r1 = x1 * 16.f; r2 = x2 * 16.f;
            }
            range_max = __builtin_fmaxf(range_max, __builtin_fmaxf(__builtin_fabsf(r1), __builtin_fabsf(r2)));
            _Float16 hh, ll;
            split_f16(r1, hh, ll);
            qh[p].h[j] = hh; ql[p].h[j] = ll;
            split_f16(r2, hh, ll);
            qh[p + NP].h[j] = hh; ql[p + NP].h[j] = ll;
        }
    }

    // ---- the staged tile: thread (key = lane, wave w) takes K channels 8 o .. 8 o + 7 of its octets o = w + 4 n with their partners (two
    // whole octets after the rotation) and V channels w, w + 4, ...
    float kr[NKO][16], vr[DK / 4];
    float4 cr[NKO][2], sr[NKO][2];
    bool valid;
    // octet w + 4 n exists: known at compile time where every wave has one
    auto has_octet = [&](int n) { return 4 * n + AT_NW - 1 < HO || 4 * n + w < HO; };
    auto load_tile = [&](int tk0) {
        const int tk = tk0 + lane;
        const int tkc = tk < T ? tk : T - 1;
        valid = tk < T && (!mk || mk[tkc] != 0);
#pragma unroll
        for (int n = 0; n < NKO; ++n) {
            if (!has_octet(n)) continue;
            const int o = w + 4 * n;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                kr[n][j] = kb[(size_t)(8 * o + j) * T + tkc];
                kr[n][8 + j] = kb[(size_t)(8 * o + j + HALF) * T + tkc];
            }
            if constexpr (ROPE) {
                const float4* cp = reinterpret_cast<const float4*>(a.cs + (size_t)tkc * HALF + 8 * o);
                const float4* sp = reinterpret_cast<const float4*>(a.sn + (size_t)tkc * HALF + 8 * o);
                cr[n][0] = cp[0]; cr[n][1] = cp[1];
                sr[n][0] = sp[0]; sr[n][1] = sp[1];
            }
        }
#pragma unroll
        for (int i = 0; i < DK / 4; ++i) vr[i] = vb[(size_t)(w + 4 * i) * T + tkc];
    };

    f32x16 O[ND][1];
#pragma unroll
    for (int db = 0; db < ND; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) O[db][0][r] = 0.f;
    float m = -INFINITY, l = 0.f;
    constexpr float LOG2E = 1.4426950408889634f;

    int nkt = (T + AT_TK - 1) / AT_TK;
    if (CAUSAL) {                                          // uniform over the workgroup: the tile of its last query
        int qlast = (int)blockIdx.x * AT_TQ + AT_TQ - 1;
        if constexpr (!ROPE) qlast = qlast > a.prefix - 1 ? qlast : a.prefix - 1;
        nkt = (qlast < T ? qlast : T - 1) / AT_TK + 1;
    }
    const int qw0 = (int)blockIdx.x * AT_TQ + 32 * w;      // the wave's first query
    load_tile(0);
    for (int kt = 0; kt < nkt; ++kt) {
        __syncthreads();                                   // every wave is done reading the previous tile
#pragma unroll
        for (int n = 0; n < NKO; ++n) {
            if (!has_octet(n)) continue;
            const int o = w + 4 * n;
            float cc[8], ss[8];
            if constexpr (ROPE) {
                const float c8[8] = {cr[n][0].x, cr[n][0].y, cr[n][0].z, cr[n][0].w, cr[n][1].x, cr[n][1].y, cr[n][1].z, cr[n][1].w};
                const float s8[8] = {sr[n][0].x, sr[n][0].y, sr[n][0].z, sr[n][0].w, sr[n][1].x, sr[n][1].y, sr[n][1].z, sr[n][1].w};
#pragma unroll
                for (int j = 0; j < 8; ++j) { cc[j] = c8[j]; ss[j] = s8[j]; }
            }
            float r1[8], r2[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float u1, u2;
                if constexpr (ROPE) {
                    u1 = (kr[n][j] * cc[j] - kr[n][8 + j] * ss[j]) * 16.f; u2 = (kr[n][8 + j] * cc[j] + kr[n][j] * ss[j]) * 16.f;
                } else {
                    u1 = kr[n][j] * 16.f; u2 = kr[n][8 + j] * 16.f;
                }
                r1[j] = valid ? u1 : 0.f;
                r2[j] = valid ? u2 : 0.f;
                range_max = __builtin_fmaxf(range_max, __builtin_fmaxf(__builtin_fabsf(r1[j]), __builtin_fabsf(r2[j])));
            }
            uint2 h0, l0, h1, l1;
            split4_f16(amp_f32x2{r1[0], r1[1]}, amp_f32x2{r1[2], r1[3]}, h0, l0);
            split4_f16(amp_f32x2{r1[4], r1[5]}, amp_f32x2{r1[6], r1[7]}, h1, l1);
            kpl[0][o * AT_TK + lane] = make_uint4(h0.x, h0.y, h1.x, h1.y);
            kpl[1][o * AT_TK + lane] = make_uint4(l0.x, l0.y, l1.x, l1.y);
            split4_f16(amp_f32x2{r2[0], r2[1]}, amp_f32x2{r2[2], r2[3]}, h0, l0);
            split4_f16(amp_f32x2{r2[4], r2[5]}, amp_f32x2{r2[6], r2[7]}, h1, l1);
            kpl[0][(o + HO) * AT_TK + lane] = make_uint4(h0.x, h0.y, h1.x, h1.y);
            kpl[1][(o + HO) * AT_TK + lane] = make_uint4(l0.x, l0.y, l1.x, l1.y);
        }
        {
#pragma unroll
            for (int i = 0; i < DK / 4; ++i) {
                const float u = valid ? vr[i] * 16.f : 0.f;
                range_max = __builtin_fmaxf(range_max, __builtin_fabsf(u));
                _Float16 hh, ll;
                split_f16(u, hh, ll);
                vpl[0][(w + 4 * i) * AT_VS + lane] = hh;
                vpl[1][(w + 4 * i) * AT_VS + lane] = ll;
            }
        }
        const unsigned long long km = __ballot(valid);     // the tile's valid keys: lane = key in every wave
        __syncthreads();
        if (kt + 1 < nkt) load_tile((kt + 1) * AT_TK);     // in flight behind the products below

        // ---- S^T = K'^T Q' over the DK channels
        f32x16 S[2][1];
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int r = 0; r < 16; ++r) S[rb][0][r] = 0.f;
#pragma unroll
        for (int s = 0; s < NF; ++s) {
            Frag ah[2], al[2];
#pragma unroll
            for (int rb = 0; rb < 2; ++rb) {
                ah[rb].u = kpl[0][(2 * s + hi) * AT_TK + 32 * rb + l31];
                al[rb].u = kpl[1][(2 * s + hi) * AT_TK + 32 * rb + l31];
            }
            mfma3_tiles<2, 1>(S, ah, al, &qh[s], &ql[s]);
        }

        // ---- online softmax of the lane's query column (its 32 of the tile's 64 keys)
        float sv[2][16];
        float mx = -INFINITY;
        const bool all_valid = km == ~0ull;
        const bool diag = CAUSAL && kt * AT_TK + AT_TK - 1 > qw0;      // uniform over the wave: some key of the tile is beyond some query
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) {
            const unsigned mw = (unsigned)(km >> (32 * rb)) >> (4 * hi);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float s = S[rb][0][r] * a.c;
                if (!all_valid) s = ((mw >> acc_row(r)) & 1u) ? s : -INFINITY;
                if (CAUSAL) {
                    if constexpr (ROPE) {
                        if (diag) s = acc_row(r, hi, kt * AT_TK + 32 * rb) <= tq ? s : -INFINITY;
                    } else {
                        const int key = acc_row(r, hi, kt * AT_TK + 32 * rb);
                        if (diag) s = (key <= tq || key < a.prefix) ? s : -INFINITY;
                    }
                }
                sv[rb][r] = s;
                mx = __builtin_fmaxf(mx, s);
            }
        }
        mx = __builtin_fmaxf(mx, __shfl_xor(mx, 32));
        const float m_new = __builtin_fmaxf(m, mx);
        const float m_use = m_new == -INFINITY ? 0.f : m_new;          // no valid key so far: every p below is exp2(-inf) = 0
        if (!__all(m_new == m)) {                                      // the running maximum moved: rescale what is accumulated
            const float alpha = __builtin_amdgcn_exp2f((m - m_use) * LOG2E);
            l *= alpha;
#pragma unroll
            for (int db = 0; db < ND; ++db)
#pragma unroll
                for (int r = 0; r < 16; ++r) O[db][0][r] *= alpha;
            m = m_new;
        }
        Frag ph[4], pl[4];
        float psum = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float p = __builtin_amdgcn_exp2f((sv[c >> 1][8 * (c & 1) + j] - m_use) * LOG2E);
                psum += p;
                _Float16 hh, ll;
                split_f16(p * 1024.f, hh, ll);
                ph[c].h[j] = hh; pl[c].h[j] = ll;
            }
        }
        l += psum;

        // ---- O += V P^T: chunk c's k-slot (hi, j) is key 16 c + 8 (j >> 2) + 4 hi + (j & 3)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            Frag vh[ND], vl[ND];
#pragma unroll
            for (int db = 0; db < ND; ++db) {
                const int off = (32 * db + l31) * AT_VS + 16 * c + 4 * hi;
                const uint2 x0 = *reinterpret_cast<const uint2*>(&vpl[0][off]), x1 = *reinterpret_cast<const uint2*>(&vpl[0][off + 8]);
                const uint2 y0 = *reinterpret_cast<const uint2*>(&vpl[1][off]), y1 = *reinterpret_cast<const uint2*>(&vpl[1][off + 8]);
                vh[db].u = make_uint4(x0.x, x0.y, x1.x, x1.y);
                vl[db].u = make_uint4(y0.x, y0.y, y1.x, y1.y);
            }
            mfma3_tiles<ND, 1>(O, vh, vl, &ph[c], &pl[c]);
        }
    }

    const float lt = l + __shfl_xor(l, 32);
    const float inv = (1.0f / lt) * (1.0f / 16384.f);      // x16 of V, x1024 of P
    if (tq < Tq) {
        float* ob = a.out + ((size_t)blockIdx.y * AT_DK) * Tq + tq;
#pragma unroll
        for (int db = 0; db < ND; ++db)
#pragma unroll
            for (int r = 0; r < 16; ++r) ob[(size_t)acc_row(r, hi, 32 * db) * Tq] = O[db][0][r] * inv;
    }
    raise_range(a.range_flag, range_max, lane);
}

// ---- amp_rms_norm_c_adaptive: y[b, c, t] = w[b, c] * (x[b, c, t] * rsqrt(mean_c x[b, :, t]^2 + eps)) ------------------------------
// amp_layer_norm_c_style's workgroup: 32 time columns x 8 channel groups, thread (tx, g) holds channels g, g + 8, ... of column tx in
// registers (NC of them; more are re-read), rows are read as 128-B segments, the reduction over C goes through LDS in a fixed order.
constexpr int RN_TT = 32, RN_G = 8;
template <int NC>
__global__ __launch_bounds__(256) void rms_norm_c_adaptive_kernel(const float* __restrict__ x, const float* __restrict__ w, long long wbs,
                                                                  float* __restrict__ y, int C, int T, float eps) {
    __shared__ float red[RN_G][RN_TT + 1];
    const int tx = threadIdx.x & (RN_TT - 1), g = threadIdx.x / RN_TT;
    const int t = blockIdx.x * RN_TT + tx;
    const int b = blockIdx.y;
    const bool ok = t < T;
    const size_t base = (size_t)b * C * T + (ok ? t : 0);
    const float* xb = x + base;
    const float* wb = w + (size_t)b * (size_t)wbs;
    float v[NC];
    float part = 0.f;
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        const int c = g + RN_G * i;
        v[i] = xb[(size_t)(c < C ? c : C - 1) * T];
    }
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        v[i] = (ok && g + RN_G * i < C) ? v[i] : 0.f;
        part = fmaf(v[i], v[i], part);
    }
    for (int c = g + RN_G * NC; c < C; c += RN_G) {
        const float u = ok ? xb[(size_t)c * T] : 0.f;
        part = fmaf(u, u, part);
    }
    red[g][tx] = part;
    __syncthreads();
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < RN_G; ++k) s += red[k][tx];
    const float rs = 1.0f / sqrtf(s / (float)C + eps);
    if (!ok) return;
    float* yb = y + base;
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        const int c = g + RN_G * i;
        if (c < C) yb[(size_t)c * T] = wb[c] * (v[i] * rs);
    }
    for (int c = g + RN_G * NC; c < C; c += RN_G) yb[(size_t)c * T] = wb[c] * (xb[(size_t)c * T] * rs);
}

// ---- amp_silu / amp_swiglu ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float silu_f(float v) { return v / (1.0f + expf(-v)); }

// element-wise, amp_gelu's shape: vec = both bases 16-byte aligned -- threads [0, n / 4) take quads, the next n % 4 threads the tail
__global__ __launch_bounds__(256) void silu_kernel(const float* x, float* y, size_t n, int vec) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (vec) {
        const size_t nq = n >> 2;
        if (i < nq) {
            const float4 t = reinterpret_cast<const float4*>(x)[i];
            reinterpret_cast<float4*>(y)[i] = make_float4(silu_f(t.x), silu_f(t.y), silu_f(t.z), silu_f(t.w));
        } else {
            const size_t k = 4 * nq + (i - nq);
            if (k < n) y[k] = silu_f(x[k]);
        }
    } else if (i < n) {
        y[i] = silu_f(x[i]);
    }
}

// gu [B, 2F, T]: item blockIdx.y, n = F * T elements of gate followed by n of up.  vec: n % 4 == 0 and both bases 16-byte aligned.
__global__ __launch_bounds__(256) void swiglu_kernel(const float* __restrict__ gu, float* __restrict__ y, size_t n, int vec) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const float* g = gu + (size_t)blockIdx.y * 2 * n;
    const float* u = g + n;
    float* yb = y + (size_t)blockIdx.y * n;
    if (vec) {
        if (i < (n >> 2)) {
            const float4 a = reinterpret_cast<const float4*>(g)[i], c = reinterpret_cast<const float4*>(u)[i];
            reinterpret_cast<float4*>(yb)[i] = make_float4(silu_f(a.x) * c.x, silu_f(a.y) * c.y, silu_f(a.z) * c.z, silu_f(a.w) * c.w);
        }
    } else if (i < n) {
        yb[i] = silu_f(g[i]) * u[i];
    }
}

// ---- amp_cross_attention at Tk = 1: out[b, c, tq] = v[b, c, 0] for every query (the softmax over one key is exactly 1) -------------------
__global__ __launch_bounds__(256) void attn_one_key_kernel(const float* __restrict__ v, long long vbs, float* __restrict__ out, int C, int Tq) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < Tq) out[((size_t)blockIdx.z * C + blockIdx.y) * Tq + t] = v[(size_t)blockIdx.z * (size_t)vbs + blockIdx.y];
}

}  // namespace amp

using namespace amp;

// the six attention entries: `who` names the entry in the messages, `causal` and `rope` pick the instantiation (rope = false: amp_mh_attention at
// dk = 128, with `cross` = 1 amp_cross_attention at dk = 64, with `cross` = 2 amp_cross_attention_hd at dk = 32, 64 or 128, with `causal` amp_prefix_attention at
// dk = 64 and its `prefix`; cos / sin unused).  Tq != Tk and q_stride != kv_stride come from the two cross entries only.
static int rope_attention_run(const char* who, bool causal, bool rope, int cross, const float* q_dev, long long q_stride, const float* k_dev, const float* v_dev,
                              long long kv_stride, const float* cos_dev, const float* sin_dev, const unsigned char* key_mask_dev, int B, int H, int dk,
                              int Tq, int T, float scale, float* out_dev, void* stream, int prefix = 0) {
    const bool pfx = causal && !rope;
    if (!q_dev || !k_dev || !v_dev || (rope && (!cos_dev || !sin_dev)) || !out_dev) { set_error("%s: null argument", who); return AMP_ERR_INVALID; }
    if (rope && dk != 64 && dk != 96) { set_error("%s: head dimension %d is not covered (dk = 64 or 96)", who, dk); return AMP_ERR_INVALID; }
    if (pfx && dk != 64) { set_error("%s: head dimension %d is not covered (dk = 64)", who, dk); return AMP_ERR_INVALID; }
    if (!rope && !cross && !pfx && dk != 128) { set_error("%s: head dimension %d is not covered (dk = 128)", who, dk); return AMP_ERR_INVALID; }
    if (cross == 1 && dk != 64) { set_error("%s: head dimension %d is not covered (dk = 64)", who, dk); return AMP_ERR_INVALID; }
    if (cross == 2 && dk != 32 && dk != 64 && dk != 128) { set_error("%s: head dimension %d is not covered (dk = 32, 64 or 128)", who, dk); return AMP_ERR_INVALID; }
    if (cross) {
        if (B < 1 || H < 1 || Tq < 1 || T < 1) { set_error("%s: B=%d H=%d Tq=%d Tk=%d", who, B, H, Tq, T); return AMP_ERR_INVALID; }
        if (Tq > AT_MAX_T || T > AT_MAX_T) { set_error("%s: Tq=%d / Tk=%d is beyond %d", who, Tq, T, AT_MAX_T); return AMP_ERR_INVALID; }
    } else {
        if (B < 1 || H < 1 || T < 1) { set_error("%s: B=%d H=%d T=%d", who, B, H, T); return AMP_ERR_INVALID; }
        if (T > AT_MAX_T) { set_error("%s: T=%d is beyond %d", who, T, AT_MAX_T); return AMP_ERR_INVALID; }
    }
    if (pfx && (prefix < 0 || prefix > T)) { set_error("%s: prefix=%d is outside [0, T=%d]", who, prefix, T); return AMP_ERR_INVALID; }
    if ((long long)B * H > 65535) { set_error("%s: B*H=%lld is beyond the grid (65535)", who, (long long)B * H); return AMP_ERR_INVALID; }
    if (!(scale > 0.f) || !(scale < 1e30f)) { set_error("%s: scale=%g", who, (double)scale); return AMP_ERR_INVALID; }
    if (kv_stride == 0) kv_stride = (long long)H * dk * T;
    if (q_stride == 0) q_stride = (long long)H * dk * Tq;
    if (kv_stride < (long long)H * dk * T) { set_error("%s: batch stride %lld < H*dk*T", who, kv_stride); return AMP_ERR_INVALID; }
    if (q_stride < (long long)H * dk * Tq) { set_error("%s: q batch stride %lld < H*dk*Tq", who, q_stride); return AMP_ERR_INVALID; }
    if (rope && ((reinterpret_cast<uintptr_t>(cos_dev) | reinterpret_cast<uintptr_t>(sin_dev)) & 15)) {
        set_error("%s: cos / sin must be 16-byte aligned", who);
        return AMP_ERR_INVALID;
    }
    const size_t qspan = (size_t)(B - 1) * (size_t)q_stride + (size_t)H * dk * Tq;
    const size_t kspan = (size_t)(B - 1) * (size_t)kv_stride + (size_t)H * dk * T;
    const float* olo = out_dev;
    const float* ohi = out_dev + (size_t)B * H * dk * Tq;
    if ((q_dev < ohi && olo < q_dev + qspan) || (k_dev < ohi && olo < k_dev + kspan) || (v_dev < ohi && olo < v_dev + kspan)) {
        set_error("%s: out must not overlap q / k / v", who);
        return AMP_ERR_INVALID;
    }
    if (T == 1 && Tq == 1) {
        // One key (query 0 sees key 0 under the causal rule too): the softmax over it is exactly 1 whatever q and k hold (the item's one key
        // is valid, see the header), so the attention is the identity on v and there is no product to form.  A strided copy returns v's bits, as the fp32 reference does (1.0f * v),
        // where the split-f16 operand of the kernel would return 22 of its 24 mantissa bits.
        AMP_HIP(hipMemcpy2DAsync(out_dev, (size_t)H * dk * sizeof(float), v_dev, (size_t)kv_stride * sizeof(float),
                                 (size_t)H * dk * sizeof(float), (size_t)B, hipMemcpyDeviceToDevice, (hipStream_t)stream));
        return AMP_OK;
    }
    if (T == 1) {
        // amp_cross_attention with one key and several queries: the same identity, v's column written to every query column
        const dim3 grid((unsigned)((Tq + 255) / 256), (unsigned)(H * dk), (unsigned)B);
        if (grid.y > 65535 || grid.z > 65535) { set_error("%s: H*dk=%d or B=%d is beyond the grid (65535)", who, H * dk, B); return AMP_ERR_INVALID; }
        note_kernel("attn_one_key_kernel");
        note_work((unsigned long long)grid.x * grid.y * grid.z, 0.0, 4.0 * (double)B * H * dk * Tq / 1e6, "cross attention Tk=1 B=%d H=%d dk=%d Tq=%d", B, H, dk, Tq);
        hipLaunchKernelGGL(attn_one_key_kernel, grid, dim3(256), 0, (hipStream_t)stream, v_dev, kv_stride, out_dev, H * dk, Tq);
        AMP_HIP(hipGetLastError());
        return AMP_OK;
    }
    AttnArgs a{};
    a.q = q_dev; a.k = k_dev; a.v = v_dev;
    a.qbstride = q_stride; a.kvbstride = kv_stride;
    a.cs = cos_dev; a.sn = sin_dev;
    a.mask = key_mask_dev;
    a.out = out_dev;
    a.H = H; a.Tq = Tq; a.Tk = T;
    a.c = scale * (1.0f / 256.f);
    a.range_flag = range_flag_for_current_device();
    a.prefix = prefix;
    const dim3 grid((unsigned)((Tq + AT_TQ - 1) / AT_TQ), (unsigned)(B * H));
    if (rope) note_kernel("rope_attention_kernel", dk, causal ? 1 : 0);
    else note_kernel("rope_attention_kernel", dk, pfx ? 1 : 0, 0);
    if (pfx) {
        note_work((unsigned long long)grid.x * grid.y, 4.0 * 3.0 * (double)B * H * dk * ((double)T * prefix + 0.5 * (double)(T - prefix) * (T - prefix)) / 1e9,
                  16.0 * (double)B * H * dk * T / 1e6, "prefix attention B=%d H=%d dk=%d T=%d prefix=%d mask=%d", B, H, dk, T, prefix, key_mask_dev ? 1 : 0);
        hipLaunchKernelGGL((rope_attention_kernel<64, true, false>), grid, dim3(64 * AT_NW), 0, (hipStream_t)stream, a);
        AMP_HIP(hipGetLastError());
        return AMP_OK;
    }
    if (cross) {
        note_work((unsigned long long)grid.x * grid.y, 4.0 * 3.0 * (double)B * H * dk * (double)Tq * T / 1e9, 8.0 * (double)B * H * dk * ((double)Tq + T) / 1e6,
                  "cross attention B=%d H=%d dk=%d Tq=%d Tk=%d mask=%d", B, H, dk, Tq, T, key_mask_dev ? 1 : 0);
        if (dk == 128) {                                   // amp_mh_attention's instantiation and LDS plan, with the extents apart
            constexpr size_t lds = attn_lds_bytes<128>();
            AMP_HIP((ensure_dynamic_lds<rope_attention_kernel<128, false, false>>(lds)));
            hipLaunchKernelGGL((rope_attention_kernel<128, false, false>), grid, dim3(64 * AT_NW), lds, (hipStream_t)stream, a);
        } else if (dk == 32) {
            hipLaunchKernelGGL((rope_attention_kernel<32, false, false>), grid, dim3(64 * AT_NW), 0, (hipStream_t)stream, a);
        } else {
            hipLaunchKernelGGL((rope_attention_kernel<64, false, false>), grid, dim3(64 * AT_NW), 0, (hipStream_t)stream, a);
        }
        AMP_HIP(hipGetLastError());
        return AMP_OK;
    }
    note_work((unsigned long long)grid.x * grid.y, (causal ? 0.5 : 1.0) * 4.0 * 3.0 * (double)B * H * dk * (double)T * T / 1e9, 16.0 * (double)B * H * dk * T / 1e6,
              "rope attention%s B=%d H=%d dk=%d T=%d mask=%d", causal ? " causal" : "", B, H, dk, T, key_mask_dev ? 1 : 0);
    if (!rope) {
        constexpr size_t lds = attn_lds_bytes<128>();
        AMP_HIP((ensure_dynamic_lds<rope_attention_kernel<128, false, false>>(lds)));
        hipLaunchKernelGGL((rope_attention_kernel<128, false, false>), grid, dim3(64 * AT_NW), lds, (hipStream_t)stream, a);
        AMP_HIP(hipGetLastError());
        return AMP_OK;
    }
    auto kern = dk == 64 ? (causal ? rope_attention_kernel<64, true> : rope_attention_kernel<64, false>)
                         : (causal ? rope_attention_kernel<96, true> : rope_attention_kernel<96, false>);
    hipLaunchKernelGGL(kern, grid, dim3(64 * AT_NW), 0, (hipStream_t)stream, a);
    AMP_HIP(hipGetLastError());
    return AMP_OK;
}

extern "C" {

int amp_rope_attention(const float* q_dev, const float* k_dev, const float* v_dev, long long batch_stride, const float* cos_dev,
                       const float* sin_dev, const unsigned char* key_mask_dev, int B, int H, int dk, int T, float scale, float* out_dev,
                       void* stream) {
    return rope_attention_run("amp_rope_attention", false, true, false, q_dev, batch_stride, k_dev, v_dev, batch_stride, cos_dev, sin_dev, key_mask_dev, B, H, dk,
                              T, T, scale, out_dev, stream);
}

int amp_rope_attention_causal(const float* q_dev, const float* k_dev, const float* v_dev, long long batch_stride, const float* cos_dev,
                              const float* sin_dev, const unsigned char* key_mask_dev, int B, int H, int dk, int T, float scale, float* out_dev,
                              void* stream) {
    return rope_attention_run("amp_rope_attention_causal", true, true, false, q_dev, batch_stride, k_dev, v_dev, batch_stride, cos_dev, sin_dev, key_mask_dev, B,
                              H, dk, T, T, scale, out_dev, stream);
}

int amp_mh_attention(const float* q_dev, const float* k_dev, const float* v_dev, long long batch_stride, const unsigned char* key_mask_dev, int B,
                     int H, int dk, int T, float scale, float* out_dev, void* stream) {
    return rope_attention_run("amp_mh_attention", false, false, false, q_dev, batch_stride, k_dev, v_dev, batch_stride, nullptr, nullptr, key_mask_dev, B, H, dk, T,
                              T, scale, out_dev, stream);
}

int amp_cross_attention(const float* q_dev, long long q_batch_stride, const float* k_dev, const float* v_dev, long long kv_batch_stride,
                        const unsigned char* key_mask_dev, int B, int H, int dk, int Tq, int Tk, float scale, float* out_dev, void* stream) {
    return rope_attention_run("amp_cross_attention", false, false, 1, q_dev, q_batch_stride, k_dev, v_dev, kv_batch_stride, nullptr, nullptr, key_mask_dev, B,
                              H, dk, Tq, Tk, scale, out_dev, stream);
}

int amp_cross_attention_hd(const float* q_dev, long long q_batch_stride, const float* k_dev, const float* v_dev, long long kv_batch_stride,
                           const unsigned char* key_mask_dev, int B, int H, int dk, int Tq, int Tk, float scale, float* out_dev, void* stream) {
    return rope_attention_run("amp_cross_attention_hd", false, false, 2, q_dev, q_batch_stride, k_dev, v_dev, kv_batch_stride, nullptr, nullptr, key_mask_dev, B,
                              H, dk, Tq, Tk, scale, out_dev, stream);
}

int amp_prefix_attention(const float* q_dev, const float* k_dev, const float* v_dev, long long batch_stride, const unsigned char* key_mask_dev, int B,
                         int H, int dk, int T, int prefix, float scale, float* out_dev, void* stream) {
    return rope_attention_run("amp_prefix_attention", true, false, false, q_dev, batch_stride, k_dev, v_dev, batch_stride, nullptr, nullptr, key_mask_dev, B, H, dk,
                              T, T, scale, out_dev, stream, prefix);
}

int amp_rms_norm_c_adaptive(const float* x_dev, const float* w_dev, long long w_batch_stride, int B, int C, int T, float eps, float* y_dev,
                            void* stream) {
    if (!x_dev || !w_dev || !y_dev || B < 1 || C < 1 || T < 1 || B > 65535 || w_batch_stride < 0 || !(eps >= 0.f)) {
        set_error("amp_rms_norm_c_adaptive: bad argument (B=%d C=%d T=%d w_batch_stride=%lld)", B, C, T, w_batch_stride);
        return AMP_ERR_INVALID;
    }
    const dim3 grid((unsigned)((T + RN_TT - 1) / RN_TT), (unsigned)B);
    auto kern = C <= 32 * RN_G ? rms_norm_c_adaptive_kernel<32> : rms_norm_c_adaptive_kernel<128>;
    note_kernel("rms_norm_c_adaptive_kernel", C <= 32 * RN_G ? 32 : 128);
    note_work((unsigned long long)grid.x * grid.y, 0.0, 8.0 * (double)B * C * T / 1e6, "adaptive rms norm C=%d T=%d B=%d", C, T, B);
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, (hipStream_t)stream, x_dev, w_dev, w_batch_stride, y_dev, C, T, eps);
    AMP_HIP(hipGetLastError());
    return AMP_OK;
}

int amp_silu(const float* x_dev, long long n, float* y_dev, void* stream) {
    if (!x_dev || !y_dev || n <= 0) { set_error("amp_silu: bad argument (n=%lld)", n); return AMP_ERR_INVALID; }
    const int vec = ((reinterpret_cast<uintptr_t>(x_dev) | reinterpret_cast<uintptr_t>(y_dev)) & 15) == 0 ? 1 : 0;
    const long long threads = vec ? (n >> 2) + (n & 3) : n;
    const long long blocks = (threads + 255) / 256;
    if (blocks > 0x7fffffffll) { set_error("amp_silu: n=%lld is beyond the grid", n); return AMP_ERR_UNSUPPORTED; }
    note_kernel("silu_kernel");
    note_work((unsigned long long)blocks, 0.0, 8.0 * (double)n / 1e6, "silu n=%lld", n);
    hipLaunchKernelGGL(silu_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x_dev, y_dev, (size_t)n, vec);
    AMP_HIP(hipGetLastError());
    return AMP_OK;
}

int amp_swiglu(const float* gu_dev, int B, int F, int T, float* y_dev, void* stream) {
    if (!gu_dev || !y_dev || B < 1 || F < 1 || T < 1 || B > 65535) { set_error("amp_swiglu: bad argument (B=%d F=%d T=%d)", B, F, T); return AMP_ERR_INVALID; }
    const size_t n = (size_t)F * T;
    const float* ylo = y_dev;
    const float* yhi = y_dev + (size_t)B * n;
    if (gu_dev < yhi && ylo < gu_dev + 2 * (size_t)B * n) { set_error("amp_swiglu: y must not overlap gu"); return AMP_ERR_INVALID; }
    const int vec = (n & 3) == 0 && ((reinterpret_cast<uintptr_t>(gu_dev) | reinterpret_cast<uintptr_t>(y_dev)) & 15) == 0 ? 1 : 0;
    const size_t threads = vec ? n >> 2 : n;
    const size_t blocks = (threads + 255) / 256;
    if (blocks > 0x7fffffffull) { set_error("amp_swiglu: F*T=%zu is beyond the grid", n); return AMP_ERR_UNSUPPORTED; }
    note_kernel("swiglu_kernel");
    note_work((unsigned long long)blocks * B, 0.0, 12.0 * (double)B * n / 1e6, "swiglu F=%d T=%d B=%d", F, T, B);
    hipLaunchKernelGGL(swiglu_kernel, dim3((unsigned)blocks, (unsigned)B), dim3(256), 0, (hipStream_t)stream, gu_dev, y_dev, n, vec);
    AMP_HIP(hipGetLastError());
    return AMP_OK;
}

}  // extern "C"
