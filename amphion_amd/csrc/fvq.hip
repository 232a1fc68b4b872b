// Residual factorized vector quantizer of the Amphion acoustic codec in eval mode (models/codec/amphion_codec/quantize/residual_vq.py:68-152,
// factorized_vector_quantize.py:52-127; quantizer_type "fvq"): amp_fvq_encode = ResidualVQ.forward (codes + quantized_out) in ONE launch,
// amp_fvq_decode = ResidualVQ.vq2emb.  amp_fvq_encode_ex / amp_fvq_decode_add are the same two kernels with DualCodec's DAC.encode /
// DAC.decode_from_codes folded in (model_codec/dac_model.py:301-312,319-320): z read as the crop [..., :T] of a longer tensor, the residual
// started as z - sub, quantized_out stored as sum z_q + sub, every level's z_e stored as `latents`; decode stores sum + add.  Each of the
// folded operations is ONE fp32 add or subtract of two stored values -- the bits of torch's separate passes.
//
// Everything here decides or reproduces INTEGERS, so it is plain fp32 on the vector ALU -- no f16x3, no MFMA.  A workgroup of 256 threads owns
// FVQ_TF = 16 frames of one item and keeps their residual [D][16] and the running sum of the levels' z_q [D][16] in LDS across all levels:
// z is read once and quantized_out written once, whatever N is.  Per level, in the reference's order:
//   z_e  = in_project(residual)                      wave w owns rows j = w, w + 4, ..; lane = frame + 16 * part, part p sums channels p, p + 4, ..
//                                                    as one fmaf chain, the four parts meet in a fixed shuffle tree
//   e    = z_e / max(||z_e||, 1e-12)                 F.normalize (use_l2_normlize; the codebook is normalised once, at create time)
//   dist = (sum e^2 - 2 e.c_k) + sum c_k^2           the reference's expression with its order of operations; e.c_k one fmaf chain over d
//   code = lowest k of the smallest dist             (-dist).max(1)[1]: a thread scans its k ascending with a strict <, ties between threads
//                                                    go to the lower index
//   z_q  = out_project(z_e + (codebook[code] - z_e)) the straight-through form the reference evaluates in eval mode too; the RAW codebook row
//   residual -= z_q;  quantized_out += z_q
// Codebooks are NOT staged in LDS: lane = frame + 16 * kpart, so the 16 frames of a part read row k as ONE broadcast request and every row
// reaches a workgroup exactly once per level -- what a staging pass would fetch too, without its LDS write, barrier and the K * d cap (16384 x 32
// rows are 2 MB).  All N codebooks of the recipe (12 x 32 KB) sit in one L2.  Rows are zero-padded to DP = 8 / 16 / 32 floats so that e stays in
// registers; a padded term is fmaf(0, 0, acc) = acc, bit for bit.
#include <string.h>

#include <memory>

#include "amp_host.h"

namespace amp {

constexpr int FVQ_TF = 16;

struct FvqArgs {
    const float* z;          // [B, D, zT], columns [0, T) read
    const float* sub;        // [B, D, T] or nullptr: the residual starts as z - sub, zq receives the sum + sub
    float* lat;              // [B, n * d, T] every level's z_e (torch.cat(latents, 1)) or nullptr
    long long* codes;        // [n, B, T]
    float* zq;               // [B, D, T] or nullptr
    float* allq;             // [n, B, D, T] every level's z_q (ResidualVQ.forward's all_quantized) or nullptr
    const float* w_in;       // [N][d][D] or nullptr (identity)
    const float* b_in;       // [N][d]
    const float* cb;         // [N][K][DP] raw codebook rows, zero-padded
    const float* cbn;        // [N][K][DP] rows the distance is taken to (normalised when l2), zero-padded
    const float* cn2;        // [N][K] sum of cbn^2
    const float* w_out;      // [N][D][d] or nullptr
    const float* b_out;      // [N][D]
    int B, D, d, K, T, n, l2;
    int tiles_per_item;
    long long zT;            // row stride of z (>= T)
};

template <int DP>
__global__ __launch_bounds__(256) void fvq_encode_kernel(const FvqArgs a) {
    extern __shared__ __attribute__((aligned(16))) float fvq_smem[];
    const int D = a.D, d = a.d, K = a.K, T = a.T;
    float* R = fvq_smem;                       // [D][TF] residual
    float* Q = R + (size_t)D * FVQ_TF;         // [D][TF] sum of z_q
    float* E = Q + (size_t)D * FVQ_TF;         // [DP][TF] z_e
    float* EN = E + DP * FVQ_TF;               // [DP][TF] normalised z_e (or z_e)
    float* E2 = EN + DP * FVQ_TF;              // [TF]
    float* BD = E2 + FVQ_TF;                   // [4][TF] best distance per wave
    int* BI = reinterpret_cast<int*>(BD + 4 * FVQ_TF);   // [4][TF] its index
    int* CODE = BI + 4 * FVQ_TF;               // [TF]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int f = tid & 15;
    const int part = (lane >> 4);              // 0 .. 3 within the wave
    const int part16 = tid >> 4;               // 0 .. 15 within the workgroup
    const int item = blockIdx.x / a.tiles_per_item;
    const int t0 = (blockIdx.x - item * a.tiles_per_item) * FVQ_TF;
    const int t = t0 + f;
    const bool tok = t < T;
    const float* zb = a.z + (size_t)item * D * a.zT;
    const float* sb = a.sub ? a.sub + (size_t)item * D * T : nullptr;

    for (int c = part16; c < D; c += 16) {
        float r = tok ? zb[(size_t)c * a.zT + t] : 0.f;
        if (sb && tok) r -= sb[(size_t)c * T + t];
        R[c * FVQ_TF + f] = r;
        Q[c * FVQ_TF + f] = 0.f;
    }
    for (int i = tid; i < DP * FVQ_TF; i += 256) { E[i] = 0.f; EN[i] = 0.f; }
    __syncthreads();

    for (int l = 0; l < a.n; ++l) {
        // ---- z_e = in_project(residual) ----
        if (a.w_in) {
            const float* W = a.w_in + (size_t)l * d * D;
            for (int j = wave; j < d; j += 4) {
                const float* wr = W + (size_t)j * D;
                float s = 0.f;
                for (int c = part; c < D; c += 4) s = fmaf(wr[c], R[c * FVQ_TF + f], s);
                s += __shfl_xor(s, 16, 64);
                s += __shfl_xor(s, 32, 64);
                if (part == 0) E[j * FVQ_TF + f] = s + a.b_in[l * d + j];
            }
        } else {
            for (int i = tid; i < d * FVQ_TF; i += 256) E[i] = R[i];     // D == d
        }
        __syncthreads();
        // ---- F.normalize(z_e) and sum e^2 ----
        if (tid < FVQ_TF) {
            float inv = 1.f;
            if (a.l2) {
                float n2 = 0.f;
                for (int j = 0; j < d; ++j) n2 = fmaf(E[j * FVQ_TF + tid], E[j * FVQ_TF + tid], n2);
                const float nrm = sqrtf(n2);
                inv = nrm > 1e-12f ? nrm : 1e-12f;
            }
            float e2 = 0.f;
            for (int j = 0; j < d; ++j) {
                const float v = a.l2 ? E[j * FVQ_TF + tid] / inv : E[j * FVQ_TF + tid];
                EN[j * FVQ_TF + tid] = v;
                e2 = fmaf(v, v, e2);
            }
            E2[tid] = e2;
        }
        __syncthreads();
        // ---- all K distances of frame f, K / 16 per thread ----
        {
            float e[DP];
#pragma unroll
            for (int j = 0; j < DP; ++j) e[j] = 2.f * EN[j * FVQ_TF + f];      // (2 * encodings) @ codebook.t(): the doubling is exact
            const float e2 = E2[f];
            const float* cbn = a.cbn + (size_t)l * K * DP;
            const float* cn2 = a.cn2 + (size_t)l * K;
            float best = __builtin_inff();
            int bi = 0;
            for (int k = part16; k < K; k += 16) {
                const float4* row = reinterpret_cast<const float4*>(cbn + (size_t)k * DP);
                float dot = 0.f;
#pragma unroll
                for (int j4 = 0; j4 < DP / 4; ++j4) {
                    const float4 c4 = row[j4];
                    dot = fmaf(e[4 * j4 + 0], c4.x, dot);
                    dot = fmaf(e[4 * j4 + 1], c4.y, dot);
                    dot = fmaf(e[4 * j4 + 2], c4.z, dot);
                    dot = fmaf(e[4 * j4 + 3], c4.w, dot);
                }
                const float dist = (e2 - dot) + cn2[k];
                if (dist < best) { best = dist; bi = k; }
            }
            // the four parts of a wave, then the four waves: smaller distance wins, equal distances go to the lower index
#pragma unroll
            for (int o = 16; o <= 32; o <<= 1) {
                const float ob = __shfl_xor(best, o, 64);
                const int oi = __shfl_xor(bi, o, 64);
                if (ob < best || (ob == best && oi < bi)) { best = ob; bi = oi; }
            }
            if (part == 0) { BD[wave * FVQ_TF + f] = best; BI[wave * FVQ_TF + f] = bi; }
        }
        __syncthreads();
        if (tid < FVQ_TF) {
            float best = BD[tid];
            int bi = BI[tid];
            for (int w = 1; w < 4; ++w) {
                const float ob = BD[w * FVQ_TF + tid];
                const int oi = BI[w * FVQ_TF + tid];
                if (ob < best || (ob == best && oi < bi)) { best = ob; bi = oi; }
            }
            CODE[tid] = bi;
            if (t0 + tid < T) a.codes[((size_t)l * a.B + item) * T + t0 + tid] = bi;
        }
        __syncthreads();
        // ---- z_q in the codebook space: z_e + (codebook[code] - z_e), into EN ----
        for (int i = tid; i < d * FVQ_TF; i += 256) {
            const int j = i / FVQ_TF, ff = i - j * FVQ_TF;
            const float ze = E[i];
            EN[i] = ze + (a.cb[((size_t)l * K + CODE[ff]) * DP + j] - ze);
            if (a.lat && t0 + ff < T) a.lat[(((size_t)item * a.n + l) * d + j) * T + t0 + ff] = ze;
        }
        __syncthreads();
        // ---- out_project, residual and sum ----
        if (a.w_out) {
            const float* W = a.w_out + (size_t)l * D * d;
            for (int c = part16; c < D; c += 16) {
                const float* wr = W + (size_t)c * d;
                float s = 0.f;
                for (int j = 0; j < d; ++j) s = fmaf(wr[j], EN[j * FVQ_TF + f], s);
                s += a.b_out[l * D + c];
                R[c * FVQ_TF + f] -= s;
                Q[c * FVQ_TF + f] += s;
                if (a.allq && tok) a.allq[(((size_t)l * a.B + item) * D + c) * T + t] = s;
            }
        } else {
            for (int c = part16; c < d; c += 16) {
                const float s = EN[c * FVQ_TF + f];
                R[c * FVQ_TF + f] -= s;
                Q[c * FVQ_TF + f] += s;
                if (a.allq && tok) a.allq[(((size_t)l * a.B + item) * D + c) * T + t] = s;
            }
        }
        __syncthreads();
    }
    if (a.zq && tok) {
        float* qb = a.zq + (size_t)item * D * T;
        if (sb) {
            for (int c = part16; c < D; c += 16) qb[(size_t)c * T + t] = Q[c * FVQ_TF + f] + sb[(size_t)c * T + t];
        } else {
            for (int c = part16; c < D; c += 16) qb[(size_t)c * T + t] = Q[c * FVQ_TF + f];
        }
    }
}

struct FvqDecArgs {
    const long long* codes;  // [n, B, T]
    float* out;              // [B, D, T]
    const float* add;        // [B, D, T] or nullptr: out = sum + add
    const float* cb;         // [N][K][DP]
    const float* w_out;      // [N][D][d] or nullptr
    const float* b_out;      // [N][D]
    unsigned* flag;          // set when a code lies outside [0, K)
    int B, D, d, DP, K, T, n;
    int tiles_per_item;
};

// vq2emb: out = sum over levels of out_project(codebook[code]), the levels added in order.  The code rows of ALL levels of the tile's 16 frames are
// staged first ([n][d][16] floats of LDS), so each output element is summed in a register by its one owner and stored once.  An index outside
// [0, K) raises the flag and reads row 0 instead: nothing is ever read out of bounds.
__global__ __launch_bounds__(256) void fvq_decode_kernel(const FvqDecArgs a) {
    extern __shared__ __attribute__((aligned(16))) float fvq_dec_smem[];
    const int D = a.D, d = a.d, T = a.T, n = a.n;
    float* EN = fvq_dec_smem;                                    // [n][d][TF]
    int* CODE = reinterpret_cast<int*>(EN + (size_t)n * d * FVQ_TF);   // [n][TF]
    const int tid = threadIdx.x;
    const int f = tid & 15, part16 = tid >> 4;
    const int item = blockIdx.x / a.tiles_per_item;
    const int t0 = (blockIdx.x - item * a.tiles_per_item) * FVQ_TF;
    const int t = t0 + f;
    for (int i = tid; i < n * FVQ_TF; i += 256) {
        const int l = i / FVQ_TF, ff = i - l * FVQ_TF;
        long long c = (t0 + ff < T) ? a.codes[((size_t)l * a.B + item) * T + t0 + ff] : 0;
        if (c < 0 || c >= a.K) { atomicOr(a.flag, 1u); c = 0; }
        CODE[i] = (int)c;
    }
    __syncthreads();
    for (int i = tid; i < n * d * FVQ_TF; i += 256) {
        const int l = i / (d * FVQ_TF), r = i - l * d * FVQ_TF;
        const int j = r / FVQ_TF, ff = r - j * FVQ_TF;
        EN[i] = a.cb[((size_t)l * a.K + CODE[l * FVQ_TF + ff]) * a.DP + j];
    }
    __syncthreads();
    if (t >= T) return;
    float* ob = a.out + (size_t)item * D * T;
    const float* ab = a.add ? a.add + (size_t)item * D * T : nullptr;
    for (int c = part16; c < D; c += 16) {
        float acc = 0.f;
        for (int l = 0; l < n; ++l) {
            const float* en = EN + (size_t)l * d * FVQ_TF;
            float s;
            if (a.w_out) {
                const float* wr = a.w_out + ((size_t)l * D + c) * d;
                s = 0.f;
                for (int j = 0; j < d; ++j) s = fmaf(wr[j], en[j * FVQ_TF + f], s);
                s += a.b_out[l * D + c];
            } else {
                s = en[c * FVQ_TF + f];
            }
            acc = l ? acc + s : s;
        }
        ob[(size_t)c * T + t] = ab ? acc + ab[(size_t)c * T + t] : acc;
    }
}

}  // namespace amp

using namespace amp;

struct amp_fvq {
    int D = 0, d = 0, DP = 0, K = 0, N = 0, l2 = 0;
    bool proj = false;
    float *w_in = nullptr, *b_in = nullptr, *cb = nullptr, *cbn = nullptr, *cn2 = nullptr, *w_out = nullptr, *b_out = nullptr;
    unsigned* flag = nullptr;
    DeviceAllocs dev;
};

static size_t fvq_lds_bytes(int D, int DP) { return ((size_t)2 * D * FVQ_TF + 2 * DP * FVQ_TF + FVQ_TF * 10) * sizeof(float); }

extern "C" {

int amp_fvq_create(int input_dim, int codebook_dim, int codebook_size, int num_quantizers, int use_l2_normalize,
                   const float* const* in_w_host, const float* const* in_b_host, const float* const* codebook_host,
                   const float* const* out_w_host, const float* const* out_b_host, amp_fvq** out) {
    if (!codebook_host || !out) { set_error("amp_fvq_create: null argument"); return AMP_ERR_INVALID; }
    const int D = input_dim, d = codebook_dim, K = codebook_size, N = num_quantizers;
    if (D < 1 || d < 1 || K < 1 || N < 1) { set_error("amp_fvq_create: D=%d d=%d K=%d N=%d", D, d, K, N); return AMP_ERR_INVALID; }
    if (D > 1024 || d > 32 || K > 16384 || N > 32) {
        set_error("amp_fvq_create: D=%d d=%d K=%d N=%d is outside the kernel (D <= 1024, d <= 32, K <= 16384, N <= 32)", D, d, K, N);
        return AMP_ERR_UNSUPPORTED;
    }
    const bool proj = in_w_host != nullptr;
    if (proj != (out_w_host != nullptr) || proj != (in_b_host != nullptr) || proj != (out_b_host != nullptr)) {
        set_error("amp_fvq_create: in_project and out_project come together, with their biases, or not at all");
        return AMP_ERR_INVALID;
    }
    if (!proj && D != d) { set_error("amp_fvq_create: identity projections need input_dim == codebook_dim (%d != %d)", D, d); return AMP_ERR_INVALID; }
    auto h = std::make_unique<amp_fvq>();
    h->D = D; h->d = d; h->K = K; h->N = N; h->l2 = use_l2_normalize ? 1 : 0; h->proj = proj;
    const int DP = d <= 8 ? 8 : (d <= 16 ? 16 : 32);
    h->DP = DP;
    std::vector<float> cb((size_t)N * K * DP, 0.f), cbn((size_t)N * K * DP, 0.f), cn2((size_t)N * K, 0.f);
    std::vector<float> wi, bi, wo, bo;
    if (proj) { wi.resize((size_t)N * d * D); bi.resize((size_t)N * d); wo.resize((size_t)N * D * d); bo.resize((size_t)N * D); }
    for (int l = 0; l < N; ++l) {
        if (!codebook_host[l] || (proj && (!in_w_host[l] || !in_b_host[l] || !out_w_host[l] || !out_b_host[l]))) {
            set_error("amp_fvq_create: null weight at level %d", l);
            return AMP_ERR_INVALID;
        }
        for (int k = 0; k < K; ++k) {
            const float* r = codebook_host[l] + (size_t)k * d;
            float* raw = &cb[((size_t)l * K + k) * DP];
            float* nr = &cbn[((size_t)l * K + k) * DP];
            float inv = 1.f;
            if (h->l2) {                       // F.normalize(codebook): v / max(||v||, 1e-12), fp32 as the reference forms it
                float n2 = 0.f;
                for (int j = 0; j < d; ++j) n2 = fmaf(r[j], r[j], n2);
                const float nrm = sqrtf(n2);
                inv = nrm > 1e-12f ? nrm : 1e-12f;
            }
            float s = 0.f;
            for (int j = 0; j < d; ++j) {
                if (!(fabsf(r[j]) < 1e30f)) { set_error("amp_fvq_create: non-finite codebook entry (level %d)", l); return AMP_ERR_INVALID; }
                raw[j] = r[j];
                nr[j] = h->l2 ? r[j] / inv : r[j];
                s = fmaf(nr[j], nr[j], s);
            }
            cn2[(size_t)l * K + k] = s;
        }
        if (proj) {
            memcpy(&wi[(size_t)l * d * D], in_w_host[l], sizeof(float) * d * D);
            memcpy(&bi[(size_t)l * d], in_b_host[l], sizeof(float) * d);
            memcpy(&wo[(size_t)l * D * d], out_w_host[l], sizeof(float) * D * d);
            memcpy(&bo[(size_t)l * D], out_b_host[l], sizeof(float) * D);
        }
    }
    // every refusal above is the host's alone: the arguments are judged the same with or without a device
    if (amp_device_count() <= 0) { set_error("amp_fvq_create: no HIP device visible (the HIP path has no CPU fallback)"); return AMP_ERR_HIP; }
    AMP_RC(h->dev.upload(cb, &h->cb));
    AMP_RC(h->dev.upload(cbn, &h->cbn));
    AMP_RC(h->dev.upload(cn2, &h->cn2));
    if (proj) {
        AMP_RC(h->dev.upload(wi, &h->w_in));
        AMP_RC(h->dev.upload(bi, &h->b_in));
        AMP_RC(h->dev.upload(wo, &h->w_out));
        AMP_RC(h->dev.upload(bo, &h->b_out));
    }
    const std::vector<float> zero(1, 0.f);
    AMP_RC(h->dev.upload(zero, &h->flag));
    *out = h.release();
    return AMP_OK;
}

void amp_fvq_destroy(amp_fvq* h) { delete h; }

static int fvq_check_shape(const amp_fvq* h, int n_quantizers, int B, int T, const char* who) {
    if (!h) { set_error("%s: null handle", who); return AMP_ERR_INVALID; }
    if (B <= 0 || T <= 0) { set_error("%s: B=%d T=%d", who, B, T); return AMP_ERR_INVALID; }
    if (n_quantizers < 1 || n_quantizers > h->N) { set_error("%s: n_quantizers=%d of %d", who, n_quantizers, h->N); return AMP_ERR_INVALID; }
    if ((long long)B * ((T + FVQ_TF - 1) / FVQ_TF) > 0x7fffffffll) { set_error("%s: B=%d x T=%d is beyond the grid", who, B, T); return AMP_ERR_UNSUPPORTED; }
    return AMP_OK;
}

static int fvq_encode_run(const char* who, const amp_fvq* h, const float* z_dev, long long z_row_stride, const float* sub_dev, int B, int T,
                          int n_quantizers, long long* codes_dev, float* zq_dev, float* all_zq_dev, float* latents_dev, void* stream) {
    AMP_RC(fvq_check_shape(h, n_quantizers, B, T, who));
    if (!z_dev || !codes_dev) { set_error("%s: null argument", who); return AMP_ERR_INVALID; }
    if (z_dev == zq_dev) { set_error("%s: z and zq must not alias", who); return AMP_ERR_INVALID; }
    if (z_row_stride < T) { set_error("%s: z row stride %lld is shorter than T = %d", who, z_row_stride, T); return AMP_ERR_INVALID; }
    FvqArgs a{};
    a.z = z_dev; a.codes = codes_dev; a.zq = zq_dev; a.allq = all_zq_dev; a.sub = sub_dev; a.lat = latents_dev; a.zT = z_row_stride;
    a.w_in = h->w_in; a.b_in = h->b_in; a.cb = h->cb; a.cbn = h->cbn; a.cn2 = h->cn2; a.w_out = h->w_out; a.b_out = h->b_out;
    a.B = B; a.D = h->D; a.d = h->d; a.K = h->K; a.T = T; a.n = n_quantizers; a.l2 = h->l2;
    a.tiles_per_item = (T + FVQ_TF - 1) / FVQ_TF;
    const unsigned grid = (unsigned)((size_t)B * a.tiles_per_item);
    const size_t lds = fvq_lds_bytes(h->D, h->DP);
    const double frames = (double)B * T;
    const double gf = frames * n_quantizers * (2.0 * h->d * h->D * (h->proj ? 2 : 0) + 2.0 * h->K * h->d) / 1e9;
    const double mb = (frames * h->D * 4.0 * (1 + (sub_dev ? (zq_dev ? 2 : 1) : 0) + (zq_dev ? 1 : 0) + (all_zq_dev ? n_quantizers : 0)) +
                       frames * n_quantizers * (8.0 + (latents_dev ? 4.0 * h->d : 0.0))) / 1e6;
    note_kernel("fvq_encode_kernel", h->DP);
    note_work(grid, gf, mb, "fvq encode D=%d d=%d K=%d n=%d T=%d B=%d", h->D, h->d, h->K, n_quantizers, T, B);
    hipStream_t st = (hipStream_t)stream;
    if (h->DP == 8) {
        AMP_HIP(ensure_dynamic_lds<&fvq_encode_kernel<8>>(lds));
        hipLaunchKernelGGL(fvq_encode_kernel<8>, dim3(grid), dim3(256), lds, st, a);
    } else if (h->DP == 16) {
        AMP_HIP(ensure_dynamic_lds<&fvq_encode_kernel<16>>(lds));
        hipLaunchKernelGGL(fvq_encode_kernel<16>, dim3(grid), dim3(256), lds, st, a);
    } else {
        AMP_HIP(ensure_dynamic_lds<&fvq_encode_kernel<32>>(lds));
        hipLaunchKernelGGL(fvq_encode_kernel<32>, dim3(grid), dim3(256), lds, st, a);
    }
    AMP_HIP(hipGetLastError());
    return AMP_OK;
}

int amp_fvq_encode(const amp_fvq* h, const float* z_dev, int B, int T, int n_quantizers, long long* codes_dev, float* zq_dev, float* all_zq_dev,
                   void* stream) {
    return fvq_encode_run("amp_fvq_encode", h, z_dev, T, nullptr, B, T, n_quantizers, codes_dev, zq_dev, all_zq_dev, nullptr, stream);
}

int amp_fvq_encode_ex(const amp_fvq* h, const float* z_dev, long long z_row_stride, const float* sub_dev, int B, int T, int n_quantizers,
                      long long* codes_dev, float* zq_dev, float* all_zq_dev, float* latents_dev, void* stream) {
    if (sub_dev && sub_dev == zq_dev) { set_error("amp_fvq_encode_ex: sub and zq must not alias"); return AMP_ERR_INVALID; }
    return fvq_encode_run("amp_fvq_encode_ex", h, z_dev, z_row_stride, sub_dev, B, T, n_quantizers, codes_dev, zq_dev, all_zq_dev, latents_dev,
                          stream);
}

static int fvq_decode_run(const char* who, const amp_fvq* h, const long long* codes_dev, int n_quantizers, int B, int T, const float* add_dev,
                          float* out_dev, void* stream) {
    AMP_RC(fvq_check_shape(h, n_quantizers, B, T, who));
    if (!codes_dev || !out_dev) { set_error("%s: null argument", who); return AMP_ERR_INVALID; }
    FvqDecArgs a{};
    a.codes = codes_dev; a.out = out_dev; a.add = add_dev; a.cb = h->cb; a.w_out = h->w_out; a.b_out = h->b_out; a.flag = h->flag;
    a.B = B; a.D = h->D; a.d = h->d; a.DP = h->DP; a.K = h->K; a.T = T; a.n = n_quantizers;
    a.tiles_per_item = (T + FVQ_TF - 1) / FVQ_TF;
    const unsigned grid = (unsigned)((size_t)B * a.tiles_per_item);
    const double frames = (double)B * T;
    note_kernel("fvq_decode_kernel");
    note_work(grid, frames * n_quantizers * 2.0 * h->d * h->D * (h->proj ? 1 : 0) / 1e9,
              (frames * h->D * 4.0 * (add_dev ? 2 : 1) + frames * n_quantizers * 8.0) / 1e6,
              "fvq decode D=%d d=%d K=%d n=%d T=%d B=%d", h->D, h->d, h->K, n_quantizers, T, B);
    const size_t lds = ((size_t)n_quantizers * h->d + n_quantizers) * FVQ_TF * sizeof(float);
    AMP_HIP(ensure_dynamic_lds<&fvq_decode_kernel>(lds));
    hipLaunchKernelGGL(fvq_decode_kernel, dim3(grid), dim3(256), lds, (hipStream_t)stream, a);
    AMP_HIP(hipGetLastError());
    return AMP_OK;
}

int amp_fvq_decode(const amp_fvq* h, const long long* codes_dev, int n_quantizers, int B, int T, float* out_dev, void* stream) {
    return fvq_decode_run("amp_fvq_decode", h, codes_dev, n_quantizers, B, T, nullptr, out_dev, stream);
}

int amp_fvq_decode_add(const amp_fvq* h, const long long* codes_dev, int n_quantizers, int B, int T, const float* add_dev, float* out_dev,
                       void* stream) {
    return fvq_decode_run("amp_fvq_decode_add", h, codes_dev, n_quantizers, B, T, add_dev, out_dev, stream);
}

int amp_fvq_check(amp_fvq* h, void* stream) {
    if (!h) { set_error("amp_fvq_check: null handle"); return AMP_ERR_INVALID; }
    unsigned v = 0;
    hipStream_t st = (hipStream_t)stream;
    AMP_HIP(hipMemcpyAsync(&v, h->flag, sizeof(v), hipMemcpyDeviceToHost, st));
    AMP_HIP(hipStreamSynchronize(st));
    if (v) {
        AMP_HIP(hipMemsetAsync(h->flag, 0, sizeof(v), st));
        AMP_HIP(hipStreamSynchronize(st));
        set_error("amp_fvq_decode: a code index outside [0, %d) was given since the last check (the output of that call used row 0 in its place)", h->K);
        return AMP_ERR_INVALID;
    }
    return AMP_OK;
}

}  // extern "C"
