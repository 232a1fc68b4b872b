// DiffWave (models/vocoders/diffusion/diffwave/diffwave.py:127-179) and one step of its sampler
// (models/vocoders/diffusion/diffusion_vocoder_inference.py:55-71): the amp_dw_* handle, the small streaming kernels around the residual
// layer (dw_layer_f16x3.hip) and the host side that chains them.  Per noise prediction: step embedding (1 launch), input projection (1),
// N residual layers (N), tail (1, fused with the sampler update in amp_dw_sample_step).  The conditioner is written once per utterance
// by amp_dw_condition as plain fp32 [B, n_mel, L]: both arithmetics and the op-level entry read ONE form.
#include <cmath>
#include <map>
#include <memory>
#include <string>

#include "amp_host.h"

namespace amp {

// ---- SpectrogramUpsampler (diffwave.py:68-93): ConvTranspose2d(1, 1, [3, 2u], stride [1, u], padding [1, u / 2]) + leaky_relu(0.4) ----
// out[m, t] = bias + sum_{km < 3} sum_{it} in[m + 1 - km, it] * w[km, t + u/2 - it * u]: two time taps per output (u even)
__global__ __launch_bounds__(256) void dw_upsample_kernel(const float* __restrict__ in, float* __restrict__ out, const float* __restrict__ w,
                                                          const float* __restrict__ bias, int rows_per_item, int Fin, int u, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int Fout = Fin * u;
    const int t = (int)(i % (size_t)Fout);
    const size_t row = i / (size_t)Fout;
    const int m = (int)(row % (size_t)rows_per_item);
    const int s = t + u / 2;
    const int it1 = s / u, kt1 = s - it1 * u;
    float acc = bias[0];
#pragma unroll
    for (int km = 0; km < 3; ++km) {
        const int im = m + 1 - km;
        if (im < 0 || im >= rows_per_item) continue;
        const float* r = in + (row - m + im) * (size_t)Fin;
        if (it1 < Fin) acc = fmaf(r[it1], w[km * 2 * u + kt1], acc);
        if (it1 >= 1) acc = fmaf(r[it1 - 1], w[km * 2 * u + kt1 + u], acc);
    }
    out[i] = acc > 0.f ? acc : acc * 0.4f;
}

// ---- relu(input_projection(audio)) (diffwave.py:163-165): Conv1d(1, C, 1) ----
__global__ __launch_bounds__(256) void dw_input_kernel(const float* __restrict__ audio, const float* __restrict__ w, const float* __restrict__ b,
                                                       float* __restrict__ x, int C, int L, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int t = (int)(i % (size_t)L);
    const size_t bc = i / (size_t)L;
    const int c = (int)(bc % (size_t)C);
    const size_t item = bc / (size_t)C;
    const float v = fmaf(w[c], audio[item * L + t], b[c]);
    x[i] = v > 0.f ? v : 0.f;
}

// ---- DiffusionEmbedding (diffwave.py:42-58) + every layer's diffusion_projection (:113): one workgroup per step value ----
__device__ __forceinline__ float dw_silu(float v) { return v / (1.f + expf(-v)); }

// y[r] = act(W[r, :] . x + b[r]) for r < rows: one wave per row, lanes stride the columns, fixed shuffle tree
template <bool SILU>
__device__ __forceinline__ void dw_matvec(const float* __restrict__ W, const float* __restrict__ b, const float* x, float* y, int rows, int cols,
                                          int wave, int lane, int nwaves) {
    for (int r = wave; r < rows; r += nwaves) {
        const float* wr = W + (size_t)r * cols;
        float s = 0.f;
        for (int c = lane; c < cols; c += 64) s = fmaf(wr[c], x[c], s);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        s += b[r];
        if (lane == 0) y[r] = SILU ? dw_silu(s) : s;
    }
}

struct DwEmbedArgs {
    const float* steps_dev;   // [S] or nullptr: step_host
    float step_host;
    const float* table;       // [max_steps, 128]
    const float *w1, *b1, *w2, *b2;   // 128 -> 512 -> 512
    const float *wd, *bd;     // [N * C, 512], [N * C]
    float* out;               // [S, N * C]
    int max_steps, NC;
};

__global__ __launch_bounds__(512) void dw_embed_kernel(const DwEmbedArgs a) {
    __shared__ float e0[128], h1[512], h2[512];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float t = a.steps_dev ? a.steps_dev[blockIdx.x] : a.step_host;
    if (tid < 128) {
        // integer steps index the table, float steps interpolate between floor and ceil (:53-58); an integer-valued float gives
        // low + (high - low) * 0 = the row itself.  The host refuses steps outside [0, max_steps - 1]; the clamp keeps a device-side
        // step from indexing outside the table.
        int lo = (int)floorf(t), hi = (int)ceilf(t);
        lo = lo < 0 ? 0 : (lo > a.max_steps - 1 ? a.max_steps - 1 : lo);
        hi = hi < 0 ? 0 : (hi > a.max_steps - 1 ? a.max_steps - 1 : hi);
        const float l = a.table[lo * 128 + tid], h = a.table[hi * 128 + tid];
        e0[tid] = l + (h - l) * (t - (float)lo);
    }
    __syncthreads();
    dw_matvec<true>(a.w1, a.b1, e0, h1, 512, 128, wave, lane, 8);
    __syncthreads();
    dw_matvec<true>(a.w2, a.b2, h1, h2, 512, 512, wave, lane, 8);
    __syncthreads();
    dw_matvec<false>(a.wd, a.bd, h2, a.out + (size_t)blockIdx.x * a.NC, a.NC, 512, wave, lane, 8);
}

// ---- tail (diffwave.py:175-178): eps = output_projection(relu(skip_projection(skip / sqrt(N)))), one thread per sample; with `audio`
// set, the sampler update (diffusion_vocoder_inference.py:58-71) on top: audio = clamp(c1 * (audio - c2 * eps) + sigma * noise, -1, 1) ----
struct DwTailArgs {
    const float* skip;    // [B, C, L]
    const float *ws, *bs; // skip_projection [C, C], [C]
    const float *wo, *bo; // output_projection [C], [1]
    float sqrt_n;
    float* eps;           // [B, L] or nullptr
    float* audio;         // [B, L] updated in place, or nullptr
    const float* noise;   // [B, L] or nullptr
    float c1, c2, sigma;
    int L;
    size_t n;             // B * L
};

template <int C>
__global__ __launch_bounds__(256) void dw_tail_kernel(const DwTailArgs a) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const size_t item = i / (size_t)a.L;
    const int t = (int)(i - item * a.L);
    const float* sp = a.skip + item * (size_t)C * a.L + t;
    float s[C];
#pragma unroll
    for (int c = 0; c < C; ++c) s[c] = sp[(size_t)c * a.L] / a.sqrt_n;
    float eps = a.bo[0];
    for (int m = 0; m < C; ++m) {
        const float* w = a.ws + m * C;
        float h = a.bs[m];
#pragma unroll
        for (int c = 0; c < C; ++c) h = fmaf(w[c], s[c], h);
        eps = fmaf(a.wo[m], h > 0.f ? h : 0.f, eps);
    }
    if (a.eps) a.eps[i] = eps;
    if (a.audio) {
        float v = a.c1 * (a.audio[i] - a.c2 * eps);
        if (a.noise) v += a.sigma * a.noise[i];
        a.audio[i] = v < -1.f ? -1.f : (v > 1.f ? 1.f : v);
    }
}

}  // namespace amp

using namespace amp;

struct DwLayer {
    uint4 *wp1 = nullptr, *wp2 = nullptr;
    float *w1f = nullptr, *w2f = nullptr, *b1 = nullptr, *b2 = nullptr;
    float inv1 = 1.f, inv2 = 1.f;
    int d = 1;
};

struct amp_dw {
    amp_dw_desc d{};
    int precision = PREC_F16X3;
    bool finalized = false;
    std::map<std::string, size_t> expected;          // key -> element count
    std::map<std::string, std::vector<float>> w;     // host copies until finalize()
    std::vector<DwLayer> layers;
    DeviceAllocs dev;                                // every device allocation of the handle
    float *table = nullptr, *p1w = nullptr, *p1b = nullptr, *p2w = nullptr, *p2b = nullptr, *wd = nullptr, *bd = nullptr;
    float *up_w[2] = {nullptr, nullptr}, *up_b[2] = {nullptr, nullptr};
    float *in_w = nullptr, *in_b = nullptr, *sk_w = nullptr, *sk_b = nullptr, *out_w = nullptr, *out_b = nullptr;
};

// [rows, cols] fp32 (rows a multiple of 32) -> f16x3 A fragments after a per-matrix 2^s
static int dw_pack(const std::vector<float>& W, int rows, int cols, std::vector<_Float16>* wp, float* inv_scale) {
    return pack_matrix_f16x3("amp_dw_finalize", rows, cols, rows / 32, (cols + 15) / 16, [&](int m, int i) { return W[(size_t)m * cols + i]; }, wp, inv_scale);
}

// shape checks shared by every entry that takes (B, L): refusals come before any launch
static int dw_check_BL(const amp_dw* h, int B, long long L, const char* who) {
    if (!h) { set_error("%s: null handle", who); return AMP_ERR_INVALID; }
    if (!h->finalized) { set_error("%s: amp_dw_finalize has not run", who); return AMP_ERR_STATE; }
    if (B <= 0 || L <= 0) { set_error("%s: bad shape B=%d L=%lld", who, B, L); return AMP_ERR_INVALID; }
    // column indices are formed as int (tile start + 64 + dilation), workgroups as unsigned
    if (L > (1ll << 30) || (long long)B * ((L + DW_TN - 1) / DW_TN) > 0x7fffffffll) {
        set_error("%s: B=%d x L=%lld is beyond the kernels' index arithmetic (L <= 2^30, B * ceil(L / 64) < 2^31)", who, B, L);
        return AMP_ERR_UNSUPPORTED;
    }
    return AMP_OK;
}

static int dw_layer_run(const amp_dw* h, int layer, const float* x, const float* cond, const float* dconst, long long dconst_bs,
                        const float* skip_in, float* x_out, float* skip_out, int B, int L, hipStream_t stream) {
    const DwLayer& ly = h->layers[layer];
    DwLayerArgs a{};
    a.x = x; a.cond = cond; a.dconst = dconst; a.dconst_bs = dconst_bs; a.skip_in = skip_in; a.x_out = x_out; a.skip_out = skip_out;
    a.wp1 = ly.wp1; a.wp2 = ly.wp2; a.w1f = ly.w1f; a.w2f = ly.w2f; a.bias1 = ly.b1; a.bias2 = ly.b2;
    a.C = h->d.residual_channels; a.n_mel = h->d.n_mel; a.L = L; a.d = ly.d;
    a.inv1 = ly.inv1; a.inv2 = ly.inv2;
    const bool f32 = h->precision == PREC_F32;
    a.range_flag = f32 ? nullptr : range_flag_for_current_device();
    AMP_HIP(launch_dw_layer(a, B, f32, stream));
    return AMP_OK;
}

static int dw_embed_run(const amp_dw* h, const float* steps_dev, int S, float step_host, float* out, hipStream_t stream) {
    DwEmbedArgs a{};
    a.steps_dev = steps_dev; a.step_host = step_host; a.table = h->table;
    a.w1 = h->p1w; a.b1 = h->p1b; a.w2 = h->p2w; a.b2 = h->p2b; a.wd = h->wd; a.bd = h->bd;
    a.out = out; a.max_steps = h->d.max_steps; a.NC = h->d.residual_layers * h->d.residual_channels;
    note_kernel("dw_embed_kernel");
    note_work((unsigned)S, 2.0 * S * (128.0 * 512 + 512.0 * 512 + 512.0 * a.NC) / 1e9, 4.0 * (128.0 * 512 + 512.0 * 512 + 512.0 * a.NC) / 1e6,
              "diffwave step embedding S=%d -> [%d, %d]", S, h->d.residual_layers, h->d.residual_channels);
    hipLaunchKernelGGL(dw_embed_kernel, dim3((unsigned)S), dim3(512), 0, stream, a);
    AMP_HIP(hipGetLastError());
    return AMP_OK;
}

static int dw_input_run(const amp_dw* h, const float* audio, int B, int L, float* x, hipStream_t stream) {
    const int C = h->d.residual_channels;
    const size_t n = (size_t)B * C * L;
    const unsigned nb = (unsigned)((n + 255) / 256);
    note_kernel("dw_input_kernel");
    note_work(nb, 2.0 * n / 1e9, 4.0 * ((double)B * L + n) / 1e6, "diffwave input projection 1->%d L=%d B=%d", C, L, B);
    hipLaunchKernelGGL(dw_input_kernel, dim3(nb), dim3(256), 0, stream, audio, h->in_w, h->in_b, x, C, L, n);
    AMP_HIP(hipGetLastError());
    return AMP_OK;
}

static int dw_tail_run(const amp_dw* h, const float* skip, int B, int L, float* eps, float* audio, const float* noise, float c1, float c2,
                       float sigma, hipStream_t stream) {
    const int C = h->d.residual_channels;
    DwTailArgs a{};
    a.skip = skip; a.ws = h->sk_w; a.bs = h->sk_b; a.wo = h->out_w; a.bo = h->out_b;
    a.sqrt_n = (float)sqrt((double)h->d.residual_layers);
    a.eps = eps; a.audio = audio; a.noise = noise; a.c1 = c1; a.c2 = c2; a.sigma = sigma; a.L = L; a.n = (size_t)B * L;
    const unsigned nb = (unsigned)((a.n + 255) / 256);
    note_kernel("dw_tail_kernel", C);
    note_work(nb, (2.0 * C * C + 2.0 * C) * a.n / 1e9, 4.0 * a.n * (C + 1 + (audio ? 2 : 0) + (noise ? 1 : 0)) / 1e6,
              "diffwave tail C=%d L=%d B=%d%s", C, L, B, audio ? " +sampler update" : "");
    switch (C) {
        case 32: hipLaunchKernelGGL(dw_tail_kernel<32>, dim3(nb), dim3(256), 0, stream, a); break;
        case 64: hipLaunchKernelGGL(dw_tail_kernel<64>, dim3(nb), dim3(256), 0, stream, a); break;
        case 96: hipLaunchKernelGGL(dw_tail_kernel<96>, dim3(nb), dim3(256), 0, stream, a); break;
        default: hipLaunchKernelGGL(dw_tail_kernel<128>, dim3(nb), dim3(256), 0, stream, a); break;
    }
    AMP_HIP(hipGetLastError());
    return AMP_OK;
}

// workspace (floats): x ping [B, C, L] | x pong [B, C, L] | skip [B, C, L] | dconst [B, N, C] | up-sampler intermediate [B, n_mel, F * u0]
static size_t dw_ws_floats(const amp_dw* h, int B, int F) {
    const size_t L = (size_t)F * h->d.upsample0 * h->d.upsample1, C = h->d.residual_channels;
    return 3 * (size_t)B * C * L + (size_t)B * h->d.residual_layers * C + (size_t)B * h->d.n_mel * F * h->d.upsample0;
}

// eps (forward) or the in-place sampler update of `audio` (sample_step) from x0 = relu(input_projection(audio))
static int dw_predict(const amp_dw* h, const float* audio_in, const float* steps_dev, int S, float step_host, const float* cond, int B, int F,
                      float* eps, float* audio_upd, const float* noise, float c1, float c2, float sigma, void* ws, size_t ws_bytes,
                      hipStream_t stream, const char* who) {
    const long long L = (long long)F * h->d.upsample0 * h->d.upsample1;
    if (ws_bytes < dw_ws_floats(h, B, F) * sizeof(float)) { set_error("%s: workspace of %zu bytes < amp_dw_workspace_bytes", who, ws_bytes); return AMP_ERR_INVALID; }
    const int C = h->d.residual_channels, N = h->d.residual_layers;
    const size_t n = (size_t)B * C * L;
    float* xa = (float*)ws;
    float* xb = xa + n;
    float* skip = xb + n;
    float* dconst = skip + n;
    if (int rc = dw_embed_run(h, steps_dev, S, step_host, dconst, stream); rc != AMP_OK) return rc;
    if (int rc = dw_input_run(h, audio_in, B, (int)L, xa, stream); rc != AMP_OK) return rc;
    for (int i = 0; i < N; ++i) {
        if (int rc = dw_layer_run(h, i, xa, cond, dconst + (size_t)i * C, S == 1 ? 0 : (long long)N * C, i ? skip : nullptr, xb, skip, B, (int)L, stream);
            rc != AMP_OK)
            return rc;
        std::swap(xa, xb);
    }
    return dw_tail_run(h, skip, B, (int)L, eps, audio_upd, noise, c1, c2, sigma, stream);
}

extern "C" {

int amp_dw_create(const amp_dw_desc* desc, amp_dw** out) {
    if (!desc || !out) { set_error("amp_dw_create: null argument"); return AMP_ERR_INVALID; }
    *out = nullptr;
    const amp_dw_desc& d = *desc;
    if (d.residual_channels <= 0 || d.residual_layers <= 0 || d.dilation_cycle_length <= 0 || d.n_mel <= 0 || d.upsample0 <= 0 ||
        d.upsample1 <= 0 || d.max_steps <= 0) {
        set_error("amp_dw_create: bad descriptor (C=%d N=%d cycle=%d n_mel=%d u=[%d, %d] max_steps=%d)", d.residual_channels, d.residual_layers,
                  d.dilation_cycle_length, d.n_mel, d.upsample0, d.upsample1, d.max_steps);
        return AMP_ERR_INVALID;
    }
    if (d.residual_channels % 32 != 0) {
        set_error("amp_dw_create: residual_channels = %d is not a multiple of 32 (the layer kernel's MFMA row block)", d.residual_channels);
        return AMP_ERR_UNSUPPORTED;
    }
    if (d.residual_channels > 128) { set_error("amp_dw_create: residual_channels = %d > 128 is not covered by the layer kernel", d.residual_channels); return AMP_ERR_UNSUPPORTED; }
    if ((d.upsample0 | d.upsample1) & 1) {
        // an odd factor makes the reference's ConvTranspose2d one column longer than F * u and its `+ conditioner` fail (diffwave.py:117)
        set_error("amp_dw_create: odd upsample factor [%d, %d]", d.upsample0, d.upsample1);
        return AMP_ERR_UNSUPPORTED;
    }
    if (d.dilation_cycle_length > 24) { set_error("amp_dw_create: dilation_cycle_length = %d > 24", d.dilation_cycle_length); return AMP_ERR_UNSUPPORTED; }
    if (dw_layer_lds_bytes(d.residual_channels, d.n_mel, false) > 160 * 1024 || dw_layer_lds_bytes(d.residual_channels, d.n_mel, true) > 160 * 1024) {
        set_error("amp_dw_create: C=%d with n_mel=%d does not fit the layer kernel's 160 KB of LDS", d.residual_channels, d.n_mel);
        return AMP_ERR_UNSUPPORTED;
    }
    if (amp_device_count() <= 0) { set_error("amp_dw_create: no HIP device visible (the HIP path has no CPU fallback)"); return AMP_ERR_HIP; }
    std::unique_ptr<amp_dw> h(new amp_dw);
    h->d = d;
    h->precision = amp_get_precision();
    const size_t C = d.residual_channels;
    auto& ex = h->expected;
    ex["input_projection.weight"] = C;
    ex["input_projection.bias"] = C;
    ex["diffusion_embedding.embedding"] = (size_t)d.max_steps * 128;
    ex["diffusion_embedding.projection1.weight"] = 512 * 128;
    ex["diffusion_embedding.projection1.bias"] = 512;
    ex["diffusion_embedding.projection2.weight"] = 512 * 512;
    ex["diffusion_embedding.projection2.bias"] = 512;
    ex["spectrogram_upsampler.conv1.weight"] = 3 * 2 * (size_t)d.upsample0;
    ex["spectrogram_upsampler.conv1.bias"] = 1;
    ex["spectrogram_upsampler.conv2.weight"] = 3 * 2 * (size_t)d.upsample1;
    ex["spectrogram_upsampler.conv2.bias"] = 1;
    for (int i = 0; i < d.residual_layers; ++i) {
        const std::string p = "residual_layers." + std::to_string(i) + ".";
        ex[p + "dilated_conv.weight"] = 2 * C * C * 3;
        ex[p + "dilated_conv.bias"] = 2 * C;
        ex[p + "diffusion_projection.weight"] = C * 512;
        ex[p + "diffusion_projection.bias"] = C;
        ex[p + "conditioner_projection.weight"] = 2 * C * d.n_mel;
        ex[p + "conditioner_projection.bias"] = 2 * C;
        ex[p + "output_projection.weight"] = 2 * C * C;
        ex[p + "output_projection.bias"] = 2 * C;
    }
    ex["skip_projection.weight"] = C * C;
    ex["skip_projection.bias"] = C;
    ex["output_projection.weight"] = C;
    ex["output_projection.bias"] = 1;
    *out = h.release();
    return AMP_OK;
}

int amp_dw_set_weight(amp_dw* h, const char* key, const float* data_host, long long count) {
    if (!h || !key || !data_host) { set_error("amp_dw_set_weight: null argument"); return AMP_ERR_INVALID; }
    if (h->finalized) { set_error("amp_dw_set_weight: the handle is finalized"); return AMP_ERR_STATE; }
    auto it = h->expected.find(key);
    if (it == h->expected.end()) { set_error("amp_dw_set_weight: unknown key '%s'", key); return AMP_ERR_INVALID; }
    if (count < 0 || (size_t)count != it->second) { set_error("amp_dw_set_weight: '%s' has %lld elements, expected %zu", key, count, it->second); return AMP_ERR_INVALID; }
    for (long long i = 0; i < count; ++i)
        if (!std::isfinite(data_host[i])) { set_error("amp_dw_set_weight: non-finite value in '%s'", key); return AMP_ERR_INVALID; }
    h->w[key].assign(data_host, data_host + count);
    return AMP_OK;
}

int amp_dw_finalize(amp_dw* h) {
    if (!h) { set_error("amp_dw_finalize: null handle"); return AMP_ERR_INVALID; }
    if (h->finalized) return AMP_OK;
    for (const auto& kv : h->expected)
        if (!h->w.count(kv.first)) { set_error("amp_dw_finalize: missing weight '%s'", kv.first.c_str()); return AMP_ERR_MISSING_WEIGHT; }
    const int C = h->d.residual_channels, N = h->d.residual_layers, M = h->d.n_mel, K = 3 * C + M;
    auto up = [&](const std::string& key, float** dst) { return h->dev.upload(h->w[key], dst); };
#define DW_UP(key, dst) if (int rc = up(key, dst); rc != AMP_OK) return rc
    DW_UP("input_projection.weight", &h->in_w);
    DW_UP("input_projection.bias", &h->in_b);
    DW_UP("diffusion_embedding.embedding", &h->table);
    DW_UP("diffusion_embedding.projection1.weight", &h->p1w);
    DW_UP("diffusion_embedding.projection1.bias", &h->p1b);
    DW_UP("diffusion_embedding.projection2.weight", &h->p2w);
    DW_UP("diffusion_embedding.projection2.bias", &h->p2b);
    DW_UP("spectrogram_upsampler.conv1.weight", &h->up_w[0]);
    DW_UP("spectrogram_upsampler.conv1.bias", &h->up_b[0]);
    DW_UP("spectrogram_upsampler.conv2.weight", &h->up_w[1]);
    DW_UP("spectrogram_upsampler.conv2.bias", &h->up_b[1]);
    DW_UP("skip_projection.weight", &h->sk_w);
    DW_UP("skip_projection.bias", &h->sk_b);
    DW_UP("output_projection.weight", &h->out_w);
    DW_UP("output_projection.bias", &h->out_b);
#undef DW_UP
    std::vector<float> wd((size_t)N * C * 512), bd((size_t)N * C);
    h->layers.resize(N);
    for (int i = 0; i < N; ++i) {
        const std::string p = "residual_layers." + std::to_string(i) + ".";
        DwLayer& ly = h->layers[i];
        ly.d = 1 << (i % h->d.dilation_cycle_length);
        const std::vector<float>&wc = h->w[p + "dilated_conv.weight"], &wm = h->w[p + "conditioner_projection.weight"];
        // [2C, 3C + n_mel]: column tap * C + c is dilated_conv.weight[m, c, tap] (tap reads t + (tap - 1) d), then the conditioner
        std::vector<float> W1((size_t)2 * C * K);
        for (int m = 0; m < 2 * C; ++m) {
            for (int tap = 0; tap < 3; ++tap)
                for (int c = 0; c < C; ++c) W1[(size_t)m * K + tap * C + c] = wc[((size_t)m * C + c) * 3 + tap];
            for (int j = 0; j < M; ++j) W1[(size_t)m * K + 3 * C + j] = wm[(size_t)m * M + j];
        }
        const std::vector<float>& W2 = h->w[p + "output_projection.weight"];
        std::vector<float> b1(h->w[p + "dilated_conv.bias"]);
        const std::vector<float>& bc = h->w[p + "conditioner_projection.bias"];
        for (int m = 0; m < 2 * C; ++m) b1[m] += bc[m];
        AMP_RC(h->dev.upload(b1, &ly.b1));
        AMP_RC(up(p + "output_projection.bias", &ly.b2));
        // both arithmetics are uploaded: amp_dw_set_precision switches a finalized handle (the sampler's exact-fp32 repeat)
        AMP_RC(h->dev.upload(W1, &ly.w1f));
        AMP_RC(h->dev.upload(W2, &ly.w2f));
        std::vector<_Float16> p1, p2;
        AMP_RC(dw_pack(W1, 2 * C, K, &p1, &ly.inv1));
        AMP_RC(dw_pack(W2, 2 * C, C, &p2, &ly.inv2));
        AMP_RC(h->dev.upload(p1, &ly.wp1));
        AMP_RC(h->dev.upload(p2, &ly.wp2));
        std::copy(h->w[p + "diffusion_projection.weight"].begin(), h->w[p + "diffusion_projection.weight"].end(), wd.begin() + (size_t)i * C * 512);
        std::copy(h->w[p + "diffusion_projection.bias"].begin(), h->w[p + "diffusion_projection.bias"].end(), bd.begin() + (size_t)i * C);
    }
    AMP_RC(h->dev.upload(wd, &h->wd));
    AMP_RC(h->dev.upload(bd, &h->bd));
    h->w.clear();
    h->finalized = true;
    return AMP_OK;
}

int amp_dw_precision(const amp_dw* h) { return h ? h->precision : -1; }

int amp_dw_set_precision(amp_dw* h, int precision) {
    if (!h || (precision != AMP_PRECISION_F32 && precision != AMP_PRECISION_F16X3)) { set_error("amp_dw_set_precision: bad argument"); return AMP_ERR_INVALID; }
    h->precision = precision;
    return AMP_OK;
}

size_t amp_dw_workspace_bytes(const amp_dw* h, int B, int F) {
    if (!h || B <= 0 || F <= 0) return 0;
    return dw_ws_floats(h, B, F) * sizeof(float);
}

int amp_dw_condition(const amp_dw* h, const float* mel_dev, int B, int F, float* cond_dev, void* ws_dev, size_t ws_bytes, void* stream_) {
    if (!h) { set_error("amp_dw_condition: null handle"); return AMP_ERR_INVALID; }
    const long long L = (long long)F * h->d.upsample0 * h->d.upsample1;
    if (int rc = dw_check_BL(h, B, F > 0 ? L : 0, "amp_dw_condition"); rc != AMP_OK) return rc;
    if (!mel_dev || !cond_dev || !ws_dev) { set_error("amp_dw_condition: null pointer"); return AMP_ERR_INVALID; }
    if (ws_bytes < dw_ws_floats(h, B, F) * sizeof(float)) { set_error("amp_dw_condition: workspace of %zu bytes < amp_dw_workspace_bytes", ws_bytes); return AMP_ERR_INVALID; }
    hipStream_t stream = (hipStream_t)stream_;
    const int M = h->d.n_mel, u0 = h->d.upsample0, u1 = h->d.upsample1;
    float* mid = (float*)ws_dev + 3 * (size_t)B * h->d.residual_channels * L + (size_t)B * h->d.residual_layers * h->d.residual_channels;
    const size_t n0 = (size_t)B * M * F * u0, n1 = (size_t)B * M * L;
    note_kernel("dw_upsample_kernel");
    note_work((n0 + 255) / 256, 12.0 * n0 / 1e9, 4.0 * ((double)B * M * F + n0) / 1e6, "diffwave upsampler x%d F=%d B=%d", u0, F, B);
    hipLaunchKernelGGL(dw_upsample_kernel, dim3((unsigned)((n0 + 255) / 256)), dim3(256), 0, stream, mel_dev, mid, h->up_w[0], h->up_b[0], M, F, u0, n0);
    AMP_HIP(hipGetLastError());
    note_kernel("dw_upsample_kernel");
    note_work((n1 + 255) / 256, 12.0 * n1 / 1e9, 4.0 * ((double)n0 + n1) / 1e6, "diffwave upsampler x%d F=%d B=%d", u1, F * u0, B);
    hipLaunchKernelGGL(dw_upsample_kernel, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, stream, mid, cond_dev, h->up_w[1], h->up_b[1], M, F * u0, u1, n1);
    AMP_HIP(hipGetLastError());
    return AMP_OK;
}

int amp_dw_embed(const amp_dw* h, const float* steps_dev, int n_steps, float* dconst_dev, void* stream_) {
    if (!h || !h->finalized || !steps_dev || !dconst_dev || n_steps <= 0) { set_error("amp_dw_embed: bad argument"); return AMP_ERR_INVALID; }
    return dw_embed_run(h, steps_dev, n_steps, 0.f, dconst_dev, (hipStream_t)stream_);
}

int amp_dw_input(const amp_dw* h, const float* audio_dev, int B, int L, float* x_dev, void* stream_) {
    if (int rc = dw_check_BL(h, B, L, "amp_dw_input"); rc != AMP_OK) return rc;
    if (!audio_dev || !x_dev) { set_error("amp_dw_input: null pointer"); return AMP_ERR_INVALID; }
    return dw_input_run(h, audio_dev, B, L, x_dev, (hipStream_t)stream_);
}

int amp_dw_layer(const amp_dw* h, int layer, const float* x_dev, const float* cond_dev, const float* dconst_dev, long long dconst_batch_stride,
                 const float* skip_in_dev, float* x_out_dev, float* skip_out_dev, int B, int L, void* stream_) {
    if (int rc = dw_check_BL(h, B, L, "amp_dw_layer"); rc != AMP_OK) return rc;
    if (layer < 0 || layer >= h->d.residual_layers) { set_error("amp_dw_layer: layer %d of %d", layer, h->d.residual_layers); return AMP_ERR_INVALID; }
    if (!x_dev || !cond_dev || !dconst_dev || !x_out_dev || !skip_out_dev || dconst_batch_stride < 0) { set_error("amp_dw_layer: bad argument"); return AMP_ERR_INVALID; }
    const size_t bytes = (size_t)B * h->d.residual_channels * L * sizeof(float);
    if (ranges_overlap(x_dev, bytes, x_out_dev, bytes)) {
        set_error("amp_dw_layer: x_out must not overlap x (other tiles read x at +- the dilation): ping-pong two buffers");
        return AMP_ERR_INVALID;
    }
    if (ranges_overlap(skip_out_dev, bytes, x_dev, bytes) || ranges_overlap(skip_out_dev, bytes, x_out_dev, bytes)) { set_error("amp_dw_layer: skip_out overlaps x or x_out"); return AMP_ERR_INVALID; }
    if (skip_in_dev && skip_in_dev != skip_out_dev && ranges_overlap(skip_in_dev, bytes, skip_out_dev, bytes)) { set_error("amp_dw_layer: skip_in must be skip_out or not overlap it"); return AMP_ERR_INVALID; }
    return dw_layer_run(h, layer, x_dev, cond_dev, dconst_dev, dconst_batch_stride, skip_in_dev, x_out_dev, skip_out_dev, B, L, (hipStream_t)stream_);
}

int amp_dw_tail(const amp_dw* h, const float* skip_dev, int B, int L, float* eps_dev, void* stream_) {
    if (int rc = dw_check_BL(h, B, L, "amp_dw_tail"); rc != AMP_OK) return rc;
    if (!skip_dev || !eps_dev) { set_error("amp_dw_tail: null pointer"); return AMP_ERR_INVALID; }
    return dw_tail_run(h, skip_dev, B, L, eps_dev, nullptr, nullptr, 0.f, 0.f, 0.f, (hipStream_t)stream_);
}

int amp_dw_forward(const amp_dw* h, const float* audio_dev, int L, const float* steps_dev, int n_steps, const float* cond_dev, int B, int F,
                   float* eps_dev, void* ws_dev, size_t ws_bytes, void* stream_) {
    if (int rc = dw_check_BL(h, B, L, "amp_dw_forward"); rc != AMP_OK) return rc;
    if (F <= 0 || (long long)F * h->d.upsample0 * h->d.upsample1 != L) {
        set_error("amp_dw_forward: audio length %d != frames %d x upsample %d x %d", L, F, h->d.upsample0, h->d.upsample1);
        return AMP_ERR_INVALID;
    }
    if (!audio_dev || !steps_dev || !cond_dev || !eps_dev || !ws_dev) { set_error("amp_dw_forward: null pointer"); return AMP_ERR_INVALID; }
    if (n_steps != 1 && n_steps != B) { set_error("amp_dw_forward: %d diffusion steps for a batch of %d (1 or B)", n_steps, B); return AMP_ERR_INVALID; }
    return dw_predict(h, audio_dev, steps_dev, n_steps, 0.f, cond_dev, B, F, eps_dev, nullptr, nullptr, 0.f, 0.f, 0.f, ws_dev, ws_bytes,
                      (hipStream_t)stream_, "amp_dw_forward");
}

int amp_dw_sample_step(const amp_dw* h, float* audio_dev, int L, float step, float c1, float c2, float sigma, const float* noise_dev,
                       const float* cond_dev, int B, int F, void* ws_dev, size_t ws_bytes, void* stream_) {
    if (int rc = dw_check_BL(h, B, L, "amp_dw_sample_step"); rc != AMP_OK) return rc;
    if (F <= 0 || (long long)F * h->d.upsample0 * h->d.upsample1 != L) {
        set_error("amp_dw_sample_step: audio length %d != frames %d x upsample %d x %d", L, F, h->d.upsample0, h->d.upsample1);
        return AMP_ERR_INVALID;
    }
    if (!audio_dev || !cond_dev || !ws_dev) { set_error("amp_dw_sample_step: null pointer"); return AMP_ERR_INVALID; }
    if (!(step >= 0.f && step <= (float)(h->d.max_steps - 1))) { set_error("amp_dw_sample_step: step %g outside [0, %d]", (double)step, h->d.max_steps - 1); return AMP_ERR_INVALID; }
    return dw_predict(h, audio_dev, nullptr, 1, step, cond_dev, B, F, nullptr, audio_dev, noise_dev, c1, c2, sigma, ws_dev, ws_bytes,
                      (hipStream_t)stream_, "amp_dw_sample_step");
}

void amp_dw_destroy(amp_dw* h) { delete h; }

}  // extern "C"
