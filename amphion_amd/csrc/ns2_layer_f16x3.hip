// One residual layer of NaturalSpeech2's WaveNet (models/tts/naturalspeech2/wavenet.py:96-127, ResidualBlock.forward with x_mask = None) at
// hidden sizes the whole-K kernels (dw_layer_f16x3.hip: C <= 128, conv_small_f16x3.hip's gate: H <= 256) do not reach:
//     y     = x + dconst[b, :]                          (diffusion_proj(step embedding): one row per item)
//     a     = dilated_conv_k3(y) + bias + cterm         (ZERO padding of y; cterm = cond_proj(cond_ln(cond)) with its bias, step-invariant)
//     a     = a * gain + fbias                          (FiLM, layers with cross-attention only; gain | fbias = rows [0, 2H) | [2H, 4H) of one tensor)
//     z     = sigmoid(a[:H]) * tanh(a[H:])
//     r     = out_proj(z)                               (H -> 2H, k = 1)
//     x_out = (x + r[:H]) / sqrt(2),   skip_out = skip_in + r[H:]
// in TWO launches.  Launch 1, ns2_gate_f16x3_kernel: a workgroup owns 64 columns of one item and a slab of NL_SLAB gate row
// blocks with their filter row blocks; K = 3H streams through two LDS buffers in chunks of 64 channels of ONE tap (H is a multiple of 64,
// so a chunk never straddles taps; the tap's columns t + (tap - 1) d are staged separately, as dw_layer_f16x3.hip does: the dilation never
// enters a halo).  The [2H, T] pre-activation stays in the accumulators: + bias + cterm, FiLM and the gate are formed in registers and
// z [B, H, T] is stored.  Launch 2 is the pointwise GEMM (pw_f16x3.hip) with its residual | skip epilogue.
// Layouts, wave grid (2 x 2: wave (wm, wn) owns columns 32 wn .. 32 wn + 31) and arithmetic: wholek_f16x3.h / f16x3_device.h.
// Deterministic: one workgroup forms each output's full-K sum in a fixed order; no atomics except the range flag; a batch item never
// depends on what it is batched with.  Under AMP_PRECISION_F32 the layer is the exact conv (conv_mfma.hip) between element-wise launches.
#include <memory>

#include "amp_host.h"
#include "wholek_f16x3.h"

namespace amp {

constexpr int NL_TN = 64;     // columns per workgroup
constexpr int NL_KS = 4;      // MFMA k-extents (16 channels each) per K chunk
constexpr int NL_KC = 16 * NL_KS;
constexpr int NL_SLAB = 4;    // gate row blocks per workgroup: two per wave row (with their filter blocks: 64 accumulator registers)
constexpr int NL_NPW = NL_SLAB / 2;

struct Ns2GateArgs {
    const float* x;            // [B, H, T]
    const float* dconst;       // [H] per item, dconst_bs apart (0: one row for the batch)
    long long dconst_bs;
    const float* cterm;        // [B, 2H, T], rows T apart, items cterm_bs apart
    long long cterm_bs;
    const float* film;         // [B, 4H, T] dense: gain rows [0, 2H), bias rows [2H, 4H); or nullptr
    const uint4* wp1;          // [2H, 3H] (K index = tap * H + channel) as packed A fragments
    const float* bias1;        // [2H]
    float* z;                  // [B, H, T]
    int H, T, d;
    int K16;                   // 3H / 16
    int tiles_per_item;
    float inv1;
    unsigned* range_flag;
};

__global__ __launch_bounds__(256, 2) void ns2_gate_f16x3_kernel(const Ns2GateArgs a) {
    constexpr int TN = NL_TN;
    constexpr int PLANE = 2 * NL_KS * TN;       // uint4 per plane: [channel octet][TN]
    constexpr int BUF = 2 * PLANE;              // uint4 per buffer: [plane hi | lo]
    constexpr int NST = (4 * NL_KS * TN) / 256; // staging items (channel quad x column) per thread
    __shared__ __attribute__((aligned(16))) uint4 nl_smem[2 * BUF];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int hi = lane >> 5, l31 = lane & 31;
    const int item = blockIdx.x / a.tiles_per_item;
    const int q0 = (blockIdx.x - item * a.tiles_per_item) * TN;
    const int H = a.H, T = a.T, d = a.d, K16 = a.K16;
    const int NP = H >> 5;
    const int nsteps = (3 * H) / NL_KC;

    const float* xb = a.x + (size_t)item * H * T;
    const float* dc = a.dconst + (size_t)item * (size_t)a.dconst_bs;

    // ---- staging: item (quad qd = 4 it + wave, column lane) of chunk s holds K indices 64 s + 4 qd .. + 3 = channels c0 .. c0 + 3 of ONE tap ----
    float range_max = 0.f;
    float xs[NST][4], ds[NST][4];
    auto stage_load = [&](int s) {
        const int k0 = s * NL_KC;
        const int tap = k0 / H;
        const int cb = k0 - tap * H;
        const int t = q0 + lane + (tap - 1) * d;
        const int tc = t < 0 ? 0 : (t > T - 1 ? T - 1 : t);
#pragma unroll
        for (int it = 0; it < NST; ++it) {
            const int c0 = cb + 4 * (4 * it + wave);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                xs[it][e] = xb[(size_t)(c0 + e) * T + tc];
                ds[it][e] = dc[c0 + e];
            }
        }
    };
    auto stage_store = [&](int s, int buf) {
        const int tap = (s * NL_KC) / H;
        const int t = q0 + lane + (tap - 1) * d;
        const bool ok = t >= 0 && t < T;
        uint2* dst = reinterpret_cast<uint2*>(nl_smem + buf * BUF);
#pragma unroll
        for (int it = 0; it < NST; ++it) {
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = ok ? xs[it][e] + ds[it][e] : 0.f;      // the conv pads y, not x: a tap outside [0, T) contributes 0
            uint2 fh, fl;
            stage4_f16(v[0], v[1], v[2], v[3], 16.f, 16.f, range_max, fh, fl);
            bplane_store(dst, 2 * PLANE, bplane_idx(4 * it + wave, lane, TN), fh, fl);
        }
    };

    // ---- the wave's gate / filter row-block pairs: p = slab * NL_SLAB + wm + 2 pi (gate block p, filter block NP + p) ----
    f32x16 acc[NL_NPW][2][1];
    Frag ah[NL_NPW][2], al[NL_NPW][2];
    const size_t mbs = (size_t)NP * K16 * 128;
#pragma unroll
    for (int pi = 0; pi < NL_NPW; ++pi) {
        acc_zero(acc[pi][0][0]);
        acc_zero(acc[pi][1][0]);
        const int p = blockIdx.y * NL_SLAB + wm + 2 * pi;
        if (p < NP) afrag_load<2>(ah[pi], al[pi], a.wp1 + (size_t)p * K16 * 128 + lane, mbs);
    }

    stage_load(0);
    AMP_PIN_VMEM();
    stage_store(0, 0);
    __syncthreads();

    const int rd0 = hi * TN + wn * 32 + l31;
    for (int s = 0; s < nsteps; ++s) {
        const bool more = s + 1 < nsteps;
        if (more) {
            stage_load(s + 1);
            AMP_PIN_VMEM();
        }
        const uint4* buf = nl_smem + (s & 1) * BUF;
#pragma unroll
        for (int pi = 0; pi < NL_NPW; ++pi) {
            const int p = blockIdx.y * NL_SLAB + wm + 2 * pi;
            if (p < NP) {
                const APack A{a.wp1 + (size_t)p * K16 * 128 + lane, mbs, K16};
                gemm_wholek<2, true>(acc[pi], ah[pi], al[pi], A, s * NL_KS, NL_KS, buf, PLANE, TN, rd0);
            }
        }
        if (more) stage_store(s + 1, (s + 1) & 1);
        __syncthreads();
    }
    raise_range(a.range_flag, range_max, lane);

    // ---- + bias + cterm, FiLM, gate: lane (hi, l31), register r of pair pi holds rows acc_row(r, hi, 32 p) and H + that, column q ----
    const int q = q0 + wn * 32 + l31;
    if (q >= T) return;
    const float* ct = a.cterm + (size_t)item * (size_t)a.cterm_bs + q;
    const float* fm = a.film ? a.film + (size_t)item * 4 * H * T + q : nullptr;
    float* zb = a.z + (size_t)item * H * T + q;
#pragma unroll
    for (int pi = 0; pi < NL_NPW; ++pi) {
        const int p = blockIdx.y * NL_SLAB + wm + 2 * pi;
        if (p >= NP) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = acc_row(r, hi, p * 32);
            float g = acc[pi][0][0][r] * a.inv1 + a.bias1[m] + ct[(size_t)m * T];
            float f = acc[pi][1][0][r] * a.inv1 + a.bias1[H + m] + ct[(size_t)(H + m) * T];
            if (fm) {
                g = g * fm[(size_t)m * T] + fm[(size_t)(2 * H + m) * T];
                f = f * fm[(size_t)(H + m) * T] + fm[(size_t)(3 * H + m) * T];
            }
            zb[(size_t)m * T] = (1.f / (1.f + expf(-g))) * tanhf(f);
        }
    }
}

// ---- the exact-fp32 form's element-wise launches (not meant to be fast) ----
__global__ __launch_bounds__(256) void ns2_add_dconst_kernel(const float* __restrict__ x, const float* __restrict__ dc, long long dbs, float* __restrict__ y,
                                                             int H, int T) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const size_t o = ((size_t)blockIdx.z * H + blockIdx.y) * T + t;
    y[o] = x[o] + dc[(size_t)blockIdx.z * (size_t)dbs + blockIdx.y];
}

__global__ __launch_bounds__(256) void ns2_gate_f32_kernel(const float* __restrict__ pre, const float* __restrict__ cterm, long long cbs,
                                                           const float* __restrict__ film, float* __restrict__ z, int H, int T) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const int c = blockIdx.y, b = blockIdx.z;
    const float* ab = pre + (size_t)b * 2 * H * T + t;
    const float* ct = cterm + (size_t)b * (size_t)cbs + t;
    float g = ab[(size_t)c * T] + ct[(size_t)c * T];
    float f = ab[(size_t)(H + c) * T] + ct[(size_t)(H + c) * T];
    if (film) {
        const float* fm = film + (size_t)b * 4 * H * T + t;
        g = g * fm[(size_t)c * T] + fm[(size_t)(2 * H + c) * T];
        f = f * fm[(size_t)(H + c) * T] + fm[(size_t)(3 * H + c) * T];
    }
    z[((size_t)b * H + c) * T + t] = (1.f / (1.f + expf(-g))) * tanhf(f);
}

__global__ __launch_bounds__(256) void ns2_res_skip_kernel(const float* __restrict__ r, const float* x, const float* skip_in, float* x_out,
                                                           float* skip_out, int H, int T) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const int c = blockIdx.y, b = blockIdx.z;
    const float* rb = r + (size_t)b * 2 * H * T + t;
    const size_t o = ((size_t)b * H + c) * T + t;
    const float sqrt2 = 1.41421356237309504880f;
    x_out[o] = (x[o] + rb[(size_t)c * T]) / sqrt2;
    const float s = rb[(size_t)(H + c) * T];
    skip_out[o] = skip_in ? skip_in[o] + s : s;
}

// pw_f16x3.hip: z [B, H, T] -> out_proj with the residual | skip epilogue (f16x3 handles only)
int pw_run_res_skip(const amp_pw* p, const float* z_dev, int B, int T, const float* x_dev, const float* skip_in_dev, float* x_out_dev,
                    float* skip_out_dev, hipStream_t stream);

}  // namespace amp

using namespace amp;

struct amp_ns2_layer {
    int H = 0, d = 0;
    int precision = PREC_F16X3;
    // f16x3
    DeviceAllocs mem;
    uint4* wp1 = nullptr;
    float* bias1 = nullptr;
    float inv1 = 1.f;
    amp_pw* out = nullptr;       // out_proj: the pointwise GEMM handle (f16x3) or its k = 1 conv (f32)
    // f32
    amp_conv* conv = nullptr;    // the dilated conv with its bias
    ~amp_ns2_layer() {
        amp_pw_destroy(out);
        delete conv;
    }
};

extern "C" {

int amp_ns2_layer_create(int hidden, int dilation, const float* conv_weight_host, const float* conv_bias_host, const float* out_weight_host,
                         const float* out_bias_host, amp_ns2_layer** out) {
    if (!out || !conv_weight_host || !out_weight_host) { set_error("amp_ns2_layer_create: null argument"); return AMP_ERR_INVALID; }
    *out = nullptr;
    if (hidden < 128 || hidden > 512 || hidden % 64) {
        set_error("amp_ns2_layer_create: hidden=%d is not covered (a multiple of 64 in [128, 512])", hidden);
        return AMP_ERR_UNSUPPORTED;
    }
    if (dilation < 1 || dilation > 8) { set_error("amp_ns2_layer_create: dilation=%d is not covered (1 .. 8)", dilation); return AMP_ERR_UNSUPPORTED; }
    if (amp_device_count() <= 0) { set_error("amp_ns2_layer_create: no HIP device visible (the HIP path has no CPU fallback)"); return AMP_ERR_HIP; }
    const int H = hidden;
    std::unique_ptr<amp_ns2_layer> h(new amp_ns2_layer);
    h->H = H;
    h->d = dilation;
    h->precision = amp_get_precision();
    AMP_RC(amp_pw_create(H, 2 * H, out_weight_host, out_bias_host, &h->out));
    if (h->precision == PREC_F32) {
        h->conv = new amp_conv;
        h->conv->cin = H; h->conv->cout = 2 * H; h->conv->k = 3; h->conv->dilation = dilation; h->conv->padding = dilation;
        std::vector<float> bias((size_t)2 * H, 0.f);
        if (conv_bias_host) std::copy(conv_bias_host, conv_bias_host + 2 * H, bias.begin());
        AMP_RC(conv_build(h->conv, conv_weight_host, bias.data()));
    } else {
        std::vector<_Float16> wp;
        // K index = tap * H + channel of the Conv1d weight [2H, H, 3]
        AMP_RC(pack_matrix_f16x3("amp_ns2_layer_create", 2 * H, 3 * H, 2 * H / 32, 3 * H / 16,
                                 [&](int m, int i) { return conv_weight_host[((size_t)m * H + (i % H)) * 3 + i / H]; }, &wp, &h->inv1));
        AMP_RC(h->mem.upload(wp, &h->wp1));
        std::vector<float> bias((size_t)2 * H, 0.f);
        if (conv_bias_host) std::copy(conv_bias_host, conv_bias_host + 2 * H, bias.begin());
        AMP_RC(h->mem.upload(bias, &h->bias1));
    }
    *out = h.release();
    return AMP_OK;
}

int amp_ns2_layer_precision(const amp_ns2_layer* h) { return h ? h->precision : -1; }

size_t amp_ns2_layer_workspace_bytes(const amp_ns2_layer* h, int B, int T) {
    if (!h || B < 1 || T < 1) return 0;
    return (size_t)(h->precision == PREC_F32 ? 4 : 1) * B * h->H * T * sizeof(float);
}

int amp_ns2_layer_forward(const amp_ns2_layer* h, const float* x_dev, const float* dconst_dev, long long dconst_batch_stride, const float* cterm_dev,
                          long long cterm_batch_stride, const float* film_dev, const float* skip_in_dev, int B, int T, float* x_out_dev,
                          float* skip_out_dev, void* ws_dev, size_t ws_bytes, void* stream_) {
    if (!h || !x_dev || !dconst_dev || !cterm_dev || !x_out_dev || !skip_out_dev || !ws_dev) { set_error("amp_ns2_layer_forward: null argument"); return AMP_ERR_INVALID; }
    if (B < 1 || T < 1 || B > 65535) { set_error("amp_ns2_layer_forward: B=%d T=%d", B, T); return AMP_ERR_INVALID; }
    const int H = h->H;
    if ((long long)B * ((T + NL_TN - 1) / NL_TN) > 0x7fffffffll || (long long)2 * H * T > 0x7fffffffll) {
        set_error("amp_ns2_layer_forward: B=%d T=%d is beyond the grid", B, T);
        return AMP_ERR_UNSUPPORTED;
    }
    if (dconst_batch_stride != 0 && dconst_batch_stride < H) { set_error("amp_ns2_layer_forward: dconst batch stride %lld < H", dconst_batch_stride); return AMP_ERR_INVALID; }
    if (cterm_batch_stride == 0) cterm_batch_stride = (long long)2 * H * T;
    if (cterm_batch_stride < (long long)2 * H * T) { set_error("amp_ns2_layer_forward: cterm batch stride %lld < 2*H*T", cterm_batch_stride); return AMP_ERR_INVALID; }
    if (ws_bytes < amp_ns2_layer_workspace_bytes(h, B, T)) {
        set_error("amp_ns2_layer_forward: workspace of %zu bytes, %zu needed", ws_bytes, amp_ns2_layer_workspace_bytes(h, B, T));
        return AMP_ERR_INVALID;
    }
    const size_t n = (size_t)B * H * T, bytes = n * sizeof(float);
    const size_t wsn = amp_ns2_layer_workspace_bytes(h, B, T);
    if (x_out_dev != x_dev && ranges_overlap(x_out_dev, bytes, x_dev, bytes)) { set_error("amp_ns2_layer_forward: x_out must be x or not overlap it"); return AMP_ERR_INVALID; }
    if (ranges_overlap(skip_out_dev, bytes, x_dev, bytes) || ranges_overlap(skip_out_dev, bytes, x_out_dev, bytes)) {
        set_error("amp_ns2_layer_forward: skip_out overlaps x or x_out");
        return AMP_ERR_INVALID;
    }
    if (skip_in_dev && skip_in_dev != skip_out_dev && ranges_overlap(skip_in_dev, bytes, skip_out_dev, bytes)) {
        set_error("amp_ns2_layer_forward: skip_in must be skip_out or not overlap it");
        return AMP_ERR_INVALID;
    }
    for (const void* p : {(const void*)x_dev, (const void*)x_out_dev, (const void*)skip_out_dev, (const void*)skip_in_dev})
        if (p && ranges_overlap(ws_dev, wsn, p, bytes)) { set_error("amp_ns2_layer_forward: the workspace overlaps a tensor"); return AMP_ERR_INVALID; }
    hipStream_t stream = (hipStream_t)stream_;
    float* ws = (float*)ws_dev;
    const dim3 egrid((unsigned)((T + 255) / 256), (unsigned)H, (unsigned)B);
    const double samples = (double)B * T;
    if (h->precision == PREC_F32) {
        float* y = ws;
        float* pre = ws + n;            // [B, 2H, T]: the conv's output, later out_proj's
        float* z = ws + 3 * n;
        note_kernel("ns2_add_dconst_kernel");
        note_work((unsigned long long)egrid.x * H * B, 0.0, 8.0 * n / 1e6, "ns2 layer f32: x + dconst H=%d T=%d B=%d", H, T, B);
        hipLaunchKernelGGL(ns2_add_dconst_kernel, egrid, dim3(256), 0, stream, x_dev, dconst_dev, dconst_batch_stride, y, H, T);
        AMP_HIP(hipGetLastError());
        AMP_RC(conv_run(h->conv, y, B, T, 1.f, nullptr, 1.f, pre, 0, 1.f, stream));
        note_kernel("ns2_gate_f32_kernel");
        note_work((unsigned long long)egrid.x * H * B, 0.0, 4.0 * n * (film_dev ? 9 : 5) / 1e6, "ns2 layer f32: gate H=%d T=%d B=%d film=%d", H, T, B, film_dev ? 1 : 0);
        hipLaunchKernelGGL(ns2_gate_f32_kernel, egrid, dim3(256), 0, stream, pre, cterm_dev, cterm_batch_stride, film_dev, z, H, T);
        AMP_HIP(hipGetLastError());
        AMP_RC(conv_run(h->out->conv, z, B, T, 1.f, nullptr, 1.f, pre, 0, 1.f, stream));
        note_kernel("ns2_res_skip_kernel");
        note_work((unsigned long long)egrid.x * H * B, 0.0, 4.0 * n * (skip_in_dev ? 6 : 5) / 1e6, "ns2 layer f32: residual | skip H=%d T=%d B=%d", H, T, B);
        hipLaunchKernelGGL(ns2_res_skip_kernel, egrid, dim3(256), 0, stream, pre, x_dev, skip_in_dev, x_out_dev, skip_out_dev, H, T);
        AMP_HIP(hipGetLastError());
        return AMP_OK;
    }
    Ns2GateArgs a{};
    a.x = x_dev;
    a.dconst = dconst_dev; a.dconst_bs = dconst_batch_stride;
    a.cterm = cterm_dev; a.cterm_bs = cterm_batch_stride;
    a.film = film_dev;
    a.wp1 = h->wp1; a.bias1 = h->bias1;
    a.z = ws;
    a.H = H; a.T = T; a.d = h->d;
    a.K16 = 3 * H / 16;
    a.tiles_per_item = (T + NL_TN - 1) / NL_TN;
    a.inv1 = h->inv1;
    a.range_flag = range_flag_for_current_device();
    const int NP = H / 32;
    const dim3 grid((unsigned)(B * a.tiles_per_item), (unsigned)((NP + NL_SLAB - 1) / NL_SLAB));
    note_kernel("ns2_gate_f16x3_kernel");
    note_work((unsigned long long)grid.x * grid.y, 2.0 * 3 * H * 2 * H * samples / 1e9, 4.0 * samples * (H * grid.y + 2 * H + (film_dev ? 4 * H : 0) + H) / 1e6,
              "ns2 layer gate H=%d d=%d T=%d B=%d film=%d", H, h->d, T, B, film_dev ? 1 : 0);
    hipLaunchKernelGGL(ns2_gate_f16x3_kernel, grid, dim3(256), 0, stream, a);
    AMP_HIP(hipGetLastError());
    return pw_run_res_skip(h->out, ws, B, T, x_dev, skip_in_dev, x_out_dev, skip_out_dev, stream);
}

void amp_ns2_layer_destroy(amp_ns2_layer* h) { delete h; }

}  // extern "C"
