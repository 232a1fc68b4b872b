// Host side of the Amphion codec encoder's building blocks (models/codec/amphion_codec/codec.py:60-143): the residual-unit handle
// (amp_codec_unit_*: the fused kernel of codec_unit_f16x3.hip where it is built, else the four launches it replaces) and the strided
// down-sampling conv (amp_sconv_*: Snake + space-to-depth in one small kernel, then a k = 2 conv on the implicit-GEMM kernels); and of the
// decoder blocks' up-sampling step (amp_tconv_*: Snake + ConvTranspose1d(k = 2 s, stride s) as the fused kernel of tconv_f16x3.hip where it is
// built, else amp_snake -> the polyphase transposed conv); and of FACodec's residual unit (amp_aa_unit_*: the same unit with Activation1d in
// place of Snake1d, the fused kernel of aa_unit_f16x3.hip where it is built, else act1d -> conv -> act1d -> conv).
#include <memory>

#include "act1d_math.h"
#include "amp_host.h"

namespace amp {

// EncoderBlock's Snake1d -> Conv1d(C, 2C, k = 2s, stride s, padding p) (codec.py:86-93) as a stride-1 conv: with xp the zero-padded
// activation, y[o, t] = sum_{c, a < 2, r < s} w[o, c, a s + r] xp[c, (t + a) s + r], so X'[c s + r, u] = xp[c, u s + r] (u <= T_out) turns it
// into a k = 2 conv over C s channels with w'[o, c s + r, a] = w[o, c, a s + r].  This kernel writes X' and applies the activation on the way;
// the conv pads its INPUT, i.e. the activation's output: positions outside [0, T) are 0, not snake(0).  One thread per padded position: the
// reads of x are contiguous.
__global__ __launch_bounds__(256) void sconv_repack_kernel(const float* __restrict__ x, float* __restrict__ xs, const float* __restrict__ alpha,
                                                           int C, int T, int s, int p, int U /* T_out + 1 */, int blocks_per_row) {
    const unsigned row = blockIdx.x / blocks_per_row;            // b * C + c
    const int c = (int)(row % C);
    const int j = (int)(blockIdx.x - row * blocks_per_row) * 256 + threadIdx.x;
    if (j >= U * s) return;
    const int u = j / s, r = j - u * s;
    const int t = j - p;
    float v = 0.f;
    if (t >= 0 && t < T) {
        v = x[(size_t)row * T + t];
        if (alpha) {
            const float al = alpha[c];
            v = fmaf(1.0f / (al + 0.000000001f), snake_sin2(v * al), v);
        }
    }
    xs[((size_t)row * s + r) * U + u] = v;
}

}  // namespace amp

using namespace amp;

// amp_set_codec_unit_fusion: -1 the measured policy, 0 never (the four launches), 1 wherever the fused kernel is built.  Read at create time.
static int g_unit_fusion = -1;
// widest unit the policy hands to the fused kernel.  Measured (B = 16, both routes as captured graphs, alternating): C = 96 fused
// 1.04 ms vs 1.37 ms, C = 192 fused 1.08 ms vs 1.00 ms -- every workgroup streams the whole packed weight (C x 8C x 4 B) for 64 columns, which the
// conv kernels' wider tiles amortise better at C = 192.  Widths between the two are not measured and stay on the four launches.
constexpr int kUnitFusedPolicyMaxC = 96;

struct amp_codec_unit {
    int C = 0, d = 1, precision = PREC_F16X3;
    bool fused = false;
    uint4 *wp1 = nullptr, *wp2 = nullptr;
    float *b1 = nullptr, *b2 = nullptr, *al1 = nullptr, *ib1 = nullptr, *al2 = nullptr, *ib2 = nullptr;
    float inv1 = 1.f, inv2 = 1.f;
    std::unique_ptr<amp_conv> c1, c2;     // the unfused route
    DeviceAllocs dev;
};

// amp_set_aa_unit_fusion: -1 the measured policy, 0 never (the four launches), 1 wherever the fused kernel is built.  Read at create time.
static int g_aa_unit_fusion = -1;
// the widths the policy hands to the fused kernel: none.  Measured (B = 16, both routes through amp_aa_unit_forward as captured
// graphs, alternating): C = 32 fused 1.02 - 1.20 ms vs 0.69, C = 64 2.04 - 2.62 vs 1.47, C = 128 4.00 - 4.18 vs 1.80 -- the fused kernel is
// VALU-bound on its two activations and loses at every width
static bool aa_unit_policy_fused(int C) { (void)C; return false; }

struct amp_aa_unit {
    int C = 0, d = 1, precision = PREC_F16X3;
    bool fused = false;
    uint4 *wp1 = nullptr, *wp2 = nullptr;
    float *b1 = nullptr, *b2 = nullptr;
    float inv1 = 1.f, inv2 = 1.f;
    float *a1 = nullptr, *ib1 = nullptr, *a2 = nullptr, *ib2 = nullptr;   // alpha (exp'ed when logscale), 1 / (beta + 1e-9)
    float* filt = nullptr;                // 12 up taps, 12 down taps
    std::unique_ptr<amp_conv> c1, c2;     // the four-launch route
    DeviceAllocs dev;
};

// amp_set_tconv_fusion: -1 the policy, 0 never (snake, then the transposed conv), 1 wherever the fused kernel is built.  Read at create time.
static int g_tconv_fusion = -1;
// widest input the policy hands to the fused kernel
constexpr int kTconvFusedPolicyMaxCin = 384;

struct amp_tconv {
    int cin = 0, cout = 0, s = 1, p = 0, op = 0, precision = PREC_F16X3;
    bool fused = false;
    uint4* wp = nullptr;
    float* bias = nullptr;
    float inv = 1.f;
    std::unique_ptr<amp_conv> conv;       // the two-launch route: ConvTranspose1d(cin, cout, 2 s, s, p) with out_pad = op
    DeviceAllocs dev;
};

static long long tconv_out_len(const amp_tconv* h, long long T) { return (T - 1) * h->s - 2ll * h->p + 2ll * h->s + h->op; }

struct amp_sconv {
    int cin = 0, cout = 0, s = 1, p = 0;
    std::unique_ptr<amp_conv> conv;       // Conv1d(cin * s, cout, k = 2, padding 0)
};

// the [C, C, taps] conv weight as the [C, taps * C] GEMM matrix: column i = tap * C + c
static int cu_pack(const float* W, int C, int taps, std::vector<_Float16>* wp, float* inv_scale) {
    return pack_matrix_f16x3("amp_codec_unit_create", C, taps * C, C / 32, taps * C / 16,
                             [&](int m, int i) { const int tap = i / C, c = i - tap * C; return W[((size_t)m * C + c) * taps + tap]; }, wp, inv_scale);
}

static long long sconv_out_len(const amp_sconv* h, long long T) {
    const long long n = T + 2ll * h->p - 2ll * h->s;
    return n < 0 ? 0 : n / h->s + 1;
}

extern "C" {

int amp_codec_unit_create(int channels, int dilation, const float* alpha1_host, const float* w1_host, const float* b1_host, const float* alpha2_host,
                          const float* w2_host, const float* b2_host, amp_codec_unit** out) {
    if (!alpha1_host || !w1_host || !b1_host || !alpha2_host || !w2_host || !b2_host || !out) { set_error("amp_codec_unit_create: null argument"); return AMP_ERR_INVALID; }
    if (amp_device_count() <= 0) { set_error("amp_codec_unit_create: no HIP device visible (the HIP path has no CPU fallback)"); return AMP_ERR_HIP; }
    const int C = channels, d = dilation;
    if (C < 1 || d < 1) { set_error("amp_codec_unit_create: C=%d dilation=%d", C, d); return AMP_ERR_INVALID; }
    auto h = std::make_unique<amp_codec_unit>();
    h->C = C; h->d = d; h->precision = default_precision();
    const bool built = h->precision == PREC_F16X3 && C % 32 == 0 && C <= 192 && d <= 9;
    h->fused = built && g_unit_fusion != 0 && (g_unit_fusion == 1 || C <= kUnitFusedPolicyMaxC);
    // the fused route's packer refuses non-finite weights itself; the four-launch route (both precisions) has this check only
    if (!h->fused) {
        for (size_t i = 0; i < (size_t)C * C * 7; ++i)
            if (!(fabsf(w1_host[i]) < 1e30f)) { set_error("amp_codec_unit_create: non-finite weight"); return AMP_ERR_INVALID; }
        for (size_t i = 0; i < (size_t)C * C; ++i)
            if (!(fabsf(w2_host[i]) < 1e30f)) { set_error("amp_codec_unit_create: non-finite weight"); return AMP_ERR_INVALID; }
    }
    AMP_RC(h->dev.upload(alpha1_host, sizeof(float) * C, (void**)&h->al1));
    AMP_RC(h->dev.upload(alpha2_host, sizeof(float) * C, (void**)&h->al2));
    if (h->fused) {
        std::vector<float> ib1(C), ib2(C);
        for (int c = 0; c < C; ++c) { ib1[c] = 1.0f / (alpha1_host[c] + 0.000000001f); ib2[c] = 1.0f / (alpha2_host[c] + 0.000000001f); }
        AMP_RC(h->dev.upload(ib1, &h->ib1));
        AMP_RC(h->dev.upload(ib2, &h->ib2));
        AMP_RC(h->dev.upload(b1_host, sizeof(float) * C, (void**)&h->b1));
        AMP_RC(h->dev.upload(b2_host, sizeof(float) * C, (void**)&h->b2));
        std::vector<_Float16> p1, p2;
        AMP_RC(cu_pack(w1_host, C, 7, &p1, &h->inv1));
        AMP_RC(cu_pack(w2_host, C, 1, &p2, &h->inv2));
        AMP_RC(h->dev.upload(p1, &h->wp1));
        AMP_RC(h->dev.upload(p2, &h->wp2));
    } else {
        h->c1 = std::make_unique<amp_conv>();
        h->c1->cin = C; h->c1->cout = C; h->c1->k = 7; h->c1->dilation = d; h->c1->padding = 3 * d;
        AMP_RC(conv_build(h->c1.get(), w1_host, b1_host));
        h->c2 = std::make_unique<amp_conv>();
        h->c2->cin = C; h->c2->cout = C; h->c2->k = 1;
        AMP_RC(conv_build(h->c2.get(), w2_host, b2_host));
    }
    *out = h.release();
    return AMP_OK;
}

int amp_set_codec_unit_fusion(int mode) {
    if (mode < -1 || mode > 1) { set_error("amp_set_codec_unit_fusion: mode %d (-1 policy, 0 off, 1 wherever built)", mode); return AMP_ERR_INVALID; }
    g_unit_fusion = mode;
    return AMP_OK;
}

int amp_codec_unit_fused(const amp_codec_unit* h) { return h ? (h->fused ? 1 : 0) : -1; }

size_t amp_codec_unit_workspace_bytes(const amp_codec_unit* h, int B, int T) {
    if (!h || h->fused || B <= 0 || T <= 0) return 0;
    return (size_t)2 * B * h->C * T * sizeof(float);
}

int amp_codec_unit_forward(const amp_codec_unit* h, const float* x_dev, int B, int T, float* y_dev, void* ws_dev, size_t ws_bytes, void* stream_) {
    if (!h || !x_dev || !y_dev) { set_error("amp_codec_unit_forward: null argument"); return AMP_ERR_INVALID; }
    if (B <= 0 || T <= 0) { set_error("amp_codec_unit_forward: B=%d T=%d", B, T); return AMP_ERR_INVALID; }
    if (x_dev == y_dev) { set_error("amp_codec_unit_forward: x and y must not alias (the conv reads a halo)"); return AMP_ERR_INVALID; }
    hipStream_t st = (hipStream_t)stream_;
    if (h->fused) {
        if (T > (1 << 30) || (long long)B * ((T + CU_TN - 1) / CU_TN) > 0x7fffffffll) {
            set_error("amp_codec_unit_forward: B=%d x T=%d is beyond the kernel's index arithmetic", B, T);
            return AMP_ERR_UNSUPPORTED;
        }
        CodecUnitArgs a{};
        a.x = x_dev; a.y = y_dev; a.wp1 = h->wp1; a.wp2 = h->wp2; a.bias1 = h->b1; a.bias2 = h->b2;
        a.alpha1 = h->al1; a.invb1 = h->ib1; a.alpha2 = h->al2; a.invb2 = h->ib2;
        a.C = h->C; a.T = T; a.d = h->d; a.inv1 = h->inv1; a.inv2 = h->inv2;
        a.range_flag = range_flag_for_current_device();
        AMP_HIP(launch_codec_unit(a, B, st));
        return AMP_OK;
    }
    const size_t need = amp_codec_unit_workspace_bytes(h, B, T);
    if (!ws_dev || ws_bytes < need) { set_error("amp_codec_unit_forward: workspace %zu < %zu bytes", ws_bytes, need); return AMP_ERR_INVALID; }
    float* s0 = (float*)ws_dev;
    float* s1 = s0 + (size_t)B * h->C * T;
    AMP_HIP(launch_snake(x_dev, s0, B, h->C, T, h->al1, nullptr, 0, st));
    AMP_RC(conv_run(h->c1.get(), s0, B, T, 1.f, nullptr, 1.f, s1, 0, 1.f, st));
    AMP_HIP(launch_snake(s1, s0, B, h->C, T, h->al2, nullptr, 0, st));
    AMP_RC(conv_run(h->c2.get(), s0, B, T, 1.f, x_dev, 1.f, y_dev, 0, 1.f, st));
    return AMP_OK;
}

void amp_codec_unit_destroy(amp_codec_unit* h) { delete h; }

int amp_aa_unit_create(int channels, int dilation, const float* alpha1_host, const float* beta1_host, const float* w1_host, const float* b1_host,
                       const float* alpha2_host, const float* beta2_host, const float* w2_host, const float* b2_host, int logscale,
                       const float* filt_up_host, const float* filt_down_host, amp_aa_unit** out) {
    if (!alpha1_host || !w1_host || !b1_host || !alpha2_host || !w2_host || !b2_host || !filt_up_host || !filt_down_host || !out) {
        set_error("amp_aa_unit_create: null argument");
        return AMP_ERR_INVALID;
    }
    if (amp_device_count() <= 0) { set_error("amp_aa_unit_create: no HIP device visible (the HIP path has no CPU fallback)"); return AMP_ERR_HIP; }
    const int C = channels, d = dilation;
    if (C < 1 || d < 1) { set_error("amp_aa_unit_create: C=%d dilation=%d", C, d); return AMP_ERR_INVALID; }
    auto h = std::make_unique<amp_aa_unit>();
    h->C = C; h->d = d; h->precision = default_precision();
    const bool built = h->precision == PREC_F16X3 && C % 32 == 0 && C <= 128 && d <= 9;
    h->fused = built && g_aa_unit_fusion != 0 && (g_aa_unit_fusion == 1 || aa_unit_policy_fused(C));
    // a = alpha, 1 / (beta + 1e-9) with beta = alpha for plain Snake, both exp'ed first when logscale: act_params_upload's expressions
    std::vector<float> a1(C), ib1(C), a2(C), ib2(C), filt(24);
    for (int c = 0; c < C; ++c) {
        float av = alpha1_host[c], bv = beta1_host ? beta1_host[c] : alpha1_host[c];
        if (logscale) { av = expf(av); bv = expf(bv); }
        a1[c] = av; ib1[c] = 1.0f / (bv + 0.000000001f);
        av = alpha2_host[c]; bv = beta2_host ? beta2_host[c] : alpha2_host[c];
        if (logscale) { av = expf(av); bv = expf(bv); }
        a2[c] = av; ib2[c] = 1.0f / (bv + 0.000000001f);
    }
    for (int i = 0; i < 12; ++i) { filt[i] = filt_up_host[i]; filt[12 + i] = filt_down_host[i]; }
    AMP_RC(h->dev.upload(a1, &h->a1));
    AMP_RC(h->dev.upload(ib1, &h->ib1));
    AMP_RC(h->dev.upload(a2, &h->a2));
    AMP_RC(h->dev.upload(ib2, &h->ib2));
    AMP_RC(h->dev.upload(filt, &h->filt));
    if (h->fused) {
        AMP_RC(h->dev.upload(b1_host, sizeof(float) * C, (void**)&h->b1));
        AMP_RC(h->dev.upload(b2_host, sizeof(float) * C, (void**)&h->b2));
        std::vector<_Float16> p1, p2;
        float inv1 = 1.f, inv2 = 1.f;
        if (int rc = pack_matrix_f16x3("amp_aa_unit_create", C, 7 * C, C / 32, 7 * C / 16,
                                       [&](int m, int i) { const int tap = i / C, c = i - tap * C; return w1_host[((size_t)m * C + c) * 7 + tap]; }, &p1, &inv1);
            rc != AMP_OK) return rc;
        if (int rc = pack_matrix_f16x3("amp_aa_unit_create", C, C, C / 32, C / 16, [&](int m, int i) { return w2_host[(size_t)m * C + i]; }, &p2, &inv2);
            rc != AMP_OK) return rc;
        h->inv1 = inv1; h->inv2 = inv2;
        AMP_RC(h->dev.upload(p1, &h->wp1));
        AMP_RC(h->dev.upload(p2, &h->wp2));
    } else {
        for (size_t i = 0; i < (size_t)C * C * 7; ++i)
            if (!(fabsf(w1_host[i]) < 1e30f)) { set_error("amp_aa_unit_create: non-finite weight"); return AMP_ERR_INVALID; }
        for (size_t i = 0; i < (size_t)C * C; ++i)
            if (!(fabsf(w2_host[i]) < 1e30f)) { set_error("amp_aa_unit_create: non-finite weight"); return AMP_ERR_INVALID; }
        h->c1 = std::make_unique<amp_conv>();
        h->c1->cin = C; h->c1->cout = C; h->c1->k = 7; h->c1->dilation = d; h->c1->padding = 3 * d;
        AMP_RC(conv_build(h->c1.get(), w1_host, b1_host));
        h->c2 = std::make_unique<amp_conv>();
        h->c2->cin = C; h->c2->cout = C; h->c2->k = 1;
        AMP_RC(conv_build(h->c2.get(), w2_host, b2_host));
    }
    *out = h.release();
    return AMP_OK;
}

int amp_set_aa_unit_fusion(int mode) {
    if (mode < -1 || mode > 1) { set_error("amp_set_aa_unit_fusion: mode %d (-1 policy, 0 off, 1 wherever built)", mode); return AMP_ERR_INVALID; }
    g_aa_unit_fusion = mode;
    return AMP_OK;
}

int amp_aa_unit_fused(const amp_aa_unit* h) { return h ? (h->fused ? 1 : 0) : -1; }

size_t amp_aa_unit_workspace_bytes(const amp_aa_unit* h, int B, int T) {
    if (!h || h->fused || B <= 0 || T <= 0) return 0;
    return (size_t)2 * B * h->C * T * sizeof(float);
}

int amp_aa_unit_forward(const amp_aa_unit* h, const float* x_dev, int B, int T, float* y_dev, void* ws_dev, size_t ws_bytes, void* stream_) {
    if (!h || !x_dev || !y_dev) { set_error("amp_aa_unit_forward: null argument"); return AMP_ERR_INVALID; }
    if (B <= 0 || T <= 0) { set_error("amp_aa_unit_forward: B=%d T=%d", B, T); return AMP_ERR_INVALID; }
    if (x_dev == y_dev) { set_error("amp_aa_unit_forward: x and y must not alias (the conv reads a halo)"); return AMP_ERR_INVALID; }
    hipStream_t st = (hipStream_t)stream_;
    if (h->fused) {
        // the kernel forms 2 T (the last Snake index) as an int
        if (T > (1 << 29) || (long long)B * ((T + AA_TN - 1) / AA_TN) > 0x7fffffffll) {
            set_error("amp_aa_unit_forward: B=%d x T=%d is beyond the kernel's index arithmetic", B, T);
            return AMP_ERR_UNSUPPORTED;
        }
        AaUnitArgs a{};
        a.x = x_dev; a.y = y_dev; a.wp1 = h->wp1; a.wp2 = h->wp2; a.bias1 = h->b1; a.bias2 = h->b2;
        a.a1 = h->a1; a.invb1 = h->ib1; a.a2 = h->a2; a.invb2 = h->ib2; a.filt = h->filt;
        a.C = h->C; a.T = T; a.d = h->d; a.inv1 = h->inv1; a.inv2 = h->inv2;
        a.range_flag = range_flag_for_current_device();
        AMP_HIP(launch_aa_unit(a, B, st));
        return AMP_OK;
    }
    const size_t need = amp_aa_unit_workspace_bytes(h, B, T);
    if (!ws_dev || ws_bytes < need) { set_error("amp_aa_unit_forward: workspace %zu < %zu bytes", ws_bytes, need); return AMP_ERR_INVALID; }
    float* s0 = (float*)ws_dev;
    float* s1 = s0 + (size_t)B * h->C * T;
    AMP_HIP(launch_act1d(x_dev, s0, B, h->C, T, h->a1, h->ib1, h->filt, h->filt + 12, nullptr, 1, st));
    AMP_RC(conv_run(h->c1.get(), s0, B, T, 1.f, nullptr, 1.f, s1, 0, 1.f, st));
    AMP_HIP(launch_act1d(s1, s0, B, h->C, T, h->a2, h->ib2, h->filt, h->filt + 12, nullptr, 1, st));
    AMP_RC(conv_run(h->c2.get(), s0, B, T, 1.f, x_dev, 1.f, y_dev, 0, 1.f, st));
    return AMP_OK;
}

void amp_aa_unit_destroy(amp_aa_unit* h) { delete h; }

int amp_sconv_create(int cin, int cout, int stride, int padding, const float* weight_host, const float* bias_host, amp_sconv** out) {
    if (!weight_host || !out) { set_error("amp_sconv_create: null argument"); return AMP_ERR_INVALID; }
    if (amp_device_count() <= 0) { set_error("amp_sconv_create: no HIP device visible (the HIP path has no CPU fallback)"); return AMP_ERR_HIP; }
    if (cin < 1 || cout < 1 || stride < 1 || padding < 0) { set_error("amp_sconv_create: cin=%d cout=%d stride=%d padding=%d", cin, cout, stride, padding); return AMP_ERR_INVALID; }
    if ((long long)cin * stride > 65536) { set_error("amp_sconv_create: cin * stride = %lld channels", (long long)cin * stride); return AMP_ERR_UNSUPPORTED; }
    auto h = std::make_unique<amp_sconv>();
    h->cin = cin; h->cout = cout; h->s = stride; h->p = padding;
    const int s = stride, k = 2 * s;
    std::vector<float> w2((size_t)cout * cin * s * 2);
    for (int o = 0; o < cout; ++o)
        for (int c = 0; c < cin; ++c)
            for (int r = 0; r < s; ++r)
                for (int a = 0; a < 2; ++a) w2[(((size_t)o * cin + c) * s + r) * 2 + a] = weight_host[((size_t)o * cin + c) * k + a * s + r];
    h->conv = std::make_unique<amp_conv>();
    h->conv->cin = cin * s; h->conv->cout = cout; h->conv->k = 2;
    AMP_RC(conv_build(h->conv.get(), w2.data(), bias_host));
    *out = h.release();
    return AMP_OK;
}

int amp_sconv_out_len(const amp_sconv* h, int T) { return h ? (int)sconv_out_len(h, T) : 0; }

size_t amp_sconv_workspace_bytes(const amp_sconv* h, int B, int T) {
    if (!h || B <= 0 || T <= 0) return 0;
    return (size_t)B * h->cin * h->s * (size_t)(sconv_out_len(h, T) + 1) * sizeof(float);
}

int amp_sconv_forward(const amp_sconv* h, const float* x_dev, int B, int T, const float* alpha_dev, void* ws_dev, size_t ws_bytes, float* y_dev,
                      void* stream_) {
    if (!h || !x_dev || !y_dev || !ws_dev) { set_error("amp_sconv_forward: null argument"); return AMP_ERR_INVALID; }
    if (B <= 0 || T <= 0) { set_error("amp_sconv_forward: B=%d T=%d", B, T); return AMP_ERR_INVALID; }
    const long long Tout = sconv_out_len(h, T);
    if (Tout <= 0) { set_error("amp_sconv_forward: input too short (T=%d gives T_out=%lld)", T, Tout); return AMP_ERR_INVALID; }
    const size_t need = amp_sconv_workspace_bytes(h, B, T);
    if (ws_bytes < need) { set_error("amp_sconv_forward: workspace %zu < %zu bytes", ws_bytes, need); return AMP_ERR_INVALID; }
    const long long rows = (long long)B * h->cin;
    const long long U = Tout + 1;
    const long long bpr = (U * h->s + 255) / 256;
    if (U * h->s > (1ll << 30) || rows * bpr > 0x7fffffffll) { set_error("amp_sconv_forward: B * cin = %lld rows of %lld padded columns: beyond the grid", rows, U * h->s); return AMP_ERR_UNSUPPORTED; }
    hipStream_t st = (hipStream_t)stream_;
    const dim3 grid((unsigned)(rows * bpr));
    note_kernel("sconv_repack_kernel");
    note_work((unsigned long long)grid.x * grid.y, 0.0, 4.0 * rows * ((double)T + (double)U * h->s) / 1e6, "snake + space-to-depth C=%d s=%d T=%d B=%d", h->cin, h->s, T, B);
    hipLaunchKernelGGL(sconv_repack_kernel, grid, dim3(256), 0, st, x_dev, (float*)ws_dev, alpha_dev, h->cin, T, h->s, h->p, (int)U, (int)bpr);
    AMP_HIP(hipGetLastError());
    AMP_RC(conv_run(h->conv.get(), (const float*)ws_dev, B, (int)U, 1.f, nullptr, 1.f, y_dev, 0, 1.f, st));
    return AMP_OK;
}

void amp_sconv_destroy(amp_sconv* h) { delete h; }

int amp_tconv_create(int cin, int cout, int stride, int padding, int output_padding, const float* weight_host, const float* bias_host, amp_tconv** out) {
    if (!weight_host || !out) { set_error("amp_tconv_create: null argument"); return AMP_ERR_INVALID; }
    if (amp_device_count() <= 0) { set_error("amp_tconv_create: no HIP device visible (the HIP path has no CPU fallback)"); return AMP_ERR_HIP; }
    if (cin < 1 || cout < 1 || stride < 1 || padding < 0 || output_padding < 0) {
        set_error("amp_tconv_create: cin=%d cout=%d stride=%d padding=%d output_padding=%d", cin, cout, stride, padding, output_padding);
        return AMP_ERR_INVALID;
    }
    if (output_padding >= stride) { set_error("amp_tconv_create: output_padding %d must be smaller than the stride %d", output_padding, stride); return AMP_ERR_INVALID; }
    // the q = T column is the last one either route walks: its samples reach t = T s + s - 1 - p, and T_out - 1 = T s + s - 1 - 2 p + op
    if (output_padding > padding) { set_error("amp_tconv_create: output_padding %d > padding %d", output_padding, padding); return AMP_ERR_UNSUPPORTED; }
    if ((long long)cout * stride > (1 << 24)) { set_error("amp_tconv_create: cout * stride = %lld rows", (long long)cout * stride); return AMP_ERR_UNSUPPORTED; }
    auto h = std::make_unique<amp_tconv>();
    h->cin = cin; h->cout = cout; h->s = stride; h->p = padding; h->op = output_padding; h->precision = default_precision();
    const int s = stride, k = 2 * s;
    const bool built = h->precision == PREC_F16X3 && cin % 32 == 0 && cin <= 384 && s >= 2 && s <= 8;
    h->fused = built && g_tconv_fusion != 0 && (g_tconv_fusion == 1 || cin <= kTconvFusedPolicyMaxCin);
    if (h->fused) {
        const int M = cout * s;
        std::vector<_Float16> wp;
        AMP_RC(pack_matrix_f16x3("amp_tconv_create", M, 2 * cin, (M + 31) / 32, 2 * cin / 16,
                                 [&](int m, int i) { const int tap = i / cin, c = i - tap * cin, o = m / s, r = m - o * s;
                                                     return weight_host[((size_t)c * cout + o) * k + r + tap * s]; }, &wp, &h->inv));
        AMP_RC(h->dev.upload(wp, &h->wp));
        std::vector<float> b(cout, 0.f);
        if (bias_host) b.assign(bias_host, bias_host + cout);
        AMP_RC(h->dev.upload(b, &h->bias));
    } else {
        h->conv = std::make_unique<amp_conv>();
        h->conv->transposed = 1; h->conv->cin = cin; h->conv->cout = cout; h->conv->k = k; h->conv->stride = s; h->conv->padding = padding;
        h->conv->out_pad = output_padding;
        AMP_RC(conv_build(h->conv.get(), weight_host, bias_host));
    }
    *out = h.release();
    return AMP_OK;
}

int amp_set_tconv_fusion(int mode) {
    if (mode < -1 || mode > 1) { set_error("amp_set_tconv_fusion: mode %d (-1 policy, 0 off, 1 wherever built)", mode); return AMP_ERR_INVALID; }
    g_tconv_fusion = mode;
    return AMP_OK;
}

int amp_tconv_fused(const amp_tconv* h) { return h ? (h->fused ? 1 : 0) : -1; }

int amp_tconv_out_len(const amp_tconv* h, int T) {
    if (!h) return 0;
    const long long n = tconv_out_len(h, T);
    return n < 0 ? 0 : (n > 0x7fffffffll ? 0x7fffffff : (int)n);
}

size_t amp_tconv_workspace_bytes(const amp_tconv* h, int B, int T) {
    if (!h || h->fused || B <= 0 || T <= 0) return 0;
    return (size_t)B * h->cin * T * sizeof(float);
}

int amp_tconv_forward(const amp_tconv* h, const float* x_dev, int B, int T, const float* alpha_dev, void* ws_dev, size_t ws_bytes, float* y_dev,
                      void* stream_) {
    if (!h || !x_dev || !y_dev) { set_error("amp_tconv_forward: null argument"); return AMP_ERR_INVALID; }
    if (B <= 0 || T <= 0) { set_error("amp_tconv_forward: B=%d T=%d", B, T); return AMP_ERR_INVALID; }
    const long long Tout = tconv_out_len(h, T);
    if (Tout <= 0) { set_error("amp_tconv_forward: input too short (T=%d gives T_out=%lld)", T, Tout); return AMP_ERR_INVALID; }
    if (Tout > (1ll << 30)) { set_error("amp_tconv_forward: T_out=%lld is beyond the kernels' index arithmetic", Tout); return AMP_ERR_UNSUPPORTED; }
    hipStream_t st = (hipStream_t)stream_;
    if (h->fused) {
        const long long nq = (Tout - 1 + h->p) / h->s - h->p / h->s + 1;
        if ((long long)B * ((nq + TC_TN - 1) / TC_TN) > 0x7fffffffll) {
            set_error("amp_tconv_forward: B=%d x T=%d is beyond the grid", B, T);
            return AMP_ERR_UNSUPPORTED;
        }
        TconvArgs a{};
        a.x = x_dev; a.y = y_dev; a.wp = h->wp; a.bias = h->bias; a.alpha = alpha_dev;
        a.cin = h->cin; a.cout = h->cout; a.s = h->s; a.p = h->p; a.T = T; a.Tout = (int)Tout;
        a.M = h->cout * h->s; a.NRB = (a.M + 31) / 32; a.q_first = h->p / h->s; a.inv = h->inv;
        a.range_flag = range_flag_for_current_device();
        AMP_HIP(launch_tconv(a, B, st));
        return AMP_OK;
    }
    const float* in = x_dev;
    if (alpha_dev) {
        const size_t need = amp_tconv_workspace_bytes(h, B, T);
        if (!ws_dev || ws_bytes < need) { set_error("amp_tconv_forward: workspace %zu < %zu bytes", ws_bytes, need); return AMP_ERR_INVALID; }
        AMP_HIP(launch_snake(x_dev, (float*)ws_dev, B, h->cin, T, alpha_dev, nullptr, 0, st));
        in = (const float*)ws_dev;
    }
    AMP_RC(conv_run(h->conv.get(), in, B, T, 1.f, nullptr, 1.f, y_dev, 0, 1.f, st));
    return AMP_OK;
}

void amp_tconv_destroy(amp_tconv* h) { delete h; }

}  // extern "C"
