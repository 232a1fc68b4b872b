// Host-only declarations shared by the host units of libamphion_hip.so (runtime.hip, conv_host.hip, generator.hip, ops_abi.hip,
// fvq.hip, codec.hip, diffwave.hip and the host half of pw_f16x3.hip).  Kernel argument structs and launch_* prototypes stay in
// amp_internal.h.
#pragma once
#include <math.h>

#include <vector>

#include "amp_internal.h"

// ---- error plumbing (runtime.hip holds the text: set_error / amp_last_error) ---------------------------------------
#define AMP_HIP(expr)                                                                  \
    do {                                                                               \
        hipError_t e__ = (expr);                                                       \
        if (e__ != hipSuccess) {                                                       \
            set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
            return AMP_ERR_HIP;                                                        \
        }                                                                              \
    } while (0)

#define AMP_RC(expr) do { int rc__ = (expr); if (rc__ != AMP_OK) return rc__; } while (0)

// do the byte ranges [p, p + pn) and [q, q + qn) share a byte?  An empty range overlaps nothing.
inline bool ranges_overlap(const void* p, size_t pn, const void* q, size_t qn) {
    const char* a = static_cast<const char*>(p);
    const char* b = static_cast<const char*>(q);
    return pn && qn && a < b + qn && b < a + pn;
}

// ---- amp_conv: one (transposed) convolution with packed weights on the device (conv_host.hip) -----------------------
struct amp_conv {
    int transposed = 0, cin = 0, cout = 0, k = 0, stride = 1, dilation = 1, padding = 0;
    // GEMM view
    int M = 0, ntaps = 0, KT = 0, off0 = 0, dstep = 0, halo_left = 0, halo_right = 0, up = 1, up_pad = 0;
    int nchunks = 0;
    int precision = amp::PREC_F32;  // arithmetic of the contraction, fixed at build time
    int pad_reflect = 0, tanh_out = 0;  // amp_conv_set_option
    int out_pad = 0;           // ConvTranspose1d output_padding (< stride, <= padding: no new taps, T_out only); set by amp_tconv_create alone
    int gated_H = 0;           // > 0: rows packed for the gate epilogue of conv_small_f16x3.hip (amp_conv_create_gated)
    int Mpad = 0;              // rows of the packed weight
    float wscale = 1.f;        // f16x3: power of two applied to the packed weights
    amp::ConvPlan plan{};
    void* wp_dev = nullptr;
    float* bias_dev = nullptr;
    ~amp_conv() {
        if (wp_dev) (void)hipFree(wp_dev);
        if (bias_dev) (void)hipFree(bias_dev);
    }
};

// ---- amp_pw: one nn.Linear along the channel axis (pw_f16x3.hip; the T = 1 form of pw_vec.hip reads the same packed weights) ----------
struct amp_pw {
    int cin = 0, cout = 0;
    int precision = amp::PREC_F16X3;
    int nsteps = 0;
    float inv_scale = 1.f;
    uint4* wp_dev = nullptr;     // f16x3: packed fragments
    float* bias_dev = nullptr;   // [cout] (zeros when the Linear has no bias)
    amp_conv* conv = nullptr;    // exact-fp32 mode: the k = 1 conv
    ~amp_pw() {
        if (wp_dev) (void)hipFree(wp_dev);
        if (bias_dev) (void)hipFree(bias_dev);
        delete conv;
    }
};

namespace amp {

// hipMalloc + hipMemcpy of `bytes` host bytes; on success the caller owns *out (hipFree), on failure nothing is left allocated
int device_upload(const void* host, size_t bytes, void** out);

// Every device allocation of a handle: upload() is device_upload() into memory the owner frees with the handle.
struct DeviceAllocs {
    std::vector<void*> owned;
    DeviceAllocs() = default;
    DeviceAllocs(const DeviceAllocs&) = delete;
    DeviceAllocs& operator=(const DeviceAllocs&) = delete;
    ~DeviceAllocs() {
        for (void* p : owned) (void)hipFree(p);
    }
    int upload(const void* host, size_t bytes, void** out) {
        if (int rc = device_upload(host, bytes, out); rc != AMP_OK) return rc;
        owned.push_back(*out);
        return AMP_OK;
    }
    template <class T, class P>
    int upload(const std::vector<T>& v, P** out) { return upload(v.data(), v.size() * sizeof(T), (void**)out); }
};

// Process-wide default for handles created from now on: AMP_PRECISION=f32|f16x3, amp_set_precision() (runtime.hip)
int default_precision();

// ---- launch-policy switches: ONE configuration, read from the environment once (first use) and changed afterwards only
// through the amp_set_* entry points the tests use for their bitwise A/B comparisons.  Nothing on a launch path calls getenv.
// Environment forms exist for the switches a deployment may want without code (round 5 dropped AMP_FUSE_PAIRS, AMP_PAIR_STRIP,
// AMP_CONV_BLK, AMP_RB_SUM_FRAMES, AMP_RB_HORIZONTAL, AMP_RB_HORIZONTAL_FRAMES and AMP_GROUP_MB: amp_set_* or nothing):
//   AMP_PRECISION     f32 | f16x3       arithmetic of the conv contractions (amp_set_precision), read in default_precision()
//   AMP_RB_FUSION     0 .. 3            whole-ResBlock kernel: off | policy (default) | wherever built | + four-wave tiles
//   AMP_AMPB_FUSION   0 .. 3            whole-AMPBlock kernel (BigVGAN): off | policy (default) | wherever built | + four-wave tiles
//   AMP_RB_GUARDS     -1 .. 1           real x in the whole-ResBlock kernel's guard columns: policy (default) | never | always
//   AMP_RB_SPLIT_PLAN a[,b[,c]]         pairs per launch of a three-pair resblock, forced ("3", "2,1", "1,2", "1,1,1"); unset: the plan
//   AMP_RB_STREAMS    -1 .. 1           a stage's resblocks on concurrent streams: small launches only (default) | never | always
// (+ AMP_LAUNCH_MANIFEST=<file>, the profiling manifest of runtime.hip, and AMP_GRAPH_CACHE=0 on the Python side.)
// The policies these steer are in conv_host.hip (generator.hip for group_bytes / rb_streams); the amp_set_* entry points in runtime.hip.
constexpr int kConvBlkDefault = 3;
constexpr int kConvRgFastDefault = 1;
constexpr int kPingPongDefault = 1;
struct Config {
    int pair_strips = -1;      // -1 policy, 0 per-tile kernel, 1 four-wave strips
    int strip_fit = -1;        // fitted strips of the fused-pair strip kernel: -1 the plan (strip_geometry, conv_host.hip), 0 never, 1 every strip launch
    int rb_fusion = 1;
    int rb_guards = -1;        // RbArgs::gx: -1 the policy (conv_host.hip rb_geometry), 0 never, 1 wherever the first conv's reach fits the guard
    int rb_plan[3] = {0, 0, 0};   // forced pairs per launch of a three-pair resblock (amp_set_rb_split_plan); {0, 0, 0}: rb_plan()'s cost model
    int ampb_fusion = 1;
    int conv_blk = kConvBlkDefault;
    size_t group_bytes = 0;
    // no environment form: bit-identical A/B switches for the tests (amp_set_small_conv / _conv_rg_fast / _pingpong)
    int small_conv = 1;
    int conv_rg_fast = 1;
    int pingpong = 1;
    int narrow_blk = 1;        // row-blocked conv kernel for 128- / 64-row convs (amp_set_conv_blk_narrow)
    int rb_streams = -1;       // resblocks of a stage on concurrent streams: -1 small launches only, 0 never, 1 always (amp_set_resblock_streams)
    Config();                  // reads the environment forms
};
Config& cfg();

// ---- f16 operand-range guard (runtime.hip) ---------------------------------------------------------------------------
// The f16x3 kernels OR 1 into a per-device word when a staged operand does not fit the split-f16 form (|x| > 4094
// after the exact x16, or non-finite): the fp32 reference has no such cliff, so the result of that launch is NOT the
// reference's.  A generator handle has its OWN word: amp_gen_forward copies it to pinned host memory behind its last
// kernel (no synchronisation) and the NEXT forward of that handle that finds the copy complete returns AMP_ERR_RANGE;
// amp_gen_range_check() synchronises and reports immediately.  Op-level launches (amp_conv_forward, amp_pair_forward)
// report to one word per device, read by amp_range_check().  Every report clears its word.
struct RangeGuard {
    unsigned* dev = nullptr;       // device word the kernels write
    unsigned* host = nullptr;      // pinned mirror
    hipEvent_t ev = nullptr;
    bool pending = false;          // an async copy of `dev` is in flight / unread
};
bool guard_init(RangeGuard& g);
void guard_free(RangeGuard& g);
int range_poll(RangeGuard* g, hipStream_t st);                            // non-blocking: reports (and clears) a flag whose copy has already landed
int range_publish(RangeGuard* g, hipStream_t st);                         // enqueue the copy of the flag behind everything launched so far on `st`
int range_check_sync(RangeGuard* g, hipStream_t st, const char* who);     // synchronising check of one guard
// while alive, the calling thread's f16x3 launches report to `word` (a handle's own) instead of the per-device word
struct RangeFlagScope {
    explicit RangeFlagScope(unsigned* word);
    ~RangeFlagScope();
    RangeFlagScope(const RangeFlagScope&) = delete;
    RangeFlagScope& operator=(const RangeFlagScope&) = delete;
};

// ---- f16x3 A fragments: the one host routine whose bits decide the numerics ----------------------------------------
// 2^s with max|w| * 2^s in (2^12, 2^13]: lo = f16(w * 2^s - hi) is then a normal f16 for every weight above 2^-16 of the
// largest, and hi stays far from the f16 overflow (conv_f16x3.hip).  1 for wmax == 0.
inline float pow2_weight_scale(float wmax) {
    int e2 = 0;
    if (wmax > 0.f) { (void)frexpf(wmax, &e2); if (ldexpf(1.f, e2 - 1) == wmax) e2 -= 1; }  // wmax <= 2^e2
    return wmax > 0.f ? ldexpf(1.f, 13 - e2) : 1.f;
}

// [row block][k16][tap][plane hi | lo][lane][8 x f16]: lane l holds row 32 mb + (l & 31), channels 16 c + 8 (l >> 5) + 0 .. 7 of
// view(m, i, g) * wscale (view: the fp32 weight of GEMM row m, channel i, tap g, 0 outside the matrix), split as hi = f16(v),
// lo = f16(v - hi).  pad_entries zero (plane, lane) fragments follow for kernels whose A reload runs ahead of the contraction.
template <class View>
std::vector<_Float16> pack_a_f16x3(int row_blocks, int k16, int taps, size_t pad_entries, float wscale, View view) {
    std::vector<_Float16> wp(((size_t)row_blocks * k16 * taps * 2 + pad_entries) * 64 * 8, (_Float16)0.f);
    for (int mb = 0; mb < row_blocks; ++mb)
        for (int c = 0; c < k16; ++c)
            for (int g = 0; g < taps; ++g)
                for (int lane = 0; lane < 64; ++lane)
                    for (int e = 0; e < 8; ++e) {
                        const float v = view(mb * 32 + (lane & 31), c * 16 + 8 * (lane >> 5) + e, g) * wscale;
                        const _Float16 hi = (_Float16)v;
                        const _Float16 lo = (_Float16)(v - (float)hi);
                        const size_t ent = (((size_t)mb * k16 + c) * taps + g) * 2;
                        wp[((ent + 0) * 64 + lane) * 8 + e] = hi;
                        wp[((ent + 1) * 64 + lane) * 8 + e] = lo;
                    }
    return wp;
}

// One fp32 matrix W(m, i), m < rows, i < cols -> the A fragments of row_blocks x k16 (zero outside the matrix) after the per-matrix 2^s:
// the packed operand of pw_f16x3.hip, dw_layer_f16x3.hip, codec_unit_f16x3.hip and tconv_f16x3.hip.  *inv_scale = 1 / (16 * 2^s) undoes it and the x16
// of the staged activations.  Refuses a non-finite weight in `who`'s name.  (conv_build has taps and pad entries: its own pack_a_f16x3.)
template <class View>
int pack_matrix_f16x3(const char* who, int rows, int cols, int row_blocks, int k16, View W, std::vector<_Float16>* wp, float* inv_scale) {
    float wmax = 0.f;
    for (int m = 0; m < rows; ++m)
        for (int i = 0; i < cols; ++i) {
            const float w = fabsf(W(m, i));
            if (!(w < 1e30f)) { set_error("%s: non-finite weight", who); return AMP_ERR_INVALID; }
            wmax = fmaxf(wmax, w);
        }
    const float wscale = pow2_weight_scale(wmax);
    *inv_scale = 1.f / (16.f * wscale);
    *wp = pack_a_f16x3(row_blocks, k16, 1, 0, wscale, [&](int m, int i, int) { return (m < rows && i < cols) ? W(m, i) : 0.f; });
    return AMP_OK;
}

// ---- convs and the fused forms built from them (conv_host.hip) ------------------------------------------------------
int conv_build(amp_conv* c, const float* w, const float* bias);
// mode 0: y = v, 1: y += v, 2: y = (y + v) / div
// plan_small != nullptr: launch nothing -- if this call would run the whole-K kernel with the standard epilogue, hand back its arguments and
// tile width (for conv_small3_f16x3.hip, which runs three such convs in one grid), else AMP_ERR_UNSUPPORTED.
int conv_run(const amp_conv* c, const float* x, int B, int T, float slope_in, const float* res, float slope_out, float* y, int mode, float div,
             hipStream_t stream, long long xbs = 0, const int* lens = nullptr, int len_mul = 1, ConvArgs* plan_small = nullptr,
             int* plan_ni = nullptr);
// Ping-pong tile order (conv_host.hip): ONE per-thread parity shared by the conv, pair, resblock, AMPBlock and act1d launches
int next_rev(const int* lens);

bool pair_supported(const amp_conv* c1, const amp_conv* c2);
int pair_run(const amp_conv* c1, const amp_conv* c2, const float* x, int B, int T, float slope, float* y, int mode, float div,
             hipStream_t stream, const int* lens = nullptr, int len_mul = 1);
bool pair_strip_plan(int B, int T, int k, bool ragged, int* form, int* strip_len, int* spi, int* steps);
bool pair_tile_args(const amp_conv* c1, const amp_conv* c2, const float* x, int B, int T, float slope, float* y, int mode, float div,
                    const int* lens, int len_mul, PairArgs* out);

bool rb_supported(const amp_conv* const* c1, const amp_conv* const* c2, int np, int B, int T);
// geometry of one whole-resblock launch and the launches of a resblock (conv_host.hip rb_geometry / rb_plan)
struct RbGeom {
    int W;             // columns per tile, 0: the form does not cover these pairs
    int rh0, rh;       // columns a tile loses either side with zero guards / in this launch (gx: less the first conv's reach)
    int gx;            // RbArgs::gx
    int NT0, NT;       // W - 2 * rh0, W - 2 * rh: output columns per tile
    int tiles0, tiles; // ceil(T / NT0), ceil(T / NT)
};
struct RbPlan {
    int n;                           // launches
    int count[AMP_RB_MAX_PAIRS];     // pairs in each
};
RbGeom rb_geometry(int C, int k, const int* dil, int first, int count, int T, int form);
RbPlan rb_plan(int C, int k, const int* dil, int np, int B, int T, bool ragged);
RbPlan rb_plan(const amp_conv* const* c1, int np, int B, int T, bool ragged);
int rb_form_of(int C, int k);
// pairs [first, first + count) of the resblock's np (count < 0: all from `first`): x -> y
int rb_run(const amp_conv* const* c1, const amp_conv* const* c2, int np, const float* x, int B, int T, float slope, float* y, int mode,
           float div, hipStream_t stream, const int* lens = nullptr, int len_mul = 1, int first = 0, int count = -1);

struct ActParams {  // one Activation1d
    float* a_dev = nullptr;     // alpha (exp'ed when logscale)
    float* invb_dev = nullptr;  // 1 / (beta + 1e-9)
    float* fu_dev = nullptr;    // 12 taps
    float* fd_dev = nullptr;
    float* fu2_dev = nullptr;   // 2 * the up taps (UpSample1d's gain folded in, resample.py:41): what ampb_f16x3.hip reads into SGPRs
};
// Op-level convenience (tests): derive a = alpha (exp'ed when logscale) and 1 / (beta + 1e-9) on the host and upload them
// with the two 12-tap filters: scratch = [a (C) | invb (C) | up taps (12) | down taps (12) | 2 * up taps (12)].  The caller frees `*out`.
int act_params_upload(const float* alpha_dev, const float* beta_dev, int C, int logscale, const float* filt_up_host,
                      const float* filt_down_host, float** out);
bool ampb_supported(const amp_conv* const* c1, const amp_conv* const* c2, int np, const ActParams* acts, size_t nacts, int B, int T);
int ampb_run(const amp_conv* const* c1, const amp_conv* const* c2, int np, const ActParams* acts, const float* x, int B, int T, float* y,
             int mode, float div, hipStream_t stream, const int* lens = nullptr, int len_mul = 1);

}  // namespace amp
