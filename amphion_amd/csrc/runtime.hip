// Process-wide state of libamphion_hip.so: error text, the kernel log and launch manifest, the f16 operand-range guard, the default
// precision, the launch-policy Config with its amp_set_* switches, and device_upload.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <string>

#include "amp_host.h"

namespace amp {

// ------------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// ---- f16 operand-range guard (amp_host.h: RangeGuard) ------------------------------------------------------------
static RangeGuard g_guard[64];                    // op-level launches (amp_conv_forward, amp_pair_forward, ...): one word per device
__thread std::string* tl_kernel_log = nullptr;    // amp_internal.h: note_kernel()
__thread char tl_last_kernel[160] = "";
__thread int tl_conv_transposed = 0;              // amp_internal.h: note_conv_work()
// launch manifest (amp_internal.h): AMP_LAUNCH_MANIFEST=<file>, read once; lines are appended and flushed per launch (profiling runs only)
static FILE* manifest_file() {
    static FILE* f = [] {
        const char* p = getenv("AMP_LAUNCH_MANIFEST");
        return (p && *p) ? fopen(p, "a") : nullptr;
    }();
    return f;
}
bool manifest_on() {
    static const bool on = manifest_file() != nullptr;
    return on;
}
void manifest_add(const char* name, unsigned long long workgroups, double gflop, double mb, const char* what) {
    static std::mutex mu;
    std::lock_guard<std::mutex> lk(mu);
    FILE* f = manifest_file();
    if (!f) return;
    fprintf(f, "%s\t%llu\t%.6f\t%.6f\t%s\n", name, workgroups, gflop, mb, what);
    fflush(f);
    tl_last_kernel[0] = '\0';   // a launcher that forgets note_kernel() shows up as an EMPTY name, not as the previous kernel's
}
static thread_local unsigned* tl_range_flag = nullptr;   // set while an amp_gen forward is launching: that handle's own word
RangeFlagScope::RangeFlagScope(unsigned* word) { tl_range_flag = word; }
RangeFlagScope::~RangeFlagScope() { tl_range_flag = nullptr; }

bool guard_init(RangeGuard& g) {
    if (g.dev) return true;
    if (hipMalloc(&g.dev, sizeof(unsigned)) != hipSuccess) { g.dev = nullptr; return false; }
    if (hipMemset(g.dev, 0, sizeof(unsigned)) != hipSuccess || hipHostMalloc(&g.host, sizeof(unsigned)) != hipSuccess ||
        hipEventCreateWithFlags(&g.ev, hipEventDisableTiming) != hipSuccess) {
        (void)hipFree(g.dev);
        g.dev = nullptr;
        return false;
    }
    *g.host = 0;
    return true;
}

void guard_free(RangeGuard& g) {
    if (g.dev) (void)hipFree(g.dev);
    if (g.host) (void)hipHostFree(g.host);
    if (g.ev) (void)hipEventDestroy(g.ev);
    g = RangeGuard{};
}

static RangeGuard* guard_for_current_device() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    return guard_init(g_guard[dev]) ? &g_guard[dev] : nullptr;
}

// the word the f16x3 kernels of the launch being set up report to
unsigned* range_flag_for_current_device() {
    if (tl_range_flag) return tl_range_flag;
    RangeGuard* g = guard_for_current_device();
    return g ? g->dev : nullptr;
}

static bool stream_is_capturing(hipStream_t st) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
}

static const char kRangeMsg[] =
    "an activation left the split-f16 operand range of the f16x3 kernels (|x| > 4094 or infinite) in a previous "
    "launch: its output is not the fp32 reference's; re-run with amp_set_precision(AMP_PRECISION_F32)";

int range_poll(RangeGuard* g, hipStream_t st) {
    if (!g || !g->dev || !g->pending || stream_is_capturing(st)) return AMP_OK;
    if (hipEventQuery(g->ev) != hipSuccess) return AMP_OK;       // still in flight
    g->pending = false;
    if (*g->host == 0) return AMP_OK;
    *g->host = 0;
    AMP_HIP(hipMemsetAsync(g->dev, 0, sizeof(unsigned), st));
    set_error("%s", kRangeMsg);
    return AMP_ERR_RANGE;
}

int range_publish(RangeGuard* g, hipStream_t st) {
    if (!g || !g->dev || stream_is_capturing(st)) return AMP_OK;
    AMP_HIP(hipMemcpyAsync(g->host, g->dev, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    AMP_HIP(hipEventRecord(g->ev, st));
    g->pending = true;
    return AMP_OK;
}

int range_check_sync(RangeGuard* g, hipStream_t st, const char* who) {
    if (!g || !g->dev) return AMP_OK;
    if (stream_is_capturing(st)) { set_error("%s: the stream is capturing", who); return AMP_ERR_STATE; }
    // copy into the pinned mirror (a pageable destination would make the copy itself a second, staged wait), then ONE blocking
    // wait: the thread sleeps until the stream drains -- it must not spin, CPU time is what a container's quota meters
    // (profiles/r3_o_list_api_cgroup_throttle.txt: the list API's 37 / 60 ms alternation was the host being throttled)
    AMP_HIP(hipMemcpyAsync(g->host, g->dev, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    AMP_HIP(hipStreamSynchronize(st));
    g->pending = false;
    const unsigned v = *g->host;
    *g->host = 0;
    if (v == 0) return AMP_OK;
    AMP_HIP(hipMemsetAsync(g->dev, 0, sizeof(unsigned), st));
    set_error("%s", kRangeMsg);
    return AMP_ERR_RANGE;
}

// Process-wide default for handles created from now on: AMP_PRECISION=f32|f16x3, amp_set_precision().
static int g_precision = -1;
int default_precision() {
    if (g_precision < 0) {
        const char* e = getenv("AMP_PRECISION");
        g_precision = (e && (!strcmp(e, "f32") || !strcmp(e, "fp32"))) ? PREC_F32 : PREC_F16X3;
    }
    return g_precision;
}

// ---- launch-policy switches (amp_host.h: Config) ------------------------------------------------------------
Config::Config() {
    auto num = [](const char* name, int lo, int hi, int dflt) {
        const char* e = getenv(name);
        if (!e || !*e) return dflt;
        const int v = atoi(e);
        return (v < lo || v > hi) ? dflt : v;
    };
    rb_fusion = num("AMP_RB_FUSION", 0, 3, 1);
    rb_guards = num("AMP_RB_GUARDS", -1, 1, -1);
    if (const char* e = getenv("AMP_RB_SPLIT_PLAN")) {   // "3" | "2,1" | "1,2" | "1,1,1"; anything else: the plan
        int v[3] = {0, 0, 0};
        const int n = sscanf(e, "%d,%d,%d", &v[0], &v[1], &v[2]);
        int sum = 0;
        for (int i = 0; i < 3; ++i) sum += (i < n && v[i] > 0) ? v[i] : 0;
        if (n >= 1 && sum == 3 && v[0] > 0 && (n < 2 || v[1] > 0) && (n < 3 || v[2] > 0))
            for (int i = 0; i < 3; ++i) rb_plan[i] = i < n ? v[i] : 0;
    }
    ampb_fusion = num("AMP_AMPB_FUSION", 0, 3, 1);
    rb_streams = num("AMP_RB_STREAMS", -1, 1, -1);
    // a deployment that still sets one of the switches round 5 removed must hear about it -- once, here (AMP_GROUP_MB bounded the
    // generator workspace: 168 MB instead of 2.7 GB at config 2; without a word the full-size workspace comes back after an upgrade)
    static const char* const kRemoved[][2] = {
        {"AMP_GROUP_MB", "amp_set_group_mb(megabytes)"}, {"AMP_PAIR_STRIP", "amp_set_pair_strips(mode)"}, {"AMP_CONV_BLK", "amp_set_conv_blk(mode)"},
        {"AMP_FUSE_PAIRS", "nothing (the fused pairs are the only form)"}, {"AMP_RB_SUM_FRAMES", "nothing"},
        {"AMP_RB_HORIZONTAL", "amp_set_resblock_streams(mode)"}, {"AMP_RB_HORIZONTAL_FRAMES", "amp_set_resblock_streams(mode)"}};
    for (const auto& r : kRemoved) {
        const char* e = getenv(r[0]);
        if (e && *e) fprintf(stderr, "libamphion_hip: the environment variable %s=%s is no longer read (removed in ABI 142); use %s\n", r[0], e, r[1]);
    }
}
Config& cfg() { static Config c; return c; }

int device_upload(const void* host, size_t bytes, void** out) {
    void* p = nullptr;
    AMP_HIP(hipMalloc(&p, bytes));
    const hipError_t e = hipMemcpy(p, host, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(p);
        set_error("hipMemcpy of %zu bytes to the device failed: %s", bytes, hipGetErrorString(e));
        return AMP_ERR_HIP;
    }
    *out = p;
    return AMP_OK;
}

}  // namespace amp

using namespace amp;

extern "C" {

// 100: round 1; 120: + amp_conv_create_gated / amp_wn_forward / amp_conv_act_forward, switches; 122: + amp_set_conv_blk / _conv_rg_fast /
// _pingpong; 130 (round 3's ABI, numbered in round 4): amp_mel_desc grew four trailing fields, + amp_resblock_forward /
// amp_set_resblock_fusion / amp_gen_kernel_name; 140: amp_mel_desc.struct_size, + amp_ampblock_forward / amp_set_ampblock_fusion / amp_mel_init;
// 141 (additive): the ragged / fused entry points of the VITS text side (amp_conv_forward_ragged, amp_layer_norm_c_ragged, amp_dwconv_layer_norm_c,
// amp_rel_attention_strided, amp_set_rel_attention_tiled, amp_expand_path_strided); 142 (round 5, REMOVALS): amp_conv_act_forward, amp_set_fuse_act,
// amp_set_wn_layer_fusion are gone with the kernels behind them (never chosen by the launch policy), amp_set_pair_strips(1) is refused; amp_mel_forward
// accepts every n_fft in [64, 4096]; 143 (additive): the Vocos entry points amp_pw_create / amp_pw_forward / amp_pw_precision / amp_pw_destroy and
// amp_istft_same_polar, amp_dwconv_layer_norm_c takes K = 7; 144 (additive): the DiffWave entry points amp_dw_* (diffwave.hip); 145 / 146 (additive): the codec entry
// points (fvq.hip, codec.hip); 147 (additive): amp_dwconv_layer_norm_c_causal, amp_fvq_encode_ex, amp_fvq_decode_add, amp_semantic_prepare;
// 148 (additive): FACodec's anti-aliased residual unit amp_aa_unit_* and amp_set_aa_unit_fusion (codec.hip, aa_unit_f16x3.hip);
// 149 (additive): SpeechTokenizer's amp_elu_pad (seanet.hip), amp_lstm_* (lstm.hip) and amp_evq_* (evq.hip); 150 (additive): amp_dsconv_* and amp_gelu;
// 151 (additive): amp_set_strip_fit and amp_pair_strip_plan (fitted strips of the fused-pair strip kernel, conv_host.hip strip_geometry);
// 152 (additive): FACodec voice conversion's amp_layer_norm_c_style, amp_embed_sum_c and amp_embed_sum_check (vits_text.hip);
// 153 (additive): the flow-matching transformer's amp_rope_attention, amp_rms_norm_c_adaptive, amp_silu and amp_swiglu (llama_nar.hip)
// 154 (additive): amp_mask_sample (maskgct.hip); amp_rope_attention at head dimension 96
// 155 (additive): the autoregressive transformer's amp_rope_attention_causal (llama_nar.hip) and amp_kv_append, amp_attention_decode,
// amp_pw_forward_vec and amp_ar_sample with their workspace queries (llama_ar.hip)
// 156 (additive): FastSpeech2 / JETS inference -- amp_mh_attention (llama_nar.hip's kernel without rotation, head dimension 128) and
// amp_fs2_durations, amp_bucketize_embed_add, amp_layer_norm_c_head (fastspeech.hip)
// 157 (additive): NaturalSpeech2 inference -- amp_cross_attention (llama_nar.hip's kernel without rotation at head dimension 64, separate query and
// key extents), amp_ns2_layer_* (ns2_layer_f16x3.hip) and amp_ns2_ode_step (ns2.hip)
// 158 (additive): VALL-E inference -- amp_prefix_attention (llama_nar.hip's causal kernel without rotation, with a run-time prefix) and
// amp_pw_forward_vec_ln, amp_embed_pos (valle.hip)
// 159 (additive): AudioLDM text-to-audio -- amp_conv2d_* (conv2d_f16x3.hip), amp_group_norm_stats, amp_group_norm, amp_geglu (tta.hip) and
// amp_cross_attention_hd: amp_cross_attention at head dimensions 32 and 128 beside 64 (llama_nar.hip)
// 160 (additive): amp_set_rb_guards, amp_set_rb_split_plan, amp_rb_launch_plan and amp_resblock_forward_ex (real x in the whole-ResBlock
// kernel's guard columns and the launch plan of a resblock, conv_host.hip rb_geometry / rb_plan)
int amp_version(void) { return 160; }
const char* amp_last_error(void) { return g_err; }

int amp_set_precision(int precision) {
    if (precision != AMP_PRECISION_F32 && precision != AMP_PRECISION_F16X3) {
        set_error("amp_set_precision: unknown precision %d", precision);
        return AMP_ERR_INVALID;
    }
    g_precision = precision;
    return AMP_OK;
}

int amp_get_precision(void) { return default_precision(); }

int amp_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int amp_set_pair_strips(int on) {
    if (on < -1 || on > 0) { set_error("amp_set_pair_strips: %d (-1 the policy, 0 the per-tile kernel everywhere; the four-wave strips of mode 1 left in ABI 142)", on); return AMP_ERR_INVALID; }
    cfg().pair_strips = on;
    return AMP_OK;
}

int amp_set_strip_fit(int mode) {
    if (mode < -1 || mode > 1) { set_error("amp_set_strip_fit: %d (-1 the plan, 0 never: shifted strips, 1 every strip launch)", mode); return AMP_ERR_INVALID; }
    cfg().strip_fit = mode;
    return AMP_OK;
}

int amp_pair_strip_plan(int B, int T, int k, int ragged, int* form, int* strip_len, int* strips_per_item, int* steps) {
    if (B < 1 || T < 1 || !form || !strip_len || !strips_per_item || !steps) { set_error("amp_pair_strip_plan: B=%d T=%d or a null result pointer", B, T); return AMP_ERR_INVALID; }
    if (!pair_strip_plan(B, T, k, ragged != 0, form, strip_len, strips_per_item, steps)) { set_error("amp_pair_strip_plan: no strip kernel for k=%d", k); return AMP_ERR_UNSUPPORTED; }
    return AMP_OK;
}

int amp_set_group_mb(int megabytes) {
    if (megabytes < 0) { set_error("amp_set_group_mb: %d", megabytes); return AMP_ERR_INVALID; }
    cfg().group_bytes = (size_t)megabytes << 20;
    return AMP_OK;
}

int amp_set_resblock_streams(int mode) {
    if (mode < -1 || mode > 1) { set_error("amp_set_resblock_streams: mode=%d", mode); return AMP_ERR_INVALID; }
    cfg().rb_streams = mode;
    return AMP_OK;
}

int amp_set_small_conv(int on) {
    cfg().small_conv = on ? 1 : 0;
    return AMP_OK;
}

int amp_set_pingpong(int on) {
    cfg().pingpong = on < 0 ? kPingPongDefault : (on ? 1 : 0);   // -1: back to the default
    return AMP_OK;
}

int amp_set_conv_rg_fast(int on) {
    cfg().conv_rg_fast = on < 0 ? kConvRgFastDefault : (on ? 1 : 0);   // -1: back to the default
    return AMP_OK;
}

int amp_set_conv_blk_narrow(int on) {
    if (on < -1 || on > 2) { set_error("amp_set_conv_blk_narrow: %d (0 off, 1 policy: 128-row convs with k >= 7, 2 every 128-row conv, -1 default)", on); return AMP_ERR_INVALID; }
    cfg().narrow_blk = on < 0 ? 1 : on;
    return AMP_OK;
}

int amp_set_conv_blk(int mode) {
    if (mode < -1 || mode > 3) { set_error("amp_set_conv_blk: mode %d (0 off, 1 | 2 chunks per staging round, 3 = 2 + k = 7 / 11, -1 default)", mode); return AMP_ERR_INVALID; }
    cfg().conv_blk = mode < 0 ? kConvBlkDefault : mode;
    return AMP_OK;
}

int amp_set_resblock_fusion(int mode) {
    if (mode < -1 || mode > 3) { set_error("amp_set_resblock_fusion: mode=%d", mode); return AMP_ERR_INVALID; }
    cfg().rb_fusion = mode < 0 ? 1 : mode;
    return AMP_OK;
}

int amp_set_rb_guards(int mode) {
    if (mode < -1 || mode > 1) { set_error("amp_set_rb_guards: %d (-1 the policy, 0 never: zero guards, 1 wherever the first conv's reach fits)", mode); return AMP_ERR_INVALID; }
    cfg().rb_guards = mode;
    return AMP_OK;
}

int amp_set_rb_split_plan(int n, const int* counts) {
    int v[3] = {0, 0, 0}, sum = 0;
    if (n < 0 || n > 3 || (n > 0 && !counts)) { set_error("amp_set_rb_split_plan: n=%d (0 the plan, 1 .. 3 launches)", n); return AMP_ERR_INVALID; }
    for (int i = 0; i < n; ++i) { v[i] = counts[i]; sum += v[i]; if (v[i] < 1) sum = -99; }
    if (n > 0 && sum != 3) { set_error("amp_set_rb_split_plan: the launches must hold 1+ pairs each and 3 together"); return AMP_ERR_INVALID; }
    for (int i = 0; i < 3; ++i) cfg().rb_plan[i] = v[i];
    return AMP_OK;
}

int amp_rb_launch_plan(int C, int k, const int* dilations, int n_pairs, int B, int T, int ragged, int* n_launches, int* pairs, int* gx,
                       int* out_columns, int* tiles_per_item) {
    if (B < 1 || T < 1 || n_pairs < 1 || n_pairs > AMP_RB_MAX_PAIRS || !dilations || !n_launches || !pairs || !gx || !out_columns || !tiles_per_item) {
        set_error("amp_rb_launch_plan: B=%d T=%d n_pairs=%d or a null pointer", B, T, n_pairs);
        return AMP_ERR_INVALID;
    }
    const int form = rb_form_of(C, k);
    int dil[AMP_RB_MAX_PAIRS] = {1, 1, 1};
    for (int p = 0; p < n_pairs; ++p) dil[p] = dilations[p];
    const RbPlan pl = rb_plan(C, k, dil, n_pairs, B, T, ragged != 0);
    *n_launches = pl.n;
    for (int l = 0, first = 0; l < pl.n; first += pl.count[l++]) {
        const RbGeom g = rb_geometry(C, k, dil, first, pl.count[l], T, form);
        if (g.W <= 0 || g.NT <= 0) { set_error("amp_rb_launch_plan: no whole-resblock kernel for C=%d k=%d under the current fusion mode", C, k); return AMP_ERR_UNSUPPORTED; }
        pairs[l] = pl.count[l]; gx[l] = g.gx; out_columns[l] = g.NT; tiles_per_item[l] = g.tiles;
    }
    return AMP_OK;
}

int amp_set_ampblock_fusion(int mode) {
    if (mode < -1 || mode > 3) { set_error("amp_set_ampblock_fusion: mode=%d", mode); return AMP_ERR_INVALID; }
    cfg().ampb_fusion = mode < 0 ? 1 : mode;
    return AMP_OK;
}

int amp_range_check(void* stream_) {
    return range_check_sync(guard_for_current_device(), (hipStream_t)stream_, "amp_range_check");
}

}  // extern "C"
