// Host side of libamphion_hip.so: handles, weight-norm folding, MFMA-fragment packing, forward
// orchestration and the extern "C" entry points declared in include/amphion_hip.h.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "amp_internal.h"

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

#define AMP_HIP(expr)                                                                  \
    do {                                                                               \
        hipError_t e__ = (expr);                                                       \
        if (e__ != hipSuccess) {                                                       \
            set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
            return AMP_ERR_HIP;                                                        \
        }                                                                              \
    } while (0)

// ------------------------------------------------------------------------------------------------
// per-tap-count kernel dispatch
// ------------------------------------------------------------------------------------------------
// The tap counts each per-tap-count kernel family is compiled for: CONV_TAPS, BLK_TAPS, SMALL_TAPS, PAIR_TAPS, RB_TAPS and AMPB_TAPS in
// build.py (a count listed here but not built there is an undefined symbol when the library links).
template <int... K> struct Taps { static constexpr int list[] = {K...}; };
using ConvTaps = Taps<1, 2, 3, 5, 7, 11>;   // conv_mfma.hip, conv_f16x3.hip
using BlkTaps = Taps<2, 3, 7, 11>;          // conv_blk_f16x3.hip
using SmallTaps = Taps<1, 3, 5, 7, 11>;     // conv_small_f16x3.hip
using PairTaps = Taps<3, 5, 7, 11>;         // pair_f16x3.hip, pair_strip_f16x3.hip
using RbTaps = Taps<3, 5, 7, 11>;           // rb_f16x3.hip
using AmpbTaps = Taps<3, 5, 7, 11>;         // ampb_f16x3.hip

// f(std::integral_constant<int, K>{}) for the K of the list that equals the runtime tap count k; `dflt` when k is not in the list
template <int... K, typename R, typename F>
static R with_taps(Taps<K...>, int k, R dflt, F&& f) {
    R r = dflt;
    (void)((k == K && (r = f(std::integral_constant<int, K>{}), true)) || ...);
    return r;
}

static hipError_t launch_conv(const ConvPlan& p, const ConvArgs& a, hipStream_t s) {
    return with_taps(ConvTaps{}, p.KT, hipErrorInvalidValue, [&](auto K) { return launch_conv<K>(p, a, s); });
}
static hipError_t launch_conv_f16x3(const ConvPlan& p, const ConvArgs& a, hipStream_t s) {
    return with_taps(ConvTaps{}, p.KT, hipErrorInvalidValue, [&](auto K) { return launch_conv_f16x3<K>(p, a, s); });
}
static int conv_blk_nt(int k, int cm, int halo) { return with_taps(BlkTaps{}, k, 0, [&](auto K) { return conv_blk_nt<K>(cm, halo); }); }
static hipError_t launch_conv_blk(int k, int cm, int wn, const ConvArgs& a, hipStream_t s) {
    return with_taps(BlkTaps{}, k, hipErrorInvalidValue, [&](auto K) { return launch_conv_blk<K>(cm, wn, a, s); });
}
static hipError_t launch_conv_small(int k, int ni, int epi, const ConvArgs& a, hipStream_t s) {
    return with_taps(SmallTaps{}, k, hipErrorInvalidValue, [&](auto K) { return launch_conv_small<K>(ni, epi, a, s); });
}
static int pair_tile(int k, int C, int dil) { return with_taps(PairTaps{}, k, 0, [&](auto K) { return pair_tile<K>(C, dil); }); }
static hipError_t launch_pair(int k, const PairArgs& a, hipStream_t s) {
    return with_taps(PairTaps{}, k, hipErrorInvalidValue, [&](auto K) { return launch_pair<K>(a, s); });
}
static int strip_step(int k, int C, int dil, int wide, int* wg) {
    return with_taps(PairTaps{}, k, 0, [&](auto K) { return strip_step<K>(C, dil, wide, wg); });
}
static hipError_t launch_strip(int k, const PairArgs& a, hipStream_t s) {
    return with_taps(PairTaps{}, k, hipErrorInvalidValue, [&](auto K) { return launch_strip<K>(a, s); });
}
static int rb_tile(int k, int C, int max_dil, int wide) { return with_taps(RbTaps{}, k, 0, [&](auto K) { return rb_tile<K>(C, max_dil, wide); }); }
static hipError_t launch_rb(int k, const RbArgs& a, int wide, hipStream_t s) {
    return with_taps(RbTaps{}, k, hipErrorInvalidValue, [&](auto K) { return launch_rb<K>(a, wide, s); });
}
static int ampb_tile(int k, int C, int max_dil, int wide) {
    return with_taps(AmpbTaps{}, k, 0, [&](auto K) { return ampb_tile<K>(C, max_dil, wide); });
}
static hipError_t launch_ampb(int k, const AmpbArgs& a, int wide, hipStream_t s) {
    return with_taps(AmpbTaps{}, k, hipErrorInvalidValue, [&](auto K) { return launch_ampb<K>(a, wide, s); });
}

// ---- f16 operand-range guard -------------------------------------------------------------------------------------
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
static RangeGuard g_guard[64];                    // op-level launches (amp_conv_forward, amp_pair_forward, ...): one word per device
__thread std::string* tl_kernel_log = nullptr;    // amp_internal.h: note_kernel()
__thread char tl_last_kernel[160] = "";
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

static bool guard_init(RangeGuard& g) {
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

static void guard_free(RangeGuard& g) {
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

// non-blocking: reports (and clears) a flag whose copy has already landed
static int range_poll(RangeGuard* g, hipStream_t st) {
    if (!g || !g->dev || !g->pending || stream_is_capturing(st)) return AMP_OK;
    if (hipEventQuery(g->ev) != hipSuccess) return AMP_OK;       // still in flight
    g->pending = false;
    if (*g->host == 0) return AMP_OK;
    *g->host = 0;
    AMP_HIP(hipMemsetAsync(g->dev, 0, sizeof(unsigned), st));
    set_error("%s", kRangeMsg);
    return AMP_ERR_RANGE;
}

// enqueue the copy of the flag behind everything launched so far on `st`
static int range_publish(RangeGuard* g, hipStream_t st) {
    if (!g || !g->dev || stream_is_capturing(st)) return AMP_OK;
    AMP_HIP(hipMemcpyAsync(g->host, g->dev, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    AMP_HIP(hipEventRecord(g->ev, st));
    g->pending = true;
    return AMP_OK;
}

// synchronising check of one guard
static int range_check_sync(RangeGuard* g, hipStream_t st, const char* who) {
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
static int default_precision() {
    if (g_precision < 0) {
        const char* e = getenv("AMP_PRECISION");
        g_precision = (e && (!strcmp(e, "f32") || !strcmp(e, "fp32"))) ? PREC_F32 : PREC_F16X3;
    }
    return g_precision;
}

static int round_up_taps(int ntaps) {
    for (int kt : ConvTaps::list)
        if (kt >= ntaps) return kt;
    return -1;
}

bool choose_plan(int KT, int M, int halo_total, int /*Tq*/, ConvPlan* plan) {
    bool ok = false;
    for (int kt : ConvTaps::list) ok |= (kt == KT);
    if (!ok || halo_total > 128) return false;
    plan->KT = KT;
    plan->HALO = halo_total <= 64 ? 64 : 128;
    if (M > 64) { plan->WM = 4; plan->WN = 1; plan->NI = 8; }
    else if (M > 32) { plan->WM = 2; plan->WN = 2; plan->NI = 8; }
    else { plan->WM = 1; plan->WN = 4; plan->NI = 4; }
    return true;
}

// ---- launch-policy switches: ONE configuration, read from the environment once (first use) and changed afterwards only
// through the amp_set_* entry points the tests use for their bitwise A/B comparisons.  Nothing on a launch path calls getenv.
// Environment forms exist for the FOUR switches a deployment may want without code (round 5 dropped AMP_FUSE_PAIRS, AMP_PAIR_STRIP,
// AMP_CONV_BLK, AMP_RB_SUM_FRAMES, AMP_RB_HORIZONTAL, AMP_RB_HORIZONTAL_FRAMES and AMP_GROUP_MB: amp_set_* or nothing):
//   AMP_PRECISION     f32 | f16x3       arithmetic of the conv contractions (amp_set_precision), read in precision()
//   AMP_RB_FUSION     0 .. 3            whole-ResBlock kernel: off | policy (default) | wherever built | + four-wave tiles
//   AMP_AMPB_FUSION   0 .. 3            whole-AMPBlock kernel (BigVGAN): off | policy (default) | wherever built | + four-wave tiles
//   AMP_RB_STREAMS    -1 .. 1           a stage's resblocks on concurrent streams: small launches only (default) | never | always
// (+ AMP_LAUNCH_MANIFEST=<file>, the profiling manifest above, and AMP_GRAPH_CACHE=0 on the Python side.)
constexpr int kConvBlkDefault = 3;
struct Config {
    int pair_strips = -1;      // -1 policy, 0 per-tile kernel, 1 four-wave strips
    int rb_fusion = 1;
    int ampb_fusion = 1;
    int conv_blk = kConvBlkDefault;
    size_t group_bytes = 0;
    // no environment form: bit-identical A/B switches for the tests (amp_set_small_conv / _conv_rg_fast / _pingpong)
    int small_conv = 1;
    int conv_rg_fast = 1;
    int pingpong = 1;
    int narrow_blk = 1;        // row-blocked conv kernel for 128- / 64-row convs (amp_set_conv_blk_narrow)
    int rb_streams = -1;       // resblocks of a stage on concurrent streams: -1 small launches only, 0 never, 1 always (amp_set_resblock_streams)
    Config() {
        auto num = [](const char* name, int lo, int hi, int dflt) {
            const char* e = getenv(name);
            if (!e || !*e) return dflt;
            const int v = atoi(e);
            return (v < lo || v > hi) ? dflt : v;
        };
        rb_fusion = num("AMP_RB_FUSION", 0, 3, 1);
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
};
static Config& cfg() { static Config c; return c; }

// Which fused-pair kernel a (C, k) pair runs.  Results are bit-identical either way (tests/test_gpu_pair.py); the choice
// is measured (profiles/r2_cd_strip_kernel.txt, r2_j_strip_policy.txt): the strip-mined kernel (pair_strip_f16x3.hip)
// removes the k - 1 seam columns and most of the halo re-staging but gives up the free load balancing of 12 000
// independent tiles: in its 4-wave form it wins 1.5 % on the k = 11, C = 128 pairs and loses everywhere else.  Its
// 2 x 2-blocked form (a wave owns 64 rows x 96 columns, one workgroup per CU, 512 registers: half the LDS reads per
// MFMA) wins 2-5 % for k >= 7 at C = 128 -- the policy at the end of strip_choice().
//   amp_set_pair_strips(-1): the measured policy below;  0: per-tile kernel everywhere (the bitwise cross-check of the strips).
struct StripChoice { bool use; int wide; int steps; };   // wide: 3 the A-ring form (the only strip form left); steps = 0: the planner sizes the strips
static StripChoice strip_choice(int C, int k) {
    const int mode = cfg().pair_strips;
    if (mode == 0) return {false, 0, 0};
    // measured policy.  C = 128, k in {7, 11}: the 2 x 2-blocked strips with an A-fragment ring, 64 x 128-column wave tiles, one
    // 256-column step per strip (pair_strip_f16x3.hip; profiles/r2_aw_strip_ring.txt: k = 11 1.86 ms against 2.23 for the per-tile
    // kernel, k = 7 1.27 against 1.43; inside the forward 1.88 / 1.31 ms, profiles/r3_a_kernel_stats.csv).  Everything else: per-tile
    // kernel (the four-wave strips win 1.5 % at C = 128, k = 11 only; wide 8-wave tiles, de-phased workgroups and the whole-chunk
    // 2 x 2 form were measured neutral or slower in round 2 and are gone; the C = 64 ring strips won 5 % at k = 11 in round 3's
    // first visit and were then overtaken by the whole-resblock kernel, rb_form() below -- removed as unreachable).
    if (C == 128 && (k == 7 || k == 11)) return {true, 3, 1};
    return {false, 0, 0};
}

// Strip plan: `spi` workgroups per item, each walking ceil((L + k - 1) / n1) steps of n1 columns.  The chip holds
// `slots` workgroups at a time; cost = rounds of workgroups x steps per workgroup (+ a per-workgroup constant for
// the pipeline fill), minimised over spi -- long strips waste the least (k - 1 columns once per strip), but a
// single utterance still has to spread over all CUs.
static void strip_plan(int B, int T, int n1, int hb, int wg_per_cu, int* strip_len, int* spi_out) {
    const int slots = wg_per_cu * 256;
    long best = -1; int best_spi = 1;
    const int max_spi = (T + n1 - 1) / n1;
    for (int spi = 1; spi <= max_spi; ++spi) {
        const int L = (T + spi - 1) / spi;
        if ((long)(spi - 1) * L >= T) continue;              // the last strip would be empty
        const long steps = (L + hb + n1 - 1) / n1;
        const long rounds = ((long)B * spi + slots - 1) / slots;
        const long cost = rounds * (4 * steps + 1);          // quarter-step fill per workgroup
        if (best < 0 || cost < best) { best = cost; best_spi = spi; }
    }
    *spi_out = best_spi;
    *strip_len = (T + best_spi - 1) / best_spi;
}

// The strips a launch gets: the planner's, or `steps` fixed steps per strip where the launch policy names them (steps = 1: the measured
// choice of rounds 2-4 -- with long strips every CU walks its own 16-KB-spaced region in lockstep and a step takes 15 % longer, round 5
// re-measured it: profiles/r5_j_pair_strip_stamps.txt table 5).  Round 5: FOUR steps per strip where the grid still fills the chip four
// times over -- the k - 1 columns a strip computes and throws away and the pipeline fill are paid once per 1 014 outputs instead of
// once per 246: -1 % per launch at B = 64, T = 16 384 (k = 11: 1.928 -> 1.892 ms), same bits (every output's operation order is that of
// any other cut, tests/test_gpu_pair.py).  Ragged batches keep the one-step strips they were measured with.
static void strip_geometry(int B, int T, int n1, int hb, int wg_per_cu, int steps, bool ragged, int* strip_len, int* spi) {
    strip_plan(B, T, n1, hb, wg_per_cu, strip_len, spi);
    if (steps > 0 && steps * n1 - hb < T) { *strip_len = steps * n1 - hb; *spi = (T + *strip_len - 1) / *strip_len; }
    if (steps == 1 && !ragged && 4 * n1 - hb < T) {
        const int len4 = 4 * n1 - hb, spi4 = (T + len4 - 1) / len4;
        if ((long long)B * spi4 >= 1024) { *strip_len = len4; *spi = spi4; }
    }
}

// Half-width conv tiles (NI = 2) for launches that would leave most CUs idle (a single utterance): conv_run()
// picks them when the full-width grid has fewer workgroups than kSmallGridWorkgroups (the chip holds 2 per CU).
// One 3-s utterance 1.56 -> 1.24 ms, one 10-s utterance 2.80 -> 2.38 ms; the frame-rate convs of VITS (short
// contractions) neither gain nor lose (profiles/r1_exp_small_tiles.txt).
constexpr long long kSmallGridWorkgroups = 384;

// Frame-rate convs (K = Cin * k short, grids of a few hundred workgroups) run on conv_small_f16x3.hip: whole-K
// staging, one memory latency instead of one per chunk (same bits as conv_f16x3.hip).
// amp_set_small_conv(0) keeps them on the pipelined kernel (A/B switch, tests/test_gpu_conv.py).
static bool small_conv_enabled() { return cfg().small_conv != 0; }

// Row-blocked conv kernel (conv_blk_f16x3.hip: 64 rows per wave, 256 per workgroup) for the short tap loops -- the
// transposed convs (2 taps per chunk) and k = 3 convs -- whose GEMM rows are a multiple of 256; same bits as
// conv_f16x3.hip.  amp_set_conv_blk: 0 off, 1 one 16-channel chunk per staging round, 2 two chunks per
// round where the kernel has that variant (transposed convs), 3 (default) = 2 + the A-fragment-ring form for k = 7 / 11.
static int conv_blk_mode() { return cfg().conv_blk; }
static int narrow_blk_mode() { return cfg().narrow_blk; }
// Convs with more than one row group (M > 32 * WM rows: the C = 256 stage, the transposed convs' polyphase rows) launch a
// 1-D grid with the row group as the fastest index, so that the row groups of one x tile run back to back on one XCD and x
// comes from HBM once (ConvArgs::row_groups).  amp_set_conv_rg_fast(0): the 2-D grid (row group =
// blockIdx.y, dispatched a whole grid.x apart).
// Only while the packed weights of ALL row groups fit one XCD's 4-MB L2 beside the activations (<= 3 MB): the workgroups
// resident on an XCD then stream every row group's A fragments at once.  Measured (profiles/r2_ak_row_group_order.txt,
// FETCH_SIZE per launch): ConvT 256 -> 128 (2.1 MB of weights) 627 -> 459 MB, C = 256 k = 11 / 7 (2.9 / 1.8 MB) 422 -> 369 /
// 386 -> 293 MB, but ConvT 512 -> 256 (8.4 MB) 269 -> 417 MB; launch times unchanged either way (these kernels are not
// HBM-bound: the bytes are energy, not time).
constexpr size_t kConvRgFastMaxWeightBytes = 3u << 20;
constexpr int kConvRgFastDefault = 1;
static bool conv_rg_fast() { return cfg().conv_rg_fast != 0; }
// Ping-pong tile order: every other conv / pair launch walks its tiles from the last item's end backwards, so that it starts
// on the part of its input the previous launch wrote last (still in the Infinity Cache).  amp_set_pingpong.
// Measured (profiles/r2_am_pingpong.txt, one box, alternating runs): config 2 30.99 -> 30.87 ms, the gain in the HBM-leaning
// stages (C = 64: 7.20 -> 7.15 ms, C = 32: 4.40 -> 4.32 ms); C3 / C5 unchanged.
constexpr int kPingPongDefault = 1;
static thread_local unsigned g_launch_parity = 0;
static int next_rev(const int* lens) {
    if (!cfg().pingpong || lens) return 0;   // ragged batches keep the dispatch order
    return (int)(g_launch_parity++ & 1u);
}
// the blocked launch fills the chip only when its (half as many) workgroups still give every CU its two
constexpr long long kConvBlkMinWorkgroups = 512;

}  // namespace amp

using namespace amp;

// ------------------------------------------------------------------------------------------------
// amp_conv: one (transposed) convolution with packed weights on the device
// ------------------------------------------------------------------------------------------------
struct amp_conv {
    int transposed = 0, cin = 0, cout = 0, k = 0, stride = 1, dilation = 1, padding = 0;
    // GEMM view
    int M = 0, ntaps = 0, KT = 0, off0 = 0, dstep = 0, halo_left = 0, halo_right = 0, up = 1, up_pad = 0;
    int nchunks = 0;
    int precision = PREC_F32;  // arithmetic of the contraction, fixed at build time
    int pad_reflect = 0, tanh_out = 0;  // amp_conv_set_option
    int gated_H = 0;           // > 0: rows packed for the gate epilogue of conv_small_f16x3.hip (amp_conv_create_gated)
    int Mpad = 0;              // rows of the packed weight
    float wscale = 1.f;        // f16x3: power of two applied to the packed weights
    ConvPlan plan{};
    void* wp_dev = nullptr;
    float* bias_dev = nullptr;
    // folded weights kept on the host for the Cout==1 path (conv_post)
    ~amp_conv() {
        if (wp_dev) (void)hipFree(wp_dev);
        if (bias_dev) (void)hipFree(bias_dev);
    }
};

static int conv_build(amp_conv* c, const float* w, const float* bias) {
    if (c->cin <= 0 || c->cout <= 0 || c->k <= 0 || c->stride <= 0 || c->dilation <= 0) {
        set_error("amp_conv: bad dimensions cin=%d cout=%d k=%d stride=%d dilation=%d", c->cin, c->cout, c->k, c->stride,
                  c->dilation);
        return AMP_ERR_INVALID;
    }
    if (!c->transposed) {
        if (c->stride != 1) { set_error("amp_conv: strided Conv1d is not on the vocoder path"); return AMP_ERR_UNSUPPORTED; }
        c->up = 1; c->up_pad = 0;
        c->M = c->cout;
        c->ntaps = c->k;
        c->off0 = -c->padding;     // y[t] = sum_j w[j] x[t - pad + j*dil]
        c->dstep = c->dilation;
    } else {
        if (c->dilation != 1) { set_error("amp_conv: dilated ConvTranspose1d unsupported"); return AMP_ERR_UNSUPPORTED; }
        c->up = c->stride; c->up_pad = c->padding;
        c->M = c->cout * c->stride;
        c->ntaps = (c->k + c->stride - 1) / c->stride;
        c->off0 = 0;
        c->dstep = -1;             // tap s reads x[q - s]
    }
    c->KT = round_up_taps(c->ntaps);
    if (c->KT < 0) { set_error("amp_conv: %d taps unsupported (max 11)", c->ntaps); return AMP_ERR_UNSUPPORTED; }
    const int omin = c->dstep >= 0 ? c->off0 : c->off0 + (c->KT - 1) * c->dstep;
    const int omax = c->dstep >= 0 ? c->off0 + (c->KT - 1) * c->dstep : c->off0;
    c->halo_left = omin < 0 ? -omin : 0;
    c->halo_right = omax > 0 ? omax : 0;
    if (!choose_plan(c->KT, c->M, c->halo_left + c->halo_right, 0, &c->plan)) {
        set_error("amp_conv: receptive field (k=%d, dilation=%d) exceeds the 128-column staged halo", c->k, c->dilation);
        return AMP_ERR_UNSUPPORTED;
    }
    c->precision = default_precision();
    if (c->precision == PREC_F16X3) c->plan.NI = 4;  // conv_f16x3.hip keeps 4 accumulator tiles per wave
    const int Mg = c->plan.Mgroup();
    const int Mpad = ((c->M + Mg - 1) / Mg) * Mg;
    c->Mpad = Mpad;
    const int nmb = Mpad / 32;
    const int cin = c->cin, cout = c->cout, k = c->k, up = c->up;
    // W'[m, i, g]: the GEMM-view weight (polyphase rows for a transposed conv), 0 outside
    auto wview = [&](int m, int i, int g) -> float {
        if (m >= c->M || i >= cin || g >= c->ntaps) return 0.f;
        if (!c->transposed) return w[((size_t)m * cin + i) * k + g];
        const int o = m / up, r = m - o * up;
        const int j = r + g * up;
        return j < k ? w[((size_t)i * cout + o) * k + j] : 0.f;
    };
    if (c->precision == PREC_F32) {
        // ---- f32 MFMA A-fragment order: [mb][chunk8][tap][lane][p] ----
        c->nchunks = (c->cin + KC - 1) / KC;
        const size_t n = ((size_t)nmb * c->nchunks + 1) * c->KT * 64 * 4;   // +1 chunk: the kernel's A reload runs one chunk ahead
        std::vector<float> wp(n, 0.f);
        for (int mb = 0; mb < nmb; ++mb)
            for (int ch = 0; ch < c->nchunks; ++ch)
                for (int g = 0; g < c->KT; ++g)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int p = 0; p < 4; ++p)
                            wp[((((size_t)mb * c->nchunks + ch) * c->KT + g) * 64 + lane) * 4 + p] =
                                wview(mb * 32 + (lane & 31), ch * KC + 2 * p + (lane >> 5), g);
        AMP_HIP(hipMalloc(&c->wp_dev, n * sizeof(float)));
        AMP_HIP(hipMemcpy(c->wp_dev, wp.data(), n * sizeof(float), hipMemcpyHostToDevice));
    } else {
        // ---- f16x3: [mb][chunk16][tap][plane hi|lo][lane][8 x f16], weights scaled by 2^s so that
        //      max|w| lands in (2^12, 2^13]: lo = f16(w*2^s - hi) is then a normal f16 for every weight
        //      above 2^-16 of the largest, and hi stays far from the f16 overflow (conv_f16x3.hip) ----
        c->nchunks = (c->cin + KC16 - 1) / KC16;
        float wmax = 0.f;
        const size_t nw = (size_t)cin * cout * k;
        for (size_t i = 0; i < nw; ++i) wmax = fmaxf(wmax, fabsf(w[i]));
        if (!(wmax < 1e30f)) { set_error("amp_conv: non-finite weight"); return AMP_ERR_INVALID; }
        int e2 = 0;
        if (wmax > 0.f) { (void)frexpf(wmax, &e2); if (ldexpf(1.f, e2 - 1) == wmax) e2 -= 1; }  // wmax <= 2^e2
        c->wscale = wmax > 0.f ? ldexpf(1.f, 13 - e2) : 1.f;
        const size_t n16 = ((size_t)nmb * c->nchunks + 2) * c->KT * 2 * 64 * 8;  // + pad: the kernels' A reload runs one chunk (conv_blk_f16x3.hip: one round of up to 2 chunks) ahead
        std::vector<_Float16> wp(n16, (_Float16)0.f);
        for (int mb = 0; mb < nmb; ++mb)
            for (int ch = 0; ch < c->nchunks; ++ch)
                for (int g = 0; g < c->KT; ++g)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int e = 0; e < 8; ++e) {
                            const float v = wview(mb * 32 + (lane & 31), ch * KC16 + 8 * (lane >> 5) + e, g) * c->wscale;
                            const _Float16 h = (_Float16)v;
                            const _Float16 l = (_Float16)(v - (float)h);
                            const size_t ent = (((size_t)mb * c->nchunks + ch) * c->KT + g) * 2;
                            wp[((ent + 0) * 64 + lane) * 8 + e] = h;
                            wp[((ent + 1) * 64 + lane) * 8 + e] = l;
                        }
        AMP_HIP(hipMalloc(&c->wp_dev, n16 * sizeof(_Float16)));
        AMP_HIP(hipMemcpy(c->wp_dev, wp.data(), n16 * sizeof(_Float16), hipMemcpyHostToDevice));
    }
    if (bias) {
        AMP_HIP(hipMalloc((void**)&c->bias_dev, (size_t)cout * sizeof(float)));
        AMP_HIP(hipMemcpy(c->bias_dev, bias, (size_t)cout * sizeof(float), hipMemcpyHostToDevice));
    }
    return AMP_OK;
}

// bytes of the packed f16x3 A fragments of all row blocks (hi + lo planes)
static size_t conv_weight_bytes(const amp_conv* c) { return (size_t)c->Mpad * c->nchunks * KC16 * c->KT * 4; }

static int conv_out_len(const amp_conv* c, int T) {
    if (!c->transposed) return T + 2 * c->padding - c->dilation * (c->k - 1);
    return (T - 1) * c->stride - 2 * c->padding + c->k;
}

// conv_small_f16x3.hip covers: Conv1d (no polyphase rows), zero padding, 128-row workgroups, k in {1, 3, 5, 7, 11},
// Cin <= 256, receptive field <= 64 columns
static bool small_conv_static_ok(const amp_conv* c) {
    return c->precision == PREC_F16X3 && !c->transposed && !c->pad_reflect && c->plan.WM == 4 &&
           (c->KT == 1 || c->KT == 3 || c->KT == 5 || c->KT == 7 || c->KT == 11) && c->KT == c->ntaps &&
           c->nchunks <= kSmallConvMaxChunks && c->halo_left + c->halo_right <= 64;
}
static bool small_conv_covers(const amp_conv* c) { return small_conv_enabled() && small_conv_static_ok(c); }
// tile width of the whole-K kernel in 32-column units: 128 x 32 tiles (two workgroups per CU) when the receptive field
// fits their 32-column halo, else 128 x 64.
static int small_conv_ni(const amp_conv* c) { return (c->halo_left + c->halo_right <= 32) ? 1 : 2; }

// mode 0: y = v, 1: y += v, 2: y = (y + v) / div
// plan_small != nullptr: launch nothing -- if this call would run the whole-K kernel with the standard epilogue, hand back its arguments and
// tile width (for conv_small3_f16x3.hip, which runs three such convs in one grid), else AMP_ERR_UNSUPPORTED.
static int conv_run(const amp_conv* c, const float* x, int B, int T, float slope_in, const float* res, float slope_out,
                    float* y, int mode, float div, hipStream_t stream, long long xbs = 0, const int* lens = nullptr,
                    int len_mul = 1, ConvArgs* plan_small = nullptr, int* plan_ni = nullptr) {
    if (B <= 0 || T <= 0) { set_error("amp_conv_forward: B=%d T=%d", B, T); return AMP_ERR_INVALID; }
    const int Tout = conv_out_len(c, T);
    if (Tout <= 0) { set_error("amp_conv_forward: input too short (T=%d)", T); return AMP_ERR_INVALID; }
    ConvArgs a{};
    a.x = x; a.wp = c->wp_dev; a.bias = c->bias_dev; a.res = res; a.y = y;
    a.B = B; a.Cin = c->cin; a.Tin = T; a.xbs = xbs > 0 ? xbs : (long long)c->cin * T; a.nchunks = c->nchunks; a.M = c->M;
    a.Tq = c->transposed ? T + c->ntaps - 1 : Tout;
    ConvPlan plan = c->plan;
    if (c->precision == PREC_F16X3) {
        // a grid that leaves most CUs idle (a single utterance): half-width tiles, twice the workgroups
        const long long wgs = (long long)B * ((a.Tq + plan.NT() - 1) / plan.NT()) * ((c->M + plan.Mgroup() - 1) / plan.Mgroup());
        if (wgs < kSmallGridWorkgroups) plan.NI = 2;
    }
    const int NT = plan.NT();
    a.tiles_per_item = (a.Tq + NT - 1) / NT;
    a.off0 = c->off0; a.dstep = c->dstep; a.halo_left = c->halo_left;
    a.wd = NT + c->halo_left + c->halo_right;
    a.Cout = c->cout; a.Tout = Tout; a.up = c->up; a.up_pad = c->up_pad;
    a.slope_in = slope_in; a.slope_out = slope_out; a.mode = mode; a.div = div;
    a.lens = lens; a.len_mul = len_mul;
    a.pad_reflect = c->pad_reflect; a.tanh_out = c->tanh_out;
    a.range_flag = c->precision == PREC_F16X3 ? range_flag_for_current_device() : nullptr;
    a.rev = c->precision == PREC_F16X3 ? next_rev(lens) : 0;
    if (c->pad_reflect && (c->halo_left >= T || c->halo_right >= T)) {
        set_error("amp_conv_forward: reflection padding %d needs more than %d input samples", c->halo_left > c->halo_right ? c->halo_left : c->halo_right, T);
        return AMP_ERR_INVALID;
    }
    if (c->gated_H) { set_error("amp_conv_forward: a gated conv (amp_conv_create_gated) only runs inside amp_wn_forward"); return AMP_ERR_STATE; }
    if (c->precision == PREC_F16X3 && slope_in > 1.f) {
        // the f16x3 kernels form leaky_relu-on-load as max(16 x, 16 slope x) (f16x3_device.h: stage4_f16)
        set_error("amp_conv_forward: leaky_relu slope %g > 1 on the input is outside the f16x3 kernels (use AMP_PRECISION_F32)", (double)slope_in);
        return AMP_ERR_UNSUPPORTED;
    }
    if (c->precision == PREC_F32) {
        if (plan_small) return AMP_ERR_UNSUPPORTED;
        a.acc_scale = a.inv_scale = 1.f;
        AMP_HIP(launch_conv(plan, a, stream));
    } else {
        a.acc_scale = 16.f * c->wscale;
        a.inv_scale = 1.f / a.acc_scale;
        // k = 7 / 11 (long contractions: the pipelined kernel is efficient per tile) only gain from the whole-K kernel's
        // narrower tiles while the chip is badly under-filled: one 3-s utterance 1.16 -> 1.06 ms, a 10-s one 2.28 -> 2.30
        const long long wgs_half = (long long)B * ((a.Tq + 63) / 64) * ((c->M + plan.Mgroup() - 1) / plan.Mgroup());
        int blk_cm = 0, blk_nt = 0, blk_wn = 1;
        const bool blk_kt = c->KT == 2 || c->KT == 3 || (conv_blk_mode() == 3 && (c->KT == 7 || c->KT == 11));   // mode 3: + the A-ring form for k = 7 / 11
        // row groups of 256 (four waves along M), or -- round 4, Conv1d only -- 128 rows with two waves along the columns: the AMPBlock
        // convs of BigVGAN's C = 128 stage (unpaired: an activation sits between them), k = 7 / 11 under the policy (mode 1), any k in mode 2
        if (c->M % 256 == 0) blk_wn = 1;
        else if (c->M % 128 == 0 && c->KT != 2 && (narrow_blk_mode() >= 2 || (narrow_blk_mode() == 1 && c->KT >= 7))) blk_wn = 2;
        else blk_wn = 0;
        if (conv_blk_mode() > 0 && plan.NI == 4 && blk_wn > 0 && blk_kt && !c->tanh_out && !c->pad_reflect) {
            int cm = (conv_blk_mode() >= 2 && c->KT == 2 && c->nchunks % 2 == 0) ? 2 : 1;
            const int halo = c->halo_left + c->halo_right;
            const int nt = blk_wn * conv_blk_nt(c->KT, cm, halo);
            if (nt > 0 && (long long)B * ((a.Tq + nt - 1) / nt) * (c->M / (256 / blk_wn)) >= kConvBlkMinWorkgroups) { blk_cm = cm; blk_nt = nt; }
        }
        if (plan_small && !(blk_cm == 0 && plan.NI == 2 && small_conv_covers(c) && (c->KT <= 5 || wgs_half <= 128))) return AMP_ERR_UNSUPPORTED;
        if (blk_cm > 0) {
            const int rows = 256 / blk_wn;
            a.tiles_per_item = (a.Tq + blk_nt - 1) / blk_nt;
            a.wd = blk_nt + c->halo_left + c->halo_right;
            a.row_groups = (conv_rg_fast() && c->M / rows > 1 && conv_weight_bytes(c) <= kConvRgFastMaxWeightBytes) ? c->M / rows : 0;
            AMP_HIP(launch_conv_blk(c->KT, blk_cm, blk_wn, a, stream));
        } else if (plan.NI == 2 && small_conv_covers(c) && (c->KT <= 5 || wgs_half <= 128)) {
            // a small grid of a short contraction: the whole-K kernel (128 x 32 or 128 x 64 tiles, same bits)
            const int ni = small_conv_ni(c);
            a.Mpad = c->Mpad;
            a.tiles_per_item = (a.Tq + 32 * ni - 1) / (32 * ni);
            a.wd = 32 * ni + c->halo_left + c->halo_right;
            if (plan_small) { *plan_small = a; *plan_ni = ni; return AMP_OK; }
            AMP_HIP(launch_conv_small(c->KT, ni, 0, a, stream));
        } else {
            const int nrg = (c->M + plan.Mgroup() - 1) / plan.Mgroup();
            a.row_groups = (conv_rg_fast() && nrg > 1 && conv_weight_bytes(c) <= kConvRgFastMaxWeightBytes) ? nrg : 0;
            AMP_HIP(launch_conv_f16x3(plan, a, stream));
        }
    }
    return AMP_OK;
}

// Fused ResBlock1 pair (pair_f16x3.hip): y = x + c2(lrelu(c1(lrelu(x)))).  Returns false when this
// (channels, kernel, dilation, precision) is not covered and the caller must run the two convs.
static bool pair_supported(const amp_conv* c1, const amp_conv* c2) {
    if (c1->precision != PREC_F16X3 || c2->precision != PREC_F16X3) return false;
    if (c1->pad_reflect || c2->pad_reflect || c1->tanh_out || c2->tanh_out) return false;
    if (c1->transposed || c2->transposed || c1->cin != c1->cout || c2->cin != c2->cout || c1->cin != c2->cin) return false;
    if (c1->k != c2->k || c2->dilation != 1 || c1->k != c1->KT) return false;
    if (c1->padding != (c1->k - 1) / 2 * c1->dilation || c2->padding != (c2->k - 1) / 2) return false;
    if (!c1->bias_dev || !c2->bias_dev) return false;
    const StripChoice sc = strip_choice(c1->cin, c1->k);
    if (sc.use && strip_step(c1->k, c1->cin, c1->dilation, sc.wide, nullptr) > 0) return true;
    return pair_tile(c1->k, c1->cin, c1->dilation) > 0;
}

static int pair_run(const amp_conv* c1, const amp_conv* c2, const float* x, int B, int T, float slope, float* y,
                    int mode, float div, hipStream_t stream, const int* lens = nullptr, int len_mul = 1) {
    if (x == y) { set_error("pair_run: x and y must not alias"); return AMP_ERR_INVALID; }
    if (slope > 1.f) { set_error("pair_run: leaky_relu slope %g > 1 is outside the fused pair kernels", (double)slope); return AMP_ERR_UNSUPPORTED; }
    PairArgs a{};
    a.x = x; a.y = y;
    a.wp1 = c1->wp_dev; a.bias1 = c1->bias_dev; a.wp2 = c2->wp_dev; a.bias2 = c2->bias_dev;
    a.B = B; a.C = c1->cin; a.T = T;
    a.dil = c1->dilation;
    a.slope = slope;
    a.sc1 = 16.f * c1->wscale; a.isc1 = 1.f / a.sc1;
    a.sc2 = 16.f * c2->wscale; a.isc2 = 1.f / a.sc2;
    a.mode = mode; a.div = div;
    a.lens = lens; a.len_mul = len_mul;
    a.range_flag = range_flag_for_current_device();
    a.rev = next_rev(lens);
    int wg = 2;
    const StripChoice sc = strip_choice(c1->cin, c1->k);
    const int n1 = sc.use ? strip_step(c1->k, c1->cin, c1->dilation, sc.wide, &wg) : 0;
    if (n1 > 0) {
        a.wide = sc.wide;
        strip_geometry(B, T, n1, c1->k - 1, wg, sc.steps, lens != nullptr, &a.strip_len, &a.strips_per_item);
        // one workgroup per CU: a grid that cannot fill the chip twice over (a single utterance) is better served by the
        // 4x as many independent tiles of the per-tile kernel (same bits)
        if (cfg().pair_strips == -1 && sc.wide >= 2 && (long long)B * a.strips_per_item < 512 && pair_tile(c1->k, c1->cin, c1->dilation) > 0) {
            const int NT = pair_tile(c1->k, c1->cin, c1->dilation);
            a.tiles_per_item = (T + NT - 1) / NT;
            AMP_HIP(launch_pair(c1->k, a, stream));
            return AMP_OK;
        }
        AMP_HIP(launch_strip(c1->k, a, stream));
        return AMP_OK;
    }
    const int NT = pair_tile(c1->k, c1->cin, c1->dilation);
    a.tiles_per_item = (T + NT - 1) / NT;
    AMP_HIP(launch_pair(c1->k, a, stream));
    return AMP_OK;
}

// The arguments pair_run would launch the PER-TILE kernel with, without launching; false when this pair runs on the strip kernel (or
// on no fused kernel at all).  For pair3_f16x3.hip, which runs three such pairs in one grid.
static bool pair_tile_args(const amp_conv* c1, const amp_conv* c2, const float* x, int B, int T, float slope, float* y, int mode,
                           float div, const int* lens, int len_mul, PairArgs* out) {
    if (x == y || slope > 1.f || !pair_supported(c1, c2)) return false;
    PairArgs a{};
    a.x = x; a.y = y;
    a.wp1 = c1->wp_dev; a.bias1 = c1->bias_dev; a.wp2 = c2->wp_dev; a.bias2 = c2->bias_dev;
    a.B = B; a.C = c1->cin; a.T = T;
    a.dil = c1->dilation;
    a.slope = slope;
    a.sc1 = 16.f * c1->wscale; a.isc1 = 1.f / a.sc1;
    a.sc2 = 16.f * c2->wscale; a.isc2 = 1.f / a.sc2;
    a.mode = mode; a.div = div;
    a.lens = lens; a.len_mul = len_mul;
    a.range_flag = range_flag_for_current_device();
    a.rev = 0;
    int wg = 2;
    const StripChoice sc = strip_choice(c1->cin, c1->k);
    const int n1 = sc.use ? strip_step(c1->k, c1->cin, c1->dilation, sc.wide, &wg) : 0;
    if (n1 > 0) {       // pair_run's rule: the strips unless the grid cannot fill the chip twice over
        int strip_len = 0, strips_per_item = 0;
        strip_geometry(B, T, n1, c1->k - 1, wg, sc.steps, lens != nullptr, &strip_len, &strips_per_item);
        if (!(cfg().pair_strips == -1 && sc.wide >= 2 && (long long)B * strips_per_item < 512)) return false;
    }
    const int NT = pair_tile(c1->k, c1->cin, c1->dilation);
    if (NT <= 0) return false;
    a.tiles_per_item = (T + NT - 1) / NT;
    *out = a;
    return true;
}

// Whole ResBlock1 in one launch (rb_f16x3.hip): x read once, y written once per resblock, the residual carried in
// registers; bit-identical to the chain of fused pairs.  amp_set_resblock_fusion / AMP_RB_FUSION: 0 off (three pair
// launches), 1 (default) the measured policy below, 2 every shape the kernel is built for, 3 = 2 with the four-wave
// 512-column tiles at C = 32 (two workgroups per CU) instead of the eight-wave 1024-column ones.
static int rb_fusion_mode() { return cfg().rb_fusion; }
// form of the kernel for (C, k): -1 = run the pairs
static int rb_form(int C, int k) {
    const int m = rb_fusion_mode();
    if (m == 0) return -1;
    if (m == 3) return (C == 32 || (C == 64 && k <= 5)) ? 0 : 1;
    if (m == 2) return 1;
    // policy: measured INSIDE the config-2 forward at thermal steady state, one box, modes alternating
    // (profiles/r3_e_inforward_resblock_modes_and_list_api_probe.txt; ms per resblock, fused pairs -> this kernel):
    //   C = 32  k = 3 0.99 -> 0.56, k = 7 1.38 -> 1.12 with the four-wave 512-column tiles (two workgroups per CU: one's seams run
    //           under the other's MFMAs; the eight-wave 1024-column tiles: 0.66 / 1.15); k = 11 1.77 -> 1.70 with the EIGHT-wave
    //           tiles (13 % recomputed halo instead of 31 %; four-wave: 1.79)
    //   C = 64  (eight waves, 512 columns) k = 3 1.27 -> 0.98, k = 7 2.22 -> 2.05, k = 11 3.42 (ring strips) -> 3.40: a draw in time
    //           at a third of the HBM traffic -- op-level, at boost clocks, the same launch is 2.5 ms (r3_c_resblock_k11.txt): under
    //           the package power limit what counts is energy per output, and 31 % recomputed MFMAs cancel the saved HBM round trips
    //   C = 128 k = 3 (eight waves, 256 columns, 16 guard columns: 147 KB) 1.91 -> 1.70; k = 5 2.70 -> 2.53 op-level
    // forward 29.15 -> 27.5 ms on that box.
    // Round 6 (profiles/r6_h_rb_two_per_cu.txt, same method): C = 64 k = 3 as FOUR waves x 256 columns with 16 guard columns (74 KB: two workgroups per
    // CU, 232 of 256 columns kept instead of 488 of 512) 1.02-1.04 -> 0.96 ms; the same form at k = 7 (split 2 + 1: 220 of 256 kept) 2.09 -> 2.12 and
    // C = 128 k = 3 as four waves x 128 columns (104 of 128 kept) 1.74 -> 1.88 lose and were not kept.
    if (C == 32) return k >= 11 ? 1 : 0;
    if (C == 64) return k <= 5 ? 0 : 1;          // round 6: k <= 5 as four waves x 256 columns, two workgroups per CU (profiles/r6_h_rb_two_per_cu.txt)
    if (C == 128) return 1;                      // k <= 5 only (rb_tile)
    return -1;
}
// the workgroups of a launch must at least fill the chip (256 CUs): a short single utterance keeps the pairs' 4x more numerous
// tiles (same bits).  One utterance, forced either way (profiles/r3_lat_rb_threshold.txt): 3 s (134 tiles at stage 3) 1.07 ms on
// pairs against 1.11-1.17 on this kernel; 10 s (451 tiles) 2.31 against 2.23.
constexpr long long kRbMinWorkgroups = 256;

static bool rb_supported(const std::vector<std::unique_ptr<amp_conv>>& c1, const std::vector<std::unique_ptr<amp_conv>>& c2, int B, int T) {
    const int np = (int)c1.size();
    if (np < 1 || np > AMP_RB_MAX_PAIRS || (int)c2.size() != np) return false;
    int max_dil = 1, rh = 0;
    for (int p = 0; p < np; ++p) {
        if (!pair_supported(c1[p].get(), c2[p].get())) return false;
        if (c1[p]->cin != c1[0]->cin || c1[p]->k != c1[0]->k) return false;
        max_dil = c1[p]->dilation > max_dil ? c1[p]->dilation : max_dil;
        rh += (c1[p]->k - 1) / 2 * (c1[p]->dilation + 1);
    }
    const int form = rb_form(c1[0]->cin, c1[0]->k);
    if (form < 0) return false;
    const int W = rb_tile(c1[0]->k, c1[0]->cin, max_dil, form);
    if (W <= 0 || W - 2 * rh < W / 2) return false;          // at least half of every tile must be output
    const int NT = W - 2 * rh;
    if (rb_fusion_mode() == 1 && (long long)B * ((T + NT - 1) / NT) < kRbMinWorkgroups) return false;
    return true;
}

// Round 5: a resblock whose tile keeps less than 80 % of its columns (every conv is evaluated on all W columns and 2 * RH are discarded:
// C = 64, k = 11 keeps 392 of 512) runs as TWO launches, pairs [0, 2) and [2, 3): 452 of 512 columns kept in each, 13 % fewer MFMAs for one
// more trip of x through HBM.  Under the package power cap removed MFMAs convert to time in full: B = 64 3.45 -> 3.19 ms,
// B = 32 1.68 -> 1.58, B = 16 0.89 -> 0.78; B = 8 (672 workgroups) 0.431 -> 0.443, hence the 1 024-workgroup floor; k = 7 (86 % kept) and
// C = 32 k = 11 (88 %) are 1-4 % slower split (profiles/r5_l_rb_split.txt).  Same bits: what leaves a launch is the fp32 x the next pair
// would have read from registers.  Returns the number of pairs in the first launch, 0 = one launch.
static int rb_split(const std::vector<std::unique_ptr<amp_conv>>& c1, int B, int T) {
    const int np = (int)c1.size();
    if (np != 3 || rb_fusion_mode() != 1) return 0;
    int max_dil = 1, rh = 0;
    for (int p = 0; p < np; ++p) {
        max_dil = c1[p]->dilation > max_dil ? c1[p]->dilation : max_dil;
        rh += (c1[p]->k - 1) / 2 * (c1[p]->dilation + 1);
    }
    const int W = rb_tile(c1[0]->k, c1[0]->cin, max_dil, rb_form(c1[0]->cin, c1[0]->k));
    const int NT = W - 2 * rh;
    if (W <= 0 || 5 * NT >= 4 * W) return 0;
    if ((long long)B * ((T + NT - 1) / NT) < 1024) return 0;
    return 2;
}

// pairs [first, first + count) of the resblock (count < 0: all of them): x -> y
static int rb_run(const std::vector<std::unique_ptr<amp_conv>>& c1v, const std::vector<std::unique_ptr<amp_conv>>& c2v, const float* x,
                  int B, int T, float slope, float* y, int mode, float div, hipStream_t stream, const int* lens = nullptr, int len_mul = 1,
                  int first = 0, int count = -1) {
    if (x == y) { set_error("rb_run: x and y must not alias"); return AMP_ERR_INVALID; }
    if (slope > 1.f) { set_error("rb_run: leaky_relu slope %g > 1 is outside the fused kernels", (double)slope); return AMP_ERR_UNSUPPORTED; }
    RbArgs a{};
    a.x = x; a.y = y;
    a.np = count < 0 ? (int)c1v.size() - first : count;
    const std::unique_ptr<amp_conv>* c1 = c1v.data() + first;
    const std::unique_ptr<amp_conv>* c2 = c2v.data() + first;
    int max_dil = 1;
    for (int p = 0; p < a.np; ++p) {
        a.wp1[p] = c1[p]->wp_dev; a.bias1[p] = c1[p]->bias_dev; a.wp2[p] = c2[p]->wp_dev; a.bias2[p] = c2[p]->bias_dev;
        a.sc1[p] = 16.f * c1[p]->wscale; a.isc1[p] = 1.f / a.sc1[p];
        a.sc2[p] = 16.f * c2[p]->wscale; a.isc2[p] = 1.f / a.sc2[p];
        a.dil[p] = c1[p]->dilation;
        a.rh += (c1[p]->k - 1) / 2 * (c1[p]->dilation + 1);
        max_dil = c1[p]->dilation > max_dil ? c1[p]->dilation : max_dil;
    }
    for (int p = a.np; p < AMP_RB_MAX_PAIRS; ++p) {   // never dereferenced; keep the pointers valid all the same
        a.wp1[p] = a.wp1[0]; a.bias1[p] = a.bias1[0]; a.wp2[p] = a.wp2[0]; a.bias2[p] = a.bias2[0]; a.dil[p] = 1;
    }
    a.B = B; a.C = c1[0]->cin; a.T = T;
    const int form = rb_form(a.C, c1[0]->k);
    const int W = rb_tile(c1[0]->k, a.C, max_dil, form);
    const int NT = W - 2 * a.rh;
    a.tiles_per_item = (T + NT - 1) / NT;
    a.slope = slope; a.mode = mode; a.div = div;
    a.lens = lens; a.len_mul = len_mul;
    a.range_flag = range_flag_for_current_device();
    a.rev = next_rev(lens);
    AMP_HIP(launch_rb(c1[0]->k, a, form, stream));
    return AMP_OK;
}

// ------------------------------------------------------------------------------------------------
// generator handle
// ------------------------------------------------------------------------------------------------
struct HostTensor {
    std::vector<int64_t> shape;
    std::vector<float> data;
    size_t numel() const { size_t n = 1; for (auto s : shape) n *= (size_t)s; return n; }
};

struct ActParams {  // one Activation1d
    float* a_dev = nullptr;     // alpha (exp'ed when logscale)
    float* invb_dev = nullptr;  // 1 / (beta + 1e-9)
    float* fu_dev = nullptr;    // 12 taps
    float* fd_dev = nullptr;
    float* fu2_dev = nullptr;   // 2 * the up taps (UpSample1d's gain folded in, resample.py:41): what ampb_f16x3.hip reads into SGPRs
};

struct ResBlock {
    int k = 0;
    std::vector<int> dil;
    std::vector<std::unique_ptr<amp_conv>> c1, c2;  // type 2 uses c1 only
    std::vector<ActParams> acts;
};

// Whole AMPBlock1 in one launch (ampb_f16x3.hip): x read once, y written once per block, the six activations in registers;
// bit-identical to the 6 conv + 6 act1d launches.  amp_set_ampblock_fusion / AMP_AMPB_FUSION: 0 off, 1 (default) the policy
// below, 2 every shape the kernel is built for (any grid), 3 = 2 with the four-wave 512-column tiles at C = 32.
static int ampb_fusion_mode() { return cfg().ampb_fusion; }
static int ampb_form(int C, int k) {
    const int m = ampb_fusion_mode();
    if (m == 0) return -1;
    if (m == 3) return C == 32 ? 0 : 1;
    if (m == 2) return 1;
    // policy: measured INSIDE the config-3 forward (BigVGAN-base, B = 32), one box, modes alternating (tools/ampb_inforward.py,
    // profiles/r4_i_ampb_inforward.txt; ms per AMPBlock, 6 conv + 6 act1d launches -> this kernel):
    //   C = 32  k = 3 1.67 -> 1.07, k = 7 1.83 -> 1.42 with the four-wave 512-column tiles (two workgroups per CU: one's activations run
    //           under the other's MFMAs; eight-wave 1024-column tiles: 1.20 / 1.46); k = 11 2.14 -> 1.81 with the EIGHT-wave tiles (18 %
    //           recomputed halo instead of 36 %; four-wave: 1.91)
    //   C = 64  (eight waves, 512 columns, one workgroup per CU: every wave in the same phase, so MFMA and VALU time add up)
    //           k = 3 1.69 -> 1.57; k = 7 2.10 -> 2.22 and k = 11 2.51 -> 3.07 lose and stay on separate launches
    if (C == 32) return k >= 11 ? 1 : 0;
    if (C == 64) return k <= 3 ? 1 : -1;
    return -1;
}
constexpr long long kAmpbMinWorkgroups = 256;

// one-sided receptive field of the block: 5 columns per activation, (k - 1) / 2 * dilation per conv; rounded up to whole float4
static int ampb_halo(const amp_conv* const* c1, int np) {
    int rh = 0;
    for (int p = 0; p < np; ++p) rh += 10 + (c1[p]->k - 1) / 2 * (c1[p]->dilation + 1);
    return (rh + 3) & ~3;
}

static bool ampb_supported(const amp_conv* const* c1, const amp_conv* const* c2, int np, const ActParams* acts, size_t nacts, int B, int T) {
    if (np < 1 || 2 * np > AMP_AMPB_MAX_STEPS || nacts != (size_t)(2 * np)) return false;
    for (size_t i = 0; i < nacts; ++i)
        if (!acts[i].fu2_dev) return false;
    if ((T & 3) != 0) return false;                               // rows are moved as aligned float4
    int max_dil = 1;
    for (int p = 0; p < np; ++p) {
        const amp_conv *a = c1[p], *b = c2[p];
        if (!a || !b || a->precision != PREC_F16X3 || b->precision != PREC_F16X3) return false;
        if (a->pad_reflect || b->pad_reflect || a->tanh_out || b->tanh_out || a->transposed || b->transposed) return false;
        if (a->cin != a->cout || b->cin != b->cout || a->cin != b->cin || a->cin != c1[0]->cin) return false;
        if (a->k != c1[0]->k || b->k != a->k || b->dilation != 1 || a->k != a->KT) return false;
        if (a->padding != (a->k - 1) / 2 * a->dilation || b->padding != (b->k - 1) / 2) return false;
        if (!a->bias_dev || !b->bias_dev) return false;
        max_dil = a->dilation > max_dil ? a->dilation : max_dil;
    }
    const int form = ampb_form(c1[0]->cin, c1[0]->k);
    if (form < 0) return false;
    const int W = ampb_tile(c1[0]->k, c1[0]->cin, max_dil, form);
    const int rh = ampb_halo(c1, np);
    if (W <= 0 || W - 2 * rh < W / 2) return false;              // at least half of every tile must be output
    const int NT = W - 2 * rh;
    if (ampb_fusion_mode() == 1 && (long long)B * ((T + NT - 1) / NT) < kAmpbMinWorkgroups) return false;
    return true;
}

static int ampb_run(const amp_conv* const* c1, const amp_conv* const* c2, int np, const ActParams* acts, const float* x, int B, int T,
                    float* y, int mode, float div, hipStream_t stream, const int* lens = nullptr, int len_mul = 1) {
    if (x == y) { set_error("ampb_run: x and y must not alias"); return AMP_ERR_INVALID; }
    AmpbArgs a{};
    a.x = x; a.y = y;
    a.ns = 2 * np;
    int max_dil = 1;
    for (int s = 0; s < AMP_AMPB_MAX_STEPS; ++s) {
        const int sv = s < a.ns ? s : 0;                          // unused slots: valid pointers all the same
        const amp_conv* c = (sv & 1) ? c2[sv >> 1] : c1[sv >> 1];
        a.wp[s] = c->wp_dev; a.bias[s] = c->bias_dev;
        a.sc[s] = 16.f * c->wscale; a.isc[s] = 1.f / a.sc[s];
        a.dil[s] = c->dilation;
        a.act_a[s] = acts[sv].a_dev; a.act_invb[s] = acts[sv].invb_dev; a.act_fu[s] = acts[sv].fu2_dev; a.act_fd[s] = acts[sv].fd_dev;
        max_dil = c->dilation > max_dil ? c->dilation : max_dil;
    }
    a.rh = ampb_halo(c1, np);
    a.B = B; a.C = c1[0]->cin; a.T = T;
    const int form = ampb_form(a.C, c1[0]->k);
    const int W = ampb_tile(c1[0]->k, a.C, max_dil, form);
    const int NT = W - 2 * a.rh;
    a.tiles_per_item = (T + NT - 1) / NT;
    a.mode = mode; a.div = div;
    a.lens = lens; a.len_mul = len_mul;
    a.range_flag = range_flag_for_current_device();
    a.rev = next_rev(lens);
    AMP_HIP(launch_ampb(c1[0]->k, a, form, stream));
    return AMP_OK;
}

struct amp_gen {
    amp_gen_desc d{};
    std::map<std::string, std::vector<int64_t>> expected;  // key -> shape
    std::map<std::string, HostTensor> w;
    bool finalized = false;
    int hop = 1;
    std::vector<int> ch;  // channels after each stage
    std::unique_ptr<amp_conv> conv_pre, cond;
    std::vector<std::unique_ptr<amp_conv>> ups;
    std::vector<ResBlock> rbs;
    ActParams act_post;
    float* post_w_dev = nullptr;
    float* post_b_dev = nullptr;
    int post_cin = 0;
    std::vector<float*> dev_allocs;
    // profiling: a ring of event sets, one per forward, so that a caller can time EVERY forward of a region
    // without synchronising in between (bench.py reads them after its closing fence)
    struct ProfSlot {
        hipEvent_t ev_begin = nullptr, ev_end = nullptr;
        std::vector<hipEvent_t> ev_mrf;  // begin/end per (batch group, stage)
        std::vector<hipEvent_t> ev_rb;   // per (batch group, stage): n_kernels + 1 marks around the resblocks
        std::vector<std::string> rb_kernels;   // per (stage, resblock): the distinct kernels its launches ran, " | "-joined (first batch group)
        int ev_groups = 0;
        bool valid = false;
    };
    std::vector<ProfSlot> prof;          // empty = profiling off
    size_t prof_count = 0;               // forwards recorded so far
    RangeGuard guard;                    // this handle's f16 operand-range word (allocated by finalize on its device)
    // concurrent resblocks (small launches): n_kernels - 1 side streams, per stage one fork event and n_kernels - 1 join events
    std::vector<hipStream_t> side;
    std::vector<hipEvent_t> ev_side;
    // One launch sequence of this handle at a time: the side streams, their fork / join events, the profiling ring and the
    // range-guard word are per HANDLE, so two host threads (or two caller streams) enqueueing forwards of the same generator take turns
    // on the HOST -- each sequence's event records and waits are then issued as a unit (a wait binds to the record that precedes it in
    // issue order) and the device-side order per side stream is the issue order.  The forwards still overlap on the device.
    std::mutex launch_mu;
    ~amp_gen() {
        guard_free(guard);
        for (auto s_ : side) (void)hipStreamDestroy(s_);
        for (auto e : ev_side) (void)hipEventDestroy(e);
        for (float* p : dev_allocs) (void)hipFree(p);
        for (auto& p : prof) {
            if (p.ev_begin) (void)hipEventDestroy(p.ev_begin);
            if (p.ev_end) (void)hipEventDestroy(p.ev_end);
            for (auto e : p.ev_mrf) (void)hipEventDestroy(e);
            for (auto e : p.ev_rb) (void)hipEventDestroy(e);
        }
    }
};

static void expect_conv(amp_gen* g, const std::string& p, int cout, int cin, int k, bool transposed, bool wn, bool bias) {
    const int64_t d0 = transposed ? cin : cout, d1 = transposed ? cout : cin;
    if (bias) g->expected[p + ".bias"] = {cout};
    // both the weight-normed and the folded form are accepted
    (void)wn;
    g->expected[p + ".weight_g"] = {d0, 1, 1};
    g->expected[p + ".weight_v"] = {d0, d1, k};
    g->expected[p + ".weight"] = {d0, d1, k};
}

static void expect_act(amp_gen* g, const std::string& p, int c) {
    g->expected[p + ".act.alpha"] = {c};
    if (g->d.activation == AMP_ACT_SNAKEBETA) g->expected[p + ".act.beta"] = {c};
    g->expected[p + ".upsample.filter"] = {1, 1, 12};
    g->expected[p + ".downsample.lowpass.filter"] = {1, 1, 12};
}

static std::string ups_key(const amp_gen* g, int i) {
    // BigVGAN nests each upsampler in a 1-element ModuleList (bigvgan.py:261-276)
    return g->d.arch == AMP_ARCH_BIGVGAN ? "ups." + std::to_string(i) + ".0" : "ups." + std::to_string(i);
}

// Op-level convenience (tests): derive a = alpha (exp'ed when logscale) and 1 / (beta + 1e-9) on the host and upload them
// with the two 12-tap filters: scratch = [a (C) | invb (C) | up taps (12) | down taps (12) | 2 * up taps (12)].  The caller frees `*out`.
static int act_params_upload(const float* alpha_dev, const float* beta_dev, int C, int logscale, const float* filt_up_host,
                             const float* filt_down_host, float** out) {
    std::vector<float> al(C), be(C), a(C), ib(C);
    AMP_HIP(hipMemcpy(al.data(), alpha_dev, C * sizeof(float), hipMemcpyDeviceToHost));
    if (beta_dev) AMP_HIP(hipMemcpy(be.data(), beta_dev, C * sizeof(float), hipMemcpyDeviceToHost));
    for (int i = 0; i < C; ++i) {
        float av = al[i], bv = beta_dev ? be[i] : al[i];
        if (logscale) { av = expf(av); bv = expf(bv); }
        a[i] = av;
        ib[i] = 1.0f / (bv + 0.000000001f);
    }
    float* scratch = nullptr;
    AMP_HIP(hipMalloc((void**)&scratch, (2 * (size_t)C + 36) * sizeof(float)));
    float fu2[12];
    for (int i = 0; i < 12; ++i) fu2[i] = 2.f * filt_up_host[i];
    hipError_t e = hipMemcpy(scratch, a.data(), C * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(scratch + C, ib.data(), C * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(scratch + 2 * C, filt_up_host, 12 * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(scratch + 2 * C + 12, filt_down_host, 12 * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(scratch + 2 * C + 24, fu2, 12 * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(scratch); set_error("act_params_upload: %s", hipGetErrorString(e)); return AMP_ERR_HIP; }
    *out = scratch;
    return AMP_OK;
}

extern "C" {

// 100: round 1; 120: + amp_conv_create_gated / amp_wn_forward / amp_conv_act_forward, switches; 122: + amp_set_conv_blk / _conv_rg_fast /
// _pingpong; 130 (round 3's ABI, numbered in round 4): amp_mel_desc grew four trailing fields, + amp_resblock_forward /
// amp_set_resblock_fusion / amp_gen_kernel_name; 140: amp_mel_desc.struct_size, + amp_ampblock_forward / amp_set_ampblock_fusion / amp_mel_init;
// 141 (additive): the ragged / fused entry points of the VITS text side (amp_conv_forward_ragged, amp_layer_norm_c_ragged, amp_dwconv_layer_norm_c,
// amp_rel_attention_strided, amp_set_rel_attention_tiled, amp_expand_path_strided); 142 (round 5, REMOVALS): amp_conv_act_forward, amp_set_fuse_act,
// amp_set_wn_layer_fusion are gone with the kernels behind them (never chosen by the launch policy), amp_set_pair_strips(1) is refused; amp_mel_forward
// accepts every n_fft in [64, 4096]; 143 (additive): the Vocos entry points amp_pw_create / amp_pw_forward / amp_pw_precision / amp_pw_destroy and
// amp_istft_same_polar, amp_dwconv_layer_norm_c takes K = 7; 144 (additive): the DiffWave entry points amp_dw_* (diffwave.hip)
int amp_version(void) { return 144; }
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

int amp_gen_create(const amp_gen_desc* desc, amp_gen** out) {
    if (!desc || !out) { set_error("amp_gen_create: null argument"); return AMP_ERR_INVALID; }
    const amp_gen_desc& d = *desc;
    if (d.arch < AMP_ARCH_HIFIGAN || d.arch > AMP_ARCH_HIFIGAN_VITS) { set_error("amp_gen_create: unknown arch %d", d.arch); return AMP_ERR_INVALID; }
    if (d.n_in <= 0 || d.upsample_initial_channel <= 0 || d.n_stages <= 0 || d.n_stages > AMP_MAX_STAGES ||
        d.n_kernels <= 0 || d.n_kernels > AMP_MAX_KERNELS || (d.resblock_type != 1 && d.resblock_type != 2)) {
        set_error("amp_gen_create: bad descriptor (n_in=%d C0=%d stages=%d kernels=%d resblock=%d)", d.n_in,
                  d.upsample_initial_channel, d.n_stages, d.n_kernels, d.resblock_type);
        return AMP_ERR_INVALID;
    }
    if (d.arch == AMP_ARCH_BIGVGAN && d.activation != AMP_ACT_SNAKE && d.activation != AMP_ACT_SNAKEBETA) {
        // bigvgan.py:132-135 raises NotImplementedError for anything else
        set_error("activation incorrectly specified. check the config file and look for 'activation'.");
        return AMP_ERR_UNSUPPORTED;
    }
    if ((d.upsample_initial_channel >> d.n_stages) <= 0) { set_error("amp_gen_create: upsample_initial_channel too small"); return AMP_ERR_INVALID; }
    auto g = std::make_unique<amp_gen>();
    g->d = d;
    if (d.arch != AMP_ARCH_BIGVGAN) g->d.activation = AMP_ACT_LRELU;
    const bool vits = d.arch == AMP_ARCH_HIFIGAN_VITS;
    int c0 = d.upsample_initial_channel;
    expect_conv(g.get(), "conv_pre", c0, d.n_in, 7, false, !vits, true);
    g->hop = 1;
    int ch = c0;
    for (int i = 0; i < d.n_stages; ++i) {
        const int u = d.upsample_rates[i], k = d.upsample_kernel_sizes[i];
        if (u <= 0 || k < u) { set_error("amp_gen_create: stage %d rate=%d kernel=%d", i, u, k); return AMP_ERR_INVALID; }
        if ((k - u) % 2 != 0) { set_error("amp_gen_create: stage %d: kernel-rate must be even (output length = rate*T)", i); return AMP_ERR_UNSUPPORTED; }
        const int cin = c0 >> i, cout = c0 >> (i + 1);
        expect_conv(g.get(), ups_key(g.get(), i), cout, cin, k, true, true, true);
        g->hop *= u;
        ch = cout;
        g->ch.push_back(cout);
        for (int j = 0; j < d.n_kernels; ++j) {
            const int rk = d.resblock_kernel_sizes[j], nd = d.n_dilations[j];
            if (rk <= 0 || (rk & 1) == 0 || nd <= 0 || nd > AMP_MAX_DILATIONS) { set_error("amp_gen_create: resblock %d kernel=%d dilations=%d", j, rk, nd); return AMP_ERR_INVALID; }
            const std::string pre = "resblocks." + std::to_string(i * d.n_kernels + j);
            for (int p = 0; p < nd; ++p) {
                if (d.resblock_type == 1) {
                    expect_conv(g.get(), pre + ".convs1." + std::to_string(p), cout, cout, rk, false, true, true);
                    expect_conv(g.get(), pre + ".convs2." + std::to_string(p), cout, cout, rk, false, true, true);
                } else {
                    expect_conv(g.get(), pre + ".convs." + std::to_string(p), cout, cout, rk, false, true, true);
                }
            }
            if (d.arch == AMP_ARCH_BIGVGAN) {
                const int nact = d.resblock_type == 1 ? 2 * nd : nd;
                for (int m = 0; m < nact; ++m) expect_act(g.get(), pre + ".activations." + std::to_string(m), cout);
            }
        }
    }
    if (d.arch == AMP_ARCH_BIGVGAN) expect_act(g.get(), "activation_post", ch);
    expect_conv(g.get(), "conv_post", 1, ch, 7, false, !vits, !vits);
    if (vits && d.gin_channels > 0) expect_conv(g.get(), "cond", c0, d.gin_channels, 1, false, false, true);
    *out = g.release();
    return AMP_OK;
}

int amp_gen_set_weight(amp_gen* g, const char* ref_key, const float* data_host, const int64_t* shape, int ndim) {
    if (!g || !ref_key || !data_host || (!shape && ndim > 0)) { set_error("amp_gen_set_weight: null argument"); return AMP_ERR_INVALID; }
    if (g->finalized) { set_error("amp_gen_set_weight: handle already finalized"); return AMP_ERR_STATE; }
    std::string key(ref_key);
    if (key.rfind("module.", 0) == 0) key = key.substr(7);  // from_multi_gpu checkpoints, vocoder_inference.py:312-327
    auto it = g->expected.find(key);
    if (it == g->expected.end()) { set_error("amp_gen_set_weight: unexpected key '%s'", ref_key); return AMP_ERR_INVALID; }
    HostTensor t;
    t.shape.assign(shape, shape + ndim);
    if (t.shape != it->second) {
        std::string got, want;
        for (auto s : t.shape) got += std::to_string(s) + ",";
        for (auto s : it->second) want += std::to_string(s) + ",";
        set_error("amp_gen_set_weight: '%s' has shape (%s) expected (%s)", ref_key, got.c_str(), want.c_str());
        return AMP_ERR_INVALID;
    }
    // `data_host` may also be a DEVICE pointer (a parameter that already lives on the GPU): copied back here, once,
    // instead of through a host tensor the caller would have to materialise first
    hipPointerAttribute_t attr{};
    const bool on_device = hipPointerGetAttributes(&attr, data_host) == hipSuccess && attr.type == hipMemoryTypeDevice;
    if (!on_device) (void)hipGetLastError();          // a plain host pointer is not an error
    if (on_device) {
        t.data.resize(t.numel());
        AMP_HIP(hipMemcpy(t.data.data(), data_host, t.numel() * sizeof(float), hipMemcpyDeviceToHost));
    } else {
        t.data.assign(data_host, data_host + t.numel());
    }
    g->w[key] = std::move(t);
    return AMP_OK;
}

}  // extern "C"

// fold weight-norm (or take the folded weight) for `prefix`; returns false when tensors are missing
static bool get_folded(amp_gen* g, const std::string& p, std::vector<float>* wout, const float** bias, bool need_bias) {
    auto itw = g->w.find(p + ".weight");
    if (itw != g->w.end()) {
        *wout = itw->second.data;
    } else {
        auto ig = g->w.find(p + ".weight_g"), iv = g->w.find(p + ".weight_v");
        if (ig == g->w.end() || iv == g->w.end()) { set_error("amp_gen_finalize: missing weight for '%s'", p.c_str()); return false; }
        const HostTensor& V = iv->second;
        const size_t d0 = (size_t)V.shape[0], inner = V.numel() / d0;
        wout->resize(V.numel());
        for (size_t r = 0; r < d0; ++r) {
            // torch.norm_except_dim: fp32 2-norm over all dims but 0, w = v * (g / norm)
            double ss = 0.0;
            for (size_t i = 0; i < inner; ++i) { const double v = V.data[r * inner + i]; ss += v * v; }
            const float nrm = (float)sqrt(ss);
            const float sc = ig->second.data[r] / nrm;
            for (size_t i = 0; i < inner; ++i) (*wout)[r * inner + i] = V.data[r * inner + i] * sc;
        }
    }
    *bias = nullptr;
    auto ib = g->w.find(p + ".bias");
    if (ib != g->w.end()) *bias = ib->second.data.data();
    else if (need_bias) { set_error("amp_gen_finalize: missing '%s.bias'", p.c_str()); return false; }
    return true;
}

static int upload(amp_gen* g, const float* src, size_t n, float** dst) {
    AMP_HIP(hipMalloc((void**)dst, n * sizeof(float)));
    g->dev_allocs.push_back(*dst);
    AMP_HIP(hipMemcpy(*dst, src, n * sizeof(float), hipMemcpyHostToDevice));
    return AMP_OK;
}

static int build_act(amp_gen* g, const std::string& p, int c, ActParams* out) {
    auto ia = g->w.find(p + ".act.alpha");
    if (ia == g->w.end()) { set_error("amp_gen_finalize: missing '%s.act.alpha'", p.c_str()); return AMP_ERR_MISSING_WEIGHT; }
    const std::vector<float>* beta = nullptr;
    if (g->d.activation == AMP_ACT_SNAKEBETA) {
        auto ib = g->w.find(p + ".act.beta");
        if (ib == g->w.end()) { set_error("amp_gen_finalize: missing '%s.act.beta'", p.c_str()); return AMP_ERR_MISSING_WEIGHT; }
        beta = &ib->second.data;
    }
    auto iu = g->w.find(p + ".upsample.filter"), idn = g->w.find(p + ".downsample.lowpass.filter");
    if (iu == g->w.end() || idn == g->w.end()) { set_error("amp_gen_finalize: missing anti-aliasing filter buffers of '%s'", p.c_str()); return AMP_ERR_MISSING_WEIGHT; }
    std::vector<float> a(c), ib(c);
    for (int i = 0; i < c; ++i) {
        float al = ia->second.data[i];
        float be = beta ? (*beta)[i] : al;
        if (g->d.snake_logscale) { al = expf(al); be = expf(be); }  // snake.py:57-58,116-118
        a[i] = al;
        ib[i] = 1.0f / (be + 0.000000001f);                          // snake.py:59,119
    }
    int rc;
    if ((rc = upload(g, a.data(), c, &out->a_dev)) != AMP_OK) return rc;
    if ((rc = upload(g, ib.data(), c, &out->invb_dev)) != AMP_OK) return rc;
    if ((rc = upload(g, iu->second.data.data(), 12, &out->fu_dev)) != AMP_OK) return rc;
    if ((rc = upload(g, idn->second.data.data(), 12, &out->fd_dev)) != AMP_OK) return rc;
    float fu2[12];
    for (int i = 0; i < 12; ++i) fu2[i] = 2.f * iu->second.data[i];
    if ((rc = upload(g, fu2, 12, &out->fu2_dev)) != AMP_OK) return rc;
    return AMP_OK;
}

static int make_conv(amp_gen* g, const std::string& p, bool transposed, int cin, int cout, int k, int stride, int dil,
                     int pad, bool need_bias, std::unique_ptr<amp_conv>* out) {
    std::vector<float> w;
    const float* bias = nullptr;
    if (!get_folded(g, p, &w, &bias, need_bias)) return AMP_ERR_MISSING_WEIGHT;
    auto c = std::make_unique<amp_conv>();
    c->transposed = transposed; c->cin = cin; c->cout = cout; c->k = k; c->stride = stride; c->dilation = dil; c->padding = pad;
    int rc = conv_build(c.get(), w.data(), bias);
    if (rc != AMP_OK) return rc;
    *out = std::move(c);
    return AMP_OK;
}

extern "C" {

int amp_gen_finalize(amp_gen* g) {
    if (!g) { set_error("amp_gen_finalize: null handle"); return AMP_ERR_INVALID; }
    if (g->finalized) return AMP_OK;
    if (amp_device_count() <= 0) { set_error("amp_gen_finalize: no HIP device visible (the HIP path has no CPU fallback)"); return AMP_ERR_HIP; }
    const amp_gen_desc& d = g->d;
    const bool vits = d.arch == AMP_ARCH_HIFIGAN_VITS;
    const int c0 = d.upsample_initial_channel;
    int rc;
    if ((rc = make_conv(g, "conv_pre", false, d.n_in, c0, 7, 1, 1, 3, true, &g->conv_pre)) != AMP_OK) return rc;
    if (vits && d.gin_channels > 0)
        if ((rc = make_conv(g, "cond", false, d.gin_channels, c0, 1, 1, 1, 0, true, &g->cond)) != AMP_OK) return rc;
    int ch = c0;
    for (int i = 0; i < d.n_stages; ++i) {
        const int u = d.upsample_rates[i], k = d.upsample_kernel_sizes[i];
        const int cin = c0 >> i, cout = c0 >> (i + 1);
        std::unique_ptr<amp_conv> up;
        if ((rc = make_conv(g, ups_key(g, i), true, cin, cout, k, u, 1, (k - u) / 2, true, &up)) != AMP_OK) return rc;
        g->ups.push_back(std::move(up));
        ch = cout;
        for (int j = 0; j < d.n_kernels; ++j) {
            ResBlock rb;
            rb.k = d.resblock_kernel_sizes[j];
            const std::string pre = "resblocks." + std::to_string(i * d.n_kernels + j);
            for (int p = 0; p < d.n_dilations[j]; ++p) {
                const int dl = d.resblock_dilation_sizes[j][p];
                rb.dil.push_back(dl);
                std::unique_ptr<amp_conv> a, b;
                const int pad1 = (rb.k * dl - dl) / 2;  // get_padding, gan_utils.py:12-13
                if (d.resblock_type == 1) {
                    if ((rc = make_conv(g, pre + ".convs1." + std::to_string(p), false, cout, cout, rb.k, 1, dl, pad1, true, &a)) != AMP_OK) return rc;
                    if ((rc = make_conv(g, pre + ".convs2." + std::to_string(p), false, cout, cout, rb.k, 1, 1, (rb.k - 1) / 2, true, &b)) != AMP_OK) return rc;
                    rb.c1.push_back(std::move(a));
                    rb.c2.push_back(std::move(b));
                } else {
                    if ((rc = make_conv(g, pre + ".convs." + std::to_string(p), false, cout, cout, rb.k, 1, dl, pad1, true, &a)) != AMP_OK) return rc;
                    rb.c1.push_back(std::move(a));
                }
            }
            if (d.arch == AMP_ARCH_BIGVGAN) {
                const int nact = d.resblock_type == 1 ? 2 * d.n_dilations[j] : d.n_dilations[j];
                rb.acts.resize(nact);
                for (int m = 0; m < nact; ++m)
                    if ((rc = build_act(g, pre + ".activations." + std::to_string(m), cout, &rb.acts[m])) != AMP_OK) return rc;
            }
            g->rbs.push_back(std::move(rb));
        }
    }
    if (d.arch == AMP_ARCH_BIGVGAN)
        if ((rc = build_act(g, "activation_post", ch, &g->act_post)) != AMP_OK) return rc;
    {
        std::vector<float> w;
        const float* bias = nullptr;
        if (!get_folded(g, "conv_post", &w, &bias, !vits)) return AMP_ERR_MISSING_WEIGHT;
        g->post_cin = ch;
        if ((rc = upload(g, w.data(), w.size(), &g->post_w_dev)) != AMP_OK) return rc;
        if (bias) if ((rc = upload(g, bias, 1, &g->post_b_dev)) != AMP_OK) return rc;
    }
    if (!guard_init(g->guard)) { set_error("amp_gen_finalize: cannot allocate the range-guard word"); return AMP_ERR_HIP; }
    g->w.clear();  // host copies no longer needed
    g->finalized = true;
    return AMP_OK;
}

int amp_gen_hop(const amp_gen* g) { return g ? g->hop : 0; }

static size_t gen_buf_elems(const amp_gen* g, int B, int T) {
    size_t mx = (size_t)B * g->d.upsample_initial_channel * T;
    int t = T;
    for (int i = 0; i < g->d.n_stages; ++i) {
        t *= g->d.upsample_rates[i];
        const size_t e = (size_t)B * g->ch[i] * t;
        if (e > mx) mx = e;
    }
    return (mx + 63) & ~(size_t)63;
}

// scratch tensors of a forward: X, XS, U, R, TMP (+ ACT for BigVGAN).
static int gen_num_bufs(const amp_gen* g) { return g->d.arch == AMP_ARCH_BIGVGAN ? 6 : 5; }

// Concurrent resblocks.  The n_kernels resblocks of a stage read the same U and are independent until the MRF mean; run one after
// the other each of them is a chain of 1-9 dependent launches, and for a single utterance no launch fills the chip (a 3-s utterance:
// 50-300 workgroups per launch on 256 CUs, 52 launches back to back = 1.06 ms that a hipGraph replay does not shorten -- the chain
// is serialised on the GPU, not by the host).  In this mode resblocks 1 .. n - 1 run on streams of their own with their own R / TMP
// (/ ACT) buffers and the first one stays on the caller's stream; only the LAST launch of each resblock -- the one that accumulates
// into XS -- is ordered after the last launch of resblock j - 1 (an event) and keeps its sequential `=` / `+=` / `(y + v) / n` mode,
// so every sum is formed by the same kernel in the same
// order and the bits do not change (tests/test_gpu_resblock.py).  (A post-hoc mean of separately stored results would not do: the
// conv kernels add y into the accumulator BEFORE the products.)  Policy (amp_set_resblock_streams(-1) / AMP_RB_STREAMS unset): only
// while B * T <= kRbStreamsMaxFrames mel frames; at full batches every launch fills the chip and the same idea measured 28.1 vs
// 28.1 ms (round 2, BigVGAN, profiles/r2_i_bigvgan_streams.txt).  Works under stream capture (fork / join by events) once the side
// streams exist: they are created by the first eager forward or by amp_gen_prepare_streams(), never inside a capture.
constexpr long long kRbHorizontalMaxFrames = 1024;   // profiles/r4_streams_horizontal_sweep.txt: 0.81 / 0.90 / 0.91 against 0.84 / 0.94 / 0.95 on streams at 256 / 512 / 1 024 frames, equal at 2 048, behind at 4 096
constexpr long long kRbStreamsMaxFrames = 4096;   // tools/streams_sweep.py, profiles/r4_streams_sweep.txt: 0.87-0.97 of the sequential time up to here, 1.00 beyond
static int gen_side_bufs(const amp_gen* g) { return (g->d.n_kernels - 1) * (g->d.arch == AMP_ARCH_BIGVGAN ? 4 : 3); }   // R, TMP, XS (+ ACT) per extra resblock
static bool gen_streams_wanted(const amp_gen* g, int B, int T) {
    if (g->d.n_kernels < 2) return false;
    const int m = cfg().rb_streams;
    return m == 1 || (m < 0 && (long long)B * T <= kRbStreamsMaxFrames);
}

// Optional depth-first batch grouping: a group of items runs through the WHOLE generator before the
// next one starts, with a working set (the scratch tensors of its largest stage) bounded by
// amp_set_group_mb().  It bounds the workspace (168 MB instead of 2.7 GB at config 2) but
// is OFF by default (0 = whole batch per layer): sized to the 256 MiB Infinity Cache it was measured
// SLOWER on MI355X (36.2 ms ungrouped vs 45.6 / 49.9 / 62.4 ms at 200 / 144 / 104 MB groups,
// profiles/r1_exp_group.txt) -- the small grids under-fill 256 CUs and the cache brings no bandwidth win.
static size_t group_target_bytes() { return cfg().group_bytes; }

static int gen_group_items(const amp_gen* g, int B, int T) {
    const size_t target = group_target_bytes();
    if (target == 0) return B;
    // live tensors of a stage: U, R, TMP, XS (+ ACT) -- X is dead once the stage's ConvTranspose has run
    const size_t per_item = gen_buf_elems(g, 1, T) * sizeof(float) * (size_t)(gen_num_bufs(g) - 1);
    size_t n = target / (per_item ? per_item : 1);
    if (n < 1) n = 1;
    return n < (size_t)B ? (int)n : B;
}

size_t amp_gen_workspace_bytes(const amp_gen* g, int B, int T) {
    if (!g || B <= 0 || T <= 0) return 0;
    const int G = gen_group_items(g, B, T);
    const int nb = gen_num_bufs(g) + ((G == B && gen_streams_wanted(g, B, T)) ? gen_side_bufs(g) : 0);
    return gen_buf_elems(g, G, T) * sizeof(float) * nb + (size_t)G * g->d.upsample_initial_channel * sizeof(float) + 256;
}

int amp_set_pair_strips(int on) {
    if (on < -1 || on > 0) { set_error("amp_set_pair_strips: %d (-1 the policy, 0 the per-tile kernel everywhere; the four-wave strips of mode 1 left in ABI 142)", on); return AMP_ERR_INVALID; }
    cfg().pair_strips = on;
    return AMP_OK;
}

int amp_set_group_mb(int megabytes) {
    if (megabytes < 0) { set_error("amp_set_group_mb: %d", megabytes); return AMP_ERR_INVALID; }
    cfg().group_bytes = (size_t)megabytes << 20;
    return AMP_OK;
}

int amp_gen_set_profiling(amp_gen* g, int slots) {
    if (!g || slots < 0 || slots > 4096) { set_error("amp_gen_set_profiling: bad argument"); return AMP_ERR_INVALID; }
    for (auto& p : g->prof) {
        if (p.ev_begin) (void)hipEventDestroy(p.ev_begin);
        if (p.ev_end) (void)hipEventDestroy(p.ev_end);
        for (auto e : p.ev_mrf) (void)hipEventDestroy(e);
        for (auto e : p.ev_rb) (void)hipEventDestroy(e);
    }
    g->prof.clear();
    g->prof.resize((size_t)slots);
    g->prof_count = 0;
    for (auto& p : g->prof) {
        AMP_HIP(hipEventCreate(&p.ev_begin));
        AMP_HIP(hipEventCreate(&p.ev_end));
    }
    return AMP_OK;
}

int amp_gen_timing_ms(amp_gen* g, int back, int which, float* ms_out) {
    if (!g || !ms_out) { set_error("amp_gen_timing_ms: null argument"); return AMP_ERR_INVALID; }
    if (g->prof.empty() || back < 0 || (size_t)back >= g->prof.size() || (size_t)back >= g->prof_count) {
        set_error("amp_gen_timing_ms: no profiled forward %d back (slots=%zu, recorded=%zu)", back, g->prof.size(), g->prof_count);
        return AMP_ERR_STATE;
    }
    const amp_gen::ProfSlot& p = g->prof[(g->prof_count - 1 - (size_t)back) % g->prof.size()];
    if (!p.valid) { set_error("amp_gen_timing_ms: slot not recorded"); return AMP_ERR_STATE; }
    AMP_HIP(hipEventSynchronize(p.ev_end));
    if (which == 0) {
        AMP_HIP(hipEventElapsedTime(ms_out, p.ev_begin, p.ev_end));
    } else if (which >= 1 && which < 2 + g->d.n_stages) {
        // sum over the batch groups (and, for which == 1, over the stages)
        float tot = 0.f;
        for (int gi = 0; gi < p.ev_groups; ++gi)
            for (int i = 0; i < g->d.n_stages; ++i) {
                if (which >= 2 && i != which - 2) continue;
                float ms = 0.f;
                const size_t e = 2 * ((size_t)g->d.n_stages * gi + i);
                AMP_HIP(hipEventElapsedTime(&ms, p.ev_mrf[e], p.ev_mrf[e + 1]));
                tot += ms;
            }
        *ms_out = tot;
    } else if (which >= 100 && which < 100 + 16 * g->d.n_stages && (which - 100) % 16 < g->d.n_kernels) {
        // one resblock: 100 + 16 * stage + j, summed over the batch groups
        const int i = (which - 100) / 16, j = (which - 100) % 16, nk = g->d.n_kernels;
        float tot = 0.f;
        for (int gi = 0; gi < p.ev_groups; ++gi) {
            float ms = 0.f;
            const size_t e = (size_t)g->d.n_stages * (nk + 1) * gi + (size_t)i * (nk + 1) + j;
            AMP_HIP(hipEventElapsedTime(&ms, p.ev_rb[e], p.ev_rb[e + 1]));
            tot += ms;
        }
        *ms_out = tot;
    } else {
        set_error("amp_gen_timing_ms: which=%d", which);
        return AMP_ERR_INVALID;
    }
    return AMP_OK;
}

int amp_gen_last_timing_ms(amp_gen* g, int which, float* ms_out) { return amp_gen_timing_ms(g, 0, which, ms_out); }

int amp_gen_kernel_name(amp_gen* g, int back, int which, char* buf, size_t n) {
    if (!g || !buf || n == 0) { set_error("amp_gen_kernel_name: null argument"); return AMP_ERR_INVALID; }
    if (g->prof.empty() || back < 0 || (size_t)back >= g->prof.size() || (size_t)back >= g->prof_count) {
        set_error("amp_gen_kernel_name: no profiled forward %d back (slots=%zu, recorded=%zu)", back, g->prof.size(), g->prof_count);
        return AMP_ERR_STATE;
    }
    const amp_gen::ProfSlot& p = g->prof[(g->prof_count - 1 - (size_t)back) % g->prof.size()];
    const int i = (which - 100) / 16, j = (which - 100) % 16;
    if (which < 100 || i >= g->d.n_stages || j >= g->d.n_kernels || (size_t)(i * g->d.n_kernels + j) >= p.rb_kernels.size()) {
        set_error("amp_gen_kernel_name: which=%d", which);
        return AMP_ERR_INVALID;
    }
    snprintf(buf, n, "%s", p.rb_kernels[(size_t)i * g->d.n_kernels + j].c_str());
    return AMP_OK;
}

#define AMP_RC(expr) do { int rc__ = (expr); if (rc__ != AMP_OK) return rc__; } while (0)

constexpr float kLreluSlope = 0.1f;  // LRELU_SLOPE hifigan.py:14

// One stage of gen_forward_group after its ConvTranspose: what every step of it reads.
struct Stage {
    amp_gen* g;
    int i;                    // stage index
    int B, t, C, lm;          // items, columns, channels, samples per mel frame (ragged batches: valid length = lens[b] * lm)
    const int* lens;
    hipStream_t st;
    bool conc;                // resblocks 1 .. n_kernels - 1 on g->side streams, with buffers of their own (gen_forward_group)
    const float* U;           // upsampled stage tensor (input of every resblock)
    float* XS;                // MRF accumulator: the stage's output
    float *R, *TMP, *ACT;     // running x inside a resblock, xt between the two convs of a pair, activation output (BigVGAN only)
    float* SIDE;              // concurrent mode: R, TMP, XS (+ ACT) of resblocks 1 .. n_kernels - 1, side_per buffers of be floats each
    int side_per;
    size_t be;
    const ResBlock& rb(int j) const { return g->rbs[(size_t)i * g->d.n_kernels + j]; }
};

// MRF mode of resblock j's accumulating launch in the chain of nk resblocks: XS = v, XS += v, ..., XS = (XS + v) / nk
static int accumulate_mode(int j, int nk) { return j == 0 ? 0 : (j == nk - 1 ? 2 : 1); }

// Resblock j's buffers: its own ones behind the regular buffers when `own` (concurrent mode) and j > 0, else the regular ones
struct RbBufs { float *R, *TMP, *XS, *ACT; };
static RbBufs rb_bufs(const Stage& s, int j, bool own) {
    if (!own || j == 0) return {s.R, s.TMP, s.XS, s.ACT};
    float* SB = s.SIDE + (size_t)(j - 1) * s.side_per * s.be;
    return {SB, SB + s.be, SB + 2 * s.be, s.ACT ? SB + 3 * s.be : nullptr};
}

// XS = ((XS + XS_1) + XS_2 ...) / nk: the MRF mean of resblocks that stored their results separately (in their own XS).  evs: the
// concurrent mode's events, `st` waits for every side resblock's evs[1 + j] first; null: nothing to wait for.
static int launch_stage_mrf_sum(const Stage& s, const hipEvent_t* evs) {
    const int nk = s.g->d.n_kernels;
    MrfSumArgs ma{};
    ma.y = s.XS; ma.n = nk - 1; ma.div = (float)nk; ma.count = (size_t)s.B * s.C * s.t;
    for (int j = 1; j < nk; ++j) {
        if (evs) AMP_HIP(hipStreamWaitEvent(s.st, evs[1 + j], 0));
        ma.p[j - 1] = rb_bufs(s, j, true).XS;
    }
    AMP_HIP(launch_mrf_sum(ma, s.st));
    return AMP_OK;
}

// The horizontal stage forms (try_stage_pair3, try_stage_small3) take a stage of three ResBlock1 whose kernels are 11, 7 and 3 in any order:
// slot_of[0 / 1 / 2] = the resblock with k = 11 / 7 / 3.  false when the stage is not of that shape.
static bool horizontal_slots(const Stage& s, int slot_of[3]) {
    slot_of[0] = slot_of[1] = slot_of[2] = -1;
    for (int j = 0; j < 3; ++j) {
        const int k = s.rb(j).c1[0]->k;
        const int sl = k == 11 ? 0 : k == 7 ? 1 : k == 3 ? 2 : -1;
        if (sl < 0 || slot_of[sl] >= 0) return false;
        slot_of[sl] = j;
    }
    return true;
}

// Horizontal form (pair3_f16x3.hip): where the stage's three resblocks run as per-tile fused pairs, pair p of all three shares ONE launch --
// nd launches + the MRF mean instead of 3 nd launches on three streams with their fork / join events.  Every launch is planned first:
// *ran = false, nothing launched, when one of the pairs is not a per-tile fused pair.
static int try_stage_pair3(const Stage& s, const int slot_of[3], bool* ran) {
    *ran = false;
    const int nk = s.g->d.n_kernels;
    const size_t nd = s.rb(0).dil.size();
    std::vector<Pair3Args> plan(nd);
    for (int sl = 0; sl < 3; ++sl) {
        const int j = slot_of[sl];
        const ResBlock& rb = s.rb(j);
        if (rb.dil.size() != nd) return AMP_OK;
        const RbBufs b = rb_bufs(s, j, true);
        const float* cur = s.U;
        for (size_t p = 0; p < nd; ++p) {
            float* dst = p + 1 == nd ? b.XS : (cur == b.R ? b.TMP : b.R);
            if (!pair_tile_args(rb.c1[p].get(), rb.c2[p].get(), cur, s.B, s.t, kLreluSlope, dst, 0, (float)nk, s.lens, s.lm, &plan[p].a[sl]))
                return AMP_OK;
            plan[p].n[sl] = s.B * plan[p].a[sl].tiles_per_item;
            cur = dst;
        }
    }
    for (const Pair3Args& p : plan) AMP_HIP(launch_pair3(p, s.st));
    AMP_RC(launch_stage_mrf_sum(s, nullptr));
    *ran = true;
    return AMP_OK;
}

// The same for a stage of UNFUSED whole-K convs (the C = 256 stage of a single utterance): c1 of a dilation, then c2, of all three
// resblocks in one launch each (conv_small3_f16x3.hip); only the three convs that accumulate into XS stay separate launches, in resblock
// order with their `=` / `+=` / `(y + v) / n` modes (they add y BEFORE the products: no post-hoc mean).  Every launch is planned first
// (conv_run with plan_small launches nothing): *ran = false, nothing launched, when one of them is not a whole-K conv.
static int try_stage_small3(const Stage& s, const int slot_of[3], bool* ran) {
    *ran = false;
    const int nk = s.g->d.n_kernels;
    for (int j = 0; j < 3; ++j)
        if (pair_supported(s.rb(j).c1[0].get(), s.rb(j).c2[0].get())) return AMP_OK;
    const size_t nd = s.rb(0).dil.size();
    struct Step { ConvSmall3Args p; int ni[3]; };
    std::vector<Step> steps;                        // c1(d_0), c2, c1(d_1), c2, ..., c1(d_last)
    const float* cur[3] = {s.U, s.U, s.U};
    RbBufs b[3];
    for (int j = 0; j < 3; ++j) b[j] = rb_bufs(s, j, true);
    auto plan3 = [&](bool second, size_t p) -> bool {    // one merged launch: c1[p] (second = false) or c2[p] of the three resblocks
        Step sp{};
        for (int sl = 0; sl < 3; ++sl) {
            const int j = slot_of[sl];
            const amp_conv* c = second ? s.rb(j).c2[p].get() : s.rb(j).c1[p].get();
            const int rc = second ? conv_run(c, b[j].TMP, s.B, s.t, 1.f, cur[j], 1.f, b[j].R, 0, 1.f, s.st, 0, s.lens, s.lm, &sp.p.a[sl], &sp.ni[sl])
                                  : conv_run(c, cur[j], s.B, s.t, kLreluSlope, nullptr, kLreluSlope, b[j].TMP, 0, 1.f, s.st, 0, s.lens, s.lm, &sp.p.a[sl], &sp.ni[sl]);
            if (rc != AMP_OK) return false;
            sp.p.nx[sl] = s.B * sp.p.a[sl].tiles_per_item;
            sp.p.ny[sl] = (sp.p.a[sl].M + 127) / 128;
        }
        if (sp.ni[1] != 1 || sp.ni[2] != 1) return false;
        steps.push_back(sp);
        return true;
    };
    bool ok = true;
    for (size_t p = 0; ok && p < nd; ++p) {
        for (int j = 0; j < 3 && ok; ++j) ok = s.rb(j).dil.size() == nd;
        ok = ok && plan3(false, p);
        if (ok && p + 1 < nd) {
            ok = plan3(true, p);
            for (int j = 0; j < 3; ++j) cur[j] = b[j].R;
        }
    }
    // the accumulating convs must be whole-K launches too
    for (int j = 0; ok && j < 3; ++j) {
        ConvArgs unused_a; int unused_ni;
        ok = conv_run(s.rb(j).c2[nd - 1].get(), b[j].TMP, s.B, s.t, 1.f, cur[j], 1.f, s.XS, accumulate_mode(j, nk), (float)nk, s.st, 0, s.lens,
                      s.lm, &unused_a, &unused_ni) == AMP_OK;
    }
    if (!ok) return AMP_OK;
    for (const Step& sp : steps) AMP_HIP(launch_conv_small3(sp.p, sp.ni, s.st));
    for (int j = 0; j < 3; ++j)
        AMP_RC(conv_run(s.rb(j).c2[nd - 1].get(), b[j].TMP, s.B, s.t, 1.f, cur[j], 1.f, s.XS, accumulate_mode(j, nk), (float)nk, s.st, 0, s.lens, s.lm));
    *ran = true;
    return AMP_OK;
}

// Called right before a resblock's launch that writes XS: in a concurrent chain that launch reads what resblock j - 1 accumulated there and
// first waits for it (`wait` = evs[j]; null otherwise).
static int wait_before_last(hipEvent_t wait, hipStream_t sj) {
    if (wait) AMP_HIP(hipStreamWaitEvent(sj, wait, 0));
    return AMP_OK;
}

// ResBlock1 (HiFi-GAN), U -> b.XS on sj with the MRF mode mode_last: the whole resblock in one or two launches, else pair by pair (a fused
// pair, or its two convs)
static int run_resblock1(const Stage& s, const ResBlock& rb, const RbBufs& b, int mode_last, hipEvent_t wait, hipStream_t sj) {
    const int B = s.B, t = s.t;
    const float nk = (float)s.g->d.n_kernels;
    if (rb_supported(rb.c1, rb.c2, B, t)) {
        // the whole resblock in one launch: U -> XS (x and the residual never leave the CU in between) -- or in two, rb_split()
        const int sp = rb_split(rb.c1, B, t);
        if (sp > 0) AMP_RC(rb_run(rb.c1, rb.c2, s.U, B, t, kLreluSlope, b.R, 0, 1.f, sj, s.lens, s.lm, 0, sp));
        AMP_RC(wait_before_last(wait, sj));
        return rb_run(rb.c1, rb.c2, sp > 0 ? b.R : s.U, B, t, kLreluSlope, b.XS, mode_last, nk, sj, s.lens, s.lm, sp, -1);
    }
    const int nd = (int)rb.dil.size();
    const float* cur = s.U;
    for (int p = 0; p < nd; ++p) {
        const bool last = p == nd - 1;
        const amp_conv *c1 = rb.c1[p].get(), *c2 = rb.c2[p].get();
        if (pair_supported(c1, c2)) {
            // the whole pair in one kernel; the output ping-pongs R <-> TMP (never in place: other tiles still read the input's halo)
            float* dst = last ? b.XS : (cur == b.R ? b.TMP : b.R);
            if (last) AMP_RC(wait_before_last(wait, sj));
            AMP_RC(pair_run(c1, c2, cur, B, t, kLreluSlope, dst, last ? mode_last : 0, nk, sj, s.lens, s.lm));
            cur = dst;
            continue;
        }
        // xt = lrelu(c1(lrelu(x))) ; x = c2(xt) + x        hifigan.py:93-100
        if (cur == b.TMP) {  // previous pair was fused into TMP: keep the unfused ping-pong legal
            AMP_HIP(hipMemcpyAsync(b.R, b.TMP, (size_t)B * s.C * t * sizeof(float), hipMemcpyDeviceToDevice, sj));
            cur = b.R;
        }
        AMP_RC(conv_run(c1, cur, B, t, kLreluSlope, nullptr, kLreluSlope, b.TMP, 0, 1.f, sj, 0, s.lens, s.lm));
        if (!last) { AMP_RC(conv_run(c2, b.TMP, B, t, 1.f, cur, 1.f, b.R, 0, 1.f, sj, 0, s.lens, s.lm)); cur = b.R; }
        else { AMP_RC(wait_before_last(wait, sj)); AMP_RC(conv_run(c2, b.TMP, B, t, 1.f, cur, 1.f, b.XS, mode_last, nk, sj, 0, s.lens, s.lm)); }
    }
    return AMP_OK;
}

// AMPBlock1 (BigVGAN), U -> b.XS: the whole block in one launch, else per pair act1d, c1, act1d, c2 + residual
static int run_ampblock1(const Stage& s, const ResBlock& rb, const RbBufs& b, int mode_last, hipEvent_t wait, hipStream_t sj) {
    const int B = s.B, t = s.t, nd = (int)rb.dil.size();
    const float nk = (float)s.g->d.n_kernels;
    if (nd <= AMP_AMPB_MAX_STEPS / 2) {
        const amp_conv *p1[AMP_AMPB_MAX_STEPS / 2], *p2[AMP_AMPB_MAX_STEPS / 2];
        for (int p = 0; p < nd; ++p) { p1[p] = rb.c1[p].get(); p2[p] = rb.c2[p].get(); }
        if (ampb_supported(p1, p2, nd, rb.acts.data(), rb.acts.size(), B, t)) {
            // the whole AMPBlock in one launch: U -> XS (bigvgan.py:137-146)
            AMP_RC(wait_before_last(wait, sj));
            return ampb_run(p1, p2, nd, rb.acts.data(), s.U, B, t, b.XS, mode_last, nk, sj, s.lens, s.lm);
        }
    }
    const float* cur = s.U;   // U, then R: never TMP (no fused pairs here)
    for (int p = 0; p < nd; ++p) {
        // xt = c2(a2(c1(a1(x)))) ; x = xt + x              bigvgan.py:137-146
        const ActParams& a1 = rb.acts[2 * p];
        const ActParams& a2 = rb.acts[2 * p + 1];
        AMP_HIP(launch_act1d(cur, b.ACT, B, s.C, t, a1.a_dev, a1.invb_dev, a1.fu_dev, a1.fd_dev, s.lens, s.lm, sj, next_rev(s.lens)));
        AMP_RC(conv_run(rb.c1[p].get(), b.ACT, B, t, 1.f, nullptr, 1.f, b.TMP, 0, 1.f, sj, 0, s.lens, s.lm));
        AMP_HIP(launch_act1d(b.TMP, b.ACT, B, s.C, t, a2.a_dev, a2.invb_dev, a2.fu_dev, a2.fd_dev, s.lens, s.lm, sj, next_rev(s.lens)));
        if (p < nd - 1) { AMP_RC(conv_run(rb.c2[p].get(), b.ACT, B, t, 1.f, cur, 1.f, b.R, 0, 1.f, sj, 0, s.lens, s.lm)); cur = b.R; }
        else { AMP_RC(wait_before_last(wait, sj)); AMP_RC(conv_run(rb.c2[p].get(), b.ACT, B, t, 1.f, cur, 1.f, b.XS, mode_last, nk, sj, 0, s.lens, s.lm)); }
    }
    return AMP_OK;
}

// ResBlock2 / AMPBlock2, U -> b.XS: x = c(act(x)) + x per dilation          hifigan.py:140-145, bigvgan.py:218-224
static int run_resblock2(const Stage& s, const ResBlock& rb, const RbBufs& b, int mode_last, hipEvent_t wait, hipStream_t sj) {
    const bool big = s.g->d.arch == AMP_ARCH_BIGVGAN;
    const int B = s.B, t = s.t, nd = (int)rb.dil.size();
    const float* cur = s.U;
    for (int p = 0; p < nd; ++p) {
        const float* in = cur;
        float sl = kLreluSlope;
        if (big) {
            const ActParams& a1 = rb.acts[p];
            AMP_HIP(launch_act1d(cur, b.ACT, B, s.C, t, a1.a_dev, a1.invb_dev, a1.fu_dev, a1.fd_dev, s.lens, s.lm, sj, next_rev(s.lens)));
            in = b.ACT;
            sl = 1.f;
        }
        if (p < nd - 1) {
            // the conv reads a halo of `in`; never write the tensor it is reading
            float* dst = (in == cur && cur == b.R) ? b.TMP : b.R;
            AMP_RC(conv_run(rb.c1[p].get(), in, B, t, sl, cur, 1.f, dst, 0, 1.f, sj, 0, s.lens, s.lm));
            cur = dst;
        } else {
            AMP_RC(wait_before_last(wait, sj));
            AMP_RC(conv_run(rb.c1[p].get(), in, B, t, sl, cur, 1.f, b.XS, mode_last, (float)s.g->d.n_kernels, sj, 0, s.lens, s.lm));
        }
    }
    return AMP_OK;
}

// A stage whose resblocks ALL end in a fused pair / whole-resblock kernel (HiFi-GAN, C <= 128) needs no chain in the concurrent mode: those
// kernels add the accumulated y to their finished, rounded result, so each resblock stores its own result (mode 0) and one small launch
// forms ((XS0 + XS1) + XS2) / n afterwards -- the same bits with one join instead of two chained cross-queue waits (~12 us each).
static bool stage_sums_separately(const Stage& s) {
    const amp_gen_desc& d = s.g->d;
    if (!s.conc || d.resblock_type != 1 || d.arch == AMP_ARCH_BIGVGAN || d.n_kernels - 1 > AMP_MRF_MAX_PARTS) return false;
    for (int j = 0; j < d.n_kernels; ++j) {
        const ResBlock& rb = s.rb(j);
        const size_t last = rb.dil.size() - 1;
        if (!rb_supported(rb.c1, rb.c2, s.B, s.t) && !pair_supported(rb.c1[last].get(), rb.c2[last].get())) return false;
    }
    return true;
}

// profiled forward: every launch of one resblock logs its kernel's name (note_kernel, amp_internal.h)
struct KernelLogScope {
    explicit KernelLogScope(std::string* p) { tl_kernel_log = p; if (p) p->clear(); }
    ~KernelLogScope() { tl_kernel_log = nullptr; }
};

// The stage's resblocks U -> XS, one after the other on `st` -- or, concurrent mode, resblock 0 on `st` and resblocks 1 .. nk - 1 on the side
// streams: evs[0] fork, evs[1 + j] = resblock j's accumulating launch done; the launch that accumulates resblock j >= 1 waits for evs[j] and
// `st` joins on evs[nk] (a chain), or `st` waits for them all and forms the MRF mean itself (stage_sums_separately).  (Measured the other way
// round too -- the widest resblock on `st`, the others on the side streams: the same 0.81-0.83 ms as a graph replay, but 1.08 instead of
// 0.90-0.95 ms eager, where the host issues the critical stream's launches last.)  ev_rb / rb_names: the profiled forward's per-resblock
// events and kernel names.
static int run_stage_resblocks(const Stage& s, hipEvent_t* ev_rb, std::vector<std::string>* rb_names) {
    amp_gen* g = s.g;
    const int nk = g->d.n_kernels;
    const size_t ev0 = (size_t)s.i * (nk + 1);
    hipEvent_t* evs = s.conc ? &g->ev_side[ev0] : nullptr;
    const bool sum_stage = stage_sums_separately(s);
    if (s.conc) {
        AMP_HIP(hipEventRecord(evs[0], s.st));
        for (int j = 1; j < nk; ++j) AMP_HIP(hipStreamWaitEvent(g->side[j - 1], evs[0], 0));
    }
    for (int j = 0; j < nk; ++j) {
        const hipStream_t sj = (s.conc && j > 0) ? g->side[j - 1] : s.st;
        RbBufs b = rb_bufs(s, j, s.conc);
        if (!sum_stage) b.XS = s.XS;                                             // a chain: every resblock accumulates into XS
        const hipEvent_t wait = (s.conc && !sum_stage && j > 0) ? evs[j] : nullptr;
        const int mode_last = sum_stage ? 0 : accumulate_mode(j, nk);
        if (ev_rb) AMP_HIP(hipEventRecord(ev_rb[ev0 + j], sj));
        {
            KernelLogScope log_scope(rb_names ? &(*rb_names)[(size_t)s.i * nk + j] : nullptr);
            const ResBlock& rb = s.rb(j);
            if (g->d.resblock_type != 1) AMP_RC(run_resblock2(s, rb, b, mode_last, wait, sj));
            else if (g->d.arch == AMP_ARCH_BIGVGAN) AMP_RC(run_ampblock1(s, rb, b, mode_last, wait, sj));
            else AMP_RC(run_resblock1(s, rb, b, mode_last, wait, sj));
        }
        if (s.conc) AMP_HIP(hipEventRecord(evs[1 + j], sj));
    }
    if (s.conc && !sum_stage) AMP_HIP(hipStreamWaitEvent(s.st, evs[nk], 0));   // join: the last resblock's accumulating launch follows all the others
    if (sum_stage) AMP_RC(launch_stage_mrf_sum(s, evs));
    if (ev_rb) AMP_HIP(hipEventRecord(ev_rb[ev0 + nk], s.st));
    return AMP_OK;
}

// One group of `B` items through the whole generator (buffers sized for `be` elements each).
static int gen_forward_group(amp_gen* g, const float* mel_dev, const float* cond_dev, const int* lens, int B, int T,
                             float* wav_dev, float* base, size_t be, hipStream_t st,
                             hipEvent_t* ev_mrf /* 2 per stage, or null */, hipEvent_t* ev_rb /* (n_kernels+1) per stage */,
                             std::vector<std::string>* rb_names = nullptr /* per (stage, resblock), or null */,
                             bool conc = false /* resblocks of a stage on g->side streams (the buffers behind the regular ones exist) */) {
    const amp_gen_desc& d = g->d;
    const bool big = d.arch == AMP_ARCH_BIGVGAN;
    float* X = base;            // stage input / MRF accumulator (ping-pong with XS)
    float* XS = base + be;
    float* U = base + 2 * be;   // upsampled stage tensor (input of every resblock)
    Stage s{};
    s.g = g; s.B = B; s.lens = lens; s.st = st; s.conc = conc; s.U = U;
    s.R = base + 3 * be;
    s.TMP = base + 4 * be;
    s.ACT = big ? base + 5 * be : nullptr;
    s.SIDE = base + (size_t)gen_num_bufs(g) * be;
    s.side_per = big ? 4 : 3;
    s.be = be;
    float* CB = base + (size_t)(gen_num_bufs(g) + (conc ? gen_side_bufs(g) : 0)) * be;  // cond(g): [B, C0]

    AMP_RC(conv_run(g->conv_pre.get(), mel_dev, B, T, 1.f, nullptr, 1.f, X, 0, 1.f, st, 0, lens, 1));
    if (cond_dev) {  // x = x + self.cond(g), hifigan.py:426-427 (g has length 1 -> per-channel bias)
        AMP_RC(conv_run(g->cond.get(), cond_dev, B, 1, 1.f, nullptr, 1.f, CB, 0, 1.f, st));
        AMP_HIP(launch_add_channel_bias(X, CB, B, d.upsample_initial_channel, T, st));
    }
    // the horizontal stage forms: concurrent mode, at most kRbHorizontalMaxFrames mel frames, three ResBlock1 per stage
    const bool horizontal = conc && (long long)B * T <= kRbHorizontalMaxFrames && d.resblock_type == 1 && !big && d.n_kernels == 3;
    int t = T;
    int lm = 1;  // samples per mel frame at the current stage
    for (int i = 0; i < d.n_stages; ++i) {
        // HiFiGAN: leaky_relu(0.1) before the transposed conv (hifigan.py:206); BigVGAN: none (bigvgan.py:316-318)
        AMP_RC(conv_run(g->ups[i].get(), X, B, t, big ? 1.f : kLreluSlope, nullptr, 1.f, U, 0, 1.f, st, 0, lens, lm));
        t *= d.upsample_rates[i];
        lm *= d.upsample_rates[i];
        if (ev_mrf) AMP_HIP(hipEventRecord(ev_mrf[2 * i], st));
        s.i = i; s.t = t; s.C = g->ch[i]; s.lm = lm; s.XS = XS;
        bool ran = false;
        int slot_of[3];
        if (horizontal && horizontal_slots(s, slot_of)) {
            AMP_RC(try_stage_pair3(s, slot_of, &ran));
            if (!ran) AMP_RC(try_stage_small3(s, slot_of, &ran));
        }
        if (!ran) AMP_RC(run_stage_resblocks(s, ev_rb, rb_names));
        if (ev_mrf) AMP_HIP(hipEventRecord(ev_mrf[2 * i + 1], st));
        float* tmp = X; X = XS; XS = tmp;  // x = xs / num_kernels
    }
    if (big) {
        AMP_HIP(launch_act1d(X, s.ACT, B, g->post_cin, t, g->act_post.a_dev, g->act_post.invb_dev, g->act_post.fu_dev, g->act_post.fd_dev, lens, lm, st, next_rev(lens)));
        AMP_HIP(launch_conv_post(s.ACT, g->post_w_dev, g->post_b_dev, wav_dev, B, g->post_cin, t, 7, 1.f, 1, lens, lm, st));
    } else {
        // F.leaky_relu(x) with the DEFAULT slope 0.01 (hifigan.py:215,439), conv_post, tanh
        AMP_HIP(launch_conv_post(X, g->post_w_dev, g->post_b_dev, wav_dev, B, g->post_cin, t, 7, 0.01f, 1, lens, lm, st));
    }
    return AMP_OK;
}

// The side streams and fork / join events of the concurrent-resblock mode; false when they do not exist and cannot be created now
// (`st` is being captured: hipStreamCreate is not a capturable call -- the forward then runs the sequential chain, same bits).
static bool gen_ensure_side(amp_gen* g, hipStream_t st) {
    const size_t ns = (size_t)g->d.n_kernels - 1, ne = (size_t)g->d.n_stages * (g->d.n_kernels + 1);
    if (g->side.size() == ns && g->ev_side.size() == ne) return true;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) { (void)hipGetLastError(); return false; }
    while (g->side.size() < ns) {
        hipStream_t s_ = nullptr;
        if (hipStreamCreateWithFlags(&s_, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); return false; }
        g->side.push_back(s_);
    }
    while (g->ev_side.size() < ne) {
        hipEvent_t e = nullptr;
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); return false; }
        g->ev_side.push_back(e);
    }
    return true;
}

int amp_set_resblock_streams(int mode) {
    if (mode < -1 || mode > 1) { set_error("amp_set_resblock_streams: mode=%d", mode); return AMP_ERR_INVALID; }
    cfg().rb_streams = mode;
    return AMP_OK;
}

int amp_gen_prepare_streams(amp_gen* g) {
    if (!g || !g->finalized) { set_error("amp_gen_prepare_streams: null or unfinalized handle"); return AMP_ERR_STATE; }
    if (g->d.n_kernels < 2) return AMP_OK;
    if (!gen_ensure_side(g, nullptr)) { set_error("amp_gen_prepare_streams: could not create the side streams"); return AMP_ERR_HIP; }
    return AMP_OK;
}

int amp_gen_forward(amp_gen* g, const float* mel_dev, const float* cond_dev, int B, int T, float* wav_dev,
                    void* workspace_dev, size_t workspace_bytes, void* stream_) {
    return amp_gen_forward_ragged(g, mel_dev, cond_dev, nullptr, B, T, wav_dev, workspace_dev, workspace_bytes, stream_);
}

int amp_gen_forward_ragged(amp_gen* g, const float* mel_dev, const float* cond_dev, const int32_t* lens_dev, int B, int T,
                           float* wav_dev, void* workspace_dev, size_t workspace_bytes, void* stream_) {
    if (!g || !mel_dev || !wav_dev || !workspace_dev) { set_error("amp_gen_forward: null argument"); return AMP_ERR_INVALID; }
    if (!g->finalized) { set_error("amp_gen_forward: call amp_gen_finalize first"); return AMP_ERR_STATE; }
    if (B <= 0 || T <= 0) { set_error("amp_gen_forward: B=%d T=%d", B, T); return AMP_ERR_INVALID; }
    if (workspace_bytes < amp_gen_workspace_bytes(g, B, T)) { set_error("amp_gen_forward: workspace too small (%zu < %zu)", workspace_bytes, amp_gen_workspace_bytes(g, B, T)); return AMP_ERR_INVALID; }
    if (cond_dev && !g->cond) { set_error("amp_gen_forward: cond given but gin_channels == 0"); return AMP_ERR_INVALID; }
    hipStream_t st = (hipStream_t)stream_;
    std::lock_guard<std::mutex> launch_lock(g->launch_mu);
    AMP_RC(range_poll(&g->guard, st)); // a previous forward of this handle left the f16 operand range: say so now
    struct FlagScope { FlagScope(unsigned* p) { tl_range_flag = p; } ~FlagScope() { tl_range_flag = nullptr; } } flag_scope(g->guard.dev);
    const amp_gen_desc& d = g->d;
    const int G = gen_group_items(g, B, T);
    const int ngroups = (B + G - 1) / G;
    const size_t be = gen_buf_elems(g, G, T);
    const size_t L = (size_t)T * g->hop;
    amp_gen::ProfSlot* ps = g->prof.empty() ? nullptr : &g->prof[g->prof_count % g->prof.size()];
    // concurrent resblocks: small launches, the whole batch in one group, not while the per-resblock events are being recorded (they
    // time one resblock after the other on `st`)
    const bool conc = ngroups == 1 && !ps && gen_streams_wanted(g, B, T) && gen_ensure_side(g, st);
    if (ps) {
        const size_t need = 2 * (size_t)d.n_stages * ngroups;
        while (ps->ev_mrf.size() < need) {
            hipEvent_t e;
            AMP_HIP(hipEventCreate(&e));
            ps->ev_mrf.push_back(e);
        }
        const size_t need_rb = (size_t)d.n_stages * (d.n_kernels + 1) * ngroups;
        while (ps->ev_rb.size() < need_rb) {
            hipEvent_t e;
            AMP_HIP(hipEventCreate(&e));
            ps->ev_rb.push_back(e);
        }
        ps->ev_groups = ngroups;
        ps->rb_kernels.assign((size_t)d.n_stages * d.n_kernels, std::string());
        AMP_HIP(hipEventRecord(ps->ev_begin, st));
    }
    for (int gi = 0; gi < ngroups; ++gi) {
        const int b0 = gi * G;
        const int Bg = (B - b0) < G ? (B - b0) : G;
        AMP_RC(gen_forward_group(g, mel_dev + (size_t)b0 * d.n_in * T,
                                 cond_dev ? cond_dev + (size_t)b0 * d.gin_channels : nullptr,
                                 lens_dev ? lens_dev + b0 : nullptr, Bg, T,
                                 wav_dev + (size_t)b0 * L, (float*)workspace_dev, be, st,
                                 ps ? ps->ev_mrf.data() + 2 * (size_t)d.n_stages * gi : nullptr,
                                 ps ? ps->ev_rb.data() + (size_t)d.n_stages * (d.n_kernels + 1) * gi : nullptr,
                                 (ps && gi == 0) ? &ps->rb_kernels : nullptr, conc));
    }
    if (ps) { AMP_HIP(hipEventRecord(ps->ev_end, st)); ps->valid = true; ++g->prof_count; }
    AMP_RC(range_publish(&g->guard, st));
    return AMP_OK;
}

int amp_range_check(void* stream_) {
    return range_check_sync(guard_for_current_device(), (hipStream_t)stream_, "amp_range_check");
}

int amp_gen_range_check(amp_gen* g, void* stream_) {
    if (!g) { set_error("amp_gen_range_check: null handle"); return AMP_ERR_INVALID; }
    return range_check_sync(&g->guard, (hipStream_t)stream_, "amp_gen_range_check");
}

void amp_gen_destroy(amp_gen* g) { delete g; }

// ---- op level ------------------------------------------------------------------------------------
int amp_conv_create(int transposed, int cin, int cout, int k, int stride, int dilation, int padding,
                    const float* weight_host, const float* bias_host, amp_conv** out) {
    if (!weight_host || !out) { set_error("amp_conv_create: null argument"); return AMP_ERR_INVALID; }
    if (amp_device_count() <= 0) { set_error("amp_conv_create: no HIP device visible (the HIP path has no CPU fallback)"); return AMP_ERR_HIP; }
    auto c = std::make_unique<amp_conv>();
    c->transposed = transposed; c->cin = cin; c->cout = cout; c->k = k; c->stride = stride; c->dilation = dilation; c->padding = padding;
    int rc = conv_build(c.get(), weight_host, bias_host);
    if (rc != AMP_OK) return rc;
    *out = c.release();
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

// WN.in_layers[i] with its 2H rows packed for the gate epilogue: packed row 32*mb + i + 4*hi + 8*(2u + s) holds original
// row s*H + 16*mb + i + 4*hi + 8*u (s = 0: tanh half, 1: sigmoid half), so that the MFMA C layout hands one lane both
// pre-activations of a channel (conv_small_f16x3.hip, EPI_GATE).
int amp_conv_create_gated(int hidden, int k, int dilation, int padding, const float* weight_host, const float* bias_host,
                          amp_conv** out) {
    if (!weight_host || !out) { set_error("amp_conv_create_gated: null argument"); return AMP_ERR_INVALID; }
    if (amp_device_count() <= 0) { set_error("amp_conv_create_gated: no HIP device visible (the HIP path has no CPU fallback)"); return AMP_ERR_HIP; }
    if (hidden <= 0 || hidden % 32 != 0) { set_error("amp_conv_create_gated: hidden=%d must be a multiple of 32", hidden); return AMP_ERR_UNSUPPORTED; }
    if (default_precision() != PREC_F16X3) { set_error("amp_conv_create_gated: the fused WN layer exists for the f16x3 arithmetic only"); return AMP_ERR_UNSUPPORTED; }
    const int H = hidden, M = 2 * H;
    const size_t rowlen = (size_t)H * k;
    std::vector<float> wperm((size_t)M * rowlen), bperm((size_t)M, 0.f);
    for (int p = 0; p < M; ++p) {
        const int mb = p >> 5, rho = p & 31;
        const int i = rho & 3, hi = (rho >> 2) & 1, jj = rho >> 3, s = jj & 1, u = jj >> 1;
        const int orow = s * H + 16 * mb + i + 4 * hi + 8 * u;
        memcpy(&wperm[(size_t)p * rowlen], &weight_host[(size_t)orow * rowlen], rowlen * sizeof(float));
        if (bias_host) bperm[p] = bias_host[orow];
    }
    auto c = std::make_unique<amp_conv>();
    c->transposed = 0; c->cin = H; c->cout = M; c->k = k; c->stride = 1; c->dilation = dilation; c->padding = padding;
    int rc = conv_build(c.get(), wperm.data(), bperm.data());   // the gate epilogue reads the bias unconditionally (zeros when absent)
    if (rc != AMP_OK) return rc;
    if (!small_conv_static_ok(c.get()) || conv_out_len(c.get(), 64) != 64) {
        set_error("amp_conv_create_gated: H=%d k=%d dilation=%d padding=%d is outside the fused WN kernel (k in {1,3,5}, H <= 256, 'same' padding, (k-1)*dilation <= 64)", H, k, dilation, padding);
        return AMP_ERR_UNSUPPORTED;
    }
    c->gated_H = H;
    *out = c.release();
    return AMP_OK;
}

// Common ConvArgs of a conv_small launch over [B, cin, T] -> T output columns, tiles of 32 * ni columns.
static void small_args(const amp_conv* c, const float* x, int B, int T, const int* lens, int ni, ConvArgs* a) {
    *a = ConvArgs{};
    a->x = x; a->wp = c->wp_dev; a->bias = c->bias_dev;
    a->B = B; a->Cin = c->cin; a->Tin = T; a->xbs = (long long)c->cin * T; a->nchunks = c->nchunks; a->M = c->M; a->Mpad = c->Mpad;
    a->Tq = T; a->tiles_per_item = (T + 32 * ni - 1) / (32 * ni);
    a->off0 = c->off0; a->dstep = c->dstep; a->halo_left = c->halo_left; a->wd = 32 * ni + c->halo_left + c->halo_right;
    a->Cout = c->cout; a->Tout = T; a->up = 1; a->up_pad = 0;
    a->slope_in = 1.f; a->slope_out = 1.f; a->mode = 0; a->div = 1.f;
    a->lens = lens; a->len_mul = 1;
    a->acc_scale = 16.f * c->wscale; a->inv_scale = 1.f / a->acc_scale;
    a->range_flag = range_flag_for_current_device();
}

int amp_wn_forward(const amp_conv* const* in_layers, const amp_conv* const* res_skip_layers, int n_layers, float* x_dev,
                   const float* cond_dev, long long cond_batch_stride, const int32_t* lens_dev, int B, int T,
                   float* acts_ws_dev, float* out_dev, void* stream_) {
    if (!in_layers || !res_skip_layers || n_layers <= 0 || !x_dev || !acts_ws_dev || !out_dev || B <= 0 || T <= 0) {
        set_error("amp_wn_forward: bad argument");
        return AMP_ERR_INVALID;
    }
    hipStream_t stream = (hipStream_t)stream_;
    const int H = in_layers[0] ? in_layers[0]->gated_H : 0;
    for (int i = 0; i < n_layers; ++i) {
        const amp_conv* ci = in_layers[i];
        const amp_conv* cr = res_skip_layers[i];
        if (!ci || !cr) { set_error("amp_wn_forward: null layer %d", i); return AMP_ERR_INVALID; }
        const int rs_out = i < n_layers - 1 ? 2 * H : H;
        if (!ci->gated_H || ci->gated_H != H || cr->k != 1 || cr->cin != H || cr->cout != rs_out || cr->gated_H ||
            !small_conv_static_ok(cr) || cr->tanh_out || ci->tanh_out || !cr->bias_dev || !ci->bias_dev) {
            set_error("amp_wn_forward: layer %d is not an (amp_conv_create_gated in-layer, 1x1 %d -> %d res_skip) pair", i, H, rs_out);
            return AMP_ERR_INVALID;
        }
    }
    for (int i = 0; i < n_layers; ++i) {
        ConvArgs a;
        const int ni_in = small_conv_ni(in_layers[i]), ni_rs = small_conv_ni(res_skip_layers[i]);
        small_args(in_layers[i], x_dev, B, T, lens_dev, ni_in, &a);       // in_layers[i](x * mask) + g_l -> tanh * sigmoid (round 4: the mask is the kernel's
                                                                          // select at staging, so the caller's x need not be masked; tiles beyond an end are skipped)
        a.y = acts_ws_dev; a.wn_H = H;
        a.gate_cond = cond_dev ? cond_dev + (size_t)i * 2 * H : nullptr;
        a.gate_cond_bs = cond_batch_stride;
        AMP_HIP(launch_conv_small(in_layers[i]->KT, ni_in, 1, a, stream));
        small_args(res_skip_layers[i], acts_ws_dev, B, T, nullptr, ni_rs, &a);   // res_skip(acts) -> x, output
        a.lens = lens_dev;                                                // the mask of the x update (acts is read densely)
        a.wn_H = H; a.wn_x = x_dev; a.wn_out = out_dev; a.wn_first = i == 0; a.wn_last = i == n_layers - 1;
        AMP_HIP(launch_conv_small(1, ni_rs, 2, a, stream));
    }
    return AMP_OK;
}

int amp_conv_out_len(const amp_conv* c, int T) { return c ? conv_out_len(c, T) : 0; }

int amp_conv_forward(const amp_conv* c, const float* x_dev, int B, int T, float slope_in, const float* res_dev,
                     float slope_out, float* y_dev, void* stream) {
    if (!c || !x_dev || !y_dev) { set_error("amp_conv_forward: null argument"); return AMP_ERR_INVALID; }
    if (x_dev == y_dev) { set_error("amp_conv_forward: x and y must not alias (the conv reads a halo)"); return AMP_ERR_INVALID; }
    return conv_run(c, x_dev, B, T, slope_in, res_dev, slope_out, y_dev, 0, 1.f, (hipStream_t)stream);
}

int amp_conv_forward_strided(const amp_conv* c, const float* x_dev, long long x_batch_stride, int B, int T,
                             float slope_in, const float* res_dev, float slope_out, float* y_dev, void* stream) {
    if (!c || !x_dev || !y_dev) { set_error("amp_conv_forward_strided: null argument"); return AMP_ERR_INVALID; }
    if (x_batch_stride < (long long)c->cin * T) { set_error("amp_conv_forward_strided: batch stride %lld < cin*T", x_batch_stride); return AMP_ERR_INVALID; }
    return conv_run(c, x_dev, B, T, slope_in, res_dev, slope_out, y_dev, 0, 1.f, (hipStream_t)stream, x_batch_stride);
}

// conv(x * mask): the sequence mask of the callers (`conv_1(x * x_mask)`, attentions.py:392-400; DDSConv / WN inputs) taken by the
// kernel -- columns t >= lens[b] of x count as zero (a select at staging: whatever the buffer holds there, NaN included, is never
// used) and output tiles that lie wholly beyond an utterance's end are skipped, so columns t >= lens[b] of y are UNSPECIFIED.
int amp_conv_forward_ragged(const amp_conv* c, const float* x_dev, long long x_batch_stride, int B, int T, const int32_t* lens_dev,
                            float slope_in, const float* res_dev, float slope_out, float* y_dev, void* stream) {
    if (!c || !x_dev || !y_dev) { set_error("amp_conv_forward_ragged: null argument"); return AMP_ERR_INVALID; }
    if (x_dev == y_dev) { set_error("amp_conv_forward_ragged: x and y must not alias (the conv reads a halo)"); return AMP_ERR_INVALID; }
    if (x_batch_stride != 0 && x_batch_stride < (long long)c->cin * T) { set_error("amp_conv_forward_ragged: batch stride %lld < cin*T", x_batch_stride); return AMP_ERR_INVALID; }
    if (lens_dev && (c->transposed || c->pad_reflect || conv_out_len(c, T) != T)) {
        set_error("amp_conv_forward_ragged: valid lengths need a 'same' zero-padded Conv1d (output length == input length)");
        return AMP_ERR_UNSUPPORTED;
    }
    return conv_run(c, x_dev, B, T, slope_in, res_dev, slope_out, y_dev, 0, 1.f, (hipStream_t)stream, x_batch_stride, lens_dev);
}

int amp_pair_forward(const amp_conv* c1, const amp_conv* c2, const float* x_dev, int B, int T, float slope,
                     float* y_dev, void* stream) {
    if (!c1 || !c2 || !x_dev || !y_dev) { set_error("amp_pair_forward: null argument"); return AMP_ERR_INVALID; }
    if (B <= 0 || T <= 0) { set_error("amp_pair_forward: B=%d T=%d", B, T); return AMP_ERR_INVALID; }
    if (!pair_supported(c1, c2)) {
        set_error("amp_pair_forward: pair (C=%d k=%d dilation=%d) is not covered by the fused kernel", c1->cin, c1->k, c1->dilation);
        return AMP_ERR_UNSUPPORTED;
    }
    return pair_run(c1, c2, x_dev, B, T, slope, y_dev, 0, 1.f, (hipStream_t)stream);
}

int amp_resblock_forward(const amp_conv* const* c1, const amp_conv* const* c2, int n_pairs, const float* x_dev, int B, int T,
                         float slope, float* y_dev, void* stream) {
    if (!c1 || !c2 || !x_dev || !y_dev) { set_error("amp_resblock_forward: null argument"); return AMP_ERR_INVALID; }
    if (B <= 0 || T <= 0 || n_pairs < 1 || n_pairs > AMP_RB_MAX_PAIRS) { set_error("amp_resblock_forward: B=%d T=%d n_pairs=%d", B, T, n_pairs); return AMP_ERR_INVALID; }
    // borrowed handles in the containers rb_supported / rb_run take; released (not destroyed) on every path
    std::vector<std::unique_ptr<amp_conv>> v1, v2;
    for (int p = 0; p < n_pairs; ++p) { v1.emplace_back(const_cast<amp_conv*>(c1[p])); v2.emplace_back(const_cast<amp_conv*>(c2[p])); }
    struct Release { std::vector<std::unique_ptr<amp_conv>>&a, &b; ~Release() { for (auto& p : a) (void)p.release(); for (auto& p : b) (void)p.release(); } } rel{v1, v2};
    for (int p = 0; p < n_pairs; ++p) if (!c1[p] || !c2[p]) { set_error("amp_resblock_forward: null conv handle"); return AMP_ERR_INVALID; }
    if (!rb_supported(v1, v2, B, T)) {
        set_error("amp_resblock_forward: block (C=%d k=%d, %d pairs, B=%d T=%d) is not covered by the whole-resblock kernel under the "
                  "current amp_set_resblock_fusion mode", c1[0]->cin, c1[0]->k, n_pairs, B, T);
        return AMP_ERR_UNSUPPORTED;
    }
    return rb_run(v1, v2, x_dev, B, T, slope, y_dev, 0, 1.f, (hipStream_t)stream);
}

int amp_set_resblock_fusion(int mode) {
    if (mode < -1 || mode > 3) { set_error("amp_set_resblock_fusion: mode=%d", mode); return AMP_ERR_INVALID; }
    cfg().rb_fusion = mode < 0 ? 1 : mode;
    return AMP_OK;
}

int amp_set_ampblock_fusion(int mode) {
    if (mode < -1 || mode > 3) { set_error("amp_set_ampblock_fusion: mode=%d", mode); return AMP_ERR_INVALID; }
    cfg().ampb_fusion = mode < 0 ? 1 : mode;
    return AMP_OK;
}

int amp_ampblock_forward(const amp_conv* const* c1, const amp_conv* const* c2, int n_pairs, const float* alpha_dev,
                         const float* beta_dev, int logscale, const float* filt_up_host, const float* filt_down_host,
                         const float* x_dev, int B, int T, float* y_dev, int mode, float div, void* stream) {
    if (!c1 || !c2 || !alpha_dev || !filt_up_host || !filt_down_host || !x_dev || !y_dev) { set_error("amp_ampblock_forward: null argument"); return AMP_ERR_INVALID; }
    if (B <= 0 || T <= 0 || n_pairs < 1 || 2 * n_pairs > AMP_AMPB_MAX_STEPS || mode < 0 || mode > 2) {
        set_error("amp_ampblock_forward: B=%d T=%d n_pairs=%d mode=%d", B, T, n_pairs, mode);
        return AMP_ERR_INVALID;
    }
    if (x_dev == y_dev) { set_error("amp_ampblock_forward: x and y must not alias (tiles read each other's halo)"); return AMP_ERR_INVALID; }
    for (int p = 0; p < n_pairs; ++p) if (!c1[p] || !c2[p]) { set_error("amp_ampblock_forward: null conv handle"); return AMP_ERR_INVALID; }
    const int C = c1[0]->cin, na = 2 * n_pairs;
    float* scratch[AMP_AMPB_MAX_STEPS] = {};
    ActParams acts[AMP_AMPB_MAX_STEPS];
    int rc = AMP_OK;
    for (int i = 0; i < na && rc == AMP_OK; ++i) {
        rc = act_params_upload(alpha_dev + (size_t)i * C, beta_dev ? beta_dev + (size_t)i * C : nullptr, C, logscale, filt_up_host, filt_down_host, &scratch[i]);
        if (rc == AMP_OK) { acts[i].a_dev = scratch[i]; acts[i].invb_dev = scratch[i] + C; acts[i].fu_dev = scratch[i] + 2 * C; acts[i].fd_dev = scratch[i] + 2 * C + 12; acts[i].fu2_dev = scratch[i] + 2 * C + 24; }
    }
    if (rc == AMP_OK && !ampb_supported(c1, c2, n_pairs, acts, (size_t)na, B, T)) {
        set_error("amp_ampblock_forward: block (C=%d k=%d, %d pairs, B=%d T=%d) is not covered by the whole-AMPBlock kernel under the "
                  "current amp_set_ampblock_fusion mode (run the convs and activations one by one: the same bits)", c1[0]->cin, c1[0]->k, n_pairs, B, T);
        rc = AMP_ERR_UNSUPPORTED;
    }
    if (rc == AMP_OK) rc = ampb_run(c1, c2, n_pairs, acts, x_dev, B, T, y_dev, mode, div, (hipStream_t)stream);
    hipError_t e = hipStreamSynchronize((hipStream_t)stream);
    for (int i = 0; i < na; ++i) if (scratch[i]) (void)hipFree(scratch[i]);
    if (rc == AMP_OK && e != hipSuccess) { set_error("amp_ampblock_forward: %s", hipGetErrorString(e)); return AMP_ERR_HIP; }
    return rc;
}

int amp_conv_forward_mrf(const amp_conv* c, const float* x_dev, int B, int T, float slope_in, const float* res_dev,
                         float* y_dev, int mode, float div, void* stream) {
    if (!c || !x_dev || !y_dev) { set_error("amp_conv_forward_mrf: null argument"); return AMP_ERR_INVALID; }
    if (x_dev == y_dev) { set_error("amp_conv_forward_mrf: x and y must not alias (the conv reads a halo)"); return AMP_ERR_INVALID; }
    if (mode < 0 || mode > 2 || (mode == 2 && !(div > 0.f))) { set_error("amp_conv_forward_mrf: mode=%d div=%g", mode, (double)div); return AMP_ERR_INVALID; }
    return conv_run(c, x_dev, B, T, slope_in, res_dev, 1.f, y_dev, mode, div, (hipStream_t)stream);
}

int amp_apnet_polar(const float* logamp_dev, const float* r_dev, const float* i_dev, size_t n, float* pha_dev,
                    float* rea_dev, float* imag_dev, void* stream) {
    if (!logamp_dev || !r_dev || !i_dev || !pha_dev || !rea_dev || !imag_dev || n == 0) { set_error("amp_apnet_polar: bad argument"); return AMP_ERR_INVALID; }
    AMP_HIP(launch_apnet_polar(logamp_dev, r_dev, i_dev, n, pha_dev, rea_dev, imag_dev, (hipStream_t)stream));
    return AMP_OK;
}

int amp_snake(const float* x_dev, int B, int C, int T, const float* alpha_dev, const float* beta_dev, int logscale,
              float* y_dev, void* stream) {
    if (!x_dev || !y_dev || !alpha_dev) { set_error("amp_snake: null argument"); return AMP_ERR_INVALID; }
    if (B <= 0 || C <= 0 || T <= 0) { set_error("amp_snake: B=%d C=%d T=%d", B, C, T); return AMP_ERR_INVALID; }
    AMP_HIP(launch_snake(x_dev, y_dev, B, C, T, alpha_dev, beta_dev, logscale, (hipStream_t)stream));
    return AMP_OK;
}

int amp_fir_upsample(const float* x_dev, int B, int C, int T, const float* filt_host, int K, int ratio, float* y_dev,
                     void* stream) {
    if (!x_dev || !y_dev || !filt_host) { set_error("amp_fir_upsample: null argument"); return AMP_ERR_INVALID; }
    if (B <= 0 || C <= 0 || T <= 0 || ratio < 1 || K < ratio) {
        set_error("amp_fir_upsample: B=%d C=%d T=%d K=%d ratio=%d", B, C, T, K, ratio);
        return AMP_ERR_INVALID;
    }
    if (K > AMP_FIR_MAX_TAPS) { set_error("amp_fir_upsample: %d taps (max %d)", K, AMP_FIR_MAX_TAPS); return AMP_ERR_UNSUPPORTED; }
    const int pad = K / ratio - 1;                                   // resample.py:24-28
    const int pad_left = pad * ratio + (K - ratio) / 2;
    AMP_HIP(launch_fir_up(x_dev, y_dev, B * C, T, filt_host, K, ratio, pad, pad_left, (hipStream_t)stream));
    return AMP_OK;
}

int amp_fir_filter(const float* x_dev, int B, int C, int T, const float* filt_host, int K, int stride, int pad_left,
                   int pad_right, int pad_mode, float* y_dev, void* stream) {
    if (!x_dev || !y_dev || !filt_host) { set_error("amp_fir_filter: null argument"); return AMP_ERR_INVALID; }
    if (B <= 0 || C <= 0 || T <= 0 || K < 1 || stride < 1 || pad_left < 0 || pad_right < 0) {
        set_error("amp_fir_filter: B=%d C=%d T=%d K=%d stride=%d pad=(%d,%d)", B, C, T, K, stride, pad_left, pad_right);
        return AMP_ERR_INVALID;
    }
    if (K > AMP_FIR_MAX_TAPS) { set_error("amp_fir_filter: %d taps (max %d)", K, AMP_FIR_MAX_TAPS); return AMP_ERR_UNSUPPORTED; }
    if (pad_mode < AMP_PAD_REPLICATE || pad_mode > AMP_PAD_REFLECT) { set_error("amp_fir_filter: unknown pad_mode %d", pad_mode); return AMP_ERR_INVALID; }
    if (pad_mode == AMP_PAD_REFLECT && (pad_left >= T || pad_right >= T)) {
        set_error("amp_fir_filter: reflection padding (%d, %d) needs more than that many input samples (T=%d)", pad_left, pad_right, T);
        return AMP_ERR_INVALID;
    }
    const int Tp = T + pad_left + pad_right;
    if (Tp < K) { set_error("amp_fir_filter: input too short (T=%d, padded %d, K=%d)", T, Tp, K); return AMP_ERR_INVALID; }
    const int Tout = (Tp - K) / stride + 1;
    AMP_HIP(launch_fir_filter(x_dev, y_dev, B * C, T, Tout, filt_host, K, stride, pad_left, pad_mode, (hipStream_t)stream));
    return AMP_OK;
}

int amp_wav_to_pcm16(const float* wav_dev, int B, int L, long long wav_stride, const int* lens_dev, int16_t* pcm_dev,
                     long long pcm_stride, void* stream) {
    if (!wav_dev || !pcm_dev) { set_error("amp_wav_to_pcm16: null argument"); return AMP_ERR_INVALID; }
    if (B <= 0 || L <= 0 || wav_stride < L || pcm_stride < L) {
        set_error("amp_wav_to_pcm16: B=%d L=%d wav_stride=%lld pcm_stride=%lld", B, L, wav_stride, pcm_stride);
        return AMP_ERR_INVALID;
    }
    if (B > 65535) { set_error("amp_wav_to_pcm16: B=%d exceeds 65535 rows per call", B); return AMP_ERR_UNSUPPORTED; }
    AMP_HIP(launch_pcm16(wav_dev, (short*)pcm_dev, B, L, wav_stride, pcm_stride, lens_dev, (hipStream_t)stream));
    return AMP_OK;
}

int amp_conv_set_option(amp_conv* c, int option, int value) {
    if (!c) { set_error("amp_conv_set_option: null handle"); return AMP_ERR_INVALID; }
    if (option == AMP_CONV_OPT_PAD_REFLECT) {
        if (value && c->transposed) { set_error("amp_conv_set_option: reflection padding on a transposed conv"); return AMP_ERR_UNSUPPORTED; }
        c->pad_reflect = value != 0;
    } else if (option == AMP_CONV_OPT_TANH) {
        // the polyphase scatter epilogues of a transposed conv apply leaky-ReLU only (conv_f16x3.hip)
        if (value && c->transposed) { set_error("amp_conv_set_option: tanh on a transposed conv"); return AMP_ERR_UNSUPPORTED; }
        c->tanh_out = value != 0;
    } else {
        set_error("amp_conv_set_option: unknown option %d", option);
        return AMP_ERR_INVALID;
    }
    return AMP_OK;
}

void amp_conv_destroy(amp_conv* c) { delete c; }

// ---- VITS posterior encoder / flow element-wise ops ----------------------------------------------
#define AMP_EW_CHECK(name, cond) do { if (!(cond)) { set_error(name ": bad argument"); return AMP_ERR_INVALID; } } while (0)

int amp_wn_gate(const float* a_dev, const float* cond_dev, long long cond_batch_stride, float* out_dev, int B, int H,
                int T, void* stream) {
    AMP_EW_CHECK("amp_wn_gate", a_dev && out_dev && B > 0 && H > 0 && T > 0);
    AMP_HIP(launch_wn_gate(a_dev, cond_dev, cond_batch_stride, out_dev, B, H, T, (hipStream_t)stream));
    return AMP_OK;
}

int amp_wn_accumulate(float* x_dev, float* out_dev, const float* rs_dev, const int32_t* lens_dev, int B, int H, int T,
                      int first, int last, void* stream) {
    AMP_EW_CHECK("amp_wn_accumulate", x_dev && out_dev && rs_dev && B > 0 && H > 0 && T > 0);
    AMP_HIP(launch_wn_accumulate(x_dev, out_dev, rs_dev, lens_dev, B, H, T, last, first, (hipStream_t)stream));
    return AMP_OK;
}

int amp_sequence_mask(float* x_dev, const int32_t* lens_dev, int B, int C, int T, void* stream) {
    AMP_EW_CHECK("amp_sequence_mask", x_dev && lens_dev && B > 0 && C > 0 && T > 0);
    AMP_HIP(launch_mask(x_dev, lens_dev, B, C, T, (hipStream_t)stream));
    return AMP_OK;
}

int amp_coupling_apply(float* x_dev, const float* m_dev, const int32_t* lens_dev, int B, int half_channels, int T,
                       int reverse, void* stream) {
    AMP_EW_CHECK("amp_coupling_apply", x_dev && m_dev && B > 0 && half_channels > 0 && T > 0);
    AMP_HIP(launch_coupling(x_dev, m_dev, lens_dev, B, half_channels, T, reverse, (hipStream_t)stream));
    return AMP_OK;
}

int amp_flip_channels(const float* x_dev, float* y_dev, int B, int C, int T, void* stream) {
    AMP_EW_CHECK("amp_flip_channels", x_dev && y_dev && x_dev != y_dev && B > 0 && C > 0 && T > 0);
    AMP_HIP(launch_flip_channels(x_dev, y_dev, B, C, T, (hipStream_t)stream));
    return AMP_OK;
}

int amp_posterior_sample(const float* stats_dev, const float* eps_dev, const int32_t* lens_dev, float* z_dev, int B,
                         int C, int T, void* stream) {
    AMP_EW_CHECK("amp_posterior_sample", stats_dev && eps_dev && z_dev && B > 0 && C > 0 && T > 0);
    AMP_HIP(launch_posterior_sample(stats_dev, eps_dev, lens_dev, z_dev, B, C, T, (hipStream_t)stream));
    return AMP_OK;
}

int amp_antialias_snake(const float* x_dev, int B, int C, int T, const float* alpha_dev, const float* beta_dev,
                        int logscale, const float* filt_up_host, const float* filt_down_host, float* y_dev,
                        void* stream) {
    if (!x_dev || !y_dev || !alpha_dev || !filt_up_host || !filt_down_host) { set_error("amp_antialias_snake: null argument"); return AMP_ERR_INVALID; }
    if (B <= 0 || C <= 0 || T <= 0) { set_error("amp_antialias_snake: B=%d C=%d T=%d", B, C, T); return AMP_ERR_INVALID; }
    // op-level convenience path (tests): derive a / 1/(b+eps) on the host, synchronously.
    float* scratch = nullptr;
    const int rc = act_params_upload(alpha_dev, beta_dev, C, logscale, filt_up_host, filt_down_host, &scratch);
    if (rc != AMP_OK) return rc;
    hipError_t e = hipSuccess;
    if (e == hipSuccess) e = launch_act1d(x_dev, y_dev, B, C, T, scratch, scratch + C, scratch + 2 * C, scratch + 2 * C + 12, nullptr, 1, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    (void)hipFree(scratch);
    if (e != hipSuccess) { set_error("amp_antialias_snake: %s", hipGetErrorString(e)); return AMP_ERR_HIP; }
    return AMP_OK;
}

}  // extern "C"
