// amp_conv and everything built from it: per-tap-count kernel dispatch, the measured launch policies, MFMA-fragment packing (conv_build),
// conv_run and the fused forms (pair, whole ResBlock1, whole AMPBlock1), and the op-level extern "C" entry points that wrap them.
#include <string.h>

#include <memory>
#include <type_traits>
#include <vector>

#include "amp_host.h"

namespace amp {

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
//
// Fitted strips (PairArgs::fit): a strip of S steps keeps all S * n1 columns it computes and pays a halo prologue of kFitPrologueSteps
// instead of the k - 1 discarded columns (0.04 of a step).  That only pays where it saves a whole round of workgroups: at B = 64,
// T = 16 384 an item is exactly 64 steps, the shifted strips cut it into 16 x 4 + 1 steps (1 088 workgroups, 4 160 steps: a 17th round of
// steps on a quarter of the CUs), the fitted ones into 64 (4 096 steps: 16 rounds).  Both forms go through ONE cost model, rounds of
// workgroups x (steps per strip [+ the prologue]) + the quarter-step fill per workgroup; the shifted form at today's step count, the
// fitted form at four and eight steps per strip, and only where the shifted plan already walks four-step strips (the same "fills the chip
// four times over" guard) and 512+ fitted strips remain (pair_run hands smaller grids to the per-tile kernel).  A tie keeps the shifted
// form.  amp_set_strip_fit: -1 this plan, 0 never, 1 every strip launch (the shifted plan's step count, fitted; ragged batches too).
// Same bits either way (tests/test_gpu_pair_strip_fit.py).
constexpr double kFitPrologueSteps = 0.2;    // m, in steps: measured 0.17 - 0.19 with four-step strips, 0.22 - 0.23 derived from eight-step ones (profiles/r7_strip_fit.txt)
static void strip_geometry(int B, int T, int n1, int hb, int wg_per_cu, int steps, bool ragged, int* strip_len, int* spi, int* fit) {
    *fit = 0;
    strip_plan(B, T, n1, hb, wg_per_cu, strip_len, spi);
    if (steps > 0 && steps * n1 - hb < T) { *strip_len = steps * n1 - hb; *spi = (T + *strip_len - 1) / *strip_len; }
    bool four = false;
    if (steps == 1 && !ragged && 4 * n1 - hb < T) {
        const int len4 = 4 * n1 - hb, spi4 = (T + len4 - 1) / len4;
        if ((long long)B * spi4 >= 1024) { *strip_len = len4; *spi = spi4; four = true; }
    }
    const int mode = cfg().strip_fit;
    if (mode == 0) return;
    if (mode == 1) {
        const int st = (*strip_len + hb + n1 - 1) / n1;
        *strip_len = st * n1; *spi = (T + *strip_len - 1) / *strip_len; *fit = 1;
        return;
    }
    if (!four) return;
    const long long slots = (long long)wg_per_cu * 256;
    auto rounds = [&](int nspi) { return ((long long)B * nspi + slots - 1) / slots; };
    auto cost = [&](int nspi, double steps_per_strip) { return (double)rounds(nspi) * (4.0 * steps_per_strip + 1.0); };
    double best = cost(*spi, 4.0);
    const long long shifted_rounds = rounds(*spi) * 4;
    for (int S : {4, 8}) {
        const int len = S * n1, nspi = (T + len - 1) / len;
        if (len > T || (long long)B * nspi < 512) continue;
        if (rounds(nspi) * S >= shifted_rounds) continue;      // no whole round of steps saved: the model's fill term alone (one fill per eight steps) is not a measured gain
        const double c = cost(nspi, S + kFitPrologueSteps);
        if (c < best) { best = c; *strip_len = len; *spi = nspi; *fit = 1; }
    }
}

// The plan alone, for tests and tools: the strips a fused C = 128 pair of kernel k would be cut into at (B, T) under the current switches.
// form: 0 shifted, 1 fitted; steps = steps per full strip; false when (k) has no strip kernel.
bool pair_strip_plan(int B, int T, int k, bool ragged, int* form, int* strip_len, int* spi, int* steps) {
    int wg = 2;
    const StripChoice sc = strip_choice(128, k);
    const int n1 = sc.use ? strip_step(k, 128, 1, sc.wide, &wg) : 0;
    if (n1 <= 0) return false;
    strip_geometry(B, T, n1, k - 1, wg, sc.steps, ragged, strip_len, spi, form);
    *steps = (*strip_len + (*form ? 0 : k - 1) + n1 - 1) / n1;
    return true;
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
static bool conv_rg_fast() { return cfg().conv_rg_fast != 0; }
// Ping-pong tile order: every other conv / pair launch walks its tiles from the last item's end backwards, so that it starts
// on the part of its input the previous launch wrote last (still in the Infinity Cache).  amp_set_pingpong.
// Measured (profiles/r2_am_pingpong.txt, one box, alternating runs): config 2 30.99 -> 30.87 ms, the gain in the HBM-leaning
// stages (C = 64: 7.20 -> 7.15 ms, C = 32: 4.40 -> 4.32 ms); C3 / C5 unchanged.
static thread_local unsigned g_launch_parity = 0;
int next_rev(const int* lens) {
    if (!cfg().pingpong || lens) return 0;   // ragged batches keep the dispatch order
    return (int)(g_launch_parity++ & 1u);
}
// the blocked launch fills the chip only when its (half as many) workgroups still give every CU its two
constexpr long long kConvBlkMinWorkgroups = 512;

int conv_build(amp_conv* c, const float* w, const float* bias) {
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
    } else if (c->stride == 1) {
        // ConvTranspose1d(stride 1, padding p) IS the Conv1d with flipped taps and padding k - 1 - p (wview below): no polyphase rows, and
        // the kernels' up == 1 store paths (which write column q unshifted) are right for it.  c->transposed stays set: out_len, the
        // option / ragged refusals and the manifest label follow the handle.
        if (c->dilation != 1) { set_error("amp_conv: dilated ConvTranspose1d unsupported (dilation=%d)", c->dilation); return AMP_ERR_UNSUPPORTED; }
        c->up = 1; c->up_pad = 0;
        c->M = c->cout;
        c->ntaps = c->k;
        c->off0 = -(c->k - 1 - c->padding);
        c->dstep = 1;
    } else {
        if (c->dilation != 1) { set_error("amp_conv: dilated ConvTranspose1d unsupported (dilation=%d)", c->dilation); return AMP_ERR_UNSUPPORTED; }
        c->up = c->stride; c->up_pad = c->padding;
        c->M = c->cout * c->stride;
        c->ntaps = (c->k + c->stride - 1) / c->stride;
        c->off0 = 0;
        c->dstep = -1;             // tap s reads x[q - s]
    }
    c->KT = round_up_taps(c->ntaps);
    if (c->KT < 0) { set_error("amp_conv: k=%d at stride=%d is %d taps, unsupported (max 11)", c->k, c->stride, c->ntaps); return AMP_ERR_UNSUPPORTED; }
    const int omin = c->dstep >= 0 ? c->off0 : c->off0 + (c->KT - 1) * c->dstep;
    const int omax = c->dstep >= 0 ? c->off0 + (c->KT - 1) * c->dstep : c->off0;
    c->halo_left = omin < 0 ? -omin : 0;
    c->halo_right = omax > 0 ? omax : 0;
    if (!choose_plan(c->KT, c->M, c->halo_left + c->halo_right, 0, &c->plan)) {
        set_error("amp_conv: receptive field (k=%d, dilation=%d, padding=%d: %d columns) exceeds the 128-column staged halo", c->k, c->dilation,
                  c->padding, c->halo_left + c->halo_right);
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
        if (up == 1) return w[((size_t)i * cout + m) * k + (k - 1 - g)];   // stride 1: the flipped taps of the equivalent Conv1d
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
        AMP_RC(device_upload(wp.data(), n * sizeof(float), &c->wp_dev));
    } else {
        // ---- f16x3: A fragments per 16-channel chunk and tap, scaled by a power of two (amp_host.h: pack_a_f16x3) ----
        c->nchunks = (c->cin + KC16 - 1) / KC16;
        float wmax = 0.f;
        const size_t nw = (size_t)cin * cout * k;
        for (size_t i = 0; i < nw; ++i) wmax = fmaxf(wmax, fabsf(w[i]));
        if (!(wmax < 1e30f)) { set_error("amp_conv: non-finite weight"); return AMP_ERR_INVALID; }
        c->wscale = pow2_weight_scale(wmax);
        // + 2 chunks of pad: the kernels' A reload runs one chunk (conv_blk_f16x3.hip: one round of up to 2 chunks) ahead
        const std::vector<_Float16> wp = pack_a_f16x3(nmb, c->nchunks, c->KT, (size_t)2 * c->KT * 2, c->wscale, wview);
        AMP_RC(device_upload(wp.data(), wp.size() * sizeof(_Float16), &c->wp_dev));
    }
    if (bias) AMP_RC(device_upload(bias, (size_t)cout * sizeof(float), (void**)&c->bias_dev));
    return AMP_OK;
}

// bytes of the packed f16x3 A fragments of all row blocks (hi + lo planes)
static size_t conv_weight_bytes(const amp_conv* c) { return (size_t)c->Mpad * c->nchunks * KC16 * c->KT * 4; }

static int conv_out_len(const amp_conv* c, int T) {
    if (!c->transposed) return T + 2 * c->padding - c->dilation * (c->k - 1);
    return (T - 1) * c->stride - 2 * c->padding + c->k + c->out_pad;
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

int conv_run(const amp_conv* c, const float* x, int B, int T, float slope_in, const float* res, float slope_out,
             float* y, int mode, float div, hipStream_t stream, long long xbs, const int* lens, int len_mul,
             ConvArgs* plan_small, int* plan_ni) {
    if (B <= 0 || T <= 0) { set_error("amp_conv_forward: B=%d T=%d", B, T); return AMP_ERR_INVALID; }
    const int Tout = conv_out_len(c, T);
    if (Tout <= 0) { set_error("amp_conv_forward: input too short (T=%d gives T_out=%d)", T, Tout); return AMP_ERR_INVALID; }
    ConvArgs a{};
    a.x = x; a.wp = c->wp_dev; a.bias = c->bias_dev; a.res = res; a.y = y;
    a.B = B; a.Cin = c->cin; a.Tin = T; a.xbs = xbs > 0 ? xbs : (long long)c->cin * T; a.nchunks = c->nchunks; a.M = c->M;
    a.Tq = c->up > 1 ? T + c->ntaps - 1 : Tout;   // polyphase: every input column and the taps' tail; else one GEMM column per output
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
    tl_conv_transposed = c->transposed;           // the manifest label of the launch below (amp_internal.h: note_conv_work)
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
bool pair_supported(const amp_conv* c1, const amp_conv* c2) {
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

int pair_run(const amp_conv* c1, const amp_conv* c2, const float* x, int B, int T, float slope, float* y,
                    int mode, float div, hipStream_t stream, const int* lens, int len_mul) {
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
        strip_geometry(B, T, n1, c1->k - 1, wg, sc.steps, lens != nullptr, &a.strip_len, &a.strips_per_item, &a.fit);
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
bool pair_tile_args(const amp_conv* c1, const amp_conv* c2, const float* x, int B, int T, float slope, float* y, int mode,
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
        int strip_len = 0, strips_per_item = 0, fit = 0;
        strip_geometry(B, T, n1, c1->k - 1, wg, sc.steps, lens != nullptr, &strip_len, &strips_per_item, &fit);
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
int rb_form_of(int C, int k) { return rb_form(C, k); }
constexpr long long kRbMinWorkgroups = 256;
// a tile's trip through HBM in units of one conv of its form, times C * k (rb_plan): fitted per form from the forced plans of
// profiles/r8_rb_guards.txt, 160 - 295 (C = 64 k = 11: 253; k = 7: 196 - 294; C = 32 k = 11: 218 - 240; k = 7: 162 - 286; C = 64 k = 3: 206)
constexpr double kRbTripMacs = 235.0;

// guard columns either side of the LDS tile of form `form` (the RB_G of launch_rb's instantiations, rb_f16x3.hip)
static int rb_guard_columns(int C, int form) { return (C == 128 || (C == 64 && form == 0)) ? 16 : 32; }

// RbArgs::gx, real x in the guard columns for the launch's first conv: amp_set_rb_guards / AMP_RB_GUARDS -1 this policy, 0 never, 1 wherever
// the first conv's reach fits the guard.  Same bits either way (tests/test_gpu_rb_guards.py).
// policy (profiles/r8_rb_guards.txt: op level at B = 64, the benchmark's T, forms alternating in one process, ms per resblock, three rounds):
//   C = 64 k = 11 (pairs 0-1 + pair 2) 3.256 - 3.272 -> 3.092 - 3.116 (19 + 19 -> 18 + 17 rounds of workgroups)
//   C = 64 k = 7  whole 2.174 - 2.177 -> whole with guards 2.171 - 2.175 (still 19 rounds) -> pairs 0-1 + pair 2 2.135 - 2.137 (17 + 17)
//   C = 32 k = 11 (eight waves) 1.786 - 1.803 -> 1.730 - 1.746 (19 -> 18 rounds)
//   C = 32 k = 7  (four waves) 1.219 - 1.225 -> 1.217 - 1.219: inside the range, every split 5 - 15 % slower -- off
//   k = 3: no round to save (RH 12 -> 11) and the staged guards are paid: C = 64 1.071 - 1.073 -> 1.079 - 1.081, C = 32 0.687 - 0.689 ->
//   0.700 - 0.702 -- off.  k = 5 not measured: off.
static bool rb_guards_wanted(int C, int k) {
    const int m = cfg().rb_guards;
    if (m >= 0) return m != 0;
    return k >= 11 || (C == 64 && k >= 7);
}

// THE geometry of one launch of pairs [first, first + count) of a resblock (C channels, kernel k, dilations dil[]) in kernel form `form`:
// rb_supported, rb_plan and rb_run take their numbers from here.  Every conv is evaluated on all W columns of the tile and a tile loses
// rh0 = sum_p (k-1)/2 * (dil[p] + 1) columns either side -- less the first conv's reach (k-1)/2 * dil[first] where the guards hold real x
// (gx): that conv's inputs left and right of the tile are then there.  A reach wider than the guard keeps rh0 and zero guards.
RbGeom rb_geometry(int C, int k, const int* dil, int first, int count, int T, int form) {
    RbGeom g{};
    int max_dil = 1;
    for (int p = first; p < first + count; ++p) {
        max_dil = dil[p] > max_dil ? dil[p] : max_dil;
        g.rh0 += (k - 1) / 2 * (dil[p] + 1);
    }
    g.W = form < 0 ? 0 : rb_tile(k, C, max_dil, form);
    g.rh = g.rh0;
    const int reach = (k - 1) / 2 * dil[first];
    if (g.W > 0 && rb_guards_wanted(C, k) && reach <= rb_guard_columns(C, form)) { g.gx = 1; g.rh -= reach; }
    g.NT = g.W - 2 * g.rh;
    g.NT0 = g.W - 2 * g.rh0;
    if (g.W > 0 && g.NT > 0) g.tiles = (T + g.NT - 1) / g.NT;
    if (g.W > 0 && g.NT0 > 0) g.tiles0 = (T + g.NT0 - 1) / g.NT0;
    return g;
}
static RbGeom rb_geometry(const amp_conv* const* c1, int first, int count, int T) {
    int dil[AMP_RB_MAX_PAIRS] = {1, 1, 1};
    for (int p = first; p < first + count && p < AMP_RB_MAX_PAIRS; ++p) dil[p] = c1[p]->dilation;
    return rb_geometry(c1[0]->cin, c1[0]->k, dil, first, count, T, rb_form(c1[0]->cin, c1[0]->k));
}

// What the kernel covers and the grid floor are judged on the zero-guard geometry (NT0): the guards change how many tiles a launch has, not
// which shapes run on it.
bool rb_supported(const amp_conv* const* c1, const amp_conv* const* c2, int np, int B, int T) {
    if (np < 1 || np > AMP_RB_MAX_PAIRS) return false;
    for (int p = 0; p < np; ++p) {
        if (!c1[p] || !c2[p] || !pair_supported(c1[p], c2[p])) return false;
        if (c1[p]->cin != c1[0]->cin || c1[p]->k != c1[0]->k) return false;
    }
    const RbGeom g = rb_geometry(c1, 0, np, T);
    if (g.W <= 0 || g.NT0 < g.W / 2) return false;          // at least half of every tile must be output
    if (rb_fusion_mode() == 1 && (long long)B * g.tiles0 < kRbMinWorkgroups) return false;
    return true;
}

// Round 5: a resblock whose tile keeps less than 80 % of its columns (every conv is evaluated on all W columns and 2 * RH are discarded:
// C = 64, k = 11 keeps 392 of 512) runs as TWO launches, pairs [0, 2) and [2, 3): 452 of 512 columns kept in each, 13 % fewer MFMAs for one
// more trip of x through HBM.  Under the package power cap removed MFMAs convert to time in full: B = 64 3.45 -> 3.19 ms,
// B = 32 1.68 -> 1.58, B = 16 0.89 -> 0.78; B = 8 (672 workgroups) 0.431 -> 0.443, hence the 1 024-workgroup floor; k = 7 (86 % kept) and
// C = 32 k = 11 (88 %) are 1-4 % slower split (profiles/r5_l_rb_split.txt).  Same bits: what leaves a launch is the fp32 x the next pair
// would have read from registers.
//
// Round 8: the split is a PLAN, pairs per launch, chosen by one cost model in the manner of strip_geometry(): a launch of n convs takes
// ceil(workgroups / slots) rounds of workgroups, and a round costs its n convs plus the trip of the tile through HBM, which in units of one
// conv of the form is kRbTripConvs(C, k) = kRbTripMacs / (C * k) (a conv's time goes with C * C * k * W per tile, the trip's with C * W):
//     cost = sum over launches of rounds * (convs + kRbTripMacs / (C * k))
// With real x in the guards every launch sheds its own first conv's reach, so cutting before a wide conv buys columns: C = 64, k = 7 now
// runs as {2, 1} (17 + 17 rounds instead of 19), C = 64, k = 11 stays {2, 1} ({1, 1, 1} measured 1.5 % slower, as the model has it).
// Candidates: {3}, {2, 1}, {1, 2} and, with 2 048+ workgroups, {1, 1, 1}; never fewer launches than the round-5 rule above gives (that rule
// was measured on MFMA counts down to 1 024 workgroups, where whole rounds say little); a tie keeps the round-5 plan; ragged batches and
// launches under 1 024 workgroups keep it too.  amp_set_rb_split_plan / AMP_RB_SPLIT_PLAN force a plan in every fusion mode.
RbPlan rb_plan(int C, int k, const int* dil, int np, int B, int T, bool ragged) {
    RbPlan best{1, {np, 0, 0}};
    if (np != 3) return best;
    const int* f = cfg().rb_plan;
    if (f[0] > 0) {
        RbPlan forced{0, {0, 0, 0}};
        for (int i = 0; i < 3 && f[i] > 0; ++i) forced.count[forced.n++] = f[i];
        return forced;
    }
    if (rb_fusion_mode() != 1) return best;
    const int form = rb_form(C, k);
    const RbGeom whole = rb_geometry(C, k, dil, 0, np, T, form);
    if (whole.W <= 0 || whole.NT0 <= 0) return best;
    const long long wg0 = (long long)B * whole.tiles0;
    if (wg0 < 1024) return best;
    if (5 * whole.NT0 < 4 * whole.W) best = RbPlan{2, {2, 1, 0}};
    if (ragged || !rb_guards_wanted(C, k)) return best;     // zero guards: the round-5 rule as it was measured
    const long long slots = 256 * (form == 0 ? 2 : 1);
    const double trip = kRbTripMacs / ((double)C * k);
    auto cost = [&](const RbPlan& pl) {
        double c = 0.0;
        for (int l = 0, first = 0; l < pl.n; first += pl.count[l++]) {
            const RbGeom g = rb_geometry(C, k, dil, first, pl.count[l], T, form);
            if (g.W <= 0 || g.NT <= 0) return -1.0;
            c += (double)(((long long)B * g.tiles + slots - 1) / slots) * (2.0 * pl.count[l] + trip);
        }
        return c;
    };
    double best_cost = cost(best);
    const RbPlan cands[] = {{1, {3, 0, 0}}, {2, {2, 1, 0}}, {2, {1, 2, 0}}, {3, {1, 1, 1}}};
    const int min_launches = best.n;
    for (const RbPlan& pl : cands) {
        if (pl.n < min_launches || (pl.n == 3 && wg0 < 2048)) continue;
        const double c = cost(pl);
        if (c >= 0.0 && (best_cost < 0.0 || c < best_cost)) { best_cost = c; best = pl; }
    }
    return best;
}
RbPlan rb_plan(const amp_conv* const* c1, int np, int B, int T, bool ragged) {
    int dil[AMP_RB_MAX_PAIRS] = {1, 1, 1};
    for (int p = 0; p < np && p < AMP_RB_MAX_PAIRS; ++p) dil[p] = c1[p]->dilation;
    return rb_plan(c1[0]->cin, c1[0]->k, dil, np, B, T, ragged);
}

int rb_run(const amp_conv* const* c1, const amp_conv* const* c2, int np, const float* x, int B, int T, float slope, float* y, int mode,
           float div, hipStream_t stream, const int* lens, int len_mul, int first, int count) {
    if (x == y) { set_error("rb_run: x and y must not alias"); return AMP_ERR_INVALID; }
    if (slope > 1.f) { set_error("rb_run: leaky_relu slope %g > 1 is outside the fused kernels", (double)slope); return AMP_ERR_UNSUPPORTED; }
    RbArgs a{};
    a.x = x; a.y = y;
    a.np = count < 0 ? np - first : count;
    const RbGeom g = rb_geometry(c1, first, a.np, T);
    if (g.W <= 0 || g.NT <= 0) { set_error("rb_run: pairs [%d, %d) have no whole-resblock tile", first, first + a.np); return AMP_ERR_UNSUPPORTED; }
    c1 += first;
    c2 += first;
    for (int p = 0; p < a.np; ++p) {
        a.wp1[p] = c1[p]->wp_dev; a.bias1[p] = c1[p]->bias_dev; a.wp2[p] = c2[p]->wp_dev; a.bias2[p] = c2[p]->bias_dev;
        a.sc1[p] = 16.f * c1[p]->wscale; a.isc1[p] = 1.f / a.sc1[p];
        a.sc2[p] = 16.f * c2[p]->wscale; a.isc2[p] = 1.f / a.sc2[p];
        a.dil[p] = c1[p]->dilation;
    }
    for (int p = a.np; p < AMP_RB_MAX_PAIRS; ++p) {   // never dereferenced; keep the pointers valid all the same
        a.wp1[p] = a.wp1[0]; a.bias1[p] = a.bias1[0]; a.wp2[p] = a.wp2[0]; a.bias2[p] = a.bias2[0]; a.dil[p] = 1;
    }
    a.B = B; a.C = c1[0]->cin; a.T = T;
    a.rh = g.rh; a.gx = g.gx;
    a.tiles_per_item = g.tiles;
    a.slope = slope; a.mode = mode; a.div = div;
    a.lens = lens; a.len_mul = len_mul;
    a.range_flag = range_flag_for_current_device();
    a.rev = next_rev(lens);
    AMP_HIP(launch_rb(c1[0]->k, a, rb_form(a.C, c1[0]->k), stream));
    return AMP_OK;
}

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

bool ampb_supported(const amp_conv* const* c1, const amp_conv* const* c2, int np, const ActParams* acts, size_t nacts, int B, int T) {
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

int ampb_run(const amp_conv* const* c1, const amp_conv* const* c2, int np, const ActParams* acts, const float* x, int B, int T,
                    float* y, int mode, float div, hipStream_t stream, const int* lens, int len_mul) {
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

// amp_host.h
int act_params_upload(const float* alpha_dev, const float* beta_dev, int C, int logscale, const float* filt_up_host,
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

}  // namespace amp

using namespace amp;

extern "C" {

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
    for (int p = 0; p < n_pairs; ++p) if (!c1[p] || !c2[p]) { set_error("amp_resblock_forward: null conv handle"); return AMP_ERR_INVALID; }
    if (!rb_supported(c1, c2, n_pairs, B, T)) {
        set_error("amp_resblock_forward: block (C=%d k=%d, %d pairs, B=%d T=%d) is not covered by the whole-resblock kernel under the "
                  "current amp_set_resblock_fusion mode", c1[0]->cin, c1[0]->k, n_pairs, B, T);
        return AMP_ERR_UNSUPPORTED;
    }
    return rb_run(c1, c2, n_pairs, x_dev, B, T, slope, y_dev, 0, 1.f, (hipStream_t)stream);
}

int amp_resblock_forward_ex(const amp_conv* const* c1, const amp_conv* const* c2, int n_pairs, const float* x_dev, int B, int T, float slope,
                            float* y_dev, int mode, float div, float* tmp_dev, void* stream) {
    if (!c1 || !c2 || !x_dev || !y_dev) { set_error("amp_resblock_forward_ex: null argument"); return AMP_ERR_INVALID; }
    if (B <= 0 || T <= 0 || n_pairs < 1 || n_pairs > AMP_RB_MAX_PAIRS || mode < 0 || mode > 2) {
        set_error("amp_resblock_forward_ex: B=%d T=%d n_pairs=%d mode=%d", B, T, n_pairs, mode);
        return AMP_ERR_INVALID;
    }
    for (int p = 0; p < n_pairs; ++p) if (!c1[p] || !c2[p]) { set_error("amp_resblock_forward_ex: null conv handle"); return AMP_ERR_INVALID; }
    if (!rb_supported(c1, c2, n_pairs, B, T)) {
        set_error("amp_resblock_forward_ex: block (C=%d k=%d, %d pairs, B=%d T=%d) is not covered by the whole-resblock kernel under the "
                  "current amp_set_resblock_fusion mode", c1[0]->cin, c1[0]->k, n_pairs, B, T);
        return AMP_ERR_UNSUPPORTED;
    }
    const RbPlan pl = rb_plan(c1, n_pairs, B, T, false);
    if (pl.n > 1 && !tmp_dev) { set_error("amp_resblock_forward_ex: a plan of %d launches needs tmp_dev", pl.n); return AMP_ERR_INVALID; }
    const size_t be = (size_t)B * c1[0]->cin * T;
    const float* cur = x_dev;
    int first = 0;
    for (int l = 0; l + 1 < pl.n; first += pl.count[l++]) {
        float* dst = cur == tmp_dev ? tmp_dev + be : tmp_dev;
        AMP_RC(rb_run(c1, c2, n_pairs, cur, B, T, slope, dst, 0, 1.f, (hipStream_t)stream, nullptr, 1, first, pl.count[l]));
        cur = dst;
    }
    return rb_run(c1, c2, n_pairs, cur, B, T, slope, y_dev, mode, div, (hipStream_t)stream, nullptr, 1, first, -1);
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

}  // extern "C"
