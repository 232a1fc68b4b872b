// Internal declarations shared by the translation units of libamphion_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <atomic>
#include <mutex>
#include <string>
#include <vector>

#include "amphion_hip.h"

namespace amp {

constexpr int KC = 8;     // f32 kernel: input channels staged per K-chunk (2 per MFMA k-step, 4 k-steps per tap)
constexpr int KC16 = 16;  // f16x3 kernel: input channels per K-chunk (one 32x32x16 MFMA k-extent per tap)

// Arithmetic of the conv contraction (amp_set_precision / AMP_PRECISION).
enum { PREC_F32 = 0, PREC_F16X3 = 1 };

// Arguments of the implicit-GEMM conv kernel (conv_mfma.hip).
//   Y'[m, q] = sum_i sum_j  W'[m, i, j] * act_in(X[i, q + off0 + j*dstep])          (zero outside [0, Tin))
// For a Conv1d:          m = output channel, off_j = (j - (k-1)/2) * dilation, up = 1.
// For a ConvTranspose1d: m = o*up + r  (polyphase row), taps s: X[i, q - s], W' = W[i, o, r + s*up];
//                        the result is scattered to n = q*up + r - up_pad.
struct ConvArgs {
    const float* x;      // [B, Cin, Tin]
    const void* wp;      // packed A fragments (f32, or f16 hi/lo planes for f16x3), see conv_build() in conv_host.hip
    const float* bias;   // [Cout] or nullptr
    const float* res;    // [B, Cout, Tout] or nullptr (may alias y)
    float* y;            // [B, Cout, Tout]
    int B, Cin, Tin;
    long long xbs;       // batch stride of x in elements (Cin*Tin when dense; larger for a channel slice)
    int nchunks;         // ceil(Cin / KC)
    int M;               // GEMM rows = Cout * up
    int Tq;              // GEMM columns per batch item
    int tiles_per_item;  // ceil(Tq / NT)
    int rev;             // 1: walk the tiles in descending order.  Successive launches alternate (conv_run / pair_run): a launch's
                         //    input is mostly the previous launch's output, whose LAST-written part is what the 256-MB Infinity
                         //    Cache still holds when the next launch starts
    int row_groups;      // > 0: 1-D grid of B * tiles_per_item * row_groups workgroups with the row group as the FASTEST index
                         //      (the row groups of one x tile run back to back on one XCD: x is fetched into ONE L2 once
                         //      instead of once per row group from HBM); 0: 2-D grid, row group = blockIdx.y
    int off0, dstep;     // tap offsets
    int halo_left;       // max(0, -min_j off_j)
    int wd;              // staged columns actually needed: NT + halo_left + halo_right
    int Cout, Tout;
    int up, up_pad;
    float slope_in, slope_out;  // 1.0f = identity
    int mode;                   // 0: y = v   1: y = y + v   2: y = (y + v) / div
    float div;
    float acc_scale, inv_scale; // f16x3 only: 16 * 2^s (operand scaling) and its reciprocal
    // ragged batches: item b's input is valid on [0, lens[b] * len_mul) and reads as zero beyond (every
    // layer zero-pads at the utterance's OWN end, so a padded batch equals the per-utterance results)
    const int* lens;            // [B] on the device, or nullptr (all items valid on [0, Tin))
    int len_mul;
    unsigned* range_flag;       // f16x3: set to 1 when a staged operand leaves the f16 range (|x| * 16 > 65504) or is not finite
    int pad_reflect;            // 1: out-of-range columns mirror (nn.ReflectionPad1d + unpadded conv, melgan.py:39,56,92)
    int tanh_out;               // 1: tanh on store (melgan.py:94)
    // ---- conv_small_f16x3.hip only (frame-rate convs; the other kernels ignore these) ----
    int Mpad;                   // rows of the packed weight (M rounded up to the pack's row group)
    const float* gate_cond;     // EPI_GATE: additive condition per (item, ORIGINAL row) or nullptr (WN's g_l, modules.py:135-139)
    long long gate_cond_bs;     //           its batch stride in elements
    int wn_H;                   // EPI_GATE / EPI_WNACC: hidden channels H
    float* wn_x;                // EPI_WNACC: x [B, H, T], updated in place: x = (x + rs[:H]) * mask
    float* wn_out;              //            output [B, H, T]: (+)= rs[H:] (last layer: (+)= rs)
    int wn_first, wn_last;      //            first layer starts `output` from zero; last layer has H rows only
};

// Arguments of the fused ResBlock-pair kernel (pair_f16x3.hip):
//   y = x + c2(lrelu(c1(lrelu(x))))   [mode 1: y += ..., mode 2: y = (y + ...) / div]
struct PairArgs {
    const float* x;            // [B, C, T] input and residual
    float* y;                  // [B, C, T] output; must NOT alias x (other tiles read x's halo)
    const void* wp1;           // conv1 (kernel k, dilation dil): packed f16x3 A fragments
    const float* bias1;
    const void* wp2;           // conv2 (kernel k, dilation 1)
    const float* bias2;
    int B, C, T;
    int tiles_per_item;        // per-tile kernel (pair_f16x3.hip): ceil(T / NT)
    int strip_len;             // strip kernel (pair_strip_f16x3.hip): output columns per workgroup ...
    int strips_per_item;       // ... and workgroups per batch item, ceil(T / strip_len)
    int wide;                  // strip kernel: 0 = four-wave strips, 3 = the 2 x 2-blocked A-ring form (one workgroup per CU)
    int fit;                   // strip kernel: 1 = fitted strips (outputs start at the strip's first column, a halo prologue computes the k - 1
                               // carried xt columns), 0 = shifted strips (a strip starts k - 1 columns early and discards them)
    int rev;                   // 1: descending tile / strip order, see ConvArgs::rev
    int dil;
    float slope;               // leaky_relu slope (on x while staging, on conv1's output at the seam)
    float sc1, isc1, sc2, isc2;  // 16 * 2^s operand scaling of each conv and its reciprocal
    int mode;
    float div;
    const int* lens;           // ragged batches, see ConvArgs
    int len_mul;
    unsigned* range_flag;      // see ConvArgs
};

// Three whole-K convs in one grid (conv_small3_f16x3.hip): a[0] / a[1] / a[2] = the k = 11 / 7 / 3 conv (standard epilogue) of a stage's three
// resblocks, nx[j] = B * tiles_per_item column tiles x ny[j] = ceil(M / 128) row groups each
struct ConvSmall3Args {
    ConvArgs a[3];
    int nx[3], ny[3];
};
hipError_t launch_conv_small3(const ConvSmall3Args& p, const int ni[3], hipStream_t stream);

// Three fused pairs in one grid (pair3_f16x3.hip): a[0] / a[1] / a[2] = the k = 11 / 7 / 3 pair of a stage's three resblocks (per-tile form:
// tiles_per_item set), n[j] = B * a[j].tiles_per_item workgroups each
struct Pair3Args {
    PairArgs a[3];
    int n[3];
};
hipError_t launch_pair3(const Pair3Args& p, hipStream_t stream);

// Arguments of the whole-ResBlock kernel (rb_f16x3.hip): for p < np:  x = x + c2_p(lrelu(c1_p(lrelu(x))))   [then the MRF modes]
constexpr int AMP_RB_MAX_PAIRS = 3;
struct RbArgs {
    const float* x;            // [B, C, T] input of the block
    float* y;                  // [B, C, T] output; must NOT alias x (other tiles read x's halo)
    const void* wp1[AMP_RB_MAX_PAIRS];     // c1_p (kernel k, dilation dil[p]): packed f16x3 A fragments
    const float* bias1[AMP_RB_MAX_PAIRS];
    const void* wp2[AMP_RB_MAX_PAIRS];     // c2_p (kernel k, dilation 1)
    const float* bias2[AMP_RB_MAX_PAIRS];
    float sc1[AMP_RB_MAX_PAIRS], isc1[AMP_RB_MAX_PAIRS], sc2[AMP_RB_MAX_PAIRS], isc2[AMP_RB_MAX_PAIRS];   // 16 * 2^s and reciprocal
    int dil[AMP_RB_MAX_PAIRS];
    int np;                    // pairs in the block (1 .. AMP_RB_MAX_PAIRS)
    int rh;                    // columns a tile loses either side: sum_p (k-1)/2 * (dil[p] + 1), less the first conv's reach with gx
    int gx;                    // 1: the guard columns hold the real staged x for the launch's first conv (its reach must fit them), 0: zeros
    int B, C, T;
    int tiles_per_item;        // ceil(T / (W - 2 * rh))
    int rev;                   // 1: descending tile order, see ConvArgs::rev
    float slope;               // leaky_relu slope
    int mode;                  // 0: y = v   1: y = y + v   2: y = (y + v) / div   (the LAST pair's MRF mode)
    float div;
    const int* lens;           // ragged batches, see ConvArgs
    int len_mul;
    unsigned* range_flag;      // see ConvArgs
};

// Arguments of the whole-AMPBlock kernel (ampb_f16x3.hip), BigVGAN's AMPBlock1.forward (bigvgan.py:137-146):
//   for p < np:  x = x + c2_p( a_{2p+1}( c1_p( a_{2p}(x) ) ) )     [then the MRF modes]
// as ns = 2 * np STEPS  "Activation1d, then conv":  step s = 2p is (a_{2p}, c1_p), step s = 2p + 1 is (a_{2p+1}, c2_p) + residual.
constexpr int AMP_AMPB_MAX_STEPS = 6;
struct AmpbArgs {
    const float* x;            // [B, C, T] input of the block
    float* y;                  // [B, C, T] output (mode != 0: also the running MRF sum); must NOT alias x
    const void* wp[AMP_AMPB_MAX_STEPS];        // conv of step s: packed f16x3 A fragments (conv_build)
    const float* bias[AMP_AMPB_MAX_STEPS];
    float sc[AMP_AMPB_MAX_STEPS], isc[AMP_AMPB_MAX_STEPS];   // 16 * 2^s operand scaling of each conv and its reciprocal
    int dil[AMP_AMPB_MAX_STEPS];
    const float* act_a[AMP_AMPB_MAX_STEPS];    // Activation1d of step s: alpha (exp'ed when logscale), [C]
    const float* act_invb[AMP_AMPB_MAX_STEPS]; // 1 / (beta + 1e-9), [C]
    const float* act_fu[AMP_AMPB_MAX_STEPS];   // 12 up-sampling taps, each x 2 (the gain of UpSample1d folded in on the host: exact)
    const float* act_fd[AMP_AMPB_MAX_STEPS];   // 12 down-sampling taps
    int ns;                    // steps (2 per pair)
    int rh;                    // tile halo either side: the block's one-sided receptive field rounded up to a multiple of 4
    int B, C, T;               // T % 4 == 0 (16-B rows)
    int tiles_per_item;        // ceil(T / (W - 2 * rh))
    int rev;                   // 1: descending tile order, see ConvArgs::rev
    int mode;                  // 0: y = v   1: y = y + v   2: y = (y + v) / div   (the LAST conv's MRF mode)
    float div;
    const int* lens;           // ragged batches, see ConvArgs
    int len_mul;
    unsigned* range_flag;      // see ConvArgs
};

// Arguments of the DiffWave residual-layer kernels (dw_layer_f16x3.hip), diffwave.py:112-124 in one launch
constexpr int DW_TN = 64;   // output columns per workgroup
struct DwLayerArgs {
    const float* x;            // [B, C, L] input and residual
    const float* cond;         // [B, n_mel, L] up-sampled spectrogram (fp32, as the up-sampler writes it)
    const float* dconst;       // [C] diffusion_projection(e) per item (batch stride dconst_bs; 0 = one row for the whole batch)
    long long dconst_bs;
    const float* skip_in;      // [B, C, L] running skip sum or nullptr (first layer); may alias skip_out
    float* x_out;              // [B, C, L]; must NOT alias x (other tiles read x at +- d)
    float* skip_out;           // [B, C, L]
    const uint4* wp1;          // f16x3: [2C, 3C + n_mel] (taps, then conditioner) as packed A fragments
    const uint4* wp2;          //        [2C, C]
    const float* w1f;          // f32: the same two matrices, row-major, K unpadded
    const float* w2f;
    const float* bias1;        // [2C] dilated_conv.bias + conditioner_projection.bias
    const float* bias2;        // [2C]
    int C, n_mel, L, d;
    int K16;                   // f16x3: ceil((3C + n_mel) / 16), set by the launcher
    int tiles_per_item;        // set by the launcher
    float inv1, inv2;          // 1 / (16 * 2^s) of each matrix
    unsigned* range_flag;      // see ConvArgs
};
size_t dw_layer_lds_bytes(int C, int n_mel, bool f32);
hipError_t launch_dw_layer(DwLayerArgs a, int B, bool f32, hipStream_t stream);

// Arguments of the codec encoder's fused residual unit (codec_unit_f16x3.hip), codec.py:60-76 in one launch
constexpr int CU_TN = 64;   // output columns per workgroup
struct CodecUnitArgs {
    const float* x;            // [B, C, T] input and residual
    float* y;                  // [B, C, T]; must NOT alias x (other tiles read x's halo)
    const uint4* wp1;          // [C, 7 C] (tap-major K) as packed A fragments
    const uint4* wp2;          // [C, C]
    const float* bias1;        // [C]
    const float* bias2;        // [C]
    const float *alpha1, *invb1, *alpha2, *invb2;   // Snake of each conv's input: alpha and 1 / (alpha + 1e-9), [C]
    int C, T, d;
    int tiles_per_item;        // set by the launcher
    float inv1, inv2;          // 1 / (16 * 2^s) of each matrix
    unsigned* range_flag;      // see ConvArgs
};
size_t codec_unit_lds_bytes(int C, int d);
hipError_t launch_codec_unit(CodecUnitArgs a, int B, hipStream_t stream);

// Arguments of FACodec's fused anti-aliased residual unit (aa_unit_f16x3.hip): ResidualUnit with Activation1d(Snake | SnakeBeta) in one launch
constexpr int AA_N1 = 64;   // columns of GEMM 1 per workgroup ...
constexpr int AA_TN = 54;   // ... of which the inner AA_N1 - 2 * 5 are output columns (Activation1d reaches 5 columns either way)
struct AaUnitArgs {
    const float* x;            // [B, C, T] input and residual
    float* y;                  // [B, C, T]; must NOT alias x (other tiles read x's halo)
    const uint4* wp1;          // [C, 7 C] (tap-major K) as packed A fragments
    const uint4* wp2;          // [C, C]
    const float* bias1;        // [C]
    const float* bias2;        // [C]
    const float *a1, *invb1, *a2, *invb2;   // Activation1d of each conv's input: alpha (exp'ed when logscale) and 1 / (beta + 1e-9), [C]
    const float* filt;         // 12 up-sampling taps (without UpSample1d's gain of 2), 12 down-sampling taps
    int C, T, d;
    int tiles_per_item;        // set by the launcher
    float inv1, inv2;          // 1 / (16 * 2^s) of each matrix
    unsigned* range_flag;      // see ConvArgs
};
size_t aa_unit_lds_bytes(int C, int d);
hipError_t launch_aa_unit(AaUnitArgs a, int B, hipStream_t stream);

// Arguments of the fused Snake -> ConvTranspose1d(k = 2 s, stride s) kernel (tconv_f16x3.hip): the decoder blocks' up-sampling step in one launch
constexpr int TC_TN = 64;   // GEMM columns q (input positions) per workgroup
struct TconvArgs {
    const float* x;            // [B, cin, T]
    float* y;                  // [B, cout, Tout]
    const uint4* wp;           // [cout * s rows (o, r), 2 cin] (tap-major K: w[c, o, r], then w[c, o, r + s]) as packed A fragments
    const float* bias;         // [cout]
    const float* alpha;        // [cin] Snake of the input, or nullptr (no activation)
    int cin, cout, s, p;
    int T, Tout;
    int M, NRB;                // GEMM rows cout * s and their 32-row blocks
    int q_first;               // first column that owns an output sample: p / s
    int tiles_per_item;        // set by the launcher
    float inv;                 // 1 / (16 * 2^s) of the matrix
    unsigned* range_flag;      // see ConvArgs
};
size_t tconv_lds_bytes(int cin);
hipError_t launch_tconv(TconvArgs a, int B, hipStream_t stream);

struct ConvPlan {
    int KT;      // taps compiled into the kernel (1,2,3,5,7,11)
    int WM, WN;  // waves along M / N (WM*WN == 4)
    int NI;      // 32-column MFMA tiles per wave
    int HALO;    // staged halo capacity (64 or 128)
    int NT() const { return 32 * NI * WN; }
    int Mgroup() const { return 32 * WM; }
};

// Chooses the kernel variant for a conv with `ntaps` taps, GEMM rows M, halo_total columns and Tq
// columns per item.  Returns false if unsupported.
bool choose_plan(int ntaps, int M, int halo_total, int Tq, ConvPlan* plan);

// ---- per-tap-count kernels: each TU below is compiled once per tap count (-DAMP_KT=k, the lists in build.py) and instantiates these
// templates for KT = AMP_KT only; conv_host.hip maps a runtime tap count onto them
template <int KT> hipError_t launch_conv(const ConvPlan& plan, const ConvArgs& a, hipStream_t stream);        // exact f32 MFMA (conv_mfma.hip)
template <int KT> hipError_t launch_conv_f16x3(const ConvPlan& plan, const ConvArgs& a, hipStream_t stream);  // split-f16 MFMA (conv_f16x3.hip)
// row-blocked conv (conv_blk_f16x3.hip): tile width for cm chunks per staging round and a halo, 0 = not covered; launch
template <int KT> int conv_blk_nt(int cm, int halo_total);
template <int KT> hipError_t launch_conv_blk(int cm, int wn, const ConvArgs& a, hipStream_t stream);
// frame-rate convs (conv_small_f16x3.hip): whole-K staging; epi 0 standard, 1 gate, 2 WN accumulate; ni 2 | 4
constexpr int kSmallConvMaxChunks = 16;   // Cin <= 256
template <int KT> hipError_t launch_conv_small(int ni, int epi, const ConvArgs& a, hipStream_t stream);
// fused pair (pair_f16x3.hip): output columns per workgroup for (C, dilation), 0 = not covered; launch
template <int KT> int pair_tile(int C, int dil);
template <int KT> hipError_t launch_pair(const PairArgs& a, hipStream_t stream);
// strip-mined fused pair (pair_strip_f16x3.hip): columns per step for (C, dilation), 0 = not covered
template <int KT> int strip_step(int C, int dil, int wide, int* wg_per_cu);
template <int KT> hipError_t launch_strip(const PairArgs& a, hipStream_t stream);
// whole ResBlock1 (rb_f16x3.hip): tile width for (C, max dilation) in form `wide`, 0 = not covered; launch
template <int KT> int rb_tile(int C, int max_dil, int wide);
template <int KT> hipError_t launch_rb(const RbArgs& a, int wide, hipStream_t stream);
// whole AMPBlock1 (ampb_f16x3.hip): tile width for (C, max dilation) in form `wide`, 0 = not covered; launch
template <int KT> int ampb_tile(int C, int max_dil, int wide);
template <int KT> hipError_t launch_ampb(const AmpbArgs& a, int wide, hipStream_t stream);

// conv_post: y[b,0,t] = tanh( bias + sum_i sum_j w[i][j] * act_in(x[b,i,t+j-pad]) )   (Cout == 1)
hipError_t launch_conv_post(const float* x, const float* w_dev /*[Cin*K]*/, const float* bias_dev /*[1] or null*/,
                            float* y, int B, int Cin, int T, int K, float slope_in, int apply_tanh,
                            const int* lens, int len_mul, hipStream_t stream);

// Activation1d (anti-aliased Snake); a_dev = alpha (already exp'ed if logscale), invb_dev = 1/(beta+1e-9)
hipError_t launch_act1d(const float* x, float* y, int B, int C, int T, const float* a_dev, const float* invb_dev,
                        const float* filt_up12, const float* filt_dn12, const int* lens, int len_mul,
                        hipStream_t stream, int rev = 0 /* 1: descending workgroup order, ConvArgs::rev */);

// y[b,c,t] += cond[b,c]   (HiFiGAN_vits `x + self.cond(g)` with g of length 1)
hipError_t launch_add_channel_bias(float* y, const float* cb, int B, int C, int T, hipStream_t stream);
// y = ((y + p[0]) + p[1] ...) / div over `count` floats (16-byte aligned): the MRF mean of resblocks that stored their results separately
constexpr int AMP_MRF_MAX_PARTS = 3;
struct MrfSumArgs {
    float* y;
    const float* p[AMP_MRF_MAX_PARTS];
    int n;
    float div;
    size_t count;
};
hipError_t launch_mrf_sum(const MrfSumArgs& a, hipStream_t stream);

// VITS posterior-encoder / flow element-wise kernels (small_kernels.hip)
hipError_t launch_wn_gate(const float* a, const float* cond, long long cond_bs, float* out, int B, int H, int T,
                          hipStream_t stream);
hipError_t launch_wn_accumulate(float* x, float* out, const float* rs, const int* lens, int B, int H, int T, int last,
                                int first, hipStream_t stream);
hipError_t launch_mask(float* x, const int* lens, int B, int C, int T, hipStream_t stream);
hipError_t launch_coupling(float* x, const float* m, const int* lens, int B, int h, int T, int reverse,
                           hipStream_t stream);
hipError_t launch_flip_channels(const float* x, float* y, int B, int C, int T, hipStream_t stream);
hipError_t launch_posterior_sample(const float* stats, const float* eps, const int* lens, float* z, int B, int C, int T,
                                   hipStream_t stream);

hipError_t launch_fir_up(const float* x, float* y, int rows, int T, const float* taps_host, int K, int ratio, int pad,
                         int pad_left, hipStream_t stream);
hipError_t launch_fir_filter(const float* x, float* y, int rows, int T, int Tout, const float* taps_host, int K,
                             int stride, int pad_left, int mode, hipStream_t stream);
hipError_t launch_snake(const float* x, float* y, int B, int C, int T, const float* alpha, const float* beta, int logscale,
                        hipStream_t stream);
hipError_t launch_pcm16(const float* x, short* y, int B, int L, long long x_stride, long long y_stride, const int* lens,
                        hipStream_t stream);
hipError_t launch_apnet_polar(const float* logamp, const float* R, const float* I, size_t n, float* pha, float* rea,
                              float* imag, hipStream_t stream);

// mel front end (mel.hip)
hipError_t launch_mel(const amp_mel_desc& d, const float* wav, const int* lens, int B, int L, int F, const float* window,
                      const float* melbasis, float* mel, float* mag, float* re, float* im, hipStream_t stream);

void set_error(const char* fmt, ...);

// Kernels that ask for more than 64 KB of dynamic LDS need hipFuncAttributeMaxDynamicSharedMemorySize, and the attribute belongs to
// ONE device's copy of the function: set it once per (kernel, device), under a lock -- two handles may launch from two host threads
// (the per-launcher copies of this bookkeeping had no lock and mapped devices >= 64 onto bit 0 without setting anything).
// The kernel is a template ARGUMENT: one mask per kernel instantiation.  Devices beyond 63 set the attribute on every launch.
template <auto Kernel>
inline hipError_t ensure_dynamic_lds(size_t bytes) {
    if (bytes <= 64 * 1024) return hipSuccess;
    static std::atomic<unsigned long long> done{0};
    static std::mutex mu;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) dev = 0;
    if (dev < 64 && ((done.load(std::memory_order_acquire) >> dev) & 1ull)) return hipSuccess;
    std::lock_guard<std::mutex> lock(mu);
    if (dev < 64 && ((done.load(std::memory_order_acquire) >> dev) & 1ull)) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return e;
    if (dev < 64) done.fetch_or(1ull << dev, std::memory_order_release);
    return hipSuccess;
}

// set the LDS attribute, launch 256-thread workgroups on a 1-D grid, hand back the launch status
template <auto Kernel, class Args>
inline hipError_t launch_dynamic_lds(unsigned grid, size_t lds, hipStream_t stream, const Args& a) {
    if (hipError_t e = ensure_dynamic_lds<Kernel>(lds); e != hipSuccess) return e;
    hipLaunchKernelGGL(Kernel, dim3(grid), dim3(256), lds, stream, a);
    return hipGetLastError();
}

// Which kernels a stretch of launch_* calls issued, as rocprofv3 prints them ("pair_strip_kernel<11, 2, 2, 4, 320, 2, 4, 1>"):
// while the calling thread points tl_kernel_log at a string (a profiled amp_gen_forward does, per resblock), every launch
// appends its kernel's name once (" | "-joined) -- bench.py reports the variant the policy actually picked, not a literal.
extern __thread std::string* tl_kernel_log;   // (__thread: constant-initialised, no TLS init function for other TUs to import)
// AMP_LAUNCH_MANIFEST=<file> (read once per process): every launch appends one line
//     <kernel name with its template arguments>\t<workgroups>\t<algorithmic GFLOP>\t<algorithmic MB>\t<what it computes>
// -- the launcher's OWN statement of the work a launch does, which tools/roofline_table.py joins with rocprofv3's per-dispatch durations
// by (name, workgroups) instead of guessing shapes from template arguments.  Off: one predictable branch per launch.
bool manifest_on();
void manifest_add(const char* name, unsigned long long workgroups, double gflop, double mb, const char* what);
extern __thread char tl_last_kernel[160];
template <typename... A>
inline void note_kernel(const char* base, A... args) {
    if (!tl_kernel_log && !manifest_on()) return;
    char* buf = tl_last_kernel;
    constexpr int cap = (int)sizeof(tl_last_kernel);
    const int v[] = {static_cast<int>(args)...};
    int n = snprintf(buf, cap, "%s<", base);
    for (size_t i = 0; i < sizeof...(args) && n < cap - 16; ++i)
        n += snprintf(buf + n, cap - n, i ? ", %d" : "%d", v[i]);
    snprintf(buf + n, cap - n, ">");
    if (!tl_kernel_log) return;
    if (tl_kernel_log->find(buf) != std::string::npos) return;
    if (!tl_kernel_log->empty()) *tl_kernel_log += " | ";
    *tl_kernel_log += buf;
}
// after note_kernel(): a form of the kernel that is a launch argument, not a template argument -- appended once to the kernel log only
// (the manifest keeps the profiler's spelling of the name and states the form in note_work's description)
inline void note_form(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
inline void note_form(const char* fmt, ...) {
    if (!tl_kernel_log) return;
    char form[64];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(form, sizeof(form), fmt, ap);
    va_end(ap);
    if (tl_kernel_log->find(form) != std::string::npos) return;
    *tl_kernel_log += " ";
    *tl_kernel_log += form;
}
// after note_kernel(): the launch's grid and algorithmic work (manifest only)
inline void note_work(unsigned long long workgroups, double gflop, double mb, const char* fmt, ...) __attribute__((format(printf, 4, 5)));
inline void note_work(unsigned long long workgroups, double gflop, double mb, const char* fmt, ...) {
    if (!manifest_on()) return;
    char what[160];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(what, sizeof(what), fmt, ap);
    va_end(ap);
    manifest_add(tl_last_kernel, workgroups, gflop, mb, what);
}
// a Conv1d / ConvTranspose1d launch: GEMM M = Cout * up rows, K = Cin * KT, N = B * Tq columns; bytes = x read once + y written once
// (+ the residual / running sum read).  `grid=XxY` states the launch's grid: Y > 1 is the 2-D order (row group = blockIdx.y), Y = 1 with
// several row groups the row-group-fastest 1-D order (ConvArgs::row_groups)
// The label follows the HANDLE (tl_conv_transposed, set by conv_run for the launch it issues next), not a.up: a stride-1
// ConvTranspose1d runs as the equivalent Conv1d (conv_build) and is still a "ConvT".
extern __thread int tl_conv_transposed;
inline void note_conv_work(const ConvArgs& a, int KT, dim3 grid) {
    const bool convt = tl_conv_transposed != 0;
    tl_conv_transposed = 0;
    if (!manifest_on()) return;
    const double gf = 2.0 * a.M * a.Cin * KT * (double)a.Tq * a.B / 1e9;
    const double mb = 4.0 * a.B * ((double)a.Cin * a.Tin + (double)a.Cout * a.Tout * (1 + (a.res ? 1 : 0) + (a.mode ? 1 : 0))) / 1e6;
    note_work((unsigned long long)grid.x * grid.y, gf, mb, "%s %d->%d k=%d d=%d T=%d->%d B=%d%s%s grid=%ux%u", convt ? "ConvT" : "conv", a.Cin,
              a.Cout, a.up > 1 ? KT * a.up : KT, a.dstep, a.Tin, a.Tout, a.B, a.res ? " +res" : "", a.mode ? " +sum" : "", grid.x, grid.y);
}

// The f16x3 kernels stage fp32 activations as hi + lo f16 pairs after an exact x16: anything beyond |x| = 4094 (or
// non-finite) cannot be represented.  They OR 1 into this per-device word when that happens (runtime.hip; amp_host.h: RangeGuard).
unsigned* range_flag_for_current_device();
// (the kernels keep the running maximum of |staged value|: one v_max_f32 per element; a NaN operand is not flagged --
// it propagates to the output exactly as it does through the fp32 reference)

}  // namespace amp
