/*
 * amphion_hip.h -- C ABI of libamphion_hip.so: the MI355X (gfx950) vocoder-inference hot path.
 *
 * The reference (open-mmlab/Amphion) has NO native code on this path: its "kernels" are
 * torch.nn.functional calls.  The entry points below are what a ctypes binding of the reference's
 * generator / front-end would call instead of those torch ops; each one cites the reference
 * interface it replaces (paths relative to the reference tree).  INTEGRATION.md shows the
 * reference-side binding.
 *
 * Conventions
 *   - plain C, plain pointers and sizes; no torch types.
 *   - every function returns amp_status (0 = OK, <0 = error); amp_last_error() gives the text
 *     (thread-local).  Nothing calls abort().
 *   - `*_dev` pointers are device (HBM) pointers on the current HIP device; `*_host` are host
 *     pointers.  The caller owns inputs, outputs and the workspace; a handle owns only its packed
 *     weights.  No allocation and no host synchronisation inside *_forward: all work is enqueued on
 *     `stream` (a hipStream_t passed as void*; NULL = the default stream).
 *   - all tensors are fp32, contiguous, layout [B, C, T] (time fastest), as in the reference.
 */
#ifndef AMPHION_HIP_H
#define AMPHION_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum amp_status {
    AMP_OK = 0,
    AMP_ERR_INVALID = -1,        /* bad argument / shape */
    AMP_ERR_MISSING_WEIGHT = -2, /* finalize(): a tensor the architecture needs was never set */
    AMP_ERR_HIP = -3,            /* a HIP runtime call failed */
    AMP_ERR_UNSUPPORTED = -4,    /* configuration outside what the kernels cover */
    AMP_ERR_STATE = -5,          /* call order violated (e.g. forward before finalize) */
    AMP_ERR_RANGE = -6           /* an activation left the split-f16 operand range (see amp_range_check) */
} amp_status;

typedef enum amp_arch {
    AMP_ARCH_HIFIGAN = 0,      /* models/vocoders/gan/generator/hifigan.py:151-219  HiFiGAN       */
    AMP_ARCH_BIGVGAN = 1,      /* models/vocoders/gan/generator/bigvgan.py:232-331  BigVGAN       */
    AMP_ARCH_HIFIGAN_VITS = 2  /* models/vocoders/gan/generator/hifigan.py:376-449  HiFiGAN_vits  */
} amp_arch;

typedef enum amp_activation {
    AMP_ACT_LRELU = 0,     /* F.leaky_relu(x, 0.1)            hifigan.py:14,95-97          */
    AMP_ACT_SNAKE = 1,     /* Activation1d(Snake)             bigvgan.py:85-102, snake.py:51-61   */
    AMP_ACT_SNAKEBETA = 2  /* Activation1d(SnakeBeta)         bigvgan.py:104-124, snake.py:110-122 */
} amp_activation;

/* Arithmetic of the conv contractions (every Conv1d / ConvTranspose1d of the path; the reference runs
 * them as fp32 torch ops).  Inputs, outputs, accumulators and everything stored in HBM are fp32 in both
 * modes; results of both modes meet the same 1e-4 max-abs parity bound against the fp32 reference. */
typedef enum amp_precision {
    AMP_PRECISION_F32 = 0,   /* v_mfma_f32_32x32x2_f32: bit-for-bit an fp32 fmaf chain (157 TFLOP/s peak)       */
    AMP_PRECISION_F16X3 = 1  /* operands split hi+lo in f16 (22 mantissa bits), 3 x v_mfma_f32_32x32x16_f16 per
                                term, fp32 accumulate (838 TFLOP/s effective peak) -- the default                */
} amp_precision;

#define AMP_MAX_STAGES 8
#define AMP_MAX_KERNELS 8
#define AMP_MAX_DILATIONS 8

/* Mirrors cfg.model.hifigan.* / cfg.model.bigvgan.* (hifigan.py:155-199, bigvgan.py:237-306) and the
 * explicit HiFiGAN_vits constructor arguments (hifigan.py:377-387). */
typedef struct amp_gen_desc {
    int32_t arch;                     /* amp_arch */
    int32_t n_in;                     /* cfg.preprocess.n_mel, or initial_channel for HiFiGAN_vits */
    int32_t upsample_initial_channel;
    int32_t n_stages;                 /* len(upsample_rates) */
    int32_t upsample_rates[AMP_MAX_STAGES];
    int32_t upsample_kernel_sizes[AMP_MAX_STAGES];
    int32_t n_kernels;                /* len(resblock_kernel_sizes) */
    int32_t resblock_kernel_sizes[AMP_MAX_KERNELS];
    int32_t n_dilations[AMP_MAX_KERNELS];
    int32_t resblock_dilation_sizes[AMP_MAX_KERNELS][AMP_MAX_DILATIONS];
    int32_t resblock_type;            /* 1 = ResBlock1/AMPBlock1, 2 = ResBlock2/AMPBlock2 */
    int32_t activation;               /* amp_activation (BigVGAN: cfg.model.bigvgan.activation) */
    int32_t snake_logscale;           /* cfg.model.bigvgan.snake_logscale */
    int32_t gin_channels;             /* HiFiGAN_vits only; 0 = no `cond` conv */
} amp_gen_desc;

typedef struct amp_gen amp_gen;

/* Library / device probes.  amp_version: 100 = round 1's surface; 120 adds the fused-WN and conv + activation entry points, 122
 * amp_set_conv_blk / amp_set_conv_rg_fast / amp_set_pingpong; 130 (round 3) appended the four range_* fields to amp_mel_desc and
 * added amp_resblock_forward / amp_set_resblock_fusion / amp_gen_kernel_name; 140 (round 4): amp_mel_desc starts with struct_size
 * (an ABI break for every earlier consumer of that struct -- re-compile against this header), + amp_mel_init,
 * amp_ampblock_forward, amp_set_ampblock_fusion; 141 (additive): amp_conv_forward_ragged, amp_layer_norm_c_ragged,
 * amp_dwconv_layer_norm_c, amp_rel_attention_strided, amp_set_rel_attention_tiled, amp_expand_path_strided; 142 (round 5) REMOVES
 * amp_conv_act_forward, amp_set_fuse_act and amp_set_wn_layer_fusion together with the kernels behind them (bit-identical forms the launch
 * policy never chose), refuses amp_set_pair_strips(1), and lets amp_mel_forward / amp_mel_backward / amp_istft_forward / amp_istft_same take
 * any n_fft in [64, 4096] (mixed-radix kernels: compile-time butterflies for the primes 2 .. 13, a run-time radix pass for larger prime factors;
 * powers of two keep their kernels); 143 (additive): the Vocos entry points amp_pw_create / amp_pw_forward / amp_pw_precision /
 * amp_pw_destroy and amp_istft_same_polar, and amp_dwconv_layer_norm_c accepts K = 7 (C <= 1024); 144 (additive): the DiffWave entry
 * points amp_dw_*; 145 (additive): the Amphion codec entry points amp_fvq_*, amp_codec_unit_*, amp_sconv_*;
 * 146 (additive): the decoder blocks' up-sampling step amp_tconv_* and amp_set_tconv_fusion; 147 (additive): DualCodec's
 * amp_dwconv_layer_norm_c_causal, amp_fvq_encode_ex, amp_fvq_decode_add and amp_semantic_prepare; 148 (additive): FACodec's anti-aliased
 * residual unit amp_aa_unit_* and amp_set_aa_unit_fusion; 149 (additive): SpeechTokenizer's amp_elu_pad, amp_lstm_* and amp_evq_*;
 * 150 (additive): the semantic tokenizers' amp_dsconv_* and amp_gelu; 151 (additive): amp_set_strip_fit and amp_pair_strip_plan;
 * 152 (additive): amp_layer_norm_c_style, amp_embed_sum_c and amp_embed_sum_check (FACodec voice conversion);
 * 153 (additive): amp_rope_attention, amp_rms_norm_c_adaptive, amp_silu and amp_swiglu (the flow-matching transformer of Vevo);
 * 154 (additive): amp_mask_sample (MaskGCT's decoding step), and amp_rope_attention accepts head dimension 96 beside 64;
 * 155 (additive): amp_rope_attention_causal, amp_kv_append, amp_attention_decode (+ _workspace_bytes, _split), amp_pw_forward_vec
 * (+ _workspace_bytes) and amp_ar_sample (the autoregressive transformer of Vevo);
 * 156 (additive): amp_mh_attention (head dimension 128, no rotation), amp_fs2_durations, amp_bucketize_embed_add and amp_layer_norm_c_head
 * (FastSpeech2 / JETS inference);
 * 157 (additive): amp_cross_attention (head dimension 64, no rotation, separate query and key lengths), amp_ns2_layer_* and amp_ns2_ode_step
 * (NaturalSpeech2 inference);
 * 158 (additive): amp_prefix_attention (causal without rotation at head dimension 64, with a run-time prefix), amp_pw_forward_vec_ln
 * (+ _workspace_bytes) and amp_embed_pos (VALL-E inference);
 * 159 (additive): amp_conv2d_* (3 x 3 Conv2d with stride, x2 up-sampling, GroupNorm + SiLU on load and a residual epilogue),
 * amp_group_norm_stats, amp_group_norm, amp_geglu, and amp_cross_attention_hd: amp_cross_attention at head dimensions 32 and 128 beside 64 (AudioLDM);
 * 160 (additive): amp_set_rb_guards, amp_set_rb_split_plan, amp_rb_launch_plan and amp_resblock_forward_ex (whole-resblock launches). */
int amp_version(void);
const char* amp_last_error(void);
/* Number of HIP devices visible (0 when there is no GPU); never fails. */
int amp_device_count(void);

/* Process-wide default for handles created AFTER the call (also settable with the environment variable
 * AMP_PRECISION=f32|f16x3 before the first handle is created).  A handle keeps the precision it was
 * built with. */
int amp_set_precision(int precision /* amp_precision */);
int amp_get_precision(void);

/* ---- Generator handle: replaces nn.Module construction + forward of HiFiGAN / BigVGAN / HiFiGAN_vits ---- */

/* Replaces HiFiGAN.__init__ (hifigan.py:151-201) / BigVGAN.__init__ (bigvgan.py:232-311) /
 * HiFiGAN_vits.__init__ (hifigan.py:376-422): validates the architecture, allocates nothing on the device. */
int amp_gen_create(const amp_gen_desc* desc, amp_gen** out);

/* Replaces load_state_dict for one tensor (vocoder_inference.py:270-332).  `ref_key` is the
 * reference state_dict key: "...weight_g"/"...weight_v" pairs or folded
 * "...weight", "...bias", Snake "...act.alpha"/"...act.beta", "...filter" buffers.  The data is
 * copied; `data_host` may be a host pointer or a device pointer of the current context (fp32, contiguous).
 * Unknown keys are rejected (AMP_ERR_INVALID). */
int amp_gen_set_weight(amp_gen* g, const char* ref_key, const float* data_host, const int64_t* shape, int ndim);

/* Folds weight-norm (w = g*v/||v||, torch.nn.utils.weight_norm; hifigan.py:23,157,176,199),
 * packs the weights into MFMA fragment order and uploads them to the current device. */
int amp_gen_finalize(amp_gen* g);

/* Output samples per input frame (prod(upsample_rates)) and scratch size for a (B, T) forward. */
int amp_gen_hop(const amp_gen* g);
size_t amp_gen_workspace_bytes(const amp_gen* g, int B, int T);

/* amp_gen_forward can run the batch depth-first in groups of items (each group through the whole
 * generator) to bound the workspace: target working set in MiB, 0 = whole batch per layer (default; the
 * faster setting on MI355X).
 * Results do not depend on it. */
int amp_set_group_mb(int megabytes);

/* Operand-range guard of the f16x3 arithmetic.  Activations are staged as hi + lo f16 pairs after an exact x16, so
 * |x| up to 4094 is representable; the fp32 reference (F.conv1d) has no such limit.  Every f16x3 kernel raises a flag
 * when a staged value is larger (or infinite) -- the output of that launch is then NOT the reference's (inf / NaN).
 * A generator handle owns its flag: amp_gen_range_check synchronises `stream` and returns AMP_ERR_RANGE if a forward of
 * `g` since the last check was affected (and clears the flag); amp_gen_forward reports the same condition WITHOUT
 * synchronising: a call that finds the flag of an earlier, finished forward of the same handle set returns
 * AMP_ERR_RANGE instead of running.  amp_range_check does the synchronising check for the op-level entry points
 * (amp_conv_forward, amp_pair_forward, ...), which share one flag per device.  Remedy: amp_set_precision(
 * AMP_PRECISION_F32) and rebuild the handle (the exact fp32 MFMA kernels have the reference's range).  A NaN input is
 * not flagged: it propagates to the output as it does through the reference. */
int amp_range_check(void* stream);
int amp_gen_range_check(amp_gen* g, void* stream);

/* Fused ResBlock pairs (hifigan.py:93-100) have two kernels with bit-identical results (tests/test_gpu_pair.py): the
 * per-tile kernel and the strip-mined kernel (a workgroup walks a strip of one utterance and carries conv2's halo in
 * LDS; C = 128, k >= 7, launches that fill the chip).  -1 (default): the measured per-shape policy; 0: per-tile
 * everywhere (the cross-check).  Mode 1 (four-wave / C = 256 strips) left with amp_version 142. */
int amp_set_pair_strips(int on);
/* The strip-mined kernel cuts an utterance into strips in one of two forms, bit-identical (tests/test_gpu_pair_strip_fit.py): SHIFTED strips
 * start k - 1 columns early and discard them (S * 256 - (k - 1) outputs per S steps), FITTED strips keep every column of every step and
 * compute the k - 1 carried columns in a short prologue -- cheaper exactly where that saves a round of workgroups (T a multiple of the step).
 * -1 (default): the cost model of strip_geometry (conv_host.hip) chooses per (B, T, k); 0: never; 1: every strip launch.
 * amp_pair_strip_plan reports the plan of a C = 128 pair at (B, T, k) under the current switches, without a device: form 0 shifted / 1 fitted,
 * outputs per strip, strips per item and steps per full strip; AMP_ERR_UNSUPPORTED when kernel size k has no strip kernel. */
int amp_set_strip_fit(int mode);
int amp_pair_strip_plan(int B, int T, int k, int ragged, int* form, int* strip_len, int* strips_per_item, int* steps);

/* Replaces HiFiGAN.forward (hifigan.py:203-219), BigVGAN.forward (bigvgan.py:313-331) and
 * HiFiGAN_vits.forward (hifigan.py:424-443):  mel_dev [B, n_in, T]  ->  wav_dev [B, 1, T*hop].
 * cond_dev: optional speaker embedding g [B, gin_channels, 1] (HiFiGAN_vits), else NULL. */
int amp_gen_forward(amp_gen* g, const float* mel_dev, const float* cond_dev, int B, int T, float* wav_dev,
                    void* workspace_dev, size_t workspace_bytes, void* stream);

/* Ragged batch: item b holds lens_dev[b] <= T valid mel frames (int32, device) inside the zero-padded
 * [B, n_in, T] input.  Every layer then pads at the utterance's OWN end (zero padding of the convs,
 * replicate padding of the anti-aliased activations), so wav[b, : lens[b] * hop] is bit-identical to
 * running that utterance alone (the reference's per-utterance loop, gan_vocoder_inference.py:74-96);
 * samples beyond it are unspecified.  lens_dev == NULL is amp_gen_forward. */
int amp_gen_forward_ragged(amp_gen* g, const float* mel_dev, const float* cond_dev, const int32_t* lens_dev, int B,
                           int T, float* wav_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* Kernel timing with HIP events recorded on the launch stream.  amp_gen_set_profiling(g, slots) keeps a ring of
 * `slots` event sets (0 = off): every amp_gen_forward records into the next one without synchronising, so a whole
 * timed region of `slots` forwards can be read back afterwards.  amp_gen_timing_ms(g, back, which, &ms): `back` = 0
 * is the most recent forward, 1 the one before, ...; which: 0 = whole forward, 1 = MRF conv stack (all
 * ResBlock/AMPBlock convs), 2 + i = the MRF convs of upsampling stage i, 100 + 16*i + j = resblock j of stage i
 * (its back-to-back conv / fused-pair launches).  Synchronises on that forward's events.  Returns <0 on error.
 * amp_gen_last_timing_ms(g, which, &ms) == amp_gen_timing_ms(g, 0, which, &ms). */
int amp_gen_set_profiling(amp_gen* g, int slots);
int amp_gen_timing_ms(amp_gen* g, int back, int which, float* ms_out);
int amp_gen_last_timing_ms(amp_gen* g, int which, float* ms_out);
/* Which kernels the launches of resblock j of stage i (which = 100 + 16*i + j, as above) were in that profiled forward:
 * the distinct kernel names as rocprofv3 prints them (template arguments included), " | "-joined, written to buf[n].
 * This is what the launch policy actually picked for the shape -- bench.py reports it instead of assuming. */
int amp_gen_kernel_name(amp_gen* g, int back, int which, char* buf, size_t n);

void amp_gen_destroy(amp_gen* g);

/* ---- Op level (used by tests and by callers that want one fused op) ---- */

typedef struct amp_conv amp_conv;

/* One Conv1d (nn.Conv1d(cin, cout, k, 1, dilation=d, padding=get_padding(k, d)), gan_utils.py:12) or
 * ConvTranspose1d(cin, cout, k, stride, padding) (hifigan.py:176-186).  weight_host is the FOLDED
 * weight: [cout, cin, k] for a conv, [cin, cout, k] for a transposed conv.  bias_host may be NULL.
 * Geometry (tests/test_gpu_conv_geometry.py runs all of it against fp64): Conv1d with stride 1, any k, dilation and padding >= 0 whose
 * staged receptive field max(0, p) + max(0, (kt - 1) * dilation - p) is at most 128 columns (kt = k rounded up to 1, 2, 3, 5, 7, 11;
 * k <= 11); ConvTranspose1d with dilation 1, any stride >= 1, any k with ceil(k / stride) <= 11 (k < stride included) and any
 * padding >= 0 (stride 1 runs as the equivalent Conv1d).  Refused here with AMP_ERR_UNSUPPORTED: a strided Conv1d, a dilated
 * ConvTranspose1d, more than 11 taps, a receptive field beyond the halo.  Refused by the forward calls with AMP_ERR_INVALID: a T whose
 * T_out (amp_conv_out_len) is <= 0. */
int amp_conv_create(int transposed, int cin, int cout, int k, int stride, int dilation, int padding,
                    const float* weight_host, const float* bias_host, amp_conv** out);
int amp_conv_out_len(const amp_conv* c, int T);
/* y = lrelu_out( conv( lrelu_in(x) ) + bias + res ).  slope == 1.0f disables an activation;
 * res_dev may be NULL or alias y_dev (in-place residual).  x_dev [B, cin, T] -> y_dev [B, cout, T_out]. */
int amp_conv_forward(const amp_conv* c, const float* x_dev, int B, int T, float slope_in, const float* res_dev,
                     float slope_out, float* y_dev, void* stream);
/* Same, reading x from a channel slice of a wider tensor: batch item b starts at x_dev + b*x_batch_stride
 * (elements).  Used by ResidualCouplingLayer.pre on x0 = x[:, :half] (modules/flow/modules.py:380-381). */
int amp_conv_forward_strided(const amp_conv* c, const float* x_dev, long long x_batch_stride, int B, int T,
                             float slope_in, const float* res_dev, float slope_out, float* y_dev, void* stream);
/* conv(x * mask) with the sequence mask taken by the kernel (`conv_1(x * x_mask)`, modules/transformer/attentions.py:392-400;
 * `pre(x0) * x_mask`, modules/flow/modules.py:381): lens_dev int32 [B] valid lengths or NULL; input columns t >= lens[b] count
 * as zero whatever the buffer holds (a select, NaN-safe); output tiles wholly beyond an utterance's end are skipped, so columns
 * t >= lens[b] of y_dev are UNSPECIFIED (assign, do not multiply).  'same' zero-padded Conv1d only when lens_dev is given.
 * x_batch_stride 0 = cin*T. */
int amp_conv_forward_ragged(const amp_conv* c, const float* x_dev, long long x_batch_stride, int B, int T, const int32_t* lens_dev,
                            float slope_in, const float* res_dev, float slope_out, float* y_dev, void* stream);
/* amp_conv_forward with the MRF accumulation of hifigan.py:208-214 / apnet.py:355-363 exposed:
 *   v = conv(lrelu_in(x)) + bias (+ res);   mode 0: y = v   1: y = y + v   2: y = (y + v) / div. */
int amp_conv_forward_mrf(const amp_conv* c, const float* x_dev, int B, int T, float slope_in, const float* res_dev,
                         float* y_dev, int mode, float div, void* stream);

/* APNet head, element-wise over n values (models/vocoders/gan/generator/apnet.py:379-383):
 * pha = atan2(I, R); rea = exp(logamp) * cos(pha); imag = exp(logamp) * sin(pha). */
int amp_apnet_polar(const float* logamp_dev, const float* r_dev, const float* i_dev, size_t n, float* pha_dev,
                    float* rea_dev, float* imag_dev, void* stream);

/* UpSample1d.forward (modules/anti_aliasing/resample.py:36-45) as a stand-alone op: replicate-pad by
 * K/ratio - 1, depthwise ConvTranspose1d with the [K] filter at stride = ratio, x ratio, crop -> y [B, C, ratio*T].
 * filt_host: K <= AMP_FIR_MAX_TAPS floats on the host (the module's `filter` buffer). */
#define AMP_FIR_MAX_TAPS 64
int amp_fir_upsample(const float* x_dev, int B, int C, int T, const float* filt_host, int K, int ratio, float* y_dev,
                     void* stream);
/* LowPassFilter1d.forward (modules/anti_aliasing/filter.py:92-99; DownSample1d, resample.py:62-65, is this with
 * stride = ratio): pad (pad_left, pad_right) in `pad_mode`, depthwise Conv1d with the [K] filter at `stride`
 * -> y [B, C, (T + pad_left + pad_right - K) / stride + 1].  padding=False is pad_left = pad_right = 0. */
typedef enum amp_pad_mode { AMP_PAD_REPLICATE = 0, AMP_PAD_ZEROS = 1, AMP_PAD_REFLECT = 2 } amp_pad_mode;
int amp_fir_filter(const float* x_dev, int B, int C, int T, const float* filt_host, int K, int stride, int pad_left,
                   int pad_right, int pad_mode, float* y_dev, void* stream);

/* ---- frame-rate ops of the text -> duration -> alignment front of VITS
 * inference, SynthesizerTrn.infer models/tts/vits/vits.py:320-369.  All tensors [B, C, T] fp32 on the
 * device; lens_dev = int32 [B] valid lengths (NULL = all T). ---- */
/* LayerNorm over channels (modules/base/base_module.py:20-23) of x (+ res if not NULL: Encoder's norm(x + y),
 * modules/transformer/attentions.py:69,73), optionally followed by GELU and by "+ post" (DDSConv,
 * modules/flow/modules.py:64-70: x = x + gelu(norm(y))). */
int amp_layer_norm_c(const float* x_dev, const float* res_dev, const float* gamma_dev, const float* beta_dev,
                     const float* post_dev, int B, int C, int T, float eps, int gelu, float* y_dev, void* stream);
/* amp_layer_norm_c whose result is ZERO in the columns t >= lens[b] (a select: x / res may hold anything there) -- the `* x_mask`
 * that follows the Encoder's norms (attentions.py:64-76) without its own launch. */
int amp_layer_norm_c_ragged(const float* x_dev, const float* res_dev, const float* gamma_dev, const float* beta_dev,
                            const float* post_dev, const int* lens_dev, int B, int C, int T, float eps, int gelu, float* y_dev,
                            void* stream);
/* The style-adaptive LayerNorm of FACodec's conditioned transformer (models/codec/ns3_codec/transformer.py:13-32) and the
 * `timbre_norm(x) * gamma + beta` of its decoders' inference, in one launch:
 *     y[b, c, t] = style[b, c] * LN_c(x + res)[b, c, t] + style[b, C + c]
 * LN_c = the LayerNorm over the channel axis without an affine of its own; style_dev [B, 2C] holds one (scale | shift) row PER ITEM.  Mean,
 * biased variance and accumulation order are amp_layer_norm_c's: with every row of style equal to (gamma | beta) the two give the same bits.
 * res_dev may be NULL.  Plain fp32; the same C, T and B <= 65535 as amp_layer_norm_c, and y may alias x.  Each x element is read once
 * (C <= 256; more channels are re-read) and y is written once. */
int amp_layer_norm_c_style(const float* x_dev, const float* res_dev, const float* style_dev, int B, int C, int T, float eps, float* y_dev,
                           void* stream);
/* act(LN(dwconv(x * mask))) in one launch: DDSConv's convs_sep[i] -> norms_1[i] -> gelu (modules/flow/modules.py:63-65), the
 * depthwise taps evaluated on load in amp_dwconv's order (same bits as the two launches).  K = 3, or K = 7 with C <= 1024 (ConvNeXt's
 * dwconv -> LayerNorm, vocos.py:489-496,511-518) (AMP_ERR_INVALID otherwise: run amp_dwconv + amp_layer_norm_c); dw_weight [C, 1, K], dw_bias [C] or NULL; columns t >= lens[b] of y are zero; y != x. */
int amp_dwconv_layer_norm_c(const float* x_dev, const float* dw_weight_dev, const float* dw_bias_dev, int K, int dilation,
                            const float* gamma_dev, const float* beta_dev, const int* lens_dev, int B, int C, int T, float eps,
                            int gelu, float* y_dev, void* stream);
/* amp_dwconv_layer_norm_c with ALL of the depthwise padding on the left: y[t] = act(LN(b + sum_j w[j] x[t - (K - 1) + j])), the causal
 * ConvNeXt block of DualCodec (model_codec/cnn.py:85-93: F.pad(x, (6, 0)) -> dwconv(padding = 0) -> LayerNorm) in one launch.  Covered:
 * K = 7, dilation 1, C <= 1024; anything else AMP_ERR_INVALID.  Same arguments, same tap order: bit-identical to amp_dwconv_layer_norm_c
 * run on a copy of x left-padded by 6 zeros and read at columns t + 3.  y != x. */
int amp_dwconv_layer_norm_c_causal(const float* x_dev, const float* dw_weight_dev, const float* dw_bias_dev, int K, int dilation,
                                   const float* gamma_dev, const float* beta_dev, const int* lens_dev, int B, int C, int T, float eps,
                                   int gelu, float* y_dev, void* stream);
/* The seam between DDSConv layers i and i + 1 (modules/flow/modules.py:63-70) in one launch:
 *     x_out = x + gelu(LN(y; gamma2, beta2))                    norms_2[i] on the 1 x 1 conv's output y, residual x
 *     z_out = gelu(LN(dwconv(x_out * mask); gamma1, beta1))     convs_sep[i+1] -> norms_1[i+1]
 * Same bits as amp_layer_norm_c (gelu, post = x) followed by amp_dwconv_layer_norm_c.  K = 3 and C <= 192, AMP_ERR_UNSUPPORTED
 * otherwise; z_out is zero beyond lens[b], x_out is not masked; the outputs must not alias the inputs. */
int amp_dds_seam(const float* y_dev, const float* x_dev, const float* gamma2_dev, const float* beta2_dev, float eps2,
                 const float* dw_weight_dev, const float* dw_bias_dev, int K, int dilation, const float* gamma1_dev, const float* beta1_dev,
                 float eps1, const int* lens_dev, int B, int C, int T, float* x_out_dev, float* z_out_dev, void* stream);
/* x[b, c, :] += cb[b, c]: the broadcast add of a length-1 condition, x + cond(g) (hifigan.py:426-427,
 * stochastic_duration_predictor.py:64-66). */
int amp_add_channel_bias(float* x_dev, const float* cb_dev, int B, int C, int T, void* stream);
/* MultiHeadAttention.attention for self-attention with windowed relative-position embeddings shared by the heads
 * (modules/transformer/attentions.py:232-272): q, k, v, out [B, H*dk, T]; emb_k, emb_v [2*window+1, dk]. */
int amp_rel_attention(const float* q_dev, const float* k_dev, const float* v_dev, const float* emb_k_dev,
                      const float* emb_v_dev, const int* lens_dev, int B, int H, int dk, int T, int window, float* out_dev,
                      void* stream);
/* The same with q / k / v given as slices of ONE tensor (the merged q|k|v projection [B, 3*H*dk, T]): element (b, c, t) of each
 * at ptr[b*qkv_batch_stride + c*T + t]; out stays [B, H*dk, T] dense. */
int amp_rel_attention_strided(const float* q_dev, const float* k_dev, const float* v_dev, long long qkv_batch_stride,
                              const float* emb_k_dev, const float* emb_v_dev, const int* lens_dev, int B, int H, int dk, int T,
                              int window, float* out_dev, void* stream);
/* 1 (default): blocks of 16 queries share the keys / values staged in LDS; 0: one workgroup per query (rounds 2-3).  Same bits. */
int amp_set_rel_attention_tiled(int on);
/* Depthwise dilated Conv1d of x * mask, padding (K*d - d)/2 (DDSConv.convs_sep, modules/flow/modules.py:46-56,63);
 * w [C, 1, K], bias [C] or NULL. */
int amp_dwconv(const float* x_dev, const float* w_dev, const float* bias_dev, const int* lens_dev, int B, int C, int T, int K,
               int dilation, float* y_dev, void* stream);
/* ConvFlow's spline step (modules/flow/modules.py:435-458 + modules/transformer/transforms.py:56-215): the piecewise
 * rational-quadratic transform with linear tails of one channel of z [B, 2, T] given h [B, 3*num_bins - 1, T] (masked
 * here), both channels * mask; flip_in / flip_out fold the neighbouring Flip layers (:315-321) in.  z_out != z.
 * PRECONDITION: both masks are 0 / 1 FACTORS: z and h must be finite in the columns t >= lens[b] too. */
int amp_spline_flow(const float* z_dev, const float* h_dev, const int* lens_dev, int B, int T, int num_bins,
                    int filter_channels, float tail_bound, int inverse, int flip_in, int flip_out, float* z_out_dev,
                    void* stream);
/* amp_spline_flow with ConvFlow's `proj` (modules/flow/modules.py:418,427: Conv1d(C, 3*num_bins - 1, 1)) evaluated inside: hc_dev [B, C, T] is
 * the DDSConv output, proj_w_dev [3*num_bins - 1, C] / proj_b_dev [3*num_bins - 1] (or NULL) the conv's parameters as stored, on the
 * device.  The projection is a plain fp32 dot product (not the f16x3 conv arithmetic).  C <= 256; AMP_ERR_UNSUPPORTED otherwise. */
int amp_spline_flow_proj(const float* z_dev, const float* hc_dev, const float* proj_w_dev, const float* proj_b_dev, const int* lens_dev,
                         int B, int C, int T, int num_bins, int filter_channels, float tail_bound, int inverse, int flip_in, int flip_out,
                         float* z_out_dev, void* stream);
/* ElementwiseAffine reverse: (x - m) * exp(-logs) * mask (modules/flow/modules.py:338-340); m, logs [C].
 * PRECONDITION: the mask is a 0 / 1 FACTOR: x must be finite in the columns t >= lens[b] too (the duration predictor hands it the
 * output of a spline step, which is the Gaussian draw times zero there). */
int amp_affine_reverse(const float* x_dev, const float* m_dev, const float* logs_dev, const int* lens_dev, int B, int C, int T,
                       float* y_dev, void* stream);
/* emb(tokens) * scale, transposed to [B, hidden, T] and masked (TextEncoder.forward vits.py:58-62); tokens int64 [B, T],
 * weight [n_vocab, hidden].  Token ids are clamped to [0, n_vocab) in every column, so the columns t >= lens[b] may hold any id;
 * the mask is a 0 / 1 FACTOR on a (finite) weight. */
int amp_embed_tokens(const long long* tokens_dev, const float* weight_dev, const int* lens_dev, int B, int T, int hidden,
                     int n_vocab, float scale, float* y_dev, void* stream);
/* The sum of N embedding look-ups, channel-first (FACodecRedecoder.forward / vq2emb, models/codec/ns3_codec/facodec.py:698-722,736-759):
 *     y[b, :, t] = ((init[b, :, t] + W_0[codes[0, b, t]]) + W_1[codes[1, b, t]]) + ...
 * codes_dev int64 [N, B, T]; tables / rows: HOST arrays of N device pointers W_n [rows[n], D] and their row counts, 1 <= N <= 8; init_dev
 * [B, D, T] or NULL; y_dev [B, D, T], not init_dev.  The fp32 adds run left to right -- the bits of torch's emb_0(c_0) + emb_1(c_1) + ...
 * transposed -- and with init = NULL the sum starts from the row of W_0 itself.  One launch; rows are gathered as contiguous segments along D
 * and transposed through LDS, y is stored along T.  An index outside [0, rows[n]) reads row 0 of its table instead (never out of bounds) and
 * sets *flag_dev, one zero-initialised 32-bit word on the device that the caller owns.  amp_embed_sum_check synchronises the stream, returns
 * AMP_ERR_INVALID if the flag was set since the last check, and clears it.  B and ceil(D / 64) <= 65535, else AMP_ERR_UNSUPPORTED. */
int amp_embed_sum_c(const long long* codes_dev, int N, const float* const* tables, const int* rows, int D, const float* init_dev, int B, int T,
                    float* y_dev, unsigned* flag_dev, void* stream);
int amp_embed_sum_check(unsigned* flag_dev, void* stream);
/* w_ceil = ceil(exp(logw) * mask * length_scale) [B, T], its running sum (int32 [B, T]) and y_len = max(sum, 1)
 * (vits.py:341-343, utils/util.py:633). */
int amp_durations(const float* logw_dev, const int* lens_dev, int B, int T, float length_scale, float* w_ceil_dev, int* cum_dev,
                  int* ylen_dev, void* stream);
/* out[b, :, y] = src[b, :, x(y)] along the monotonic path cum[x-1] <= y < cum[x] ( = generate_path(...) @ src,
 * utils/util.py:625-640, vits.py:345-353); attn_dev [B, 1, Ty, Tx] receives the path itself when not NULL. */
int amp_expand_path(const float* src_dev, const int* cum_dev, const int* xlens_dev, const int* ylens_dev, int B, int D, int Tx,
                    int Ty, float* out_dev, float* attn_dev, void* stream);
/* The same with src a channel slice of a wider tensor (m / logs = the halves of the text encoder's stats, vits.py:65): element
 * (b, d, x) at src_dev[b*src_batch_stride + d*Tx + x]. */
int amp_expand_path_strided(const float* src_dev, long long src_batch_stride, const int* cum_dev, const int* xlens_dev,
                            const int* ylens_dev, int B, int D, int Tx, int Ty, float* out_dev, float* attn_dev, void* stream);
/* z_p = m + noise * exp(logs) * noise_scale over n elements (vits.py:355). */
int amp_gauss_sample(const float* m_dev, const float* logs_dev, const float* noise_dev, size_t n, float noise_scale,
                     float* out_dev, void* stream);

/* Snake.forward / SnakeBeta.forward as a stand-alone element-wise op (modules/activation_functions/snake.py:51-61,
 * 110-122): y = x + sin(a x)^2 / (b + 1e-9) over [B, C, T]; alpha_dev / beta_dev: [C] on the device, beta_dev NULL
 * for Snake (b = a); logscale: a = exp(alpha), b = exp(beta). */
int amp_snake(const float* x_dev, int B, int C, int T, const float* alpha_dev, const float* beta_dev, int logscale,
              float* y_dev, void* stream);

/* fp32 waveform [B, L] (row stride wav_stride elements) -> signed 16-bit PCM [B, L] (row stride pcm_stride), on
 * the device, so the D2H copy and any gather move 2 bytes per sample instead of 4.  Replaces the host conversion
 * inside the reference's save_audio (utils/io.py:68-76 -> torchaudio.save(encoding="PCM_S", bits_per_sample=16);
 * torchaudio 2.0.2 + libsox 14.4.2 semantics: sample = x * 2^31 clamped and truncated to int32, then rounded
 * half-up to 16 bits with saturation).  lens_dev (samples per row, may be NULL) zeroes the tail of each row: the
 * crop `[: l * hop_size]` of models/vocoders/vocoder_inference.py:359.  Bit-exact against oracle/pcm16.py. */
int amp_wav_to_pcm16(const float* wav_dev, int B, int L, long long wav_stride, const int* lens_dev, int16_t* pcm_dev,
                     long long pcm_stride, void* stream);

/* Per-conv options (default 0).  PAD_REFLECT: columns outside the input mirror instead of reading zero, i.e.
 * nn.ReflectionPad1d(p) followed by an unpadded conv == this conv created with padding = p (MelGAN,
 * models/vocoders/gan/generator/melgan.py:39,56,92); needs p < T.  TANH: tanh on store (melgan.py:94). */
typedef enum amp_conv_option { AMP_CONV_OPT_PAD_REFLECT = 1, AMP_CONV_OPT_TANH = 2 } amp_conv_option;
int amp_conv_set_option(amp_conv* c, int option, int value);

/* One ResBlock1 iteration fused in a single kernel (hifigan.py:93-100):
 *     y = x + c2( leaky_relu( c1( leaky_relu(x, slope) ), slope ) )
 * c1: Conv1d(C, C, k, dilation d, 'same' padding), c2: Conv1d(C, C, k, dilation 1), both with bias, built
 * with amp_conv_create under AMP_PRECISION_F16X3.  Covered: C in {32, 64, 128}, k in {3, 5, 7, 11} and
 * (k-1)*d <= 64; anything else returns AMP_ERR_UNSUPPORTED (amp_gen_forward then runs the two convs).
 * y_dev must not alias x_dev. */
int amp_pair_forward(const amp_conv* c1, const amp_conv* c2, const float* x_dev, int B, int T, float slope,
                     float* y_dev, void* stream);

/* ResBlock1.forward (hifigan.py:93-100) in ONE launch:  for p < n_pairs:  x = x + c2[p](lrelu(c1[p](lrelu(x)))), on the
 * whole-resblock kernel (csrc/rb_f16x3.hip: x read once, y written once, the residual carried in registers).  Handles from
 * amp_conv_create as for amp_pair_forward (same C and k for all pairs, c1[p] dilated, c2[p] dilation 1, 'same' padding);
 * covered: C in {32, 64} with k in {3, 5, 7, 11}, C = 128 with k in {3, 5}, (k-1)/2 * dilation within the tile's guard columns (32;
 * 16 at C = 128), n_pairs <= 3, f16x3 arithmetic, under the shapes the current
 * amp_set_resblock_fusion mode admits -- otherwise AMP_ERR_UNSUPPORTED (run amp_pair_forward n_pairs times: the same bits).
 * y_dev must not alias x_dev. */
int amp_resblock_forward(const amp_conv* const* c1, const amp_conv* const* c2, int n_pairs, const float* x_dev, int B, int T,
                         float slope, float* y_dev, void* stream);
/* 0: generators run every ResBlock1 as fused pairs; 1 (default): the measured policy (whole-resblock kernel for the narrow
 * late stages when the launch fills the chip); 2: wherever the kernel is built, any grid; 3: as 2 with the four-wave
 * tiles (two workgroups per CU) at C = 32 (512 columns) and at C = 64, k <= 5 (256 columns).  Bit-identical results in every mode (tests/test_gpu_resblock.py); env AMP_RB_FUSION. */
int amp_set_resblock_fusion(int mode);
/* amp_version 160.  The whole-resblock kernel's tile has guard columns either side that stand for its unknown outside.  For the FIRST conv of a
 * launch the outside is known (x is in memory): with the guards holding the real staged x that conv keeps all its columns and a tile loses
 * (k-1)/2 * dilation fewer columns either side.  amp_set_rb_guards: -1 (default) the measured policy, 0 never, 1 wherever that reach fits the
 * guard; env AMP_RB_GUARDS.  A three-pair resblock runs as one to three launches chosen by a cost model (rounds of workgroups x convs + the
 * extra trip through memory); amp_set_rb_split_plan(n, counts) forces n launches of counts[i] pairs (sum 3), n = 0 gives the plan back; env
 * AMP_RB_SPLIT_PLAN="2,1".  Bit-identical results under every setting (tests/test_gpu_rb_guards.py).
 * amp_rb_launch_plan reports, without a device, the launches of a resblock (C, k, dilations) at (B, T) under the current switches: pairs,
 * gx (guards hold x), output columns per tile and tiles per item of each (arrays of 3).
 * amp_resblock_forward_ex is amp_resblock_forward walking that plan, with the MRF mode of the last launch (0: y = v, 1: y += v,
 * 2: y = (y + v) / div); tmp_dev: 2 * B * C * T floats of scratch, needed when the plan has more than one launch. */
int amp_set_rb_guards(int mode);
int amp_set_rb_split_plan(int n, const int* counts);
int amp_rb_launch_plan(int C, int k, const int* dilations, int n_pairs, int B, int T, int ragged, int* n_launches, int* pairs, int* gx,
                       int* out_columns, int* tiles_per_item);
int amp_resblock_forward_ex(const amp_conv* const* c1, const amp_conv* const* c2, int n_pairs, const float* x_dev, int B, int T, float slope,
                            float* y_dev, int mode, float div, float* tmp_dev, void* stream);
/* The n_kernels resblocks of a generator stage on CONCURRENT streams (they read the same stage tensor and only meet in the MRF mean,
 * hifigan.py:208-214 / bigvgan.py:320-327): -1 (default) while B * T <= 4096 mel frames -- small batches, whose launches do not
 * fill the chip and whose forward is a chain of ~50 dependent launches; 0 never; 1 always.  Only the launch of each resblock that
 * accumulates into the mean waits for the previous resblock's (an event) and keeps its `=` / `+=` / `(y + v) / n` form: bit-identical
 * results in every mode.  amp_gen_workspace_bytes accounts for the extra R / TMP buffers; the side streams fork from and join
 * `stream` by events (legal under stream capture).  They are created by the first uncaptured forward or by amp_gen_prepare_streams
 * -- a forward captured before either runs the sequential chain.  Not used while amp_gen_set_profiling is on.  Env AMP_RB_STREAMS. */
int amp_set_resblock_streams(int mode);
int amp_gen_prepare_streams(amp_gen* g);

/* AMPBlock1.forward of BigVGAN (bigvgan.py:137-146) in ONE launch:
 *     for p < n_pairs:  x = x + c2[p]( a[2p+1]( c1[p]( a[2p](x) ) ) ),   a[i] = Activation1d(Snake | SnakeBeta)
 * on the whole-AMPBlock kernel (csrc/ampb_f16x3.hip: x read once, y written once, the six anti-aliased activations
 * (act.py:31-36, resample.py:36-65, filter.py:92-99, snake.py:51-61) evaluated in registers between the convs).  Bit-identical
 * to running amp_antialias_snake / amp_conv_forward[_mrf] one by one (tests/test_gpu_ampblock.py).
 * Handles from amp_conv_create under AMP_PRECISION_F16X3: same C and k for all convs, c1[p] dilated, c2[p] dilation 1, 'same'
 * zero padding, with bias.  alpha_dev / beta_dev: [2 * n_pairs, C] per-channel parameters AS STORED (exp() applied when
 * logscale; beta_dev NULL -> Snake); filt_up_host / filt_down_host: the 12 filter taps shared by all activations.
 * mode 0: y = v;  1: y = y + v;  2: y = (y + v) / div  (the MRF accumulation of the generator, bigvgan.py:320-327).
 * Covered: C in {32, 64}, k in {3, 5, 7, 11}, (k-1)/2 * dilation <= 32, n_pairs <= 3, T % 4 == 0, under
 * the shapes the current amp_set_ampblock_fusion mode admits -- otherwise AMP_ERR_UNSUPPORTED.  y_dev must not alias x_dev.
 * Op-level convenience: synchronises the stream. */
int amp_ampblock_forward(const amp_conv* const* c1, const amp_conv* const* c2, int n_pairs, const float* alpha_dev,
                         const float* beta_dev, int logscale, const float* filt_up_host, const float* filt_down_host,
                         const float* x_dev, int B, int T, float* y_dev, int mode, float div, void* stream);
/* 0: BigVGAN generators run every AMPBlock as separate conv / activation launches; 1 (default): the whole-AMPBlock kernel
 * where it is built and the launch fills the chip; 2: wherever it is built, any grid; 3: as 2 with the four-wave 512-column
 * tiles at C = 32.  Bit-identical results in every mode; env AMP_AMPB_FUSION.  -1: back to the default. */
int amp_set_ampblock_fusion(int mode);

void amp_conv_destroy(amp_conv* c);

/* Frame-rate convs (short contraction, small grid: the convs around the VITS decoder) run on a kernel that stages the
 * whole K extent of its input tile at once (csrc/conv_small_f16x3.hip; same bits as the pipelined kernel).  0 keeps
 * them on the pipelined kernel -- an A/B and cross-check switch (no environment form since round 3). */
int amp_set_small_conv(int on);

/* Transposed convs and k = 3 / 7 / 11 convs whose GEMM rows are a multiple of 256 (ConvTranspose1d: Cout * stride) run, on grids
 * of 512+ workgroups, on the row-blocked kernel (csrc/conv_blk_f16x3.hip: 64 rows per wave, x staged once per 256 rows;
 * same bits as the pipelined kernel).  mode 0 keeps them on the pipelined kernel, 1 = one 16-channel chunk per staging
 * round, 2 = two where available, 3 = 2 + k = 7 / 11 on the A-fragment-ring form (default), -1 = back to
 * the default -- an A/B and cross-check switch. */
int amp_set_conv_blk(int mode);
/* Conv1d with 128 output rows (BigVGAN's unpaired AMPBlock convs at C = 128) on the row-blocked kernel, two waves along the columns: 1
 * (default) the measured policy (k = 7 / 11), 2 every tap count the kernel is built for, 0 all on the pipelined kernel.  Same bits in every
 * mode (an A/B and cross-check switch); -1: default. */
int amp_set_conv_blk_narrow(int on);

/* Convs with several row groups (more GEMM rows than one workgroup holds) launch with the row group as the fastest grid
 * index: the row groups of one x tile run back to back on one XCD and share its L2 copy of x (same bits; 1 = default).
 * 0 = the 2-D grid with the row group in blockIdx.y, -1 = back to the default (on) -- an A/B switch. */
int amp_set_conv_rg_fast(int on);

/* Ping-pong tile order: every other conv / fused-pair launch walks its tiles in descending order, starting on the part of its
 * input that the previous launch wrote last (same bits).  -1 = back to the default (on) -- an A/B switch. */
int amp_set_pingpong(int on);

/* ---- WN (modules/flow/modules.py:74-151), fused: two launches per layer ---- */

/* WN.in_layers[i] = Conv1d(H, 2H, k, dilation, padding) (modules.py:106-114) built for the gate epilogue: the kernel
 * forms fused_add_tanh_sigmoid_multiply (utils/util.py:602-609) in registers and writes [B, H, T].  weight_host
 * [2H, H, k] FOLDED (weight_norm applied), bias_host [2H].  Covered: H a multiple of 32 and <= 256, k in {1, 3, 5},
 * 'same' padding, (k-1)*dilation <= 64, f16x3 arithmetic; otherwise AMP_ERR_UNSUPPORTED (run the unfused ops).
 * The handle only runs inside amp_wn_forward. */
int amp_conv_create_gated(int hidden, int k, int dilation, int padding, const float* weight_host, const float* bias_host,
                          amp_conv** out);

/* WN.forward (modules/flow/modules.py:126-151) without the final `* x_mask`:
 *   for i: acts = tanh((in_i(x) + g_i)[:H]) * sigmoid((in_i(x) + g_i)[H:]);  rs = res_skip_i(acts)
 *          i < n-1: x = (x + rs[:H]) * mask, output += rs[H:];   i == n-1: output += rs
 * in_layers[i]: amp_conv_create_gated handles; res_skip_layers[i]: amp_conv_create 1x1 convs (H -> 2H, last H -> H).
 * x_dev [B, H, T] is the caller's working copy and is MODIFIED; cond_dev = cond_layer(g) [B, 2H*n_layers] (element
 * (b, r) at cond_dev[b*cond_batch_stride + r]) or NULL; lens_dev int32 [B] or NULL; acts_ws_dev scratch [B, H, T];
 * out_dev [B, H, T] (written, not read).  With lens_dev, columns t >= lens[b] of out_dev (and of x_dev) are UNSPECIFIED --
 * whole tiles beyond an utterance's end are skipped and never stored: ASSIGN zero there (amp_sequence_mask does, as
 * WN.forward's final `* x_mask` would), do not multiply what is left in them by a mask (0 * NaN). */
int amp_wn_forward(const amp_conv* const* in_layers, const amp_conv* const* res_skip_layers, int n_layers, float* x_dev,
                   const float* cond_dev, long long cond_batch_stride, const int32_t* lens_dev, int B, int T,
                   float* acts_ws_dev, float* out_dev, void* stream);

/* ---- VITS posterior encoder + flow (config 5): element-wise pieces between the convs ---- */

/* fused_add_tanh_sigmoid_multiply (utils/util.py:602-609) as called by WN.forward
 * (modules/flow/modules.py:141): out[b,c,t] = tanh(a[b,c,t] + g[b,c]) * sigmoid(a[b,c+H,t] + g[b,c+H]).
 * a_dev [B, 2H, T]; cond_dev: this layer's slice of cond_layer(g) (time-constant), element (b, c) at
 * cond_dev[b*cond_batch_stride + c], or NULL when g is None; out_dev [B, H, T]. */
int amp_wn_gate(const float* a_dev, const float* cond_dev, long long cond_batch_stride, float* out_dev, int B, int H,
                int T, void* stream);
/* WN residual/skip update (modules/flow/modules.py:144-151): not last: x = (x + rs[:, :H]) * mask,
 * out += rs[:, H:]; last: out += rs.  first != 0 starts `out` from zero (torch.zeros_like, :127).
 * lens_dev: int32 [B] valid lengths (sequence_mask, utils/util.py:618-622) or NULL for no mask.
 * PRECONDITION: the mask is a 0 / 1 FACTOR here, as in the reference: x and rs must be finite in the columns t >= lens[b] too (WN's
 * unfused path assigns zero to x beyond the lengths before its first layer and runs its convs densely, so they are); `out` is
 * not masked at all. */
int amp_wn_accumulate(float* x_dev, float* out_dev, const float* rs_dev, const int32_t* lens_dev, int B, int H, int T,
                      int first, int last, void* stream);
/* x[b, :, t >= lens[b]] = 0   (`* x_mask`, vits.py:147,149; modules/flow/modules.py:152,381,383) */
int amp_sequence_mask(float* x_dev, const int32_t* lens_dev, int B, int C, int T, void* stream);
/* Mean-only ResidualCouplingLayer update on the second half of x [B, 2h, T] in place
 * (modules/flow/modules.py:390-397): forward x1 = m + x1*mask; reverse x1 = (x1 - m)*mask. */
int amp_coupling_apply(float* x_dev, const float* m_dev, const int32_t* lens_dev, int B, int half_channels, int T,
                       int reverse, void* stream);
/* Flip.forward: torch.flip(x, [1]) (modules/flow/modules.py:314-321); y must not alias x. */
int amp_flip_channels(const float* x_dev, float* y_dev, int B, int C, int T, void* stream);
/* PosteriorEncoder sampling (models/tts/vits/vits.py:150-151): stats = [m ; logs] [B, 2C, T],
 * z = (m + eps * exp(logs)) * mask.
 * PRECONDITION: the mask is a 0 / 1 FACTOR: stats and eps must be finite in the columns t >= lens[b] too (PosteriorEncoder assigns
 * zero to stats there just before, and eps is a full Gaussian draw); z is then zero there. */
int amp_posterior_sample(const float* stats_dev, const float* eps_dev, const int32_t* lens_dev, float* z_dev, int B,
                         int C, int T, void* stream);

/* Activation1d(Snake|SnakeBeta) (modules/anti_aliasing/act.py:31-36; resample.py:36-45,62-65;
 * filter.py:92-99; snake.py:51-61,110-122), ratio 2, 12-tap filters.  alpha_dev/beta_dev: per-channel
 * parameters AS STORED (the kernel applies exp() when logscale); beta_dev NULL -> Snake.
 * filt_up_host/filt_down_host: the 12 filter taps.  x_dev [B, C, T] -> y_dev [B, C, T]. */
int amp_antialias_snake(const float* x_dev, int B, int C, int T, const float* alpha_dev, const float* beta_dev,
                        int logscale, const float* filt_up_host, const float* filt_down_host, float* y_dev,
                        void* stream);

/* Mel / STFT front end descriptor: cfg.preprocess.{sample_rate,n_fft,win_size,hop_size,n_mel,fmin,fmax}. */
typedef struct amp_mel_desc {
    uint32_t struct_size; /* sizeof(amp_mel_desc) AS THE CALLER WAS COMPILED (since amp_version 140): the library reads nothing
                            beyond it, so fields appended by later versions default to 0 / NULL for older consumers; a value
                            below the round-2 fields (up to mel_bands_dev) is refused with AMP_ERR_INVALID */
    int32_t n_fft;
    int32_t win_size;
    int32_t hop_size;
    int32_t n_mel;       /* 0 = linear spectrogram only */
    int32_t pad_mode;    /* 0: reflect-pad (n_fft-hop)/2, center=False (utils/mel.py:145-164);
                            1: reflect-pad n_fft/2 (utils/stft.py:152-165, TacotronSTFT) */
    float mag_eps;       /* added under the sqrt: 1e-9 (mel.py:166), 1e-6 (mel.py:99), 0 (stft.py:177) */
    float log_clip;      /* clamp before log: 1e-5 (mel.py:10-12); <=0 -> no log (raw mel / magnitude) */
    const int32_t* mel_bands_dev; /* optional, device: [n_mel][2] = first and one-past-last FFT bin with a non-zero
                            weight in each row of melbasis (librosa's triangular filters touch 2..40 of the 513 bins);
                            NULL = every row is summed over all bins.  Must cover every non-zero of the basis. */
    /* Optional sample-range report of utils/mel.py:21-24 ("min value is" / "max value is" when the audio leaves [-1, 1])
     * without a reduction pass of its own.  range_dev: device int32[3] = { bits of the smallest sample < -1 seen
     * (initialised to the bits of -1.0f = nothing seen), bits of the largest sample > 1 (initialised to +1.0f), range_seq };
     * the kernel folds the samples it reads anyway into the first two (atomic max of the int bits: monotone for both) and
     * stores range_seq into the third.  range_host (pinned host memory, 3 x int32): the call enqueues a copy of the three
     * words behind the kernel; the caller knows it has landed when word 2 equals range_seq.  range_reset_dev: another
     * int32[3] the kernel re-initialises for a LATER call (a ring of slots then needs no reset launch).  NULL = off. */
    int32_t* range_dev;
    int32_t* range_host;
    int32_t* range_reset_dev;
    int32_t range_seq;
} amp_mel_desc;

/* One-time set-up of the n_fft = 1024 front-end kernel on the CURRENT device (thread-safe, idempotent, blocking): call it
 * before capturing a stream that contains amp_mel_forward.  Without it the first forward does the same lazily. */
int amp_mel_init(void);
/* Number of frames produced for L samples. */
int amp_mel_num_frames(const amp_mel_desc* d, int L);
/* Replaces extract_mel_features / mel_spectrogram_torch / extract_linear_features (utils/mel.py:20-170)
 * and TacotronSTFT.mel_spectrogram (utils/stft.py:259-278).
 * wav_dev [B, L]; window_dev [n_fft] (already centre-padded to n_fft); melbasis_dev [n_mel, n_fft/2+1]
 * (may be NULL when n_mel == 0).  Outputs (any may be NULL): mel_dev [B, n_mel, F] (log-mel),
 * mag_dev [B, n_fft/2+1, F] (magnitude), re_dev/im_dev [B, n_fft/2+1, F].
 * The first n_fft = 1024 call on a device sets the kernel up (a 4.5-KB twiddle table, uploaded with a blocking copy under a
 * lock): inside a stream capture that first call is refused with AMP_ERR_STATE -- call amp_mel_init() (or one forward) first.
 * COST by transform length (64 utterances of 65 536 samples, one MI355X): n_fft 1024 / 2048 / 512 / 1920 run one WAVE per frame (register butterflies,
 * 0.040 / 0.051 / 0.053 / 0.103 ms); other powers of two and lengths whose prime factors are <= 13 run one WORKGROUP per frame (about 0.4-1 ms); a
 * prime factor p > 13 adds a run-time radix pass of n_fft * p complex multiply-adds per frame, so a PRIME n_fft is a direct O(n_fft^2) DFT (4093: 16.7 M
 * per frame, three orders of magnitude slower per sample than 1024) -- accepted because torch.stft accepts it, not because it is a sensible choice. */
int amp_mel_forward(const amp_mel_desc* d, const float* wav_dev, int B, int L, const float* window_dev,
                    const float* melbasis_dev, float* mel_dev, float* mag_dev, float* re_dev, float* im_dev,
                    void* stream);

/* Ragged batch of the same: row b of wav_dev [B, L] holds lens_dev[b] <= L samples (int32, device), zero-padded.
 * Every utterance is reflect-padded at ITS OWN end and fills frames [0, amp_mel_num_frames(d, lens[b])) of its
 * output rows -- identical to running it alone (what the reference's one-file-at-a-time feature extraction,
 * processors/acoustic_extractor.py:376-403, computes); later frames of a row are left unwritten.
 * ZERO-FRAME ROWS: a row with lens[b] <= the reflection padding, or with lens[b] + 2 * padding < n_fft (possible with
 * pad_mode 0 whenever hop > n_fft / 3: padding < lens[b] < hop), has amp_mel_num_frames(d, lens[b]) == 0 frames: none of
 * its samples is read and none of its output rows is written. */
int amp_mel_forward_ragged(const amp_mel_desc* d, const float* wav_dev, const int32_t* lens_dev, int B, int L,
                           const float* window_dev, const float* melbasis_dev, float* mel_dev, float* mag_dev,
                           float* re_dev, float* im_dev, void* stream);

/* Backward of amp_mel_forward for the training-time mel loss (models/vocoders/gan/gan_vocoder_trainer.py:387-392:
 * 45 * L1(extract_mel_features(y_gt), extract_mel_features(y_pred)) differentiated w.r.t. y_pred).  Inputs are what a
 * forward with log_clip <= 0 returns for the same audio -- mel_linear_dev [B, n_mel, F] (mel energies BEFORE the log),
 * mag_dev / re_dev / im_dev [B, n_fft/2+1, F] -- plus grad_logmel_dev [B, n_mel, F] = d loss / d log(max(mel,
 * d->log_clip)) (d->log_clip <= 0: the gradient w.r.t. the linear mel).  Output grad_wav_dev [B, L].
 * spec_ws_dev: scratch of 2 * B * (n_fft/2+1) * F floats, frames_ws_dev: B * F * n_fft floats.  lens_dev as in
 * amp_mel_forward_ragged (NULL = full rows): row b reads frames [0, amp_mel_num_frames(d, lens[b])) of its inputs only,
 * its gradient is 0 from column lens[b] on, and a zero-frame row (see amp_mel_forward_ragged) gets an all-zero gradient. */
int amp_mel_backward(const amp_mel_desc* d, const int32_t* lens_dev, int B, int L, const float* window_dev,
                     const float* melbasis_dev, const float* mel_linear_dev, const float* mag_dev, const float* re_dev,
                     const float* im_dev, const float* grad_logmel_dev, float* spec_ws_dev, float* frames_ws_dev,
                     float* grad_wav_dev, void* stream);

/* Replaces STFT.inverse (utils/stft.py:183-222; used by STFT.forward and griffin_lim :78-95): magnitude and
 * phase [B, n_fft/2+1, F] -> waveform [B, hop*(F-1) + (n_fft & 1)] (overlap-add of the windowed inverse FFTs, divided by the
 * window-sum-square envelope where it exceeds float32 tiny, times n_fft/hop, floor(n_fft/2) cropped per side).
 * window_dev [n_fft]; wss_dev [n_fft + hop*(F-1)] = window_sumsquare (stft.py:19-75) as float32;
 * frames_ws_dev: scratch of B*F*n_fft floats. */
int amp_istft_forward(const amp_mel_desc* d, const float* mag_dev, const float* phase_dev, int B, int F,
                      const float* window_dev, const float* wss_dev, float* frames_ws_dev, float* wav_dev, void* stream);

/* APNet's ISTFT with "same" padding (apnet.py:16-101): complex spectrogram (re, im) [B, n_fft/2+1, F] ->
 * waveform [B, F * hop]: overlap-add of irfft(spec) * window, cropped by (win - hop)/2 per side, divided by the
 * window envelope.  envelope_dev [hop*(F-1) + win] = overlap-added window^2 (uncropped); needs win_size == n_fft. */
int amp_istft_same(const amp_mel_desc* d, const float* re_dev, const float* im_dev, int B, int F, const float* window_dev,
                   const float* envelope_dev, float* frames_ws_dev, float* wav_dev, void* stream);

/* Vocos's ISTFT head (vocos.py:346-359 + ISTFT "same", :84-167) in one call: reads the head Linear's output
 * head [B, n_fft + 2, F] (batch stride head_batch_stride elements, 0 = dense) in place -- rows [0, n_fft/2+1) are log-magnitude,
 * rows [n_fft/2+1, n_fft+2) phase -- forms min(exp(m), mag_clip) * (cos p, sin p) while loading each frame (exp overflowing to
 * inf clips to mag_clip; full-range sincos) and then runs amp_istft_same's overlap-add and envelope division -> wav [B, F * hop].
 * Same window / envelope / scratch contract as amp_istft_same. */
int amp_istft_same_polar(const amp_mel_desc* d, const float* head_dev, long long head_batch_stride, int B, int F, float mag_clip,
                         const float* window_dev, const float* envelope_dev, float* frames_ws_dev, float* wav_dev, void* stream);

/* ---- pointwise GEMM (csrc/pw_f16x3.hip): nn.Linear along the channel axis of [B, C, T] activations, Vocos's
 * ConvNeXtBlock.pwconv1 / pwconv2 and ISTFTHead.out (vocos.py:511-526,346).  y[b] = epi(W x[b] + bias) with
 *   AMP_PW_BIAS        y = Wx + b
 *   AMP_PW_BIAS_GELU   y = gelu(Wx + b)                (exact erf GELU, nn.GELU())
 *   AMP_PW_SCALE_RES   y = res + gamma (.) (Wx + b)    (per-row gamma [cout]; res [B, cout, T] may alias y)
 * weight_host [cout, cin] as nn.Linear.weight stores it, bias_host [cout] or NULL.  The arithmetic is fixed when the handle is
 * created (amp_set_precision): f16x3 runs the split-f16 MFMA kernel (its operand range is guarded: amp_range_check reports
 * AMP_ERR_RANGE); AMP_PRECISION_F32 runs the exact-f32 k = 1 conv and one element-wise epilogue.  x [B, cin, T] with batch stride
 * x_batch_stride elements (0 = dense), y [B, cout, T] dense; x must not overlap y.  Deterministic.  A handle holds no mutable
 * state: several streams may use one (the fp32 route with y == res takes a stream-ordered temporary, hipMallocAsync / hipFreeAsync). ---- */
typedef struct amp_pw amp_pw;
typedef enum amp_pw_epilogue { AMP_PW_BIAS = 0, AMP_PW_BIAS_GELU = 1, AMP_PW_SCALE_RES = 2 } amp_pw_epilogue;
int amp_pw_create(int cin, int cout, const float* weight_host, const float* bias_host, amp_pw** out);
int amp_pw_forward(const amp_pw* p, const float* x_dev, long long x_batch_stride, int B, int T, int epilogue,
                   const float* gamma_dev, const float* res_dev, float* y_dev, void* stream);
/* the precision the handle was created with (AMP_PRECISION_*), -1 for NULL */
int amp_pw_precision(const amp_pw* p);
void amp_pw_destroy(amp_pw* p);

/* ---- DiffWave (csrc/diffwave.hip, csrc/dw_layer_f16x3.hip): models/vocoders/diffusion/diffwave/diffwave.py:127-179 and one step of the
 * sampler of models/vocoders/diffusion/diffusion_vocoder_inference.py:55-71.  L = F * upsample0 * upsample1 samples per item.
 *   amp_dw_create / amp_dw_set_weight / amp_dw_finalize: weights under the reference's state_dict keys (flattened fp32, `count`
 *     elements), plus the non-persistent buffer "diffusion_embedding.embedding" [max_steps, 128].  Refused: residual_channels not a
 *     multiple of 32 or above 128, odd upsample factors.  The arithmetic is taken from amp_set_precision at creation;
 *     amp_dw_set_precision switches a handle later (both weight forms are kept: the sampler repeats an out-of-range call in fp32).
 *   amp_dw_condition: SpectrogramUpsampler, mel [B, n_mel, F] -> cond [B, n_mel, L]; once per utterance.
 *   amp_dw_forward: eps [B, L] = DiffWave.forward(audio [B, L], steps, mel) from cond; steps_dev holds n_steps = 1 or B FLOAT step
 *     values on the device (an integer step is its float value; fractional steps interpolate the embedding table).
 *   amp_dw_sample_step: audio = clamp(c1 * (audio - c2 * eps(audio, step)) + sigma * noise, -1, 1) in place; noise_dev NULL = none.
 *   op level (what forward chains, bit for bit): amp_dw_embed -> dconst [n_steps, N, C] (diffusion_projection of every layer),
 *     amp_dw_input -> relu(input_projection(audio)) [B, C, L], amp_dw_layer (one ResidualBlock, diffwave.py:112-124: dconst_dev points
 *     at the layer's [C] row, dconst_batch_stride elements between items, 0 = shared; skip_in_dev NULL for the first layer, may equal
 *     skip_out_dev; x_out_dev must not overlap x_dev), amp_dw_tail -> eps [B, L] from the skip sum.
 * Every launch goes to `stream`; no allocation, no synchronisation.  ws_dev: amp_dw_workspace_bytes(B, F) bytes.  Under f16x3 the layer
 * kernel feeds the op-level range flag (amp_range_check).  Deterministic; a batch row does not depend on the rest of the batch. ---- */
typedef struct amp_dw amp_dw;
typedef struct amp_dw_desc {
    int32_t residual_channels;      /* cfg.model.diffwave.residual_channels */
    int32_t residual_layers;
    int32_t dilation_cycle_length;
    int32_t n_mel;                  /* cfg.preprocess.n_mel */
    int32_t upsample0, upsample1;   /* cfg.model.diffwave.upsample_factors */
    int32_t max_steps;              /* len(noise_schedule) */
} amp_dw_desc;
int amp_dw_create(const amp_dw_desc* desc, amp_dw** out);
int amp_dw_set_weight(amp_dw* h, const char* key, const float* data_host, long long count);
int amp_dw_finalize(amp_dw* h);
int amp_dw_precision(const amp_dw* h);
int amp_dw_set_precision(amp_dw* h, int precision);
size_t amp_dw_workspace_bytes(const amp_dw* h, int B, int F);
int amp_dw_condition(const amp_dw* h, const float* mel_dev, int B, int F, float* cond_dev, void* ws_dev, size_t ws_bytes, void* stream);
int amp_dw_embed(const amp_dw* h, const float* steps_dev, int n_steps, float* dconst_dev, void* stream);
int amp_dw_input(const amp_dw* h, const float* audio_dev, int B, int L, float* x_dev, void* stream);
int amp_dw_layer(const amp_dw* h, int layer, const float* x_dev, const float* cond_dev, const float* dconst_dev, long long dconst_batch_stride,
                 const float* skip_in_dev, float* x_out_dev, float* skip_out_dev, int B, int L, void* stream);
int amp_dw_tail(const amp_dw* h, const float* skip_dev, int B, int L, float* eps_dev, void* stream);
int amp_dw_forward(const amp_dw* h, const float* audio_dev, int L, const float* steps_dev, int n_steps, const float* cond_dev, int B, int F,
                   float* eps_dev, void* ws_dev, size_t ws_bytes, void* stream);
int amp_dw_sample_step(const amp_dw* h, float* audio_dev, int L, float step, float c1, float c2, float sigma, const float* noise_dev,
                       const float* cond_dev, int B, int F, void* ws_dev, size_t ws_bytes, void* stream);
void amp_dw_destroy(amp_dw* h);

/* ---- Amphion acoustic codec (models/codec/amphion_codec/codec.py, quantize/): what MaskGCT builds as CodecEncoder + CodecDecoder ---- */

/* Residual factorized VQ in eval mode (csrc/fvq.hip; quantize/residual_vq.py:68-152, factorized_vector_quantize.py:52-127), exact fp32.
 * amp_fvq_create: per level l < num_quantizers the FOLDED in_project [d, D] + bias [d], codebook [K, d], FOLDED out_project [D, d] + bias [D],
 *   as arrays of num_quantizers host pointers; the four projection arrays are all NULL when input_dim == codebook_dim (nn.Identity).
 *   Covered: D <= 1024, d <= 32, K <= 16384, N <= 32; anything else AMP_ERR_UNSUPPORTED.  The arguments are judged on the host, before a
 *   device is asked for: a refusal reads the same with or without one.
 * amp_fvq_encode = ResidualVQ.forward: z [B, D, T] -> codes int64 [n_quantizers, B, T] and (zq_dev not NULL) quantized_out [B, D, T], the sum
 *   of the levels' z_q, and (all_zq_dev not NULL) every level's z_q [n_quantizers, B, D, T] (all_quantized); ONE launch for all levels, the residual stays on chip.  Equal distances resolve to the LOWEST index, as
 *   (-dist).max(1)[1] does.  The distance keeps the reference's expression and order, (sum e^2 - 2 e.c) + sum c^2 on normalised operands.
 * amp_fvq_decode = ResidualVQ.vq2emb: codes -> out [B, D, T].  An index outside [0, K) reads row 0 instead (never out of bounds) and sets a
 *   device flag of the handle; amp_fvq_check synchronises `stream`, returns AMP_ERR_INVALID if that happened since the last check, and clears it
 *   (the op-level counterpart of amp_range_check).
 * No allocation and no synchronisation in encode / decode; deterministic; a frame never depends on what it is batched with. */
typedef struct amp_fvq amp_fvq;
int amp_fvq_create(int input_dim, int codebook_dim, int codebook_size, int num_quantizers, int use_l2_normalize,
                   const float* const* in_w_host, const float* const* in_b_host, const float* const* codebook_host,
                   const float* const* out_w_host, const float* const* out_b_host, amp_fvq** out);
int amp_fvq_encode(const amp_fvq* h, const float* z_dev, int B, int T, int n_quantizers, long long* codes_dev, float* zq_dev, float* all_zq_dev,
                   void* stream);
int amp_fvq_decode(const amp_fvq* h, const long long* codes_dev, int n_quantizers, int B, int T, float* out_dev, void* stream);
int amp_fvq_check(amp_fvq* h, void* stream);
void amp_fvq_destroy(amp_fvq* h);
/* The same two launches with DualCodec's DAC.encode / DAC.decode_from_codes folded in (model_codec/dac_model.py:301-312,319-320).
 * amp_fvq_encode_ex: z is read as columns [0, T) of a [B, D, z_row_stride] tensor (z_row_stride >= T, else AMP_ERR_INVALID: the crop
 *   z[..., :T]); sub_dev [B, D, T] not NULL: the residual starts as z - sub and zq_dev receives (sum of the levels' z_q) + sub; latents_dev
 *   [B, n_quantizers * d, T] not NULL receives every level's z_e = in_project(residual) (torch.cat(latents, 1)); all_zq_dev as in
 *   amp_fvq_encode (level 0 = z_q_1).  sub must not alias zq.  With sub_dev = latents_dev = NULL and z_row_stride = T it IS amp_fvq_encode;
 *   with sub_dev set, codes / zq are bit for bit those of (z[..., :T] - sub) -> amp_fvq_encode -> (zq + sub) done as separate fp32 passes.
 * amp_fvq_decode_add: out = amp_fvq_decode(codes) + add (add_dev [B, D, T]; NULL: amp_fvq_decode itself), bit for bit the separate add. */
int amp_fvq_encode_ex(const amp_fvq* h, const float* z_dev, long long z_row_stride, const float* sub_dev, int B, int T, int n_quantizers,
                      long long* codes_dev, float* zq_dev, float* all_zq_dev, float* latents_dev, void* stream);
int amp_fvq_decode_add(const amp_fvq* h, const long long* codes_dev, int n_quantizers, int B, int T, const float* add_dev, float* out_dev,
                       void* stream);

/* The feature preparation in front of DualCodec's semantic branch (infer/dualcodec/inference_with_semantic.py:155-164,232):
 * hidden [B, T, C] time-major -> out [B, C, floor(T / factor)] = avg_pool1d(((hidden - mean) / std).transpose(1, 2), factor, factor).
 * mean_dev / std_dev [C]; either may be NULL to skip that step.  fp32 in this order per output element: subtract, divide, the `factor`
 * terms summed in ascending time order, then times 1 / factor.  The last T mod factor frames are not read.  factor >= 1; T < factor is
 * AMP_ERR_INVALID; B or ceil(C / 64) beyond 65535 AMP_ERR_UNSUPPORTED.  out must not alias hidden. */
int amp_semantic_prepare(const float* hidden_dev, const float* mean_dev, const float* std_dev, int B, int T, int C, int factor, float* out_dev,
                         void* stream);

/* ResidualUnit of the codec encoder (codec.py:60-76): y = x + conv1x1(snake_2(conv7(snake_1(x)))), Snake1d as codec.py:34-39
 * (x + (alpha + 1e-9)^-1 sin^2(alpha x)), conv7 = Conv1d(C, C, 7, dilation, padding 3 * dilation).  alpha*_host [C], w1_host [C, C, 7] and
 * w2_host [C, C, 1] FOLDED, biases [C].  The fused launch (csrc/codec_unit_f16x3.hip) is built for AMP_PRECISION_F16X3 with C % 32 == 0, C <= 192 and
 * dilation <= 9 and needs no workspace; the default policy uses it up to C = 96, where it is the faster route (amp_codec_unit_fused returns 1;
 * amp_set_codec_unit_fusion(1) uses it wherever it is built).  Otherwise -- wider units, and every unit under AMP_PRECISION_F32 -- the handle
 * runs amp_snake -> conv -> amp_snake -> conv (+ residual) on the existing kernels with a workspace of amp_codec_unit_workspace_bytes (two
 * [B, C, T] tensors).  The f16x3 forms feed the op-level range flag (amp_range_check).
 * y_dev must not alias x_dev. */
typedef struct amp_codec_unit amp_codec_unit;
int amp_codec_unit_create(int channels, int dilation, const float* alpha1_host, const float* w1_host, const float* b1_host, const float* alpha2_host,
                          const float* w2_host, const float* b2_host, amp_codec_unit** out);
int amp_codec_unit_fused(const amp_codec_unit* h);
/* Which route handles created AFTER the call take: -1 (default) the measured policy, 0 the four launches everywhere, 1 the fused launch wherever
 * it is built -- an A/B switch for tools/codec_bench.py and the tests. */
int amp_set_codec_unit_fusion(int mode);
size_t amp_codec_unit_workspace_bytes(const amp_codec_unit* h, int B, int T);
int amp_codec_unit_forward(const amp_codec_unit* h, const float* x_dev, int B, int T, float* y_dev, void* ws_dev, size_t ws_bytes, void* stream);
void amp_codec_unit_destroy(amp_codec_unit* h);

/* The strided down-sampling conv of EncoderBlock (codec.py:86-93): Conv1d(cin, cout, k = 2 * stride, stride, padding), optionally preceded by
 * Snake1d (alpha_dev [cin] on the device, NULL = none).  amp_conv_create keeps refusing strided convs; this entry runs one as a small
 * kernel that applies the activation and folds stride and padding into the channel axis ([B, cin, T] -> [B, cin * stride, T_out + 1], in
 * the workspace) followed by a k = 2 stride-1 conv on the implicit-GEMM kernels with the weight re-indexed at create time.
 * T_out = floor((T + 2 padding - 2 stride) / stride) + 1 (amp_sconv_out_len); T need not be a multiple of the stride.  weight_host
 * [cout, cin, 2 * stride] FOLDED.  x [B, cin, T] -> y [B, cout, T_out]; ws_dev: amp_sconv_workspace_bytes(h, B, T) bytes.
 * Grid limit: B * cin * ceil((T_out + 1) * stride / 256) < 2^31, else AMP_ERR_UNSUPPORTED. */
typedef struct amp_sconv amp_sconv;
int amp_sconv_create(int cin, int cout, int stride, int padding, const float* weight_host, const float* bias_host, amp_sconv** out);
int amp_sconv_out_len(const amp_sconv* h, int T);
size_t amp_sconv_workspace_bytes(const amp_sconv* h, int B, int T);
int amp_sconv_forward(const amp_sconv* h, const float* x_dev, int B, int T, const float* alpha_dev, void* ws_dev, size_t ws_bytes, float* y_dev,
                      void* stream);
void amp_sconv_destroy(amp_sconv* h);

/* The up-sampling step of the DAC-style decoder blocks (codec.py:146-165; DualCodec model_codec/dac_model.py:129-146):
 * ConvTranspose1d(cin, cout, k = 2 * stride, stride, padding, output_padding), optionally preceded by Snake1d (alpha_dev [cin] on the device,
 * NULL = none).  weight_host [cin, cout, 2 * stride] FOLDED (the weight-norm of a ConvTranspose1d is over dim 0 = cin), bias_host [cout] or NULL.
 * x [B, cin, T] -> y [B, cout, T_out], T_out = (T - 1) * stride - 2 * padding + 2 * stride + output_padding (amp_tconv_out_len).
 * output_padding < stride (else AMP_ERR_INVALID) and output_padding <= padding (else AMP_ERR_UNSUPPORTED: it lengthens T_out only, the column
 * of input position T is the last either route computes); the reference's blocks have padding ceil(stride / 2), output_padding stride % 2.
 * The fused launch (csrc/tconv_f16x3.hip: activation, both polyphase taps and the scatter in one kernel, no workspace) is built for
 * AMP_PRECISION_F16X3 with cin % 32 == 0, cin <= 384 and 2 <= stride <= 8, any cout; the default policy uses it wherever it is built
 * (amp_tconv_fused returns 1; the A/B measurement that could narrow this is in DESIGN.md 12).  Otherwise -- wider inputs, other strides, and every handle under AMP_PRECISION_F32 -- the
 * handle runs amp_snake -> the polyphase transposed conv of amp_conv_create(transposed = 1, ...) (bit for bit that sequence when
 * output_padding == 0) with a workspace of amp_tconv_workspace_bytes (one [B, cin, T] tensor; unused when alpha_dev is NULL).  The f16x3 forms
 * feed the op-level range flag (amp_range_check).  Limits at forward: T_out <= 0 is AMP_ERR_INVALID; T_out > 2^30, or a fused grid of
 * B * ceil((T + 1) / 64) >= 2^31 workgroups, AMP_ERR_UNSUPPORTED.  y_dev must not alias x_dev.  Deterministic; an item never depends on its batch. */
typedef struct amp_tconv amp_tconv;
int amp_tconv_create(int cin, int cout, int stride, int padding, int output_padding, const float* weight_host, const float* bias_host,
                     amp_tconv** out);
int amp_tconv_out_len(const amp_tconv* h, int T);
int amp_tconv_fused(const amp_tconv* h);
/* Which route handles created AFTER the call take: -1 (default) the policy above, 0 the two launches everywhere, 1 the fused launch wherever it
 * is built -- an A/B switch for tools/dac_bench.py and the tests. */
int amp_set_tconv_fusion(int mode);
size_t amp_tconv_workspace_bytes(const amp_tconv* h, int B, int T);
int amp_tconv_forward(const amp_tconv* h, const float* x_dev, int B, int T, const float* alpha_dev, void* ws_dev, size_t ws_bytes, float* y_dev,
                      void* stream);
void amp_tconv_destroy(amp_tconv* h);

/* ResidualUnit of FACodec (models/codec/ns3_codec/facodec.py): y = x + conv1x1(A2(conv7(A1(x)))) with A = Activation1d(Snake | SnakeBeta),
 * BigVGAN's anti-aliased activation (2x up-sampling FIR -> Snake -> 2x down-sampling FIR, 12 taps each, replicate padding at the item's
 * ends: amp_antialias_snake), conv7 = Conv1d(C, C, 7, dilation, padding 3 * dilation).  alpha*_host / beta*_host [C] as stored (beta NULL = plain
 * Snake; logscale != 0: both are exponents), w1_host [C, C, 7] and w2_host [C, C, 1] FOLDED, biases [C], filt_up12 / filt_down12 the two 12-tap
 * filters.  The fused launch (csrc/aa_unit_f16x3.hip) is built for AMP_PRECISION_F16X3 with C % 32 == 0, C <= 128 and dilation <= 9 and needs
 * no workspace; amp_aa_unit_fused tells which route a handle took.  Otherwise -- other widths, and every unit under AMP_PRECISION_F32 -- the
 * handle runs act1d -> conv -> act1d -> conv (+ residual) on the existing kernels, bit for bit amp_antialias_snake / amp_conv_forward /
 * amp_antialias_snake / amp_conv_forward_mrf(res = x), with a workspace of amp_aa_unit_workspace_bytes (two [B, C, T] tensors).  The f16x3 forms
 * feed the op-level range flag (amp_range_check).  Fused limits: T <= 2^29 and B * ceil(T / 54) < 2^31, else AMP_ERR_UNSUPPORTED.
 * y_dev must not alias x_dev.  No allocation, no synchronisation in forward; deterministic; an item never depends on its batch. */
typedef struct amp_aa_unit amp_aa_unit;
int amp_aa_unit_create(int channels, int dilation, const float* alpha1_host, const float* beta1_host, const float* w1_host, const float* b1_host,
                       const float* alpha2_host, const float* beta2_host, const float* w2_host, const float* b2_host, int logscale,
                       const float* filt_up12_host, const float* filt_down12_host, amp_aa_unit** out);
int amp_aa_unit_fused(const amp_aa_unit* h);
/* Which route handles created AFTER the call take: -1 (default) the measured policy, 0 the four launches everywhere, 1 the
 * fused launch wherever it is built -- an A/B switch for tools/facodec_bench.py and the tests. */
int amp_set_aa_unit_fusion(int mode);
size_t amp_aa_unit_workspace_bytes(const amp_aa_unit* h, int B, int T);
int amp_aa_unit_forward(const amp_aa_unit* h, const float* x_dev, int B, int T, float* y_dev, void* ws_dev, size_t ws_bytes, void* stream);
void amp_aa_unit_destroy(amp_aa_unit* h);

/* ---- SpeechTokenizer (models/codec/speechtokenizer/): SEANet stacks, LSTM, Euclidean residual VQ ---- */

/* The staging pass in front of every SEANet conv (csrc/seanet.hip; modules/conv.py:97-119): y[b, c, j] = act(x[b, c, src(j)]) for
 * j in [0, pad_left + T + pad_right).  act is ELU (v > 0 ? v : alpha * expm1(v)) when `elu` != 0, else the identity.  src is
 * F.pad(mode = "reflect") with pad1d's small-input rule: when T <= max(pad_left, pad_right) the row is first zero-extended on the right to
 * max_pad + 1 samples, then reflected, and the extension is cropped again.  With zero pads it is the element-wise ELU (y may then alias x).
 * x and y may have any 4-byte alignment (the 16-byte accesses are taken where the addresses allow).  The convs themselves stay on amp_conv_* / amp_sconv_* / amp_tconv_*, fed the padded tensor with padding = 0.  Exact fp32, one pass.
 * pad_* < 0, B / C / T <= 0 or NULL pointers: AMP_ERR_INVALID; T_out > 2^30 or more than 2^31 - 1 workgroups: AMP_ERR_UNSUPPORTED.  The
 * arguments are judged on the host alone: no device is asked for before the launch. */
int amp_elu_pad(const float* x_dev, int B, int C, int T, int pad_left, int pad_right, int elu, float alpha, float* y_dev, void* stream);

/* nn.LSTM in eval mode inside SLSTM (csrc/lstm.hip; modules/lstm.py:18-46), in the conv layout on both sides: x [B, input_size, T] ->
 * y [B, ndir * hidden, T], ndir = 2 when bidirectional (forward half first, as nn.LSTM concatenates).  Zero initial state, gate order i, f, g, o.
 * amp_lstm_create: the four arrays hold num_layers * ndir HOST pointers in nn.LSTM's own order (l0, l0_reverse, l1, ..): weight_ih
 *   [4 hidden, input_size] (layers >= 1: [4 hidden, ndir * hidden]), weight_hh [4 hidden, hidden], bias_ih / bias_hh [4 hidden].  skip != 0 folds
 *   SLSTM's y + x (x repeated over both halves when bidirectional) into the last layer's store and needs input_size == hidden (else
 *   AMP_ERR_INVALID).  Covered: hidden <= 1024, input_size <= 2048, num_layers <= 4; anything else AMP_ERR_UNSUPPORTED.  The arguments are judged
 *   on the host before a device is asked for.
 * amp_lstm_forward: per layer ONE pointwise GEMM Gx = W_ih x + (b_ih + b_hh) for all T and both directions (the arithmetic the handle was created
 *   under: f16x3, which feeds the op-level range flag, or exact fp32 under AMP_PRECISION_F32), then the recurrence.
 * amp_lstm_recur: the recurrence of one layer alone, exact fp32: gx [B, ndir * 4 hidden, T] (per direction the rows of i, f, g, o) ->
 *   y [B, ndir * hidden, T]; skip_dev [B, hidden, T] or NULL is added at the store.  One launch per time step, enqueued back to back on `stream`;
 *   both directions share a grid.  ws_dev: at least amp_lstm_workspace_bytes(h, B, T) bytes, 16-byte aligned (else AMP_ERR_INVALID; the state lives at its start).
 * No allocation and no synchronisation in forward / recur; deterministic; an item's bits do not depend on what it is batched with.
 * y must not alias x. */
typedef struct amp_lstm amp_lstm;
int amp_lstm_create(int input_size, int hidden, int num_layers, int bidirectional, int skip, const float* const* w_ih_host,
                    const float* const* w_hh_host, const float* const* b_ih_host, const float* const* b_hh_host, amp_lstm** out);
size_t amp_lstm_workspace_bytes(const amp_lstm* h, int B, int T);
int amp_lstm_out_channels(const amp_lstm* h);
int amp_lstm_forward(const amp_lstm* h, const float* x_dev, int B, int T, float* y_dev, void* ws_dev, size_t ws_bytes, void* stream);
int amp_lstm_recur(const amp_lstm* h, int layer, const float* gx_dev, int B, int T, const float* skip_dev, float* y_dev, void* ws_dev, void* stream);
void amp_lstm_destroy(amp_lstm* h);

/* Residual VQ over full-width Euclidean codebooks in eval mode (csrc/evq.hip; modules/quantization/core_vq.py:180-236,331-388), exact fp32.
 * amp_evq_create: codebooks[l] [K, D] (EuclideanCodebook.embed) as num_quantizers host pointers.  Covered: D <= 1024, K <= 4096, N <= 32; anything
 *   else AMP_ERR_UNSUPPORTED; judged on the host before a device is asked for.
 * amp_evq_encode: z [B, D, T] -> codes int64 [n_q - st, B, T] of levels [st, n_q), and (not NULL) zq [B, D, T] = the sum of those levels' rows,
 *   all_zq [n_q - st, B, D, T] = every level's rows; ONE launch for all levels, the residual stays on chip.  The distance keeps the reference's
 *   expression and order, -((sum x^2 - (2 x) . e) + sum e^2); equal distances resolve to the LOWEST index.  With st > 0 level st starts from the
 *   WHOLE input, as ResidualVectorQuantization.encode does.  0 <= st < n_q <= N, else AMP_ERR_INVALID.
 * amp_evq_decode: codes [n, B, T] of levels [st, st + n) -> out [B, D, T] = 0 + embed[st][codes[0]] + embed[st + 1][codes[1]] + ..  An index
 *   outside [0, K) reads row 0 instead (never out of bounds) and sets a device flag of the handle; amp_evq_check works as amp_fvq_check does.
 * No allocation and no synchronisation in encode / decode; deterministic; a frame never depends on what it is batched with. */
typedef struct amp_evq amp_evq;
int amp_evq_create(int dim, int codebook_size, int num_quantizers, const float* const* codebook_host, amp_evq** out);
int amp_evq_encode(const amp_evq* h, const float* z_dev, int B, int T, int st, int n_q, long long* codes_dev, float* zq_dev, float* all_zq_dev,
                   void* stream);
int amp_evq_decode(const amp_evq* h, const long long* codes_dev, int n, int st, int B, int T, float* out_dev, void* stream);
int amp_evq_check(amp_evq* h, void* stream);
void amp_evq_destroy(amp_evq* h);

/* ---- Semantic tokenizers (models/codec/kmeans/, coco/, vevo/): RepCodec, Coco, VevoRepCodec ---- */

/* Coco's down-sampling conv (csrc/dsconv_f16x3.hip; rep_coco_model.py: downsample_layers): Conv1d(cin, cout, k = 3, stride 2, padding 1),
 *     y[b, o, t] = epi( bias[o] + sum_c sum_{j<3} w[o, c, j] x[b, c, 2t + j - 1] ),  T_out = (T - 1) / 2 + 1 (amp_dsconv_out_len:
 * 0 for T < 1; the handle is not read and may be NULL).  epi = identity (gelu = 0) or the exact-erf GELU (gelu = 1).
 * x [B, cin, T] -> y [B, cout, T_out], fp32; any cin, cout, T >= 1; y must not overlap x.  weight_host [cout, cin, 3], bias_host [cout] or NULL.
 * The arithmetic is amp_set_precision's at create time.  f16x3: one kernel (host-packed weights, a two-plane staged window, each output one
 * workgroup's sum in a fixed order; feeds the op-level range flag, see amp_range_check), no workspace (ws_dev may be NULL).
 * AMP_PRECISION_F32: three launches inside the handle -- x copied with one zero column appended, amp_sconv's stride-2 form with the weight
 * extended by a zero fourth tap, amp_gelu -- on ws_dev: amp_dsconv_workspace_bytes(h, B, T) bytes, 16-byte aligned.
 * Bad arguments are AMP_ERR_INVALID and judged on the host before a device is asked for (create: NULL weight / out, cin or cout < 1, a
 * non-finite weight); a grid overflow is AMP_ERR_UNSUPPORTED.  No allocation and no synchronisation in forward; deterministic. */
typedef struct amp_dsconv amp_dsconv;
int amp_dsconv_create(int cin, int cout, const float* weight_host, const float* bias_host, amp_dsconv** out);
int amp_dsconv_out_len(const amp_dsconv* h, int T);
size_t amp_dsconv_workspace_bytes(const amp_dsconv* h, int B, int T);
int amp_dsconv_forward(const amp_dsconv* h, const float* x_dev, int B, int T, int gelu, void* ws_dev, size_t ws_bytes, float* y_dev, void* stream);
void amp_dsconv_destroy(amp_dsconv* h);

/* Element-wise exact-erf GELU (nn.GELU()), the function of the pointwise and down-sampling epilogues (csrc/gelu_erf.h): y[i] = gelu(x[i]),
 * i < n.  y may alias x; any 4-byte alignment (16-byte accesses where both bases allow).  NULL pointers or n <= 0: AMP_ERR_INVALID; more than
 * 2^31 - 1 workgroups: AMP_ERR_UNSUPPORTED; judged on the host alone. */
int amp_gelu(const float* x_dev, long long n, float* y_dev, void* stream);

/* ---- The non-autoregressive Llama of Vevo / MaskGCT (csrc/llama_nar.hip; models/vc/flow_matching_transformer/llama_nar.py: DiffLlama).
 * Channel-first [B, C, T] fp32 like everything here; the Linears are amp_pw_forward.  Deterministic, no workspace, no allocation and no
 * synchronisation; every argument is judged on the host before anything is launched. ---- */

/* Non-causal multi-head self-attention with rotary position embedding and a key mask, in one launch (flash-style: no [T, T] tensor):
 *     out[b, h*dk + d, t] = sum_s softmax_s( scale * <rope(q)[b, h, :, t], rope(k)[b, h, :, s]> + mask(b, s) ) v[b, h*dk + d, s]
 * q, k, v [B, H*dk, T] with rows T apart and ONE batch stride of batch_stride elements (0 = dense, H*dk*T): the three row blocks of a
 * stacked q | k | v GEMM output [B, 3*H*dk, T] are read in place (batch_stride = 3*H*dk*T).  out [B, H*dk, T] dense, not overlapping them.
 * cos, sin [T, dk/2] fp32, 16-byte aligned: HF's LlamaRotaryEmbedding (inv_freq = theta^(-2i/dk), positions 0 .. T-1).  The rotation is
 * HF's rotate-half form, x'[i] = x[i] cos[t, i] - x[i + dk/2] sin[t, i], x'[i + dk/2] = x[i + dk/2] cos[t, i] + x[i] sin[t, i] for i < dk/2 --
 * NOT the interleaved-pair form -- applied to q and k while they are staged.
 * key_mask [B, T] bytes, 1 = valid, any pattern; NULL = all valid.  The mask applies to KEYS only: every query column is computed, padded
 * positions included, as the reference does.  A masked key contributes exactly 0 whatever finite value its k / v columns hold.  Every item
 * needs at least one valid key (an item without one gets NaN columns; the reference gives it the mean of v).
 * scale: 1/sqrt(dk) (any positive finite value).
 * Arithmetic: both products are split-f16 MFMA (hi*hi + hi*lo + lo*hi, fp32 accumulate) whatever amp_set_precision says -- the exact-fp32
 * route of the drop-in modules is RoPE in torch + scaled_dot_product_attention; the softmax is an online fp32 softmax.  rope(q), rope(k) and v
 * are staged after an exact x16 and take part in the op-level range guard (amp_range_check; masked keys do not).
 * T = 1 is not a launch of the kernel: the softmax over one key is exactly 1, so out is a strided copy of v (its bits, no range guard).
 * AMP_ERR_INVALID with a message: a NULL pointer (key_mask excepted), dk other than 64 or 96, B, H or T < 1, T > 32768, B*H > 65535, batch_stride below
 * H*dk*T, a misaligned cos / sin, out overlapping q / k / v. */
int amp_rope_attention(const float* q_dev, const float* k_dev, const float* v_dev, long long batch_stride, const float* cos_dev,
                       const float* sin_dev, const unsigned char* key_mask_dev, int B, int H, int dk, int T, float scale, float* out_dev,
                       void* stream);

/* LlamaAdaptiveRMSNorm (llama_nar.py:32-50) over the channel axis:
 *     y[b, c, t] = w[b, c] * ( x[b, c, t] * rsqrt( mean_c x[b, :, t]^2 + eps ) )
 * x [B, C, T]; w one row of C weights PER ITEM, w_batch_stride elements apart (>= 0; the rows may be a slice of a wider tensor, e.g. of the
 * stacked to_weight GEMM of all norms of a model).  Plain fp32, the workgroup shape of amp_layer_norm_c_style; any C, T >= 1, B <= 65535;
 * y may alias x.  Each x element is read once for C <= 1024 (more channels are re-read).  Bad arguments: AMP_ERR_INVALID. */
int amp_rms_norm_c_adaptive(const float* x_dev, const float* w_dev, long long w_batch_stride, int B, int C, int T, float eps, float* y_dev,
                            void* stream);

/* Element-wise nn.SiLU, y[i] = x[i] / (1 + exp(-x[i])), i < n; the contract of amp_gelu (y may alias x, any 4-byte alignment). */
int amp_silu(const float* x_dev, long long n, float* y_dev, void* stream);
/* LlamaMLP's act_fn(gate_proj(x)) * up_proj(x) on the output of ONE stacked gate | up GEMM: gu [B, 2F, T] with the gate in rows [0, F) and
 * up in rows [F, 2F) -> y[b, f, t] = silu(gu[b, f, t]) * gu[b, F + f, t], y [B, F, T] not overlapping gu.  B <= 65535; bad arguments
 * AMP_ERR_INVALID, more than 2^31 - 1 workgroups per item AMP_ERR_UNSUPPORTED. */
int amp_swiglu(const float* gu_dev, int B, int F, int T, float* y_dev, void* stream);

/* ---- MaskGCT's decoding step (csrc/maskgct.hip; models/tts/maskgct/maskgct_t2s.py:14-32 top_k / gumbel_sample, :319-337). ---- */

/* The sampler of one decoding step, per (b, t), in one launch:
 *     kept  = the k largest logits of the row (top_k; the caller computes k = ceil((1 - filter_thres) * V) as the reference does)
 *     id    = argmax over the kept v of ( l_v / max(temperature, 1e-10) + g_v ),  g = -logf(-logf(u + 1e-10f) + 1e-10f)
 *             (u_dev NULL: greedy, id = argmax l_v, temperature ignored)
 *     score = exp(l_id - max) / sum over the kept of exp(l_v - max)      (the filtered logits' softmax at temperature 1, gathered at id)
 * logits [B, V, T] channel-first -- the pointwise GEMM's output, read in place: rows T apart, items batch_stride elements apart (0 = dense,
 * V*T).  u [B, T, V] dense, the reference's own noise tensor (zeros_like(logits).uniform_(0, 1)); it is read for the kept entries only.
 * ids int64 [B, T], score fp32 [B, T], dense.
 * Plain fp32, accurate expf / logf, a correctly rounded divide.  Deterministic: no atomics, every reduction in a fixed order.
 * TIES GO TO THE LOWER INDEX, both among logits equal to the k-th largest (which of them are kept) and among equal noisy values (torch
 * leaves both unspecified); -0 counts as +0.
 * Logits are assumed finite.  A NaN logit orders beyond +inf or below -inf by its sign bit: the id stays in [0, V), the score is NaN.
 * AMP_ERR_INVALID with a message, before any launch: a NULL logits / ids / score, V outside [2, 8192], k outside [1, V], B or T < 1,
 * B > 65535, batch_stride below V*T, a NaN temperature beside a noise tensor, ids or score overlapping logits, u or each other. */
int amp_mask_sample(const float* logits_dev, long long batch_stride, int B, int V, int T, int k, const float* u_dev, float temperature,
                    long long* ids_dev, float* score_dev, void* stream);

/* ---- Vevo's autoregressive transformer (csrc/llama_ar.hip; models/vc/autoregressive_transformer/ar_model.py: a causal LlamaForCausalLM
 * that decodes one token at a time).  Deterministic, no allocation and no synchronisation; every argument is judged on the host before
 * anything is launched.  The prefill is amp_pw_forward + amp_rope_attention_causal; a decode step has ONE column per item. ---- */

/* amp_rope_attention under the causal rule: key j is visible to query i iff j <= i AND the key mask admits it.  Same arguments, arithmetic,
 * range guard, refusals and T = 1 copy as amp_rope_attention (the same kernel with a compile-time flag: a query block walks the key tiles
 * up to its diagonal tile only).  Columns beyond a query never influence its output column: a hidden key meets p = 0 exactly, whatever
 * finite value it holds.  A query without a visible valid key (key 0 masked, query 0) gets a NaN column; right-padded batches have none. */
int amp_rope_attention_causal(const float* q_dev, const float* k_dev, const float* v_dev, long long batch_stride, const float* cos_dev,
                              const float* sin_dev, const unsigned char* key_mask_dev, int B, int H, int dk, int T, float scale, float* out_dev,
                              void* stream);

/* The KV cache of one layer is two fp32 buffers [B, H*dk, Lmax], channel-first like everything here; K is stored ALREADY ROTATED.
 * amp_kv_append takes T columns of un-rotated k and of v ([B, H*dk, T], rows T apart, one batch stride, 0 = dense: two row blocks of the
 * stacked q | k | v GEMM output are read in place) at positions pos0 .. pos0 + T - 1 and writes rope(k) (rotate-half, the formula of
 * amp_rope_attention, fp32) and the BITS of v into columns [pos0, pos0 + T) of the caches.  cos, sin: the tables' row 0, [>= pos0 + T, dk/2].
 * Once after the prefill with T = the prompt length, then once per step with T = 1.
 * AMP_ERR_INVALID with a message: a NULL pointer, dk other than 64 or 96, B, H or T < 1, B*H > 65535, pos0 < 0, pos0 + T > Lmax, batch_stride
 * below H*dk*T, caches overlapping each other or k / v. */
int amp_kv_append(const float* k_dev, const float* v_dev, long long batch_stride, const float* cos_dev, const float* sin_dev, int B, int H,
                  int dk, int T, int pos0, int Lmax, float* kcache_dev, float* vcache_dev, void* stream);

/* One decode step's attention: each (item, head) has ONE query, rotated inside the kernel with row L - 1 of cos / sin (the tables' row 0 is
 * passed), over cache columns [0, L):
 *     out[b, h*dk + d] = sum_{s < L} softmax_s( scale * <rope(q)[b, h, :], kcache[b, h, :, s]> ) vcache[b, h*dk + d, s]
 * q [B, H*dk] with items q_batch_stride elements apart (0 = dense; the first row block of a stacked [B, 3*H*dk, 1] GEMM output is read in
 * place), out [B, H*dk] dense.  Exact fp32 on the vector pipe (accurate expf, correctly rounded divide), whatever amp_set_precision says.
 * The keys are split over workgroups of amp_attention_decode_split() keys each; with more than one split the (max, sum, O) partials go
 * through the workspace (amp_attention_decode_workspace_bytes(B, H, dk, Lmax) bytes serve every L <= Lmax; L <= the split needs none) and a
 * second small launch adds them in ascending order.  Cache columns >= L are never operands: whatever they hold (NaN, 1e30) leaves the
 * result's bits alone.
 * AMP_ERR_INVALID with a message: a NULL pointer (the workspace excepted where none is needed), dk other than 64 or 96, B or H < 1,
 * B*H > 65535, L < 1, L > Lmax, a non-positive or non-finite scale, q_batch_stride below H*dk, a workspace too small, out or the workspace
 * overlapping q, the caches or each other. */
int amp_attention_decode(const float* q_dev, long long q_batch_stride, const float* cos_dev, const float* sin_dev, const float* kcache_dev,
                         const float* vcache_dev, int B, int H, int dk, int L, int Lmax, float scale, float* out_dev, float* workspace_dev,
                         size_t workspace_bytes, void* stream);
size_t amp_attention_decode_workspace_bytes(int B, int H, int dk, int Lmax);
int amp_attention_decode_split(void);

/* amp_pw_forward at T = 1 for B <= 8 items, on the same handle and from the same packed weights (no second device copy), as a
 * weight-streaming matrix-vector product: x [B, cin] with items x_batch_stride apart (0 = dense), y [B, cout] dense,
 *     AMP_PW_BIAS: y = Wx + b        AMP_PW_SCALE_RES: y = res + gamma (.) (Wx + b)   (res [B, cout]; y may alias res)
 * Every weight is read once, in 16-byte loads, and multiplied in fp32 (an f16x3 handle's weight is hi + lo, exactly the fp32 value the
 * two planes hold: about 22 of the 24 mantissa bits of the original; an exact-fp32 handle's is the weight itself); x is never split, so
 * there is no range guard.  Row blocks and K slices spread the matrix over more workgroups than the chip has CUs; the K slices' partial
 * sums go through the workspace (amp_pw_forward_vec_workspace_bytes(handle, B) bytes) and a second small launch adds them in ascending
 * order and applies the epilogue.  The order of every sum depends on the shape alone.
 * AMP_ERR_INVALID with a message: a NULL handle / x / y / workspace, B outside [1, 8], an epilogue other than the two above, AMP_PW_SCALE_RES
 * without gamma and res, x_batch_stride below cin, a workspace too small, x, y and the workspace overlapping, res overlapping y without
 * being y. */
int amp_pw_forward_vec(const amp_pw* h, const float* x_dev, long long x_batch_stride, int B, int epilogue, const float* gamma_dev,
                       const float* res_dev, float* y_dev, float* workspace_dev, size_t workspace_bytes, void* stream);
size_t amp_pw_forward_vec_workspace_bytes(const amp_pw* h, int B);

/* One decode step's sampler, one launch, one logits row per item: HF's processor chain as `generate(do_sample=True)` composes it
 * (transformers/generation/logits_process.py) and the draw.
 *   1. repetition penalty over the ids seen so far, ids[b, 0 .. n_ids): l < 0 ? l * p : l / p, once per distinct id; skipped at p = 1
 *   2. suppress_eos != 0: the logit of eos_id becomes -inf (the caller sets it while fewer than min_new_tokens have been generated)
 *   3. l / temperature
 *   4. top-k: every logit not below the k-th largest stays -- HF removes l < the k-th value, so ALL ties at the boundary are kept (unlike
 *      amp_mask_sample); top_k > V keeps everything
 *   5. top-p: with p1 the softmax of what is left, HF removes the ascending-sorted prefix whose cumulative p1 is <= 1 - top_p, i.e. the
 *      values whose mass sum{p1_u : l_u <= l_v} is <= 1 - top_p (1 - top_p formed in double, compared in fp32); the maximum always stays;
 *      top_p >= 1 disables the filter
 *   6. p = softmax of what is left; id = argmax_v p_v / q_v with q [B, V] the caller's Exp(1) noise -- the exponential race that
 *      torch.multinomial runs; an equal quotient goes to the LOWER index
 * The id is written as int64 to ids[b, n_ids]: ids [B, ids_capacity] int64 is both the history of the penalty and the token buffer.
 * logits [B, V] with items batch_stride apart (0 = dense), read in place from the lm_head output.  2 <= V <= 16384.
 * Plain fp32, accurate expf, correctly rounded divides, every reduction in a fixed order.  Logits and noise are assumed finite, q > 0.
 * AMP_ERR_INVALID with a message: a NULL logits / q / ids, V outside [2, 16384], B outside [1, 65535], top_k < 1, top_p <= 0 or NaN, a
 * temperature or penalty that is not positive and finite, n_ids < 0 or >= ids_capacity, suppress_eos with eos_id outside [0, V),
 * batch_stride below V, ids overlapping logits or q. */
int amp_ar_sample(const float* logits_dev, long long batch_stride, int B, int V, const float* q_dev, long long* ids_dev, long long ids_capacity,
                  int n_ids, int eos_id, int suppress_eos, float temperature, int top_k, double top_p, float repetition_penalty, void* stream);

/* ---- FastSpeech2 / JETS inference (csrc/fastspeech.hip, csrc/llama_nar.hip; models/tts/fastspeech2/fs2.py, models/tts/jets/jets.py,
 * modules/transformer/{Models,Layers,SubLayers,Modules}.py).  Channel-first [B, C, T] fp32.  Deterministic, no atomics on data, no
 * allocation and no synchronisation; every argument is judged on the host before anything is launched. ---- */

/* ScaledDotProductAttention inside the FFT block's MultiHeadAttention, in one launch (flash-style: no [T, T] tensor):
 *     out[b, h*dk + d, t] = sum_s softmax_s( scale * <q[b, h, :, t], k[b, h, :, s]> + mask(b, s) ) v[b, h*dk + d, s]
 * Non-causal, NO positional rotation.  This is amp_rope_attention's kernel with its compile-time rotation switched off, and everything that
 * entry point states holds here: q, k, v [B, H*dk, T] with rows T apart and ONE batch stride (0 = dense; the three row blocks of a stacked
 * q | k | v GEMM output are read in place), out dense and not overlapping them; key_mask [B, T] bytes, 1 = valid, any pattern, NULL = all
 * valid, applied to keys only; a masked key contributes exactly 0 whatever finite value its k / v columns hold; every item needs one valid
 * key; both products split-f16 MFMA with an fp32 online softmax whatever amp_set_precision says; q, k and v are staged after an exact x16
 * and take part in the op-level range guard (amp_range_check); T = 1 is a strided copy of v (its bits).
 * scale: the caller's 1 / temperature = 1 / sqrt(dk) (any positive finite value).
 * dk = 128 only (hidden 256 with 2 heads, every FastSpeech2 / JETS recipe): the K and V planes take 67 584 bytes of dynamic LDS.
 * AMP_ERR_INVALID with a message: a NULL pointer (key_mask excepted), dk other than 128, B, H or T < 1, T > 32768, B*H > 65535, batch_stride
 * below H*dk*T, out overlapping q / k / v. */
int amp_mh_attention(const float* q_dev, const float* k_dev, const float* v_dev, long long batch_stride, const unsigned char* key_mask_dev, int B,
                     int H, int dk, int T, float scale, float* out_dev, void* stream);

/* VarianceAdaptor's durations from the (masked) log-duration prediction log_d [B, T]:
 *     d_rounded[b, t] = max( rint( expf(log_d[b, t]) - 1 ) * d_control, 0 )        fp32 [B, T]
 *     cum[b, t]       = sum_{s <= t} (int) d_rounded[b, s]                         int32 [B, T], the layout amp_expand_path takes
 *     mel_len[b]      = cum[b, T - 1]                                              int32 [B]
 * rint is round-half-even (torch.round), expf the accurate one, the multiply one fp32 multiply; the clamp keeps -0 and NaN as torch.clamp
 * does.  (int) truncates as LengthRegulator.expand does (`max(int(expand_size), 0)`); a NaN counts 0, one token at most 2^24 frames, the sum
 * saturates at INT_MAX.  mel_len may be 0: the caller refuses such an item.  One workgroup per item scans in a fixed order.  JETS is the same
 * op at d_control = 1 (its .long() output is (int) d_rounded).
 * AMP_ERR_INVALID with a message: a NULL pointer, B or T < 1, d_control not positive and finite, d_rounded aliasing log_d. */
int amp_fs2_durations(const float* log_d_dev, int B, int T, float d_control, float* d_rounded_dev, int* cum_dev, int* mel_len_dev, void* stream);

/* x + embedding(bucketize(pred * control, bins)) in one launch, as torch.bucketize(right = False) + nn.Embedding + add give it, bit for bit:
 *     v = pred[b, t] * control (one fp32 multiply), written to pred_out[b, t]
 *     i = the number of boundaries < v: a value equal to a boundary takes that boundary's index, below the first gives 0, above the last --
 *         and NaN -- gives n_bounds
 *     y[b, :, t] = x[b, :, t] + table[i, :]          (one fp32 add)
 * at EVERY column, padded ones included (the reference adds the embedding of prediction 0 there).  pred [B, T]; bins [n_bounds] ascending;
 * table [n_rows, D] row-major with n_rows >= n_bounds + 1 (n_bins = n_bounds + 1 in the reference); x, y [B, D, T], y may be x.  Table rows
 * are gathered as contiguous segments and stored along T through LDS, as amp_embed_sum_c does.
 * AMP_ERR_INVALID with a message: a NULL pointer, B, D or T < 1, n_bounds < 1, a table of fewer than n_bounds + 1 rows, a NaN control,
 * pred_out aliasing pred; B or ceil(D / 64) beyond 65535 AMP_ERR_UNSUPPORTED. */
int amp_bucketize_embed_add(const float* pred_dev, float control, const float* bins_dev, int n_bounds, const float* table_dev, int n_rows,
                            const float* x_dev, int B, int D, int T, float* y_dev, float* pred_out_dev, void* stream);

/* VariancePredictor's tail, layer_norm_2 -> Linear(C, 1) -> masked_fill, without writing the normalised tensor:
 *     y[b, t] = sum_c w[c] * ( gamma[c] * (x[b, c, t] - mean_c) * rstd_c + beta[c] ) + b0,        0 (by select) where t >= lens[b]
 * x [B, C, T], y [B, T]; lens int32 [B] or NULL (no mask).  Mean, biased variance of the centred values, their order of summation and the
 * affine are amp_layer_norm_c's; the sum over c adds thread partials (fma, ascending channels) over the eight channel groups in a fixed order.
 * A masked column is 0 whatever x holds there (NaN included).  Any C, T >= 1; each x element is read once for C <= 256.
 * AMP_ERR_INVALID with a message: a NULL pointer (lens excepted), B, C or T < 1, B > 65535, a negative or NaN eps. */
int amp_layer_norm_c_head(const float* x_dev, const float* gamma_dev, const float* beta_dev, const float* w_dev, float b0, const int* lens_dev, int B,
                          int C, int T, float eps, float* y_dev, void* stream);

/* ---- NaturalSpeech2 inference (csrc/llama_nar.hip, csrc/ns2_layer_f16x3.hip, csrc/ns2.hip; models/tts/naturalspeech2/{ns2,prior_encoder,
 * diffusion,wavenet}.py, modules/naturalpseech2/transformers.py).  Channel-first [B, C, T] fp32.  Deterministic, no atomics on data, no
 * allocation and no synchronisation; every argument is judged on the host before anything is launched. ---- */

/* Non-causal multi-head attention WITHOUT rotation at head dimension 64 with separate query and key lengths, in one launch:
 *     out[b, h*dk + d, tq] = sum_s softmax_s( scale * <q[b, h, :, tq], k[b, h, :, s]> + mask(b, s) ) v[b, h*dk + d, s]
 * q [B, H*dk, Tq] with rows Tq apart and its own batch stride q_batch_stride (0 = dense, H*dk*Tq); k and v [B, H*dk, Tk] with rows Tk apart
 * and ONE batch stride kv_batch_stride (0 = dense): the two row blocks of a stacked k | v GEMM output are read in place.  Self-attention is
 * the case Tq = Tk with all three slices of one stacked q | k | v tensor (both strides 3*H*dk*T).  key_mask [B, Tk] bytes, 1 = valid, any
 * pattern, or NULL; out [B, H*dk, Tq] dense, not overlapping q / k / v.
 * This is amp_mh_attention's kernel (the rotation compiled out) at dk = 64, and everything that entry point states holds with T read as Tk
 * for keys and Tq for queries: the mask applies to keys only and every query column is computed; a masked key contributes exactly 0
 * whatever finite value its k / v columns hold; every item needs one valid key; both products split-f16 MFMA with an fp32 online softmax
 * whatever amp_set_precision says (the exact-fp32 route of the drop-in modules is torch's scaled_dot_product_attention); q, k and v are
 * staged after an exact x16 and take part in the op-level range guard (amp_range_check; masked keys do not).
 * Tk = 1 is not a launch of that kernel: the softmax over one key is exactly 1, so v's column is copied (its bits) to every query column.
 * AMP_ERR_INVALID with a message: a NULL pointer (key_mask excepted), dk other than 64, B, H, Tq or Tk < 1, Tq or Tk > 32768, B*H > 65535,
 * q_batch_stride below H*dk*Tq, kv_batch_stride below H*dk*Tk, a non-positive or non-finite scale, out overlapping q / k / v. */
int amp_cross_attention(const float* q_dev, long long q_batch_stride, const float* k_dev, const float* v_dev, long long kv_batch_stride,
                        const unsigned char* key_mask_dev, int B, int H, int dk, int Tq, int Tk, float scale, float* out_dev, void* stream);

/* One residual layer of the WaveNet (wavenet.py:96-127, ResidualBlock.forward with x_mask = None) at hidden size H:
 *     y     = x + dconst[b, :]                          diffusion_proj(step embedding): [H] per item, dconst_batch_stride apart (0 = one row)
 *     a     = dilated_conv_k3(y) + bias + cterm         the conv pads y, NOT x: a tap outside [0, T) contributes 0; cterm [B, 2H, T] with rows
 *                                                       T apart and items cterm_batch_stride apart (0 = dense): cond_proj's output with its bias,
 *                                                       e.g. one layer's row block of a GEMM stacked over all layers
 *     a     = a * gain + fbias                          film_dev [B, 4H, T] dense, gain = rows [0, 2H), fbias = rows [2H, 4H); NULL = no FiLM
 *     z     = sigmoid(a[:H]) * tanh(a[H:])
 *     r     = out_proj(z)                               H -> 2H
 *     x_out = (x + r[:H]) / sqrt(2),  skip_out = skip_in + r[H:]       skip_in NULL in the first layer
 * amp_ns2_layer_create: conv_weight [2H, H, 3], conv_bias [2H] (NULL = zeros), out_weight [2H, H], out_bias [2H] (NULL = zeros), host fp32.
 * H a multiple of 64 in [128, 512], dilation 1 .. 8 (padding = dilation); anything else AMP_ERR_UNSUPPORTED.  Any T >= 1.
 * A handle keeps the arithmetic it was created under.  f16x3: two launches -- the gated GEMM over K = 3H (the [2H, T] pre-activation never
 * goes to memory; z [B, H, T] goes to the workspace) and out_proj on the pointwise GEMM kernel with a residual | skip epilogue; staged
 * operands report to the op-level range flag (amp_range_check).  AMP_PRECISION_F32: the exact conv between element-wise launches (five
 * launches; not the hot path).  ws_dev: amp_ns2_layer_workspace_bytes(h, B, T) bytes, not overlapping any tensor.
 * x_out may be x (in place) or must not overlap it; skip_out may be skip_in; skip_out must not overlap x or x_out.
 * AMP_ERR_INVALID with a message: a NULL handle / x / dconst / cterm / x_out / skip_out / workspace, B or T < 1, B > 65535, a stride below its
 * extent, a workspace too small, the overlaps above. */
typedef struct amp_ns2_layer amp_ns2_layer;
int amp_ns2_layer_create(int hidden, int dilation, const float* conv_weight_host, const float* conv_bias_host, const float* out_weight_host,
                         const float* out_bias_host, amp_ns2_layer** out);
int amp_ns2_layer_precision(const amp_ns2_layer* h);
size_t amp_ns2_layer_workspace_bytes(const amp_ns2_layer* h, int B, int T);
int amp_ns2_layer_forward(const amp_ns2_layer* h, const float* x_dev, const float* dconst_dev, long long dconst_batch_stride, const float* cterm_dev,
                          long long cterm_batch_stride, const float* film_dev, const float* skip_in_dev, int B, int T, float* x_out_dev,
                          float* skip_out_dev, void* ws_dev, size_t ws_bytes, void* stream);
void amp_ns2_layer_destroy(amp_ns2_layer* h);

/* The element-wise tail of Diffusion.cal_dxt (diffusion.py:72-82) and the solver's update in one launch, over n elements:
 *     mean  = x0_pred * mean_scale                      mean_scale = exp(-0.5 * cum_beta / sigma^2)
 *     logp  = -(x_eval - mean) / (variance + 1e-8)      variance   = sigma^2 * (1 - exp(-cum_beta / sigma^2))
 *     dxt   = (-0.5 * h_beta) * (logp + x_eval * inv_sigma2)           h_beta = h * beta_t
 *     out   = x_base - dxt                              midpoint_half != 0: out = 0.5 * ((x_base - dxt) + x_base), the midpoint solver's x_mid
 * The caller forms the four scalars as the reference does (fp32, on a one-element tensor) and passes them by value.  euler: x_eval = x_base =
 * xt.  midpoint: first x_eval = x_base = xt with midpoint_half = 1, then x_eval = x_mid, x_base = xt.  Plain fp32, one rounding per
 * operation; out may be any of the inputs (element-wise) or must not overlap them.
 * AMP_ERR_INVALID with a message: a NULL pointer, n < 1, a NaN scalar, a partial overlap; more than 2^31 - 1 workgroups AMP_ERR_UNSUPPORTED. */
int amp_ns2_ode_step(const float* x_eval_dev, const float* x0_pred_dev, const float* x_base_dev, long long n, float mean_scale, float variance,
                     float h_beta, float inv_sigma2, int midpoint_half, float* out_dev, void* stream);

/* ---- VALL-E inference (csrc/valle.hip, csrc/llama_nar.hip; models/tts/valle/valle.py, modules/transformer/transformer.py,
 * modules/norms/norm.py).  Channel-first [B, C, T] fp32.  Deterministic, no atomics on data, no allocation and no synchronisation; every
 * argument is judged on the host before anything is launched. ---- */

/* Self-attention WITHOUT rotation at head dimension 64 under the prefix-LM rule, in one launch: key j is visible to query i iff
 * (j < prefix || j <= i) AND the key mask admits it -- text columns [0, prefix) see all text and no audio, audio columns see all text and
 * the audio up to themselves.  prefix = 0 is the plain causal rule, prefix = T full attention (then bit for bit amp_cross_attention at
 * Tq = Tk).  This is amp_rope_attention_causal's kernel with its rotation compiled out, and everything that entry point states holds here:
 * q, k, v [B, H*dk, T] with rows T apart and ONE batch stride (0 = dense; the three row blocks of a stacked q | k | v GEMM output are read
 * in place), out dense and not overlapping them; key_mask [B, T] bytes, 1 = valid, or NULL; a query block walks the key tiles up to the one
 * that holds max(its last query, prefix - 1); a hidden key is staged like any other and meets p = 0: it contributes exactly 0 whatever
 * finite value it holds, and a masked key whatever it holds; a query without a visible valid key gets a NaN column; split-f16 MFMA products
 * with an fp32 online softmax whatever amp_set_precision says; q, k, v take part in the op-level range guard; T = 1 is a copy of v.
 * AMP_ERR_INVALID with a message: a NULL pointer (key_mask excepted), dk other than 64, B, H or T < 1, T > 32768, B*H > 65535, prefix
 * outside [0, T], batch_stride below H*dk*T, a non-positive or non-finite scale, out overlapping q / k / v. */
int amp_prefix_attention(const float* q_dev, const float* k_dev, const float* v_dev, long long batch_stride, const unsigned char* key_mask_dev, int B,
                         int H, int dk, int T, int prefix, float scale, float* out_dev, void* stream);

/* amp_pw_forward_vec with the LayerNorm of its input folded into the staging of x and a ReLU epilogue beside the residual one:
 *     y = epi( W n(x) + b ),     n(x) = (x - mean) * (1 / sqrtf(var + eps)) * ln_gamma + ln_beta     over the cin channels of each item
 * (biased variance of the centred values, two passes; n(x) = x when ln_gamma and ln_beta are NULL), epi = bias, bias -> ReLU (relu != 0), or
 * res + gamma (.) (.) (gamma and res given; y may alias res).  Same handle, packed weights, grid, K slices, workspace size and order of
 * every sum as amp_pw_forward_vec: with ln_gamma = NULL and relu = 0 the result is that entry point's, bit for bit.  Every workgroup forms
 * the statistics of the whole row(s) itself, in an order fixed by cin alone, before it stages its own K slice: all of them hold the same
 * bits.  x is never split, so there is no range guard.  A constant row (variance 0) gives finite values (eps > 0).
 * AMP_ERR_INVALID with a message: a NULL handle / x / y / workspace, B outside [1, 8], one of ln_gamma / ln_beta or of gamma / res without
 * the other, the LayerNorm form at cin > 4096, a negative or non-finite eps, relu beside res, x_batch_stride below cin, a workspace too
 * small, x, y and the workspace overlapping, res overlapping y without being y. */
int amp_pw_forward_vec_ln(const amp_pw* h, const float* x_dev, long long x_batch_stride, int B, const float* ln_gamma_dev, const float* ln_beta_dev,
                          float eps, int relu, const float* gamma_dev, const float* res_dev, float* y_dev, float* workspace_dev,
                          size_t workspace_bytes, void* stream);
size_t amp_pw_forward_vec_ln_workspace_bytes(const amp_pw* h, int B);

/* TokenEmbedding followed by SinePositionalEmbedding from a running position, channel-first:
 *     y[b, :, t] = weight[tokens[b, t], :] * x_scale + alpha * pe[pos0 + t, :]
 * tokens int64 [B, T]; weight [rows, D]; pe [pe_rows, D], the table the module builds (position_embedding.py:43-48), uploaded once; alpha ONE
 * fp32 value on the device (the module's parameter, read in place); y [B, D, T].  T = the prompt once, then T = 1 per decode step.  The two
 * products and the add are three fp32 roundings, as torch evaluates the expression: no fma.  An id outside [0, rows) reads row 0 instead (never
 * out of bounds) and sets *flag_dev, a zero-initialised 32-bit word of the caller's that amp_embed_sum_check reads and clears.
 * AMP_ERR_INVALID with a message: a NULL pointer, rows, D, B, T or pe_rows < 1, pos0 < 0, pos0 + T > pe_rows; B or ceil(D / 64) beyond 65535
 * AMP_ERR_UNSUPPORTED. */
int amp_embed_pos(const long long* tokens_dev, const float* weight_dev, int rows, int D, const float* pe_dev, int pe_rows, int pos0, float x_scale,
                  const float* alpha_dev, int B, int T, float* y_dev, unsigned* flag_dev, void* stream);

/* ---- AudioLDM text-to-audio (csrc/conv2d_f16x3.hip, csrc/tta.hip, csrc/llama_nar.hip; models/tta/ldm/audioldm.py, models/tta/ldm/attention.py,
 * models/tta/autoencoder/autoencoder.py).  Channel-first fp32: a feature map [B, C, H, W] is the library's [B, C, T] with T = H*W and row
 * pitch W, and the token sequence of the spatial transformer is the same tensor.  Every launch goes to the caller's stream; no allocation,
 * no synchronisation, no workgroup waits for another; deterministic (fixed summation order, no atomics except the f16x3 range flag); an
 * item's bits do not depend on what it is batched with. ---- */

/* Conv2d 3 x 3 with zero padding 1 as a split-f16 implicit GEMM (K = 9 * Cin streamed through LDS per tap).
 * amp_conv2d_create: weight [Cout, Cin, 3, 3] and bias [Cout] (NULL = zeros), host fp32.  Cin = 4 or a multiple of 32 up to 2048, Cout = 1, 4
 * or a multiple of 32 up to 1024 (the odd ones are padded on the host); anything else AMP_ERR_UNSUPPORTED.  The kernel exists in the f16x3
 * arithmetic only: under AMP_PRECISION_F32 create returns AMP_ERR_UNSUPPORTED and the drop-in modules run torch's conv (not the hot path).
 * amp_conv2d_forward: x [B, Cin, H, W] -> y [B, Cout, Ho, Wo], any H, W >= 1 with H*W < 2^24, with the run-time options
 *     stride 1 | 2       stride 2: Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1 (the UNet's Downsample)
 *     up2                the conv reads the nearest-neighbour x2 up-sampling of x, source (y >> 1, x >> 1), Ho = 2H, Wo = 2W; the up-sampled
 *                        tensor is never written; stride must be 1
 *     mean_rstd_dev      [B, 32, 2] from amp_group_norm_stats with gamma_dev, beta_dev [Cin]: a staged element becomes
 *                        silu((x - mean_g) * rstd_g * gamma_c + beta_c) before the split (Cin a multiple of 32); the padding stays exactly 0,
 *                        as the reference pads the activated tensor.  NULL: x as it is (gamma / beta ignored)
 *     epilogue           + bias[m], then + row_add_dev[b, m] (NULL = none; items row_add_batch_stride floats apart, 0 = dense: a column block
 *                        of a wider [B, n] tensor is read in place), then + residual_dev[b, m, t] (NULL = none; y may not overlap it)
 * Where B*Ho*Wo is small against the weights the K axis is cut into slices whose partial sums go to ws_dev (amp_conv2d_workspace_bytes, 0
 * where no slice is needed; ws_dev may then be NULL) and a second launch adds them in slice order: the cut is a function of the handle and
 * of Ho*Wo alone; amp_conv2d_plan states it for one feature map (the number of K slices, 1 = one launch with the epilogue on the accumulators;
 * the row blocks a wave owns, 1 | 2; the channels of a K chunk, 32 | 64; any of the three pointers may be NULL).  Staged operands report to the op-level range flag (amp_range_check).
 * AMP_ERR_INVALID with a message: a NULL handle / x / y, B, H or W < 1, B > 65535, mean_rstd without gamma / beta, a row_add stride below Cout, a workspace too small, y
 * overlapping x or the residual, the workspace overlapping a tensor.  AMP_ERR_UNSUPPORTED: a stride other than 1 or 2, up2 with stride 2,
 * H*W >= 2^24, B*Ho*Wo beyond 2^31, the norm with Cin = 4. */
typedef struct amp_conv2d amp_conv2d;
int amp_conv2d_create(int cin, int cout, const float* weight_host, const float* bias_host, amp_conv2d** out);
int amp_conv2d_precision(const amp_conv2d* h);
int amp_conv2d_plan(const amp_conv2d* h, int H, int W, int stride, int up2, int* k_slices, int* row_blocks_per_wave, int* chunk_channels);
size_t amp_conv2d_workspace_bytes(const amp_conv2d* h, int B, int H, int W, int stride, int up2);
int amp_conv2d_forward(const amp_conv2d* h, const float* x_dev, int B, int H, int W, int stride, int up2, const float* mean_rstd_dev,
                       const float* gamma_dev, const float* beta_dev, const float* row_add_dev, long long row_add_batch_stride,
                       const float* residual_dev, float* y_dev, void* ws_dev, size_t ws_bytes, void* stream);
void amp_conv2d_destroy(amp_conv2d* h);

/* GroupNorm(32) statistics of x [B, C, T]: mean_rstd [B, 32, 2] = mean | 1 / sqrt(var + eps) over each group's (C / 32) * T elements, biased
 * variance as torch computes it.  Two passes, the second centred, summed in fp64 in an order fixed by the group's size: |mean| >> std costs
 * nothing.  C a multiple of 32 (else AMP_ERR_UNSUPPORTED).  AMP_ERR_INVALID: a NULL pointer, B, C or T < 1, a negative or non-finite eps,
 * mean_rstd overlapping x. */
int amp_group_norm_stats(const float* x_dev, int B, int C, int T, float eps, float* mean_rstd_dev, void* stream);
/* The apply: y = (x - mean_g) * rstd_g * gamma_c + beta_c, through SiLU when silu != 0; y may be x (element-wise in place) or must not overlap it.  For the places where no 3 x 3 conv
 * follows the norm (SpatialTransformer.norm -> proj_in).  C a multiple of 32; C, B <= 65535. */
int amp_group_norm(const float* x_dev, const float* mean_rstd_dev, const float* gamma_dev, const float* beta_dev, int B, int C, int T, int silu,
                   float* y_dev, void* stream);

/* amp_cross_attention at head dimension 32, 64 or 128: with num_heads = 8 the spatial transformer's head dimension is 32 / 64 / 128 at the UNet's
 * three levels.  It serves attn1 (q | k | v row blocks of one stacked GEMM output, Tq = Tk = H*W) and attn2 (Tq = H*W against the text tokens).
 * Everything amp_cross_attention states holds, with "dk other than 32, 64 or 128" as the refused head dimensions; at dk = 64 the two entries
 * launch the same kernel and return the same bits.  dk = 32 is a new instantiation of the template; dk = 128 is amp_mh_attention's
 * instantiation with its dynamic-LDS plan and the extents apart.  amp_cross_attention itself keeps refusing 32 and 128. */
int amp_cross_attention_hd(const float* q_dev, long long q_batch_stride, const float* k_dev, const float* v_dev, long long kv_batch_stride,
                           const unsigned char* key_mask_dev, int B, int H, int dk, int Tq, int Tk, float scale, float* out_dev, void* stream);

/* GEGLU (attention.py:95-96) on the output u [B, 2F, T] of one stacked GEMM: y[b, f, t] = u[b, f, t] * gelu(u[b, F + f, t]), the first half the
 * value and the second the gate, exact-erf GELU; y [B, F, T] dense, not overlapping u.  amp_swiglu's contract otherwise. */
int amp_geglu(const float* u_dev, int B, int F, int T, float* y_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AMPHION_HIP_H */
