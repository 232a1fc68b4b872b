// Device building blocks shared by the split-f16 ("f16x3") MFMA kernels (conv_f16x3.hip, conv_blk_f16x3.hip, conv_small_f16x3_body.h,
// pair_f16x3_body.h, pair_strip_f16x3.hip, rb_f16x3.hip, ampb_f16x3.hip; pw_f16x3.hip, dsconv_f16x3.hip, dw_layer_f16x3.hip, codec_unit_f16x3.hip and tconv_f16x3.hip through
// wholek_f16x3.h, which adds the blocks of the whole-K two-GEMM family; conv_mfma.hip takes the tile order and the accumulator row map).
// Every fused form is bit-identical to the launches it replaces because all of them split an operand, form a product term and walk
// the tiles through the SAME text: the one below.  Device code only; host declarations and argument structs are in amp_internal.h.
#pragma once
#include "amp_internal.h"

namespace amp {

typedef float f32x16 __attribute__((ext_vector_type(16)));    // one 32 x 32 accumulator tile: 16 registers per lane
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));   // one MFMA operand fragment: 8 channels of one row / column

// an operand fragment as it is loaded (one 16-B global / LDS read) and as the MFMA takes it
union Frag {
    uint4 u;
    f16x8 h;
};

// VMEM and MFMA may not cross (VALU, SALU, DS may): pins where the global loads are issued relative to
// the MFMA blocks and their issue ORDER, on which the
// counted s_waitcnt vmcnt(N) the compiler derives depends (loads return in order).
#define AMP_PIN_VMEM() __builtin_amdgcn_sched_barrier(0x386)
// hides a loaded value behind an empty asm: hipcc otherwise turns `cond ? loaded : 0` into a branch around the load
// (load sunk into the taken side) and, loads returning in order, waits with vmcnt(0) for the whole tile at every one
#define AMP_OPAQUE(v) asm("" : "+v"(v))

// Tile walked by workgroup `bid` of `nbx`.  Workgroups are dispatched round-robin over the 8 XCDs (block b -> XCD b % 8), each
// with its own L2: hand every XCD a contiguous run of tiles, so the halo columns two neighbouring tiles share are fetched
// into ONE L2 instead of two.  Ragged batches keep the dispatch order: with utterances of different lengths a contiguous run
// per XCD would hand one XCD the long utterances and another only tiles that exit at once (measured 43.8 vs 48.7 ms padded).
// rev: descending tile order -- start where the previous launch stopped writing (ConvArgs::rev).
// (`bid` is unsigned like blockIdx.x: the shift is logical.)
__device__ __forceinline__ int tile_order(unsigned bid, int nbx, bool ragged, int rev) {
    int bx = ((nbx & 7) == 0 && !ragged) ? (int)(bid & 7) * (nbx >> 3) + (int)(bid >> 3) : (int)bid;
    if (rev) bx = nbx - 1 - bx;
    return bx;
}

// ---- three layout facts every kernel of the family relies on --------------------------------------------------------------------
// v_mfma_f32_32x32x16_f16: register r of lane (hi = lane >> 5, l31 = lane & 31) of an accumulator tile holds column l31 of row
// acc_row(r, hi) of the 32-row block; acc_row(r) is the part without the lane term, for the sites that fold 4 * hi into a pointer.
// `base` (the block's first row) is summed first, left to right: hipcc's address arithmetic follows the association of this sum.
__device__ __forceinline__ int acc_row(int r, int hi = 0, int base = 0) { return base + (r & 3) + 8 * (r >> 2) + 4 * hi; }
// A staged B operand is [plane hi | lo][channel octet][column][8 x f16]: one ds_read_b128 per fragment.  Staging writes channel QUADS
// (uint2): the index of quad qd at column col inside a plane S columns wide.
__device__ __forceinline__ int bplane_idx(int qd, int col, int S) { return (((qd >> 1) * S + col) << 1) + (qd & 1); }
// range_max is the running maximum of |staged operand| (stage4_f16 / seam4_f16); beyond the f16 range the split form does not hold
// the value: one lane of the wave reports it (amp_host.h: RangeGuard).
__device__ __forceinline__ void raise_range(unsigned* flag, float range_max, int lane) {
    if (flag && __any(range_max > 65504.f) && lane == 0) atomicOr(flag, 1u);
}

// The split product of MI row blocks x NI column tiles over one k-extent: Whi*Xhi, Whi*Xlo, Wlo*Xhi -- three sweeps over ALL tiles in
// THIS order (the arithmetic contract every kernel form keeps; the dropped Wlo*Xlo term is 2^-22 relative).  The only
// text of the family that issues the MFMA.
template <int MI, int NI>
__device__ __forceinline__ void mfma3_tiles(f32x16 (*acc)[NI], const Frag* a_h, const Frag* a_l, const Frag* bh, const Frag* bl) {
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int t = 0; t < NI; ++t) acc[i][t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_h[i].h, bh[t].h, acc[i][t], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int t = 0; t < NI; ++t) acc[i][t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_h[i].h, bl[t].h, acc[i][t], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int t = 0; t < NI; ++t) acc[i][t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_l[i].h, bh[t].h, acc[i][t], 0, 0, 0);
}
// the same for one row block over N column tiles (one conv tap): the form the conv family uses
template <int N>
__device__ __forceinline__ void mfma3(f32x16* acc, const Frag& a_h, const Frag& a_l, const Frag* bh, const Frag* bl) {
    mfma3_tiles<1, N>(reinterpret_cast<f32x16(*)[N]>(acc), &a_h, &a_l, bh, bl);
}

// v = hi + lo with hi = f16(v), lo = f16(v - hi): the split-f16 operand form of the f16x3 kernels.
// The empty asm makes `v` opaque: under HIP's default -ffp-contract=fast hipcc otherwise folds the
// multiply that produced v into the conversions (v_fma_mix*: f16(x*k) rounded ONCE from the exact
// product) for `lo` but not for the stored `hi` (v_cvt_pk_f16_f32 of the fp32-rounded product): in the
// rare double-rounding cases the two disagree by one f16 ulp and the pair (hi, lo) is off by 2^-11.
__device__ __forceinline__ void split_f16(float v, _Float16& h, _Float16& l) {
    asm("" : "+v"(v));
    h = (_Float16)v;
    l = (_Float16)(v - (float)h);
}

// ---- the same split on FOUR operands with gfx950's packed conversions ------------------------------------------------
// Staging (and the fused pair's seam) is VALU work on a chip that runs these kernels at its power limit: per element the
// scalar form costs select + compare + select + multiply + 3 conversions + subtract + half a pack (9.5 instructions),
// the packed form 2 multiplies + max for the leaky ReLU and v_cvt_pk_f16_f32 / v_pk_add_f32 for the split (about 6).
// Every value is the one split_f16 / `v * (v > 0 ? kpos : kneg)` produce:
//   max(kpos * x, kneg * x) == x * (x > 0 ? kpos : kneg) for kneg <= kpos (slopes <= 1; the host refuses larger ones),
//   hi = RNE f16(v), v - hi is exact in fp32, lo = RNE f16(v - hi).
typedef float amp_f32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 amp_f16x2 __attribute__((ext_vector_type(2)));

// lo = f16(v - hi) is ONE v_fma_mixlo_f16 / v_fma_mixhi_f16 per element (fp32 v, constant 1.0, the f16 half of hi negated: the
// difference is exact in fp32, so the single rounding of the mix form is the rounding of the conversion): 3 VALU instructions
// per operand pair instead of 5 (v_cvt_pk_f16_f32, 2 x v_cvt_f32_f16, v_pk_add_f32, v_cvt_pk_f16_f32).  hipcc does not select
// the mix form for a subtraction (it vectorises it); tests/experiments/split_mix.hip compares both forms on the hardware over
// 2^25 operand pairs covering every sign / exponent / upper-mantissa pattern.
// CAUTION (round 5, profiles/r5_b_fir_mfma.txt): send the results to LDS (as every caller does: the store interlocks), never straight into an
// MFMA -- on gfx950 an MFMA that reads a VGPR needs two wait states after the VALU instruction that wrote it, hipcc inserts them only for
// instructions it can see, and these are inline asm: fragments fed directly came out with a stale half in ~3 % of the waves.  An MFMA consumer
// needs an `s_nop 1` at the end of the asm (profiles/negative_kernels/act1d_mfma.h: act_split4).
__device__ __forceinline__ void split4_f16(amp_f32x2 v01, amp_f32x2 v23, uint2& h, uint2& l) {
    asm("" : "+v"(v01));      // opaque, as in split_f16: no folding of the producing multiply into ONE of the conversions
    asm("" : "+v"(v23));
    const amp_f16x2 h01 = __builtin_convertvector(v01, amp_f16x2), h23 = __builtin_convertvector(v23, amp_f16x2);
    h.x = __builtin_bit_cast(unsigned, h01); h.y = __builtin_bit_cast(unsigned, h23);
#ifndef AMP_SPLIT_PACKED
    asm("v_fma_mixlo_f16 %0, %1, 1.0, -%2 op_sel_hi:[0,0,1]" : "=v"(l.x) : "v"(v01.x), "v"(h.x));
    asm("v_fma_mixhi_f16 %0, %1, 1.0, -%2 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(l.x) : "v"(v01.y), "v"(h.x));
    asm("v_fma_mixlo_f16 %0, %1, 1.0, -%2 op_sel_hi:[0,0,1]" : "=v"(l.y) : "v"(v23.x), "v"(h.y));
    asm("v_fma_mixhi_f16 %0, %1, 1.0, -%2 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(l.y) : "v"(v23.y), "v"(h.y));
#else
    const amp_f32x2 d01 = v01 - __builtin_convertvector(h01, amp_f32x2), d23 = v23 - __builtin_convertvector(h23, amp_f32x2);
    const amp_f16x2 l01 = __builtin_convertvector(d01, amp_f16x2), l23 = __builtin_convertvector(d23, amp_f16x2);
    l.x = __builtin_bit_cast(unsigned, l01); l.y = __builtin_bit_cast(unsigned, l23);
#endif
}

// leaky-ReLU-on-load + x16 of four staged values (x already zeroed where the conv pads) -> hi / lo planes; keeps the
// running maximum of |staged operand| for the range guard
__device__ __forceinline__ void stage4_f16(float x0, float x1, float x2, float x3, float kpos, float kneg, float& range_max,
                                           uint2& h, uint2& l) {
    const amp_f32x2 x01 = {x0, x1}, x23 = {x2, x3};
    const amp_f32x2 a01 = x01 * kpos, a23 = x23 * kpos, b01 = x01 * kneg, b23 = x23 * kneg;
    const amp_f32x2 v01 = {__builtin_fmaxf(a01.x, b01.x), __builtin_fmaxf(a01.y, b01.y)};
    const amp_f32x2 v23 = {__builtin_fmaxf(a23.x, b23.x), __builtin_fmaxf(a23.y, b23.y)};
    range_max = __builtin_fmaxf(range_max, __builtin_fmaxf(__builtin_fabsf(v01.x), __builtin_fabsf(v01.y)));
    range_max = __builtin_fmaxf(range_max, __builtin_fmaxf(__builtin_fabsf(v23.x), __builtin_fabsf(v23.y)));
    split4_f16(v01, v23, h, l);
}

// the fused pair's seam: four conv1 accumulators -> leaky ReLU -> conv2's zero padding (`qok`) -> x16 -> hi / lo planes.
// Same values as the scalar form (v = acc * isc; v = v > 0 ? v : v * slope; v = qok ? v * 16 : 0): max(v, v * slope) is that leaky
// ReLU for slope <= 1, and the x16 and the padding are folded into the un-scaling factor -- isc * 16 is a power of two, so
// acc * (isc * 16) == (acc * isc) * 16 and ((acc * isc) * 16) * slope == ((acc * isc) * slope) * 16 bit for bit, and a factor 0 gives
// the padding's zero (round 4: 4 packed multiplies + 4 max instead of 6 + 4 + 4 selects per four values; the seams are a fifth of
// the whole-resblock launches, all VALU).
__device__ __forceinline__ void seam4_f16(float c0, float c1, float c2, float c3, float isc, float slope, bool qok,
                                          float& range_max, uint2& h, uint2& l) {
    const float k = qok ? isc * 16.f : 0.f;
    const amp_f32x2 c01 = {c0, c1}, c23 = {c2, c3};
    const amp_f32x2 w01 = c01 * k, w23 = c23 * k;
    const amp_f32x2 n01 = w01 * slope, n23 = w23 * slope;
    const amp_f32x2 v01 = {__builtin_fmaxf(w01.x, n01.x), __builtin_fmaxf(w01.y, n01.y)};
    const amp_f32x2 v23 = {__builtin_fmaxf(w23.x, n23.x), __builtin_fmaxf(w23.y, n23.y)};
    range_max = __builtin_fmaxf(range_max, __builtin_fmaxf(__builtin_fabsf(v01.x), __builtin_fabsf(v01.y)));
    range_max = __builtin_fmaxf(range_max, __builtin_fmaxf(__builtin_fabsf(v23.x), __builtin_fabsf(v23.y)));
    split4_f16(v01, v23, h, l);
}

}  // namespace amp
