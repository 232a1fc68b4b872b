// Conv2d 3 x 3, zero padding 1, as a split-f16 implicit GEMM: every conv of AudioLDM's UNet (models/tta/ldm/audioldm.py) and of the
// AutoencoderKL decoder (models/tta/autoencoder/autoencoder.py).  A feature map [B, C, H, W] is the library's [B, C, T] with T = H W and
// row pitch W.  y[b, m, (oy, ox)] = bias[m] + sum_{tap, c} w[m, c, tap] * a(x)[b, c, (oy s + dy, ox s + dx)] with tap = (dy + 1) * 3 + (dx + 1),
// a tap outside the (virtual) input contributing exactly 0, plus the run-time options of amp_conv2d_forward:
//     stride 2         the UNet's Downsample (padding 1, output floor((H - 1) / 2) + 1)
//     up2              the conv reads the nearest-neighbour x2 up-sampling of x: source (iy >> 1, ix >> 1) of a 2H x 2W virtual input that
//                      is never written
//     norm on load     a staged element is silu((x - mean_g) * rstd_g * gamma_c + beta_c) (GroupNorm(32) + SiLU); the padding stays 0
//     epilogue         + bias, + row_add[b, m], + residual[b, m, t]
// The GEMM: K = 9 Cin' (index = tap * Cin' + channel, Cin' = Cin rounded up to 32) streams through two LDS buffers in chunks of 16 KS
// channels of ONE tap, the way ns2_layer_f16x3.hip streams its three taps; the chunk's columns are gathered per tap, so neither the row
// edge nor the stride nor the up-sampling ever enters a halo.  The N axis is the B Ho Wo output positions of the whole batch, 64 per
// workgroup: a tile may span several rows and several items (a column's sum never depends on its neighbours).  A workgroup owns 2 MI row
// blocks: wave (wm, wn) columns 32 wn .. + 31 and row blocks slab + wm + 2 i.
// Two regimes behind one entry.  At the UNet's sizes (B Ho Wo <= 390 columns against up to 18.9 M weights) the launch is a weight stream:
// MI = 1 halves the slab and K is cut into `ksplit` slices (blockIdx.z), each writing its partial sums to the workspace; a second launch
// adds the slices in slice order and applies the epilogue.  MI, KS and ksplit are functions of the conv's geometry and Ho Wo alone, never
// of B: an item's bits do not depend on what it is batched with.  At the decoder's sizes (49 920 columns at C = 128) ksplit = 1 and the
// epilogue runs on the accumulators.
// Deterministic: fixed summation order, no atomics except the range flag.  Layouts and arithmetic: wholek_f16x3.h / f16x3_device.h.
#include <memory>

#include "amp_host.h"
#include "amphion_hip.h"
#include "wholek_f16x3.h"

namespace amp {

constexpr int C2_TN = 64;          // output positions per workgroup
constexpr int C2_MAX_SPLIT = 32;        // K slices at most
constexpr int C2_WG_TARGET = 512;       // workgroups a weight-streaming launch aims at: two per CU
constexpr int C2_MIN_STEPS = 4;         // K chunks a slice keeps at least

struct Conv2dArgs {
    const float* x;            // [B, Cin, H, W]
    const float* mr;           // [B, 32, 2] mean | rstd, or nullptr
    const float* gamma;        // [Cin]
    const float* beta;         // [Cin]
    const uint4* wp;           // [Cout', 9 Cin'] as packed A fragments
    const float* bias;         // [Cout']
    const float* row_add;      // [Cout] per item, row_bs apart, or nullptr
    long long row_bs;
    const float* residual;     // [B, Cout, To] or nullptr
    float* y;                  // [B, Cout, To]
    float* part;               // ksplit > 1: [ksplit, B, Cout', To] partial sums
    int Cin, Cinp, Cout, NP;   // NP = Cout' / 32
    int H, W, Hv, Wv;          // source extent and the extent the taps are tested against (2H x 2W under up2)
    int Wo, To;
    int stride, up;            // up: 0 | 1, the shift of the source coordinates
    long long ncols;           // B * To
    int K16, nsteps, ksplit;
    float inv;
    unsigned* range_flag;
};

// silu with the hardware's exp2 / rcp (1 ulp each): the activation is formed once per tap and element, nine times per element of x
__device__ __forceinline__ float c2_silu(float v) {
    return v * __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(v * -1.4426950408889634f));
}

template <int KS, int MI, bool NORM>
__global__ __launch_bounds__(256, 2) void conv2d_f16x3_kernel(const Conv2dArgs a) {
    constexpr int TN = C2_TN;
    constexpr int KC = 16 * KS;
    constexpr int PLANE = 2 * KS * TN;          // uint4 per plane: [channel octet][TN]
    constexpr int BUF = 2 * PLANE;              // uint4 per buffer: [plane hi | lo]
    constexpr int NST = KS;                     // staging items (channel quad x column) per thread: 4 KS quads x 64 columns / 256
    __shared__ __attribute__((aligned(16))) uint4 c2_smem[2 * BUF];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int hi = lane >> 5, l31 = lane & 31;
    const int Cin = a.Cin, Cinp = a.Cinp, K16 = a.K16;
    const size_t HW = (size_t)a.H * a.W;

    // ---- the staged column of this lane: output position (item, oy, ox), clamped to the last one beyond the batch (never stored) ----
    const long long g0 = (long long)blockIdx.x * TN;
    long long gs = g0 + lane;
    if (gs > a.ncols - 1) gs = a.ncols - 1;
    const int s_item = (int)(gs / a.To);
    const int s_t = (int)(gs - (long long)s_item * a.To);
    const int s_oy = s_t / a.Wo, s_ox = s_t - s_oy * a.Wo;
    const float* xb = a.x + (size_t)s_item * Cin * HW;
    const float* mrb = NORM ? a.mr + (size_t)s_item * 64 : nullptr;
    const int cpg = Cin >> 5;                   // channels per group (NORM: Cin is a multiple of 32)

    // K slice of this workgroup: chunks [s_lo, s_hi)
    const int s_lo = (int)(((long long)a.nsteps * blockIdx.z) / a.ksplit);
    const int s_hi = (int)(((long long)a.nsteps * (blockIdx.z + 1)) / a.ksplit);

    float range_max = 0.f;
    float xs[NST][4];
    float nm[NORM ? NST : 1][4], nr[NORM ? NST : 1][4], ng[NORM ? NST : 1][4], nb[NORM ? NST : 1][4];
    // whether tap `tap` of the lane's position lies inside the (virtual) input, and its source offset (clamped inside when it does not)
    auto tap_src = [&](int tap, size_t& off) {
        const int ty = tap / 3;
        const int iy = s_oy * a.stride + ty - 1, ix = s_ox * a.stride + (tap - 3 * ty) - 1;
        const bool ok = iy >= 0 && iy < a.Hv && ix >= 0 && ix < a.Wv;
        const int cy = iy < 0 ? 0 : (iy > a.Hv - 1 ? a.Hv - 1 : iy), cx = ix < 0 ? 0 : (ix > a.Wv - 1 ? a.Wv - 1 : ix);
        off = (size_t)(cy >> a.up) * a.W + (cx >> a.up);
        return ok;
    };
    auto stage_load = [&](int s) {
        const int k0 = s * KC;
        const int tap = k0 / Cinp;
        const int cb = k0 - tap * Cinp;
        size_t off;
        (void)tap_src(tap, off);
#pragma unroll
        for (int it = 0; it < NST; ++it) {
            const int c0 = cb + 4 * (4 * it + wave);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int c = c0 + e < Cin ? c0 + e : Cin - 1;      // Cin = 4: channels [4, 32) are padding (zero weights, staged as zero)
                xs[it][e] = xb[(size_t)c * HW + off];
                if (NORM) {
                    const int grp = c / cpg;
                    nm[it][e] = mrb[2 * grp];
                    nr[it][e] = mrb[2 * grp + 1];
                    ng[it][e] = a.gamma[c];
                    nb[it][e] = a.beta[c];
                }
            }
        }
    };
    auto stage_store = [&](int s, int buf) {
        const int k0 = s * KC;
        const int tap = k0 / Cinp;
        const int cb = k0 - tap * Cinp;
        size_t off;
        const bool ok = tap_src(tap, off);
        uint2* dst = reinterpret_cast<uint2*>(c2_smem + buf * BUF);
#pragma unroll
        for (int it = 0; it < NST; ++it) {
            const int c0 = cb + 4 * (4 * it + wave);
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float t = xs[it][e];
                if (NORM) t = c2_silu((t - nm[it][e]) * nr[it][e] * ng[it][e] + nb[it][e]);
                v[e] = (ok && c0 + e < Cin) ? t : 0.f;              // the conv pads the ACTIVATED tensor: a tap outside contributes 0
            }
            uint2 fh, fl;
            stage4_f16(v[0], v[1], v[2], v[3], 16.f, 16.f, range_max, fh, fl);
            bplane_store(dst, 2 * PLANE, bplane_idx(4 * it + wave, lane, TN), fh, fl);
        }
    };

    // ---- the wave's row blocks p0 + 2 i (MI = 2: NP is a multiple of 4; MI = 1: a wave beyond NP only stages) ----
    const int p0 = blockIdx.y * 2 * MI + wm;
    const bool active = p0 < a.NP;
    f32x16 acc[MI][1];
    Frag ah[MI], al[MI];
    const size_t mbs = (size_t)2 * K16 * 128;
    const uint4* wa = a.wp + (size_t)(active ? p0 : 0) * K16 * 128 + lane;
#pragma unroll
    for (int i = 0; i < MI; ++i) acc_zero(acc[i][0]);
    if (active) afrag_load<MI>(ah, al, wa + (size_t)s_lo * KS * 128, mbs);

    stage_load(s_lo);
    AMP_PIN_VMEM();
    stage_store(s_lo, 0);
    __syncthreads();

    const int rd0 = hi * TN + wn * 32 + l31;
    const APack A{wa, mbs, K16};
    for (int s = s_lo; s < s_hi; ++s) {
        const bool more = s + 1 < s_hi;
        if (more) {
            stage_load(s + 1);
            AMP_PIN_VMEM();
        }
        const uint4* buf = c2_smem + ((s - s_lo) & 1) * BUF;
        if (active) gemm_wholek<MI, true>(acc, ah, al, A, s * KS, KS, buf, PLANE, TN, rd0);
        if (more) stage_store(s + 1, (s + 1 - s_lo) & 1);
        __syncthreads();
    }
    raise_range(a.range_flag, range_max, lane);

    // ---- epilogue: lane (hi, l31), register r of block i holds row acc_row(r, hi, 32 p), column g ----
    const long long g = g0 + wn * 32 + l31;
    if (g >= a.ncols || !active) return;
    const int item = (int)(g / a.To);
    const int t = (int)(g - (long long)item * a.To);
    if (a.ksplit > 1) {
        const int Mp = a.NP * 32;
        const int B = (int)(a.ncols / a.To);
        float* pb = a.part + (((size_t)blockIdx.z * B + item) * Mp) * a.To + t;
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) pb[(size_t)acc_row(r, hi, 32 * (p0 + 2 * i)) * a.To] = acc[i][0][r] * a.inv;
        return;
    }
    const size_t yo = (size_t)item * a.Cout * a.To + t;
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = acc_row(r, hi, 32 * (p0 + 2 * i));
            if (m >= a.Cout) continue;
            float v = acc[i][0][r] * a.inv + a.bias[m];
            if (a.row_add) v += a.row_add[(size_t)item * (size_t)a.row_bs + m];
            if (a.residual) v += a.residual[yo + (size_t)m * a.To];
            a.y[yo + (size_t)m * a.To] = v;
        }
}

// the second launch of the K-split form: the slices in slice order, then the same epilogue
__global__ __launch_bounds__(256) void conv2d_combine_kernel(const float* __restrict__ part, int ksplit, int Mp, const float* __restrict__ bias,
                                                             const float* __restrict__ row_add, long long row_bs, const float* residual, float* y, int Cout,
                                                             int To) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= To) return;
    const int m = blockIdx.y, b = blockIdx.z, B = gridDim.z;
    float v = 0.f;
    for (int s = 0; s < ksplit; ++s) v += part[(((size_t)s * B + b) * Mp + m) * To + t];
    v += bias[m];
    if (row_add) v += row_add[(size_t)b * (size_t)row_bs + m];
    const size_t o = ((size_t)b * Cout + m) * To + t;
    if (residual) v += residual[o];
    y[o] = v;
}

}  // namespace amp

using namespace amp;

struct amp_conv2d {
    int cin = 0, cout = 0, cinp = 0, np = 0;
    int precision = PREC_F16X3;
    DeviceAllocs mem;
    uint4* wp = nullptr;
    float* bias = nullptr;
    float inv = 1.f;
};

namespace {

struct C2Plan {
    int Ho, Wo, To, ks, mi, ksplit, nsteps;
    unsigned tiles, ny;
};

bool c2_geometry_ok(int cin, int cout) {
    const bool ci = cin == 4 || (cin >= 32 && cin <= 2048 && cin % 32 == 0);
    const bool co = cout == 1 || cout == 4 || (cout >= 32 && cout <= 1024 && cout % 32 == 0);
    return ci && co;
}

// everything but `tiles` is a function of the handle and the feature map alone (never of B)
int c2_plan(const amp_conv2d* h, int B, int H, int W, int stride, int up2, C2Plan* p) {
    if (B < 1 || H < 1 || W < 1 || B > 65535) { set_error("amp_conv2d: B=%d H=%d W=%d", B, H, W); return AMP_ERR_INVALID; }
    if (stride != 1 && stride != 2) { set_error("amp_conv2d: stride=%d is not covered (1 or 2)", stride); return AMP_ERR_UNSUPPORTED; }
    if (up2 && stride != 1) { set_error("amp_conv2d: up2 with stride 2 is not covered"); return AMP_ERR_UNSUPPORTED; }
    if ((long long)H * W >= (1ll << 24)) { set_error("amp_conv2d: H*W=%lld is not covered (below 2^24)", (long long)H * W); return AMP_ERR_UNSUPPORTED; }
    p->Ho = up2 ? 2 * H : (H - 1) / stride + 1;
    p->Wo = up2 ? 2 * W : (W - 1) / stride + 1;
    p->To = p->Ho * p->Wo;
    const long long ncols = (long long)B * p->To;
    if (ncols > 0x7fffffffll - C2_TN) { set_error("amp_conv2d: B*Ho*Wo=%lld is beyond the grid", ncols); return AMP_ERR_UNSUPPORTED; }
    p->ks = h->cinp % 64 == 0 ? 4 : 2;
    p->nsteps = 9 * h->cinp / (16 * p->ks);
    const int tiles1 = (p->To + C2_TN - 1) / C2_TN;            // of ONE item: the plan may not depend on B
    p->mi = (h->np % 4 == 0 && (long long)tiles1 * (h->np / 4) >= 256) ? 2 : 1;
    p->ny = (unsigned)((h->np + 2 * p->mi - 1) / (2 * p->mi));
    p->ksplit = 1;
    while ((long long)tiles1 * p->ny * p->ksplit < C2_WG_TARGET && p->ksplit < C2_MAX_SPLIT && p->nsteps / (2 * p->ksplit) >= C2_MIN_STEPS) p->ksplit *= 2;
    p->tiles = (unsigned)((ncols + C2_TN - 1) / C2_TN);
    return AMP_OK;
}

template <int KS, int MI>
void c2_launch(bool norm, dim3 grid, hipStream_t stream, const Conv2dArgs& a) {
    if (norm) hipLaunchKernelGGL((conv2d_f16x3_kernel<KS, MI, true>), grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL((conv2d_f16x3_kernel<KS, MI, false>), grid, dim3(256), 0, stream, a);
}

}  // namespace

extern "C" {

int amp_conv2d_create(int cin, int cout, const float* weight_host, const float* bias_host, amp_conv2d** out) {
    if (!out || !weight_host) { set_error("amp_conv2d_create: null argument"); return AMP_ERR_INVALID; }
    *out = nullptr;
    if (!c2_geometry_ok(cin, cout)) {
        set_error("amp_conv2d_create: %d -> %d channels is not covered (Cin 4 or a multiple of 32 up to 2048, Cout 1, 4 or a multiple of 32 up to 1024)", cin, cout);
        return AMP_ERR_UNSUPPORTED;
    }
    if (amp_get_precision() != PREC_F16X3) {
        set_error("amp_conv2d_create: built for the f16x3 arithmetic only (under f32 the drop-in modules run the conv in torch)");
        return AMP_ERR_UNSUPPORTED;
    }
    if (amp_device_count() <= 0) { set_error("amp_conv2d_create: no HIP device visible (the HIP path has no CPU fallback)"); return AMP_ERR_HIP; }
    std::unique_ptr<amp_conv2d> h(new amp_conv2d);
    h->cin = cin; h->cout = cout;
    h->cinp = (cin + 31) / 32 * 32;
    h->np = (cout + 31) / 32;
    const int cinp = h->cinp;
    std::vector<_Float16> wp;
    // K index = tap * Cin' + channel of the Conv2d weight [Cout, Cin, 3, 3]
    AMP_RC(pack_matrix_f16x3("amp_conv2d_create", cout, 9 * cinp, h->np, 9 * cinp / 16,
                             [&](int m, int i) { const int c = i % cinp; return c < cin ? weight_host[((size_t)m * cin + c) * 9 + i / cinp] : 0.f; }, &wp, &h->inv));
    AMP_RC(h->mem.upload(wp, &h->wp));
    std::vector<float> bias((size_t)h->np * 32, 0.f);
    if (bias_host) std::copy(bias_host, bias_host + cout, bias.begin());
    AMP_RC(h->mem.upload(bias, &h->bias));
    *out = h.release();
    return AMP_OK;
}

int amp_conv2d_precision(const amp_conv2d* h) { return h ? h->precision : -1; }

int amp_conv2d_plan(const amp_conv2d* h, int H, int W, int stride, int up2, int* k_slices, int* row_blocks_per_wave, int* chunk_channels) {
    if (!h) { set_error("amp_conv2d_plan: null handle"); return AMP_ERR_INVALID; }
    C2Plan p;
    AMP_RC(c2_plan(h, 1, H, W, stride, up2, &p));
    if (k_slices) *k_slices = p.ksplit;
    if (row_blocks_per_wave) *row_blocks_per_wave = p.mi;
    if (chunk_channels) *chunk_channels = 16 * p.ks;
    return AMP_OK;
}

size_t amp_conv2d_workspace_bytes(const amp_conv2d* h, int B, int H, int W, int stride, int up2) {
    C2Plan p;
    if (!h || c2_plan(h, B, H, W, stride, up2, &p) != AMP_OK) return 0;
    return p.ksplit > 1 ? (size_t)p.ksplit * B * h->np * 32 * p.To * sizeof(float) : 0;
}

int amp_conv2d_forward(const amp_conv2d* h, const float* x_dev, int B, int H, int W, int stride, int up2, const float* mean_rstd_dev,
                       const float* gamma_dev, const float* beta_dev, const float* row_add_dev, long long row_add_batch_stride,
                       const float* residual_dev, float* y_dev, void* ws_dev, size_t ws_bytes, void* stream_) {
    if (!h || !x_dev || !y_dev) { set_error("amp_conv2d_forward: null argument"); return AMP_ERR_INVALID; }
    C2Plan p;
    AMP_RC(c2_plan(h, B, H, W, stride, up2, &p));
    const bool norm = mean_rstd_dev != nullptr;
    if (norm && (!gamma_dev || !beta_dev)) { set_error("amp_conv2d_forward: mean_rstd without gamma / beta"); return AMP_ERR_INVALID; }
    if (norm && h->cin % 32) { set_error("amp_conv2d_forward: GroupNorm(32) on load needs Cin a multiple of 32, got %d", h->cin); return AMP_ERR_UNSUPPORTED; }
    if (row_add_batch_stride == 0) row_add_batch_stride = h->cout;
    if (row_add_dev && row_add_batch_stride < h->cout) { set_error("amp_conv2d_forward: row_add batch stride %lld < Cout", row_add_batch_stride); return AMP_ERR_INVALID; }
    const size_t need = amp_conv2d_workspace_bytes(h, B, H, W, stride, up2);
    if (need && (!ws_dev || ws_bytes < need)) { set_error("amp_conv2d_forward: workspace of %zu bytes, %zu needed", ws_dev ? ws_bytes : (size_t)0, need); return AMP_ERR_INVALID; }
    const size_t xbytes = (size_t)B * h->cin * H * W * sizeof(float), ybytes = (size_t)B * h->cout * p.To * sizeof(float);
    if (ranges_overlap(x_dev, xbytes, y_dev, ybytes)) { set_error("amp_conv2d_forward: y overlaps x"); return AMP_ERR_INVALID; }
    if (residual_dev && ranges_overlap(residual_dev, ybytes, y_dev, ybytes)) { set_error("amp_conv2d_forward: y overlaps the residual"); return AMP_ERR_INVALID; }
    if (need && (ranges_overlap(ws_dev, need, y_dev, ybytes) || ranges_overlap(ws_dev, need, x_dev, xbytes) ||
                 (residual_dev && ranges_overlap(ws_dev, need, residual_dev, ybytes)))) {
        set_error("amp_conv2d_forward: the workspace overlaps a tensor");
        return AMP_ERR_INVALID;
    }
    hipStream_t stream = (hipStream_t)stream_;
    Conv2dArgs a{};
    a.x = x_dev; a.mr = mean_rstd_dev; a.gamma = gamma_dev; a.beta = beta_dev;
    a.wp = h->wp; a.bias = h->bias;
    a.row_add = row_add_dev; a.row_bs = row_add_batch_stride; a.residual = residual_dev;
    a.y = y_dev; a.part = (float*)ws_dev;
    a.Cin = h->cin; a.Cinp = h->cinp; a.Cout = h->cout; a.NP = h->np;
    a.H = H; a.W = W; a.Hv = up2 ? 2 * H : H; a.Wv = up2 ? 2 * W : W;
    a.Wo = p.Wo; a.To = p.To;
    a.stride = stride; a.up = up2 ? 1 : 0;
    a.ncols = (long long)B * p.To;
    a.K16 = 9 * h->cinp / 16; a.nsteps = p.nsteps; a.ksplit = p.ksplit;
    a.inv = h->inv;
    a.range_flag = range_flag_for_current_device();
    const dim3 grid(p.tiles, p.ny, (unsigned)p.ksplit);
    note_kernel("conv2d_f16x3_kernel", p.ks, p.mi, norm ? 1 : 0);
    note_work((unsigned long long)grid.x * grid.y * grid.z, 2.0 * 9 * h->cin * h->cout * (double)a.ncols / 1e9,
              (4.0 * 9 * h->cinp * h->np * 32 * grid.x + 4.0 * a.ncols * (9.0 * h->cin * grid.y + h->cout)) / 1e6,
              "conv2d %d->%d %dx%d->%dx%d stride=%d up2=%d norm=%d B=%d ksplit=%d", h->cin, h->cout, H, W, p.Ho, p.Wo, stride, up2 ? 1 : 0, norm ? 1 : 0, B, p.ksplit);
    if (p.ks == 4) {
        if (p.mi == 2) c2_launch<4, 2>(norm, grid, stream, a); else c2_launch<4, 1>(norm, grid, stream, a);
    } else {
        if (p.mi == 2) c2_launch<2, 2>(norm, grid, stream, a); else c2_launch<2, 1>(norm, grid, stream, a);
    }
    AMP_HIP(hipGetLastError());
    if (p.ksplit > 1) {
        const dim3 cgrid((unsigned)((p.To + 255) / 256), (unsigned)h->cout, (unsigned)B);
        note_kernel("conv2d_combine_kernel");
        note_work((unsigned long long)cgrid.x * cgrid.y * cgrid.z, 0.0, 4.0 * a.ncols * h->cout * (p.ksplit + 2) / 1e6, "conv2d combine %d slices Cout=%d To=%d B=%d",
                  p.ksplit, h->cout, p.To, B);
        hipLaunchKernelGGL(conv2d_combine_kernel, cgrid, dim3(256), 0, stream, (const float*)ws_dev, p.ksplit, h->np * 32, (const float*)h->bias, row_add_dev, row_add_batch_stride, residual_dev,
                           y_dev, h->cout, p.To);
        AMP_HIP(hipGetLastError());
    }
    return AMP_OK;
}

void amp_conv2d_destroy(amp_conv2d* h) { delete h; }

}  // extern "C"
