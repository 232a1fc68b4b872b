// Down-sampling convolution of the Coco tokenizer (models/codec/coco/rep_coco_model.py: downsample_layers, Conv1d(C, C, k = 3, stride 2,
// padding 1) -> GELU) on channel-first activations:
//     y[b, o, t] = epi( bias[o] + sum_c sum_{j<3} w[o, c, j] * x[b, c, 2t + j - 1] ),   T_out = (T - 1) / 2 + 1
// with the epilogue chosen at compile time: bias, or bias + exact-erf GELU (gelu_erf.h).  Also the element-wise GELU entry (amp_gelu) that the
// up-sampling side and the exact-fp32 route need.
//
// Arithmetic and structure follow pw_f16x3.hip: the f16x3 scheme (f16x3_device.h; operand layouts and fragment loads: wholek_f16x3.h), weights
// packed on the host by pack_a_f16x3 with three taps -- [row block][k16][tap][plane][lane] x 16 B -- and streamed from L2 in that order, a K
// step of 64 channels with one barrier, two LDS buffers so that the loads of step s + 1 fly under the MFMAs of step s, four waves as 2 x 2.
//
// The staged window.  A tile of TN output columns from q0 reads input columns 2 q0 - 1 .. 2 q0 + 2 TN - 1.  A staging item is (input column,
// channel quad): consecutive lanes load consecutive input columns (coalesced rows) and write them to LDS as TWO column planes inside each
// channel octet's row of S = 2 TN + 1 columns:
//     E[i] = x[2 (q0 + i)]       at column i,           i <  TN
//     O[i] = x[2 (q0 + i) - 1]   at column TN + i,      i <= TN
// so tap 0 reads O at q, tap 1 E at q and tap 2 O at q + 1: every B fragment stays one contiguous 16-byte read.  Input column -1 and input
// columns >= T are SELECTED to 0 (the load address alone is clamped), channels >= Cin are 0, and every staged value feeds the range flag.
// Deterministic: each output is one workgroup's sum over (k-extent, tap) in that order; no split-K, no atomics except the range flag.
#include <algorithm>
#include <memory>

#include "amp_host.h"
#include "wholek_f16x3.h"
#include "gelu_erf.h"

namespace amp {

constexpr int DS_KS = 4;            // MFMA k-extents (16 channels each) per K step
constexpr int DS_KC = 16 * DS_KS;   // channels per K step
constexpr int DS_MROWS = 128;       // packed rows are padded to this (the larger tile's height)
constexpr int DS_EXT = 3 * 128;     // uint4 per packed k-extent of one row block: [tap][plane][lane]

struct DsArgs {
    const float* x;       // [B, Cin, T]
    const uint4* wp;      // packed hi / lo fragments, see amp_dsconv_create
    const float* bias;    // [Cout]
    float* y;             // [B, Cout, Tout]
    int Cin, Cout, T, Tout;
    int nsteps;           // K steps of DS_KC channels
    int nc16;             // packed k-extents per row block = nsteps * DS_KS
    int tiles_per_item;   // ceil(Tout / TN)
    float inv_scale;      // 1 / (16 * 2^s)
    unsigned* range_flag;
};

// the 128-column tile holds 2 x 66 KB of LDS: one workgroup per CU, so it may take the whole register file
template <int GELU, int MI, int NI>
__global__ __launch_bounds__(256, NI == 2 ? 1 : 2) void dsconv_f16x3_kernel(const DsArgs a) {
    constexpr int TN = 64 * NI;                     // output columns per workgroup
    constexpr int S = 2 * TN + 1;                   // staged columns per channel octet: E [0, TN), O [TN, 2 TN]
    constexpr int NST = (4 * DS_KS * 2 * TN) / 256; // staging items (input column x channel quad) per thread, without the last O column
    constexpr int PLANE = 2 * DS_KS * S;            // uint4 per plane
    constexpr int BUF = 2 * PLANE;                  // uint4 per LDS buffer: [plane][octet][S]
    extern __shared__ __attribute__((aligned(16))) uint4 ds_smem[];   // [2][BUF]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int hi = lane >> 5, l31 = lane & 31;
    const int bx = blockIdx.x;
    const int item = bx / a.tiles_per_item;
    const int q0 = (bx - item * a.tiles_per_item) * TN;
    const int mb0 = blockIdx.y * (2 * MI) + wm * MI;     // first 32-row block of this wave

    f32x16 acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int t = 0; t < NI; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][t][r] = 0.f;

    const int T = a.T, Cin = a.Cin;
    const float* xb = a.x + (size_t)item * (size_t)Cin * T;
    const int t0 = 2 * q0 - 1;                      // input column of staged column j = 0
    float range_max = 0.f;
    float xs[NST + 1][4];
    // staging item i = wave * 64 + 256 * it + lane: channel quad (i / 2 TN, wave-uniform) x window column j = i % 2 TN, input column t0 + j;
    // item NST is the window's last column j = 2 TN (= O[TN]) of quad tid & 15, stored by threads 0 .. 15
    auto item_of = [&](int it, int& qd, int& j) {
        if (it < NST) {
            const int ibase = wave * 64 + 256 * it;
            qd = ibase / (2 * TN);
            j = ibase - qd * (2 * TN) + lane;
        } else {
            qd = tid & 15;
            j = 2 * TN;
        }
    };
    auto stage_load = [&](int step) {
#pragma unroll
        for (int it = 0; it <= NST; ++it) {
            int qd, j;
            item_of(it, qd, j);
            int t = t0 + j;
            t = t > T - 1 ? T - 1 : t;
            t = t < 0 ? 0 : t;
            const int ch0 = step * DS_KC + 4 * qd;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                int ch = ch0 + e;
                ch = ch > Cin - 1 ? Cin - 1 : ch;
                xs[it][e] = xb[(size_t)ch * T + t];
            }
        }
    };
    auto stage_store = [&](int step, int buf) {
        uint2* dst = reinterpret_cast<uint2*>(ds_smem + buf * BUF);
#pragma unroll
        for (int it = 0; it <= NST; ++it) {
            int qd, j;
            item_of(it, qd, j);
            const int t = t0 + j;
            const bool tok = t >= 0 && t < T;
            const int ch0 = step * DS_KC + 4 * qd;
            uint2 fh, fl;
            stage4_f16((tok && ch0 + 0 < Cin) ? xs[it][0] : 0.f, (tok && ch0 + 1 < Cin) ? xs[it][1] : 0.f,
                       (tok && ch0 + 2 < Cin) ? xs[it][2] : 0.f, (tok && ch0 + 3 < Cin) ? xs[it][3] : 0.f, 16.f, 16.f, range_max, fh, fl);
            const int col = (j & 1) ? (j >> 1) : TN + (j >> 1);      // odd window columns are the even input columns: plane E
            if (it < NST || tid < 16) bplane_store(dst, 2 * PLANE, bplane_idx(qd, col, S), fh, fl);
        }
    };

    // A fragments: entry (mb, c16, tap, plane) of the pack at (((mb * nc16 + c16) * 3 + tap) * 2 + plane) * 64.  Two k-extents are held (slot =
    // extent & 1); a tap's fragments are re-loaded for extent + 2 right after their last use.
    const uint4* wa = a.wp + (size_t)mb0 * a.nc16 * DS_EXT + lane;
    const size_t mbs = (size_t)a.nc16 * DS_EXT;           // uint4 per row block
    Frag ah[2][3][MI], al[2][3][MI];
#pragma unroll
    for (int sl = 0; sl < 2; ++sl)
#pragma unroll
        for (int g = 0; g < 3; ++g) afrag_load<MI>(ah[sl][g], al[sl][g], wa + sl * DS_EXT + g * 128, mbs);
    stage_load(0);
    AMP_PIN_VMEM();
    stage_store(0, 0);
    __syncthreads();

    const int rd0 = hi * S + wn * (32 * NI) + l31;
    auto step = [&](const int s, const bool more) __attribute__((always_inline)) {
        if (more) {
            stage_load(s + 1);
            AMP_PIN_VMEM();
        }
        const uint4* base = ds_smem + (s & 1) * BUF + rd0;
#pragma unroll
        for (int h = 0; h < DS_KS; ++h) {
            const uint4* bg = base + (2 * h) * S;
#pragma unroll
            for (int g = 0; g < 3; ++g) {
                const int off = g == 0 ? TN : (g == 1 ? 0 : TN + 1);
                Frag bh[NI], bl[NI];
#pragma unroll
                for (int t = 0; t < NI; ++t) bfrag_load(bg, PLANE, off + 32 * t, bh[t], bl[t]);
                mfma3_tiles<MI, NI>(acc, ah[h & 1][g], al[h & 1][g], bh, bl);
                if (h + 2 < DS_KS || more) {
                    afrag_load<MI>(ah[h & 1][g], al[h & 1][g], wa + (h + 2) * DS_EXT + g * 128, mbs);
                    AMP_PIN_VMEM();
                }
            }
        }
        wa += DS_KS * DS_EXT;
        if (more) stage_store(s + 1, (s + 1) & 1);
        __syncthreads();
    };
    const int nsteps = a.nsteps;
    for (int s = 0; s + 1 < nsteps; ++s) step(s, true);
    step(nsteps - 1, false);

    raise_range(a.range_flag, range_max, lane);

    // ---- epilogue: lane (hi, l31), register r of tile (i, t) holds row acc_row(r, hi), column 32 t + l31 ----
    const int Tout = a.Tout;
    const size_t ybase = (size_t)item * a.Cout * Tout;
#pragma unroll
    for (int i = 0; i < MI; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = acc_row(r, hi, (mb0 + i) * 32);
            if (m >= a.Cout) continue;
            const float bv = a.bias[m];
            const size_t row = ybase + (size_t)m * Tout;
#pragma unroll
            for (int t = 0; t < NI; ++t) {
                const int q = q0 + wn * (32 * NI) + 32 * t + l31;
                if (q >= Tout) continue;
                float v = acc[i][t][r] * a.inv_scale + bv;
                if (GELU) v = gelu_erf(v);
                a.y[row + q] = v;
            }
        }
    }
}

template <int GELU, int MI, int NI>
static hipError_t ds_launch_one(const DsArgs& a, int B, hipStream_t stream) {
    constexpr int TN = 64 * NI;
    const size_t lds = (size_t)2 * 2 * 2 * DS_KS * (2 * TN + 1) * sizeof(uint4);
    if (hipError_t e = ensure_dynamic_lds<&dsconv_f16x3_kernel<GELU, MI, NI>>(lds); e != hipSuccess) return e;
    const dim3 grid((unsigned)(B * a.tiles_per_item), (unsigned)((a.Cout + 64 * MI - 1) / (64 * MI)));
    note_kernel("dsconv_f16x3_kernel", GELU, MI, NI);
    if (manifest_on()) {
        const double gf = 2.0 * a.Cout * (double)a.Cin * 3 * a.Tout * B / 1e9;
        const double mb = 4.0 * B * ((double)a.Cin * a.T + (double)a.Cout * a.Tout) / 1e6;
        note_work((unsigned long long)grid.x * grid.y, gf, mb, "dsconv %d->%d k=3 s=2 gelu=%d T=%d->%d B=%d grid=%ux%u", a.Cin, a.Cout, GELU, a.T, a.Tout,
                  B, grid.x, grid.y);
    }
    hipLaunchKernelGGL((dsconv_f16x3_kernel<GELU, MI, NI>), grid, dim3(256), lds, stream, a);
    return hipGetLastError();
}

// the large tile (one workgroup per CU: 2 x 66 KB of LDS) wherever it still gives every CU a workgroup; the small one otherwise
// (AMP_DS_BIG_MIN: the same-box A/B of the two tiles through AMP_BUILD_FLAGS)
#ifndef AMP_DS_BIG_MIN
#define AMP_DS_BIG_MIN 256
#endif
template <int GELU>
static hipError_t ds_launch(DsArgs a, int B, hipStream_t stream) {
    const long long big = (long long)B * ((a.Tout + 127) / 128) * ((a.Cout + 127) / 128);
    if (big >= AMP_DS_BIG_MIN) {
        a.tiles_per_item = (a.Tout + 127) / 128;
        return ds_launch_one<GELU, 2, 2>(a, B, stream);
    }
    a.tiles_per_item = (a.Tout + 63) / 64;
    return ds_launch_one<GELU, 1, 1>(a, B, stream);
}

// exact-fp32 route, step 1: x [rows, T] -> [rows, T + 1] with one zero column appended
__global__ __launch_bounds__(256) void dsconv_zero_col_kernel(const float* __restrict__ x, float* __restrict__ xp, int T, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const size_t row = i / (size_t)(T + 1);
    const int j = (int)(i - row * (size_t)(T + 1));
    xp[i] = j < T ? x[row * (size_t)T + j] : 0.f;
}

// element-wise exact-erf GELU; y may alias x (each thread reads its elements before it writes them).  vec: both bases 16-byte aligned -- threads
// [0, n / 4) take quads, the next n % 4 threads the tail.
__global__ __launch_bounds__(256) void gelu_kernel(const float* x, float* y, size_t n, int vec) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (vec) {
        const size_t nq = n >> 2;
        if (i < nq) {
            const float4 t = reinterpret_cast<const float4*>(x)[i];
            reinterpret_cast<float4*>(y)[i] = make_float4(gelu_erf(t.x), gelu_erf(t.y), gelu_erf(t.z), gelu_erf(t.w));
        } else {
            const size_t k = 4 * nq + (i - nq);
            if (k < n) y[k] = gelu_erf(x[k]);
        }
    } else if (i < n) {
        y[i] = gelu_erf(x[i]);
    }
}

}  // namespace amp

using namespace amp;

struct amp_dsconv {
    int cin = 0, cout = 0;
    int precision = PREC_F16X3;
    int nsteps = 0;
    float inv_scale = 1.f;
    uint4* wp_dev = nullptr;     // f16x3: packed fragments
    float* bias_dev = nullptr;   // [cout] (zeros when the conv has no bias)
    amp_sconv* sconv = nullptr;  // exact-fp32 mode: Conv1d(cin, cout, k = 4, stride 2, padding 1) with a zero fourth tap
    ~amp_dsconv() {
        if (wp_dev) (void)hipFree(wp_dev);
        if (bias_dev) (void)hipFree(bias_dev);
        if (sconv) amp_sconv_destroy(sconv);
    }
};

static long long dsconv_out_len(long long T) { return T < 1 ? 0 : (T - 1) / 2 + 1; }
// floats of the zero-column copy, rounded up so that the strided conv's own workspace behind it stays 16-byte aligned
static size_t dsconv_pad_floats(const amp_dsconv* h, int B, int T) { return ((size_t)B * h->cin * ((size_t)T + 1) + 3) & ~(size_t)3; }

extern "C" {

int amp_gelu(const float* x_dev, long long n, float* y_dev, void* stream) {
    if (!x_dev || !y_dev || n <= 0) { set_error("amp_gelu: bad argument (n=%lld)", n); return AMP_ERR_INVALID; }
    const int vec = ((reinterpret_cast<uintptr_t>(x_dev) | reinterpret_cast<uintptr_t>(y_dev)) & 15) == 0 ? 1 : 0;
    const long long threads = vec ? (n >> 2) + (n & 3) : n;
    const long long blocks = (threads + 255) / 256;
    if (blocks > 0x7fffffffll) { set_error("amp_gelu: n=%lld is beyond the grid", n); return AMP_ERR_UNSUPPORTED; }
    note_kernel("gelu_kernel");
    note_work((unsigned long long)blocks, 0.0, 8.0 * (double)n / 1e6, "gelu n=%lld", n);
    hipLaunchKernelGGL(gelu_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x_dev, y_dev, (size_t)n, vec);
    AMP_HIP(hipGetLastError());
    return AMP_OK;
}

int amp_dsconv_create(int cin, int cout, const float* weight_host, const float* bias_host, amp_dsconv** out) {
    if (!out || !weight_host || cin <= 0 || cout <= 0) { set_error("amp_dsconv_create: bad argument cin=%d cout=%d", cin, cout); return AMP_ERR_INVALID; }
    *out = nullptr;
    const size_t nw = (size_t)cout * cin * 3;
    float wmax = 0.f;
    for (size_t i = 0; i < nw; ++i) {
        const float w = fabsf(weight_host[i]);
        if (!(w < 1e30f)) { set_error("amp_dsconv_create: non-finite weight"); return AMP_ERR_INVALID; }
        wmax = fmaxf(wmax, w);
    }
    std::unique_ptr<amp_dsconv> p(new amp_dsconv);
    p->cin = cin;
    p->cout = cout;
    p->precision = amp_get_precision();
    if (p->precision == PREC_F32) {
        std::vector<float> w4((size_t)cout * cin * 4, 0.f);
        for (size_t r = 0; r < (size_t)cout * cin; ++r)
            for (int j = 0; j < 3; ++j) w4[r * 4 + j] = weight_host[r * 3 + j];
        AMP_RC(amp_sconv_create(cin, cout, 2, 1, w4.data(), bias_host, &p->sconv));
    } else {
        if (amp_device_count() <= 0) { set_error("amp_dsconv_create: no HIP device visible (the HIP path has no CPU fallback)"); return AMP_ERR_HIP; }
        p->nsteps = (cin + DS_KC - 1) / DS_KC;
        const int nmb = (cout + DS_MROWS - 1) / DS_MROWS * (DS_MROWS / 32);
        const float wscale = pow2_weight_scale(wmax);
        p->inv_scale = 1.f / (16.f * wscale);
        const std::vector<_Float16> wp = pack_a_f16x3(nmb, p->nsteps * DS_KS, 3, 0, wscale, [&](int m, int i, int g) {
            return (m < cout && i < cin) ? weight_host[((size_t)m * cin + i) * 3 + g] : 0.f;
        });
        std::vector<float> bias((size_t)cout, 0.f);
        if (bias_host) std::copy(bias_host, bias_host + cout, bias.begin());
        AMP_RC(device_upload(wp.data(), wp.size() * sizeof(_Float16), (void**)&p->wp_dev));
        AMP_RC(device_upload(bias.data(), (size_t)cout * sizeof(float), (void**)&p->bias_dev));
    }
    *out = p.release();
    return AMP_OK;
}

int amp_dsconv_out_len(const amp_dsconv* h, int T) { (void)h; return (int)dsconv_out_len(T); }

size_t amp_dsconv_workspace_bytes(const amp_dsconv* h, int B, int T) {
    if (!h || B <= 0 || T <= 0 || h->precision != PREC_F32) return 0;
    return dsconv_pad_floats(h, B, T) * sizeof(float) + amp_sconv_workspace_bytes(h->sconv, B, T + 1);
}

int amp_dsconv_forward(const amp_dsconv* h, const float* x_dev, int B, int T, int gelu, void* ws_dev, size_t ws_bytes, float* y_dev, void* stream_) {
    if (!h || !x_dev || !y_dev || B <= 0 || T <= 0) { set_error("amp_dsconv_forward: bad argument (B=%d T=%d)", B, T); return AMP_ERR_INVALID; }
    if (gelu != 0 && gelu != 1) { set_error("amp_dsconv_forward: gelu=%d", gelu); return AMP_ERR_INVALID; }
    if (T > 0x3fffffff) { set_error("amp_dsconv_forward: T=%d is beyond 2^30", T); return AMP_ERR_UNSUPPORTED; }
    const int Tout = (int)dsconv_out_len(T);
    const size_t nx = (size_t)B * h->cin * T, ny = (size_t)B * h->cout * Tout;
    if (x_dev < y_dev + ny && y_dev < x_dev + nx) { set_error("amp_dsconv_forward: x and y must not overlap"); return AMP_ERR_INVALID; }
    hipStream_t stream = (hipStream_t)stream_;
    if (h->precision == PREC_F32) {
        const size_t need = amp_dsconv_workspace_bytes(h, B, T);
        if (!ws_dev || ws_bytes < need) { set_error("amp_dsconv_forward: workspace %zu < %zu bytes", ws_dev ? ws_bytes : (size_t)0, need); return AMP_ERR_INVALID; }
        if (reinterpret_cast<uintptr_t>(ws_dev) & 15) { set_error("amp_dsconv_forward: the workspace must be 16-byte aligned"); return AMP_ERR_INVALID; }
        const size_t npad = (size_t)B * h->cin * ((size_t)T + 1);
        const size_t blocks = (npad + 255) / 256;
        if (blocks > 0x7fffffffull) { set_error("amp_dsconv_forward: B=%d x cin=%d x T=%d is beyond the grid", B, h->cin, T); return AMP_ERR_UNSUPPORTED; }
        float* xp = (float*)ws_dev;
        float* ws2 = xp + dsconv_pad_floats(h, B, T);
        note_kernel("dsconv_zero_col_kernel");
        note_work((unsigned long long)blocks, 0.0, 4.0 * ((double)nx + (double)npad) / 1e6, "zero column C=%d T=%d B=%d", h->cin, T, B);
        hipLaunchKernelGGL(dsconv_zero_col_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, x_dev, xp, T, npad);
        AMP_HIP(hipGetLastError());
        AMP_RC(amp_sconv_forward(h->sconv, xp, B, T + 1, nullptr, ws2, amp_sconv_workspace_bytes(h->sconv, B, T + 1), y_dev, stream_));
        if (gelu) AMP_RC(amp_gelu(y_dev, (long long)ny, y_dev, stream_));
        return AMP_OK;
    }
    const long long tiles = (long long)B * ((Tout + 63) / 64);
    if (tiles > 0x7fffffffll || (h->cout + 63) / 64 > 65535) {
        set_error("amp_dsconv_forward: B=%d x T_out=%d x cout=%d is beyond the grid", B, Tout, h->cout);
        return AMP_ERR_UNSUPPORTED;
    }
    DsArgs a{};
    a.x = x_dev;
    a.wp = h->wp_dev;
    a.bias = h->bias_dev;
    a.y = y_dev;
    a.Cin = h->cin;
    a.Cout = h->cout;
    a.T = T;
    a.Tout = Tout;
    a.nsteps = h->nsteps;
    a.nc16 = h->nsteps * DS_KS;
    a.inv_scale = h->inv_scale;
    a.range_flag = range_flag_for_current_device();
    const hipError_t e = gelu ? ds_launch<1>(a, B, stream) : ds_launch<0>(a, B, stream);
    if (e != hipSuccess) { set_error("amp_dsconv_forward: %s", hipGetErrorString(e)); return AMP_ERR_HIP; }
    return AMP_OK;
}

void amp_dsconv_destroy(amp_dsconv* h) { delete h; }

}  // extern "C"
