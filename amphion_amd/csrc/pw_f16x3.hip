// Pointwise (1 x 1) GEMM on channel-first activations for the Vocos backbone and head (models/codec/amphion_codec/vocos.py:
// ConvNeXtBlock.pwconv1 / pwconv2 :511-526, ISTFTHead.out :346) -- nn.Linear applied along the channel axis of [B, C, T]:
//     Y[b] = epi( W * X[b] + bias ),   W [Cout, Cin] as nn.Linear.weight stores it
// with the epilogue chosen at compile time:
//     AMP_PW_BIAS        y = Wx + b
//     AMP_PW_BIAS_GELU   y = gelu_erf(Wx + b)                 (nn.GELU(), exact erf form)
//     AMP_PW_SCALE_RES   y = res + gamma (.) (Wx + b)         (layer scale + residual; y may alias res)
//     PW_EPI_RES_SKIP    rows [0, H): y = (res + v) / sqrt(2); rows [H, 2H): skip_out = skip_in + v, v = Wx + b   (internal, Cout = 2H: out_proj of
//                        NaturalSpeech2's WaveNet layer, ns2_layer_f16x3.hip; y, res, skip_in, skip_out are [B, H, T]; y may alias res, skip_out skip_in)
//
// Arithmetic: the f16x3 scheme (f16x3_device.h; operand layouts and fragment loads: wholek_f16x3.h) -- weights pre-split on the host after a
// per-matrix 2^s, activations x16 and split while staged, the scale undone in the epilogue, the range flag raised by the staging.
//
// Tiling.  The contraction is K = Cin (384 .. 4096), there is no halo: a K step stages 64 channels (4 MFMA k-extents), one barrier per
// step.  Four waves as 2 x 2, each wave MI x NI 32 x 32 accumulator tiles: the 128 x 128 tile (MI = NI = 2: 64 accumulator VGPRs,
// 12 MFMAs per 8 fragment reads per k-extent) for grids that give every CU two workgroups, the 64 x 64 tile (MI = NI = 1) for
// single utterances, where T ~ 250 frames leaves two column tiles per item and the row tiles have to supply the workgroups.
//   - A (weights): packed on the host in MFMA fragment order [row block][k16][plane][lane] x 16 B and read straight from L2 into
//     VGPRs -- one 16-B load per lane per fragment, re-loaded for the next step right after its last use.
//   - B (activations): T is the contiguous axis, so the operand is transposed while staged: a staging item is (column, channel quad),
//     four coalesced row loads, split into hi / lo and written to LDS as [plane][channel octet][column][8 x f16]; a lane's B fragment
//     is then one ds_read_b128.  Two LDS buffers: the loads of step s + 1 fly under the MFMAs of step s.
// Deterministic (each output is one workgroup's full-K sum), no split-K, no atomics except the range flag.
#include <algorithm>
#include <memory>

#include "amp_host.h"
#include "wholek_f16x3.h"
#include "gelu_erf.h"

namespace amp {

constexpr int PW_KS = 4;            // MFMA k-extents (16 channels each) per K step
constexpr int PW_KC = 16 * PW_KS;   // channels per K step
constexpr int PW_MROWS = 128;       // packed rows are padded to this (the larger tile's height)
constexpr int PW_EPI_RES_SKIP = 3;  // beyond amp_pw_epilogue: reached through pw_run_res_skip only

struct PwArgs {
    const float* x;       // [B, Cin, T] with batch stride xbs
    long long xbs;
    const uint4* wp;      // packed hi / lo fragments, see amp_pw_create
    const float* bias;    // [Cout]
    const float* gamma;   // [Cout] (SCALE_RES)
    const float* res;     // [B, Cout, T] (SCALE_RES; may alias y)
    float* y;             // [B, Cout, T]
    int Cin, Cout, T;
    int nsteps;           // K steps of PW_KC channels
    int nc16;             // packed k-extents per row block = nsteps * PW_KS
    int tiles_per_item;   // ceil(T / TN)
    float inv_scale;      // 1 / (16 * 2^s)
    unsigned* range_flag;
    const float* skip_in;   // PW_EPI_RES_SKIP: [B, Cout / 2, T] running skip sum or nullptr; may alias skip_out
    float* skip_out;        //                  [B, Cout / 2, T]
};

template <int EPI, int MI, int NI>
__global__ __launch_bounds__(256, 2) void pw_f16x3_kernel(const PwArgs a) {
    constexpr int TN = 64 * NI;                 // columns per workgroup
    constexpr int NST = (4 * PW_KS * TN) / 256; // staging items (column x channel quad) per thread
    constexpr int BUF = 2 * 2 * PW_KS * TN;     // uint4 per LDS buffer: [plane][octet][TN]
    constexpr int PLANE = 2 * PW_KS * TN;       // uint4 per plane
    extern __shared__ __attribute__((aligned(16))) uint4 pw_smem[];   // [2][BUF]

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

    const float* xb = a.x + (size_t)item * (size_t)a.xbs;
    const int T = a.T, Cin = a.Cin;
    float range_max = 0.f;
    float xs[NST][4];
    // staging item i = wave * 64 + 256 * it + lane: channel quad (i / TN, wave-uniform: TN is a multiple of 64) x column (i % TN)
    auto stage_load = [&](int step) {
#pragma unroll
        for (int it = 0; it < NST; ++it) {
            const int ibase = wave * 64 + 256 * it;
            const int qd = ibase / TN;
            const int col = ibase - qd * TN + lane;
            int t = q0 + col;
            t = t > T - 1 ? T - 1 : t;
            const int ch0 = step * PW_KC + 4 * qd;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                int ch = ch0 + e;
                ch = ch > Cin - 1 ? Cin - 1 : ch;
                xs[it][e] = xb[(size_t)ch * T + t];
            }
        }
    };
    auto stage_store = [&](int step, int buf) {
        uint2* dst = reinterpret_cast<uint2*>(pw_smem + buf * BUF);
#pragma unroll
        for (int it = 0; it < NST; ++it) {
            const int ibase = wave * 64 + 256 * it;
            const int qd = ibase / TN;
            const int col = ibase - qd * TN + lane;
            const bool tok = q0 + col < T;
            const int ch0 = step * PW_KC + 4 * qd;
            uint2 fh, fl;
            stage4_f16((tok && ch0 + 0 < Cin) ? xs[it][0] : 0.f, (tok && ch0 + 1 < Cin) ? xs[it][1] : 0.f,
                       (tok && ch0 + 2 < Cin) ? xs[it][2] : 0.f, (tok && ch0 + 3 < Cin) ? xs[it][3] : 0.f, 16.f, 16.f, range_max, fh, fl);
            bplane_store(dst, 2 * PLANE, bplane_idx(qd, col, TN), fh, fl);
        }
    };

    // A fragments of one K step: [k-extent][row block][plane]; entry (mb, c16, plane) of the pack at ((mb * nc16 + c16) * 2 + plane) * 64
    const uint4* wa = a.wp + (size_t)mb0 * a.nc16 * 128 + lane;
    const size_t mbs = (size_t)a.nc16 * 128;           // uint4 per row block
    Frag ah[PW_KS][MI], al[PW_KS][MI];
#pragma unroll
    for (int h = 0; h < PW_KS; ++h)
        afrag_load<MI>(ah[h], al[h], wa + h * 128, mbs);
    stage_load(0);
    AMP_PIN_VMEM();
    stage_store(0, 0);
    __syncthreads();

    const int rd0 = hi * TN + wn * (32 * NI) + l31;
    auto step = [&](const int s, const bool more) __attribute__((always_inline)) {
        if (more) {
            stage_load(s + 1);
            AMP_PIN_VMEM();
        }
        wa += PW_KS * 128;
        const uint4* base = pw_smem + (s & 1) * BUF + rd0;
#pragma unroll
        for (int h = 0; h < PW_KS; ++h) {
            const uint4* bg = base + (2 * h) * TN;
            Frag bh[NI], bl[NI];
#pragma unroll
            for (int t = 0; t < NI; ++t) bfrag_load(bg, PLANE, 32 * t, bh[t], bl[t]);
            mfma3_tiles<MI, NI>(acc, ah[h], al[h], bh, bl);
            if (more) {
                afrag_load<MI>(ah[h], al[h], wa + h * 128, mbs);
                AMP_PIN_VMEM();
            }
        }
        if (more) stage_store(s + 1, (s + 1) & 1);
        __syncthreads();
    };
    const int nsteps = a.nsteps;
    for (int s = 0; s + 1 < nsteps; ++s) step(s, true);
    step(nsteps - 1, false);

    raise_range(a.range_flag, range_max, lane);

    // ---- epilogue: lane (hi, l31), register r of tile (i, t) holds row acc_row(r, hi), column 32 t + l31 ----
    const size_t ybase = (size_t)item * a.Cout * T;
#pragma unroll
    for (int i = 0; i < MI; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = acc_row(r, hi, (mb0 + i) * 32);
            if (m >= a.Cout) continue;
            const float bv = a.bias[m];
            if (EPI == PW_EPI_RES_SKIP) {
                const int Hh = a.Cout >> 1;
                const bool sk = m >= Hh;
                const size_t hrow = ((size_t)item * Hh + (sk ? m - Hh : m)) * T;
                const float sqrt2 = 1.41421356237309504880f;
#pragma unroll
                for (int t = 0; t < NI; ++t) {
                    const int q = q0 + wn * (32 * NI) + 32 * t + l31;
                    if (q >= T) continue;
                    const float v = acc[i][t][r] * a.inv_scale + bv;
                    if (sk) a.skip_out[hrow + q] = a.skip_in ? a.skip_in[hrow + q] + v : v;
                    else a.y[hrow + q] = (a.res[hrow + q] + v) / sqrt2;
                }
                continue;
            }
            const float gv = EPI == AMP_PW_SCALE_RES ? a.gamma[m] : 0.f;
            const size_t row = ybase + (size_t)m * T;
#pragma unroll
            for (int t = 0; t < NI; ++t) {
                const int q = q0 + wn * (32 * NI) + 32 * t + l31;
                if (q >= T) continue;
                float v = acc[i][t][r] * a.inv_scale + bv;
                if (EPI == AMP_PW_BIAS_GELU) v = gelu_erf(v);
                if (EPI == AMP_PW_SCALE_RES) v = a.res[row + q] + gv * v;
                a.y[row + q] = v;
            }
        }
    }
}

template <int EPI, int MI, int NI>
static hipError_t pw_launch_one(const PwArgs& a, int B, hipStream_t stream) {
    constexpr int TN = 64 * NI;
    const size_t lds = (size_t)2 * 2 * 2 * PW_KS * TN * sizeof(uint4);
    if (hipError_t e = ensure_dynamic_lds<&pw_f16x3_kernel<EPI, MI, NI>>(lds); e != hipSuccess) return e;
    const dim3 grid((unsigned)(B * a.tiles_per_item), (unsigned)((a.Cout + 64 * MI - 1) / (64 * MI)));
    note_kernel("pw_f16x3_kernel", EPI, MI, NI);
    if (manifest_on()) {
        const double gf = 2.0 * a.Cout * (double)a.Cin * a.T * B / 1e9;
        const double mb = 4.0 * B * ((double)a.Cin * a.T + (double)a.Cout * a.T * (EPI == AMP_PW_SCALE_RES || EPI == PW_EPI_RES_SKIP ? 2 : 1)) / 1e6;
        note_work((unsigned long long)grid.x * grid.y, gf, mb, "pw %d->%d epi=%d T=%d B=%d grid=%ux%u", a.Cin, a.Cout, EPI, a.T, B, grid.x, grid.y);
    }
    hipLaunchKernelGGL((pw_f16x3_kernel<EPI, MI, NI>), grid, dim3(256), lds, stream, a);
    return hipGetLastError();
}

// the large tile wherever it still gives every CU two workgroups; the small one otherwise (single utterances)
template <int EPI>
static hipError_t pw_launch(PwArgs a, int B, hipStream_t stream) {
    const long long big = (long long)B * ((a.T + 127) / 128) * ((a.Cout + 127) / 128);
    if (big >= 512) {
        a.tiles_per_item = (a.T + 127) / 128;
        return pw_launch_one<EPI, 2, 2>(a, B, stream);
    }
    a.tiles_per_item = (a.T + 63) / 64;
    return pw_launch_one<EPI, 1, 1>(a, B, stream);
}

// out_proj of NaturalSpeech2's WaveNet layer on an f16x3 handle with cout = 2 cin: the caller (ns2_layer_f16x3.hip) has judged the arguments
int pw_run_res_skip(const amp_pw* p, const float* z_dev, int B, int T, const float* x_dev, const float* skip_in_dev, float* x_out_dev,
                    float* skip_out_dev, hipStream_t stream) {
    if (!p || p->precision != PREC_F16X3 || p->cout != 2 * p->cin) { set_error("pw_run_res_skip: not an f16x3 H -> 2H handle"); return AMP_ERR_INVALID; }
    PwArgs a{};
    a.x = z_dev;
    a.xbs = (long long)p->cin * T;
    a.wp = p->wp_dev;
    a.bias = p->bias_dev;
    a.res = x_dev;
    a.y = x_out_dev;
    a.skip_in = skip_in_dev;
    a.skip_out = skip_out_dev;
    a.Cin = p->cin;
    a.Cout = p->cout;
    a.T = T;
    a.nsteps = p->nsteps;
    a.nc16 = p->nsteps * PW_KS;
    a.inv_scale = p->inv_scale;
    a.range_flag = range_flag_for_current_device();
    const hipError_t e = pw_launch<PW_EPI_RES_SKIP>(a, B, stream);
    if (e != hipSuccess) { set_error("pw_run_res_skip: %s", hipGetErrorString(e)); return AMP_ERR_HIP; }
    return AMP_OK;
}

// exact-fp32 mode: the k = 1 conv (conv_mfma.hip) writes Wx + b, this applies the rest of the epilogue in place
__global__ __launch_bounds__(256) void pw_epilogue_kernel(float* __restrict__ y, const float* __restrict__ res, const float* __restrict__ gamma,
                                                          int epi, int C, int T, size_t n, float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float v = y[i];
    if (epi == AMP_PW_BIAS_GELU) v = gelu_erf(v);
    else {
        const int c = (int)((i / (size_t)T) % (size_t)C);
        v = res[i] + gamma[c] * v;
    }
    out[i] = v;
}

}  // namespace amp

using namespace amp;

extern "C" {

int amp_pw_create(int cin, int cout, const float* weight_host, const float* bias_host, amp_pw** out) {
    if (!out || !weight_host || cin <= 0 || cout <= 0) { set_error("amp_pw_create: bad argument cin=%d cout=%d", cin, cout); return AMP_ERR_INVALID; }
    *out = nullptr;
    std::unique_ptr<amp_pw> p(new amp_pw);
    p->cin = cin;
    p->cout = cout;
    p->precision = amp_get_precision();
    std::vector<float> bias((size_t)cout, 0.f);
    if (bias_host) std::copy(bias_host, bias_host + cout, bias.begin());
    if (p->precision == PREC_F32) {
        // [cout, cin] is the Conv1d weight [cout, cin, 1]
        if (amp_device_count() <= 0) { set_error("amp_pw_create: no HIP device visible (the HIP path has no CPU fallback)"); return AMP_ERR_HIP; }
        p->conv = new amp_conv;
        p->conv->cin = cin; p->conv->cout = cout; p->conv->k = 1;
        AMP_RC(conv_build(p->conv, weight_host, bias.data()));
    } else {
        p->nsteps = (cin + PW_KC - 1) / PW_KC;
        const int nmb = (cout + PW_MROWS - 1) / PW_MROWS * (PW_MROWS / 32);
        std::vector<_Float16> wp;
        AMP_RC(pack_matrix_f16x3("amp_pw_create", cout, cin, nmb, p->nsteps * PW_KS, [&](int m, int i) { return weight_host[(size_t)m * cin + i]; },
                                 &wp, &p->inv_scale));
        AMP_RC(device_upload(wp.data(), wp.size() * sizeof(_Float16), (void**)&p->wp_dev));
        AMP_RC(device_upload(bias.data(), (size_t)cout * sizeof(float), (void**)&p->bias_dev));
    }
    *out = p.release();
    return AMP_OK;
}

int amp_pw_precision(const amp_pw* p) { return p ? p->precision : -1; }

int amp_pw_forward(const amp_pw* p, const float* x_dev, long long x_batch_stride, int B, int T, int epilogue, const float* gamma_dev,
                   const float* res_dev, float* y_dev, void* stream_) {
    if (!p || !x_dev || !y_dev || B <= 0 || T <= 0 || B > 65535) { set_error("amp_pw_forward: bad argument (B=%d T=%d)", B, T); return AMP_ERR_INVALID; }
    if (epilogue != AMP_PW_BIAS && epilogue != AMP_PW_BIAS_GELU && epilogue != AMP_PW_SCALE_RES) {
        set_error("amp_pw_forward: unknown epilogue %d", epilogue);
        return AMP_ERR_INVALID;
    }
    if (epilogue == AMP_PW_SCALE_RES && (!gamma_dev || !res_dev)) { set_error("amp_pw_forward: AMP_PW_SCALE_RES needs gamma and res"); return AMP_ERR_INVALID; }
    if (x_batch_stride == 0) x_batch_stride = (long long)p->cin * T;
    if (x_batch_stride < (long long)p->cin * T) { set_error("amp_pw_forward: batch stride %lld < cin*T", x_batch_stride); return AMP_ERR_INVALID; }
    const size_t xspan = (size_t)(B - 1) * (size_t)x_batch_stride + (size_t)p->cin * T;
    const float* ylo = y_dev;
    const float* yhi = y_dev + (size_t)B * p->cout * T;
    if (x_dev < yhi && ylo < x_dev + xspan) { set_error("amp_pw_forward: x and y must not overlap"); return AMP_ERR_INVALID; }
    if (epilogue == AMP_PW_SCALE_RES && res_dev != y_dev) {
        const float* rhi = res_dev + (size_t)B * p->cout * T;
        if (res_dev < yhi && ylo < rhi) { set_error("amp_pw_forward: res must be y or not overlap it"); return AMP_ERR_INVALID; }
    }
    hipStream_t stream = (hipStream_t)stream_;
    if (p->precision == PREC_F32) {
        const size_t n = (size_t)B * p->cout * T;
        // y aliasing res: Wx + b goes to a stream-ordered temporary of this call (allocated and freed on `stream`, so a handle holds
        // no mutable state and two streams may share it)
        float* tmp = nullptr;
        if (epilogue == AMP_PW_SCALE_RES && res_dev == y_dev) AMP_HIP(hipMallocAsync((void**)&tmp, n * sizeof(float), stream));
        float* dst = tmp ? tmp : y_dev;
        int rc = conv_run(p->conv, x_dev, B, T, 1.f, nullptr, 1.f, dst, 0, 1.f, stream, x_batch_stride);
        if (rc == AMP_OK && epilogue != AMP_PW_BIAS) {
            note_kernel("pw_epilogue_kernel");
            const unsigned nb = (unsigned)((n + 255) / 256);
            note_work(nb, 0.0, 4.0 * n * (epilogue == AMP_PW_SCALE_RES ? 3 : 2) / 1e6, "pw epilogue %d C=%d T=%d B=%d", epilogue, p->cout, T, B);
            hipLaunchKernelGGL(pw_epilogue_kernel, dim3(nb), dim3(256), 0, stream, dst, res_dev, gamma_dev, epilogue, p->cout, T, n, y_dev);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) { set_error("amp_pw_forward: %s", hipGetErrorString(e)); rc = AMP_ERR_HIP; }
        }
        if (tmp) {
            const hipError_t e = hipFreeAsync(tmp, stream);
            if (e != hipSuccess && rc == AMP_OK) { set_error("amp_pw_forward: hipFreeAsync: %s", hipGetErrorString(e)); rc = AMP_ERR_HIP; }
        }
        return rc;
    }
    PwArgs a{};
    a.x = x_dev;
    a.xbs = x_batch_stride;
    a.wp = p->wp_dev;
    a.bias = p->bias_dev;
    a.gamma = gamma_dev;
    a.res = res_dev;
    a.y = y_dev;
    a.Cin = p->cin;
    a.Cout = p->cout;
    a.T = T;
    a.nsteps = p->nsteps;
    a.nc16 = p->nsteps * PW_KS;
    a.inv_scale = p->inv_scale;
    a.range_flag = range_flag_for_current_device();
    hipError_t e;
    if (epilogue == AMP_PW_BIAS) e = pw_launch<AMP_PW_BIAS>(a, B, stream);
    else if (epilogue == AMP_PW_BIAS_GELU) e = pw_launch<AMP_PW_BIAS_GELU>(a, B, stream);
    else e = pw_launch<AMP_PW_SCALE_RES>(a, B, stream);
    if (e != hipSuccess) { set_error("amp_pw_forward: %s", hipGetErrorString(e)); return AMP_ERR_HIP; }
    return AMP_OK;
}

void amp_pw_destroy(amp_pw* p) { delete p; }

}  // extern "C"
