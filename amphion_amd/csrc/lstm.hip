// nn.LSTM in eval mode as SEANet's SLSTM uses it (models/codec/speechtokenizer/modules/lstm.py:18-46): num_layers stacked layers, uni- or
// bidirectional, zero initial state, in the CONV layout [B, C, T] on both sides -- the two permutes of SLSTM.forward never exist -- with the skip
// connection (y + x, x repeated over both halves when bidirectional) folded into the last layer's store.
//
// Two stages per layer.
//   Gx = W_ih x + (b_ih + b_hh) for all T and both directions is ONE pointwise GEMM: an amp_pw handle whose rows are the directions' W_ih stacked
//   ([ndir * 4H, In]); it carries the arithmetic the handle was created under (f16x3, or exact fp32 under AMP_PRECISION_F32).
//   The recurrence h_t = o * tanh(c_t), c_t = f * c_{t-1} + i * g, gates = act(Gx_t + W_hh h_{t-1}) (gate order i, f, g, o) is lstm_step_kernel,
//   exact fp32: ONE LAUNCH PER TIME STEP, both directions in the same grid (direction 1 walks t = T - 1 - step).  Launches alone order the steps:
//   no workgroup ever waits for another one.
//
// lstm_step_kernel: a workgroup of four waves owns four hidden units of one direction, one unit per wave, with all four gate rows of W_hh, so the
// cell update is local to the wave.  h_{t-1} of a tile of BT batch items (1, 4, 8 or 16 by B) is staged in LDS once per workgroup; the 64 lanes
// split K = H (16-byte loads of the four gate rows when H % 4 == 0, lane l owns columns 4 l + 256 i; else lane l owns columns l + 64 i), every
// (gate, item) sum is one
// fmaf chain in ascending column order per lane, and the 64 partial sums meet in a fixed xor-shuffle tree (32, 16, .. 1): an item's bits do not
// depend on B, BT or the grid.  The BT items of a tile share every weight read.  h is double-buffered in the workspace (read step s, write step
// s + 1): no workgroup reads what another writes in the same launch.  c is read and written by its one owner lane.  Step 0 skips the product
// (h_{-1} = c_{-1} = 0), so the workspace needs no clearing.
#include <string.h>

#include <memory>

#include "amp_host.h"

namespace amp {

struct LstmStepArgs {
    const float* w_hh;     // [ndir][4H][H] of this layer
    const float* gx;       // [B, ndir * 4H, T]
    const float* skip;     // [B, H, T] or nullptr
    float* y;              // [B, ndir * H, T]
    const float* h_prev;   // [ndir][B][H]
    float* h_next;         // [ndir][B][H]
    float* c;              // [ndir][B][H]
    int H, B, T, ndir, step;
};

__device__ __forceinline__ float lstm_sigmoid(float v) { return 1.f / (1.f + expf(-v)); }

template <int BT>
__global__ __launch_bounds__(256) void lstm_step_kernel(const LstmStepArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lstm_hs[];     // [BT][H]
    const int H = a.H, B = a.B, T = a.T;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int d = blockIdx.y;
    const int t = d ? T - 1 - a.step : a.step;
    const int j = blockIdx.x * 4 + wave;
    const bool active = j < H;
    const bool first = a.step == 0;
    const float* W = a.w_hh + (size_t)d * 4 * H * H;
    const size_t grow = (size_t)a.ndir * 4 * H;

    for (int b0 = 0; b0 < B; b0 += BT) {
        const int nb = (B - b0) < BT ? (B - b0) : BT;
        float gxv[4] = {0.f, 0.f, 0.f, 0.f};
        if (active && lane < nb) {
#pragma unroll
            for (int g = 0; g < 4; ++g) gxv[g] = a.gx[((size_t)(b0 + lane) * grow + (size_t)d * 4 * H + (size_t)g * H + j) * T + t];
        }
        float acc[4][BT];
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int b = 0; b < BT; ++b) acc[g][b] = 0.f;
        if (!first) {
            __syncthreads();                                   // the previous tile's readers are done with lstm_hs
            const float* hp = a.h_prev + ((size_t)d * B + b0) * H;
            if ((H & 3) == 0) {
                const float4* hp4 = reinterpret_cast<const float4*>(hp);
                float4* hs4w = reinterpret_cast<float4*>(lstm_hs);
                for (int i = tid; i < BT * (H >> 2); i += 256) hs4w[i] = i < nb * (H >> 2) ? hp4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
            } else {
                for (int i = tid; i < BT * H; i += 256) lstm_hs[i] = i < nb * H ? hp[i] : 0.f;
            }
            __syncthreads();
            if (active) {
                if ((H & 3) == 0) {
                    const int H4 = H >> 2;
                    const float4* w0 = reinterpret_cast<const float4*>(W + ((size_t)0 * H + j) * H);
                    const float4* w1 = reinterpret_cast<const float4*>(W + ((size_t)1 * H + j) * H);
                    const float4* w2 = reinterpret_cast<const float4*>(W + ((size_t)2 * H + j) * H);
                    const float4* w3 = reinterpret_cast<const float4*>(W + ((size_t)3 * H + j) * H);
                    const float4* hs4 = reinterpret_cast<const float4*>(lstm_hs);
                    for (int k4 = lane; k4 < H4; k4 += 64) {
                        const float4 wv[4] = {w0[k4], w1[k4], w2[k4], w3[k4]};
#pragma unroll
                        for (int b = 0; b < BT; ++b) {
                            const float4 hv = hs4[b * H4 + k4];
#pragma unroll
                            for (int g = 0; g < 4; ++g) {
                                float s = acc[g][b];
                                s = fmaf(wv[g].x, hv.x, s);
                                s = fmaf(wv[g].y, hv.y, s);
                                s = fmaf(wv[g].z, hv.z, s);
                                s = fmaf(wv[g].w, hv.w, s);
                                acc[g][b] = s;
                            }
                        }
                    }
                } else {
                    for (int k = lane; k < H; k += 64) {
                        float wv[4];
#pragma unroll
                        for (int g = 0; g < 4; ++g) wv[g] = W[((size_t)g * H + j) * H + k];
#pragma unroll
                        for (int b = 0; b < BT; ++b) {
                            const float hv = lstm_hs[b * H + k];
#pragma unroll
                            for (int g = 0; g < 4; ++g) acc[g][b] = fmaf(wv[g], hv, acc[g][b]);
                        }
                    }
                }
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int b = 0; b < BT; ++b) {
                        float s = acc[g][b];
#pragma unroll
                        for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
                        acc[g][b] = s;
                    }
            }
        }
        if (active && lane < nb) {
            float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int b = 0; b < BT; ++b)
                if (lane == b) {
#pragma unroll
                    for (int g = 0; g < 4; ++g) s[g] = acc[g][b];
                }
            const int b = b0 + lane;
            const size_t si = ((size_t)d * B + b) * H + j;
            const float ig = lstm_sigmoid(gxv[0] + s[0]);
            const float fg = lstm_sigmoid(gxv[1] + s[1]);
            const float gg = tanhf(gxv[2] + s[2]);
            const float og = lstm_sigmoid(gxv[3] + s[3]);
            const float cp = first ? 0.f : a.c[si];
            const float cn = fg * cp + ig * gg;
            const float hn = og * tanhf(cn);
            a.c[si] = cn;
            a.h_next[si] = hn;
            const size_t yi = (((size_t)b * a.ndir + d) * H + j) * T + t;
            a.y[yi] = a.skip ? hn + a.skip[((size_t)b * H + j) * T + t] : hn;
        }
    }
}

}  // namespace amp

using namespace amp;

struct amp_lstm {
    int In = 0, H = 0, L = 0, ndir = 1, skip = 0;
    std::vector<amp_pw*> proj;     // one per layer: [ndir * 4H, In_l]
    std::vector<float*> w_hh;      // one per layer: [ndir][4H][H]
    DeviceAllocs dev;
    ~amp_lstm() {
        for (amp_pw* p : proj) amp_pw_destroy(p);
    }
};

static size_t lstm_state_floats(const amp_lstm* h, int B) { return (size_t)3 * h->ndir * B * h->H; }

extern "C" {

int amp_lstm_create(int input_size, int hidden, int num_layers, int bidirectional, int skip, const float* const* w_ih_host,
                    const float* const* w_hh_host, const float* const* b_ih_host, const float* const* b_hh_host, amp_lstm** out) {
    if (!w_ih_host || !w_hh_host || !b_ih_host || !b_hh_host || !out) { set_error("amp_lstm_create: null argument"); return AMP_ERR_INVALID; }
    const int In = input_size, H = hidden, L = num_layers, ndir = bidirectional ? 2 : 1;
    if (In < 1 || H < 1 || L < 1) { set_error("amp_lstm_create: input_size=%d hidden=%d num_layers=%d", In, H, L); return AMP_ERR_INVALID; }
    if (H > 1024 || In > 2048 || L > 4) {
        set_error("amp_lstm_create: input_size=%d hidden=%d num_layers=%d is outside the kernels (hidden <= 1024, input_size <= 2048, num_layers <= 4)",
                  In, H, L);
        return AMP_ERR_UNSUPPORTED;
    }
    if (skip && In != H) { set_error("amp_lstm_create: the skip connection needs input_size == hidden (%d != %d)", In, H); return AMP_ERR_INVALID; }
    for (int i = 0; i < L * ndir; ++i)
        if (!w_ih_host[i] || !w_hh_host[i] || !b_ih_host[i] || !b_hh_host[i]) {
            set_error("amp_lstm_create: null weight at layer %d direction %d", i / ndir, i % ndir);
            return AMP_ERR_INVALID;
        }
    std::vector<std::vector<float>> wi(L), bi(L), wh(L);
    for (int l = 0; l < L; ++l) {
        const int in_l = l ? ndir * H : In;
        wi[l].resize((size_t)ndir * 4 * H * in_l);
        bi[l].resize((size_t)ndir * 4 * H);
        wh[l].resize((size_t)ndir * 4 * H * H);
        for (int d = 0; d < ndir; ++d) {
            const int s = l * ndir + d;
            memcpy(&wi[l][(size_t)d * 4 * H * in_l], w_ih_host[s], sizeof(float) * 4 * H * in_l);
            memcpy(&wh[l][(size_t)d * 4 * H * H], w_hh_host[s], sizeof(float) * 4 * H * H);
            for (int r = 0; r < 4 * H; ++r) bi[l][(size_t)d * 4 * H + r] = b_ih_host[s][r] + b_hh_host[s][r];
        }
        for (float v : wh[l])
            if (!(fabsf(v) < 1e30f)) { set_error("amp_lstm_create: non-finite recurrent weight (layer %d)", l); return AMP_ERR_INVALID; }
    }
    // every refusal above is the host's alone: the arguments are judged the same with or without a device
    if (amp_device_count() <= 0) { set_error("amp_lstm_create: no HIP device visible (the HIP path has no CPU fallback)"); return AMP_ERR_HIP; }
    auto h = std::make_unique<amp_lstm>();
    h->In = In; h->H = H; h->L = L; h->ndir = ndir; h->skip = skip ? 1 : 0;
    for (int l = 0; l < L; ++l) {
        amp_pw* p = nullptr;
        AMP_RC(amp_pw_create(l ? ndir * H : In, ndir * 4 * H, wi[l].data(), bi[l].data(), &p));
        h->proj.push_back(p);
        float* w = nullptr;
        AMP_RC(h->dev.upload(wh[l], &w));
        h->w_hh.push_back(w);
    }
    *out = h.release();
    return AMP_OK;
}

void amp_lstm_destroy(amp_lstm* h) { delete h; }

size_t amp_lstm_workspace_bytes(const amp_lstm* h, int B, int T) {
    if (!h || B <= 0 || T <= 0) return 0;
    // [state: h ping | h pong | c] [Gx: B x ndir 4H x T] [the layer output between two layers: B x ndir H x T]
    const size_t state = (lstm_state_floats(h, B) + 63) / 64 * 64;
    return (state + (size_t)B * h->ndir * 4 * h->H * T + (h->L > 1 ? (size_t)B * h->ndir * h->H * T : 0)) * sizeof(float);
}

int amp_lstm_out_channels(const amp_lstm* h) { return h ? h->ndir * h->H : -1; }

int amp_lstm_recur(const amp_lstm* h, int layer, const float* gx_dev, int B, int T, const float* skip_dev, float* y_dev, void* ws_dev, void* stream) {
    if (!h) { set_error("amp_lstm_recur: null handle"); return AMP_ERR_INVALID; }
    if (layer < 0 || layer >= h->L) { set_error("amp_lstm_recur: layer %d of %d", layer, h->L); return AMP_ERR_INVALID; }
    if (B <= 0 || T <= 0) { set_error("amp_lstm_recur: B=%d T=%d", B, T); return AMP_ERR_INVALID; }
    if (!gx_dev || !y_dev || !ws_dev) { set_error("amp_lstm_recur: null argument"); return AMP_ERR_INVALID; }
    if (reinterpret_cast<uintptr_t>(ws_dev) & 15) { set_error("amp_lstm_recur: the workspace must be 16-byte aligned (h is staged with 16-byte loads)"); return AMP_ERR_INVALID; }
    if ((long long)B * h->ndir * 4 * h->H * (long long)T > 0x7fffffff00ll) { set_error("amp_lstm_recur: B=%d x T=%d is beyond the kernel", B, T); return AMP_ERR_UNSUPPORTED; }
    const int H = h->H, ndir = h->ndir;
    float* st = static_cast<float*>(ws_dev);
    const size_t one = (size_t)ndir * B * H;
    float* hbuf[2] = {st, st + one};
    LstmStepArgs a{};
    a.w_hh = h->w_hh[layer]; a.gx = gx_dev; a.skip = skip_dev; a.y = y_dev; a.c = st + 2 * one;
    a.H = H; a.B = B; a.T = T; a.ndir = ndir;
    const dim3 grid((unsigned)((H + 3) / 4), (unsigned)ndir);
    const int BT = B == 1 ? 1 : (B <= 4 ? 4 : (B <= 8 ? 8 : 16));
    const size_t lds = (size_t)BT * H * sizeof(float);
    hipStream_t s = (hipStream_t)stream;
    for (int step = 0; step < T; ++step) {
        a.step = step;
        a.h_prev = hbuf[step & 1];
        a.h_next = hbuf[(step + 1) & 1];
        note_kernel("lstm_step_kernel", BT);
        note_work((unsigned long long)grid.x * grid.y, 2.0 * ndir * 4.0 * H * H * B / 1e9, 4.0 * ndir * 4.0 * H * H / 1e6, "lstm step H=%d ndir=%d B=%d t=%d", H,
                  ndir, B, step);
        if (BT == 1) hipLaunchKernelGGL(lstm_step_kernel<1>, grid, dim3(256), lds, s, a);
        else if (BT == 4) hipLaunchKernelGGL(lstm_step_kernel<4>, grid, dim3(256), lds, s, a);
        else if (BT == 8) hipLaunchKernelGGL(lstm_step_kernel<8>, grid, dim3(256), lds, s, a);
        else hipLaunchKernelGGL(lstm_step_kernel<16>, grid, dim3(256), lds, s, a);
    }
    AMP_HIP(hipGetLastError());
    return AMP_OK;
}

int amp_lstm_forward(const amp_lstm* h, const float* x_dev, int B, int T, float* y_dev, void* ws_dev, size_t ws_bytes, void* stream) {
    if (!h) { set_error("amp_lstm_forward: null handle"); return AMP_ERR_INVALID; }
    if (B <= 0 || T <= 0) { set_error("amp_lstm_forward: B=%d T=%d", B, T); return AMP_ERR_INVALID; }
    if (!x_dev || !y_dev || !ws_dev) { set_error("amp_lstm_forward: null argument"); return AMP_ERR_INVALID; }
    if (x_dev == y_dev) { set_error("amp_lstm_forward: y must not alias x"); return AMP_ERR_INVALID; }
    if (ws_bytes < amp_lstm_workspace_bytes(h, B, T)) {
        set_error("amp_lstm_forward: workspace of %zu bytes, %zu needed", ws_bytes, amp_lstm_workspace_bytes(h, B, T));
        return AMP_ERR_INVALID;
    }
    float* ws = static_cast<float*>(ws_dev);
    float* gx = ws + (lstm_state_floats(h, B) + 63) / 64 * 64;
    float* mid = gx + (size_t)B * h->ndir * 4 * h->H * T;
    const float* in = x_dev;
    for (int l = 0; l < h->L; ++l) {
        const bool last = l == h->L - 1;
        AMP_RC(amp_pw_forward(h->proj[l], in, 0, B, T, AMP_PW_BIAS, nullptr, nullptr, gx, stream));
        AMP_RC(amp_lstm_recur(h, l, gx, B, T, (last && h->skip) ? x_dev : nullptr, last ? y_dev : mid, ws_dev, stream));
        in = mid;
    }
    return AMP_OK;
}

}  // extern "C"
