// The staging pass in front of every SEANet convolution (models/codec/speechtokenizer/modules/conv.py:97-119, seanet.py): the activation of
// nn.ELU and the reflect padding of pad1d() in ONE pass, so that the existing conv entries (amp_conv_*, amp_sconv_*, amp_tconv_*) run on the
// padded tensor with padding = 0.
//   y[b, c, j] = act(x[b, c, src(j)]),  j in [0, pad_left + T + pad_right)
//   act        = ELU (v > 0 ? v : alpha * expm1(v)) or the identity
//   src        = F.pad(mode = "reflect") with pad1d's small-input rule: when T <= max(pad_left, pad_right) the row is first zero-extended on the
//                right to max_pad + 1 samples, reflected, and the extension cropped again.  A column that lands on the extension is 0; the
//                reference applies ELU before the padding and ELU(0) = 0, so act(0) = 0 is the same value.
// One thread owns four consecutive output columns of one row: a 16-byte store when the row length allows it (T_out % 4 == 0 keeps every row
// aligned, given an aligned y), a 16-byte load when its four sources are consecutive interior samples at a 16-byte aligned ADDRESS -- the
// base pointers may have any 4-byte alignment.  With zero pads it is the plain
// element-wise ELU.  Exact fp32; expm1f is the device library's.
#include "amp_host.h"

namespace amp {

struct EluPadArgs {
    const float* x;
    float* y;
    long long quads;     // rows * quads_per_row
    int T, Tout, pl, Lext, q4, elu, vec_store;
    float alpha;
};

__device__ __forceinline__ float elu_act(float v, float alpha, int on) { return (on && !(v > 0.f)) ? alpha * expm1f(v) : v; }

__global__ __launch_bounds__(256) void elu_pad_kernel(const EluPadArgs a) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= a.quads) return;
    const long long row = q / a.q4;
    const int j0 = (int)(q - row * a.q4) * 4;
    const float* xr = a.x + row * a.T;
    float* yr = a.y + row * a.Tout;
    float v[4];
    const int i0 = j0 - a.pl;
    if (i0 >= 0 && i0 + 3 < a.T && ((reinterpret_cast<uintptr_t>(xr + i0) & 15) == 0)) {
        const float4 t = *reinterpret_cast<const float4*>(xr + i0);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            int i = i0 + e;
            if (i < 0) i = -i;
            else if (i >= a.Lext) i = 2 * (a.Lext - 1) - i;
            v[e] = (j0 + e < a.Tout && i < a.T) ? xr[i] : 0.f;
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = elu_act(v[e], a.alpha, a.elu);
    if (a.vec_store) {
        *reinterpret_cast<float4*>(yr + j0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (j0 + e < a.Tout) yr[j0 + e] = v[e];
    }
}

}  // namespace amp

using namespace amp;

extern "C" {

int amp_elu_pad(const float* x_dev, int B, int C, int T, int pad_left, int pad_right, int elu, float alpha, float* y_dev, void* stream) {
    if (pad_left < 0 || pad_right < 0) { set_error("amp_elu_pad: pad_left=%d pad_right=%d", pad_left, pad_right); return AMP_ERR_INVALID; }
    if (B <= 0 || C <= 0 || T <= 0) { set_error("amp_elu_pad: B=%d C=%d T=%d", B, C, T); return AMP_ERR_INVALID; }
    if (!x_dev || !y_dev) { set_error("amp_elu_pad: null argument"); return AMP_ERR_INVALID; }
    if (x_dev == y_dev && (pad_left || pad_right)) { set_error("amp_elu_pad: y may alias x only with zero pads"); return AMP_ERR_INVALID; }
    const long long tout = (long long)T + pad_left + pad_right;
    const int max_pad = pad_left > pad_right ? pad_left : pad_right;
    if (tout > 0x40000000ll) { set_error("amp_elu_pad: T_out = %lld is beyond 2^30", tout); return AMP_ERR_UNSUPPORTED; }
    EluPadArgs a{};
    a.x = x_dev; a.y = y_dev; a.T = T; a.Tout = (int)tout; a.pl = pad_left; a.elu = elu ? 1 : 0; a.alpha = alpha;
    a.Lext = T <= max_pad ? max_pad + 1 : T;
    a.q4 = (a.Tout + 3) / 4;
    a.vec_store = (a.Tout % 4 == 0 && (reinterpret_cast<uintptr_t>(y_dev) & 15) == 0) ? 1 : 0;
    a.quads = (long long)B * C * a.q4;
    const long long blocks = (a.quads + 255) / 256;
    if (blocks > 0x7fffffffll) { set_error("amp_elu_pad: B=%d x C=%d x T_out=%d is beyond the grid", B, C, a.Tout); return AMP_ERR_UNSUPPORTED; }
    note_kernel("elu_pad_kernel");
    note_work((unsigned long long)blocks, 0.0, 4.0 * ((double)B * C * T + (double)B * C * a.Tout) / 1e6, "elu_pad C=%d T=%d pad=%d,%d elu=%d B=%d", C, T,
              pad_left, pad_right, a.elu, B);
    hipLaunchKernelGGL(elu_pad_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    AMP_HIP(hipGetLastError());
    return AMP_OK;
}

}  // extern "C"
