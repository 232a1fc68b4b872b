// Exact-erf GELU (nn.GELU()) shared by the VITS text kernels (vits_text.hip) and the pointwise GEMM epilogue (pw_f16x3.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace amp {

// Contraction is switched off inside these helpers and the fused operations are written out, so every kernel rounds alike; the
// opaque move keeps a CALLER from contracting across the return value (vits_text.hip explains where hipcc did and did not).
__device__ __forceinline__ float fp_opaque(float v) {
    asm volatile("" : "+v"(v));
    return v;
}
__device__ __forceinline__ float gelu_erf(float v) {
#pragma clang fp contract(off)
    const float e = 1.0f + fp_opaque(erff(v * 0.70710678118654752f));
    return fp_opaque((0.5f * v) * e);
}

}  // namespace amp
