// fp16 x 2 split-product operands, shared by the kernels that run fp32-equivalent products on
// v_mfma_f32_32x32x16_f16: an operand scaled by one exact power of two becomes h1 + h2, and a product is h2 g1 + h1 g2 +
// h1 g1 with fp32 accumulation, small terms first.
#pragma once
#include <hip/hip_runtime.h>

namespace amav {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
constexpr size_t kSplitHeader = 256;  // prepared weights: [0] float largest |w|, [1] int scale exponent

__device__ __forceinline__ int f16_scale_exp(float amax) {
    if (!(amax > 0.f)) return 0;
    return max(-100, min(100, 14 - ilogbf(amax)));
}
// Two-way split: x = a + b to 22 bits when the residual stays out of fp16's subnormals, which the callers arrange by
// pre-scaling x with 2^f16_scale_exp(bound of the tensor) (exact), so that the bound sits just under fp16's maximum.
__device__ __forceinline__ void split2(float x, _Float16 &a, _Float16 &b) {
    a = (_Float16)x;
    b = (_Float16)__builtin_fmaf((float)a, -1.0f, x);  // x - a, exact; written as an fma so it can be one mixed-precision op
}
// max(m, |a.x|, .., |a.w|): one step of the magnitude sweeps that feed f16_scale_exp
__device__ __forceinline__ float absmax4(float m, const float4 a) {
    return fmaxf(m, fmaxf(fmaxf(fabsf(a.x), fabsf(a.y)), fmaxf(fabsf(a.z), fabsf(a.w))));
}

}  // namespace amav
