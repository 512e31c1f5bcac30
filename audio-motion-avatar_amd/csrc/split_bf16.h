// bf16 x 3 split-product operands, shared by the kernels that run fp32-equivalent products on
// v_mfma_f32_32x32x16_bf16: an fp32 operand becomes x1 + x2 + x3 (24 mantissa bits, the subtractions are exact), and a
// product is the six partial products x_i y_j with i + j <= 4 with fp32 accumulation, small terms first.
#pragma once
#include <hip/hip_runtime.h>

namespace amav {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void split3(float x, __bf16 &a, __bf16 &b, __bf16 &c) {
    a = (__bf16)x;
    const float r1 = x - (float)a;
    b = (__bf16)r1;
    c = (__bf16)(r1 - (float)b);
}

}  // namespace amav
