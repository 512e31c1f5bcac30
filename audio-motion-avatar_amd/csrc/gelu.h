// Exact-erf GELU and its derivative, one expression each for the kernels that share it.
#pragma once
#include <hip/hip_runtime.h>

namespace amav {

__device__ __forceinline__ float gelu(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }
// Phi(z) + z phi(z)
__device__ __forceinline__ float gelu_grad(float z) {
    return 0.5f * (1.0f + erff(z * 0.70710678118654752440f)) + z * 0.39894228040143267794f * expf(-0.5f * z * z);
}

}  // namespace amav
