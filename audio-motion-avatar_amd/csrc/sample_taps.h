// Bilinear taps of Renderer.sample_from_triplane (amav_triplane_sample_features), shared by the sampling kernels
// (triplane.hip) and their backward (triplane_sample_backward.hip): one definition, so both see the same texels and
// the same weights, bit for bit.
#pragma once
#include <hip/hip_runtime.h>

namespace amav {
namespace triplane {

// torch grid_sampler, bilinear, align_corners=False, padding zeros: pixel = ((g + 1) * size - 1) / 2
struct Taps {
    int ix0, iy0;
    float wx0, wx1, wy0, wy1;
};

__device__ __forceinline__ Taps make_taps(float gx, float gy, int R) {
    const float ix = ((gx + 1.0f) * (float)R - 1.0f) * 0.5f;
    const float iy = ((gy + 1.0f) * (float)R - 1.0f) * 0.5f;
    const float fx = floorf(ix), fy = floorf(iy);
    Taps t;
    t.ix0 = (int)fx, t.iy0 = (int)fy;
    t.wx1 = ix - fx, t.wx0 = (fx + 1.0f) - ix;
    t.wy1 = iy - fy, t.wy0 = (fy + 1.0f) - iy;
    return t;
}

// grid coordinate of a point coordinate: clamp(p / radius, -1, 1)
__device__ __forceinline__ float sample_unit(float p, float radius) { return fminf(fmaxf(p / radius, -1.0f), 1.0f); }

}  // namespace triplane
}  // namespace amav
