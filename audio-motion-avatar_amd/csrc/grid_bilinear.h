// One axis of F.interpolate(mode="bilinear", align_corners=False) from a G-node grid to `size` pixels, evaluated at one
// pixel: the two source nodes and their weights.  Shared by amav_points_project_grid (splat.hip) and its backward
// (splat_backward.hip): one definition, so both see the same nodes and the same weights, bit for bit.
//
// Contraction is off in the helper (the pragma covers the body it is written in, not the caller), so the arithmetic
// does not depend on the flags of the file that includes it.
#pragma once
#include <hip/hip_runtime.h>

namespace amav {
namespace splat {

// value of a pixel = h * node[i0] + l * node[i1]; i0 == i1 in the clamped first and last half-cell (and when G == 1)
struct GridAxis {
    int i0, i1;
    float l, h;
};

__host__ __device__ __forceinline__ GridAxis grid_axis(int i, int size, int G) {
#pragma clang fp contract(off)
    const float scale = (float)G / (float)size;
    float s = scale * ((float)i + 0.5f) - 0.5f;
    s = s < 0.0f ? 0.0f : s;
    GridAxis a;
    a.i0 = (int)s;
    if (a.i0 > G - 1) a.i0 = G - 1;
    a.i1 = a.i0 + (a.i0 < G - 1 ? 1 : 0);
    a.l = s - (float)a.i0;
    a.h = 1.0f - a.l;
    return a;
}

// First pixel of [0, size) whose i0 is at least `node` (size if there is none).  i0 never decreases with the pixel:
// every operation of grid_axis is monotone and rounding keeps order, so a bisection over grid_axis itself finds the
// same boundary the forward used.
__host__ __device__ __forceinline__ int grid_axis_first_pixel(int node, int size, int G) {
    int lo = 0, hi = size;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (grid_axis(mid, size, G).i0 >= node)
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

}  // namespace splat
}  // namespace amav
