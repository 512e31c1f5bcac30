// The texel rectangle of a frame's plane that amav_triplane_project_region projects, shared by triplane.hip's
// project_kernel and triplane_backward.hip (which must read, write and zero exactly the same texels).
#pragma once
#include <hip/hip_runtime.h>

namespace amav {
namespace triplane {

// The texels of plane `plane` that bilinear taps of points inside the box [lo, hi] (world space) can touch, with
// sample_decode_kernel's own arithmetic (u = clamp(p / radius), pixel = ((u + 1) R - 1) / 2, taps floor and floor + 1,
// out-of-range taps read the clamped address): every step is monotonic in p, so the taps of any point of the box --
// in particular of any point the subdivision table averages from vertices inside it -- lie in the returned rectangle
// [x0, x1] x [y0, y1] (inclusive, already clamped to the plane).
struct TexelRect {
    int x0, x1, y0, y1;
};
__device__ __forceinline__ int tap_floor(float p, float radius, int R) {
    const float u = fminf(fmaxf(p / radius, -1.0f), 1.0f);
    return (int)floorf(((u + 1.0f) * (float)R - 1.0f) * 0.5f);
}
__device__ __forceinline__ TexelRect region_of(const float *__restrict__ box, int plane, float radius, int R) {
    // plane 0 <- (x, y), plane 1 <- (x, z), plane 2 <- (y, z); grid x indexes W, grid y indexes H
    const int ax = plane == 2 ? 1 : 0, ay = plane == 0 ? 1 : 2;
    TexelRect r;
    r.x0 = min(max(tap_floor(box[ax], radius, R), 0), R - 1);
    r.x1 = min(max(tap_floor(box[3 + ax], radius, R) + 1, 0), R - 1);
    r.y0 = min(max(tap_floor(box[ay], radius, R), 0), R - 1);
    r.y1 = min(max(tap_floor(box[3 + ay], radius, R) + 1, 0), R - 1);
    return r;
}

}  // namespace triplane
}  // namespace amav
