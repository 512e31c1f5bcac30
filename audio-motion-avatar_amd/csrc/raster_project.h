// Stages of the projection of one Gaussian and the staging of its blend record into a tile, shared by rasterizer.hip
// (preprocess_one, render_kernel) and rasterizer_backward.hip (gauss_grad_kernel, tile_grad_kernel), so the backward
// replays the forward's own arithmetic.  A stage returns the intermediates the backward needs; the forward leaves them
// unused and the compiler drops them.
//
// Contraction is off in every helper (the pragma covers the body it is written in, not the caller): rasterizer.o and
// rasterizer_backward.o are built with different flags, and the arithmetic must not depend on either (decode_quad.h).
#pragma once
#include "amav_common.h"

namespace amav {
namespace raster {

constexpr int kTile = AMAV_TILE;
constexpr float kLog2e = 1.4426950408889634f;

__device__ __forceinline__ const float *at(const amav_attr &a, int f, int i) {
    return a.ptr + (long long)f * a.frame_stride + (long long)i * a.elem_stride;
}

// view-space point (vm: column-major view matrix)
struct ViewPoint {
    float x, y, z;
};
__device__ __forceinline__ ViewPoint view_point(const float *vm, float px, float py, float pz) {
#pragma clang fp contract(off)
    ViewPoint v;
    v.x = vm[0] * px + vm[4] * py + vm[8] * pz + vm[12];
    v.y = vm[1] * px + vm[5] * py + vm[9] * pz + vm[13];
    v.z = vm[2] * px + vm[6] * py + vm[10] * pz + vm[14];
    return v;
}

// clip-space point (pm: column-major projection matrix): hx, hy, pw = 1 / (hw + eps) and the NDC point (ppx, ppy)
struct ClipPoint {
    float hx, hy, pw, ppx, ppy;
};
__device__ __forceinline__ ClipPoint clip_point(const float *pm, float px, float py, float pz) {
#pragma clang fp contract(off)
    ClipPoint c;
    c.hx = pm[0] * px + pm[4] * py + pm[8] * pz + pm[12];
    c.hy = pm[1] * px + pm[5] * py + pm[9] * pz + pm[13];
    const float hw = pm[3] * px + pm[7] * py + pm[11] * pz + pm[15];
    c.pw = 1.0f / (hw + 0.0000001f);
    c.ppx = c.hx * c.pw, c.ppy = c.hy * c.pw;
    return c;
}

// Activations (with apply_activations): scale min(exp(s - bias), max), with e = the raw exp (the backward splits the
// min's gradient on it); opacity sigmoid(o - bias)
__device__ __forceinline__ float scale_act(float s, float bias, float max, float &e) {
#pragma clang fp contract(off)
    e = expf(s - bias);
    return fminf(e, max);
}
__device__ __forceinline__ float opacity_act(float o, float bias) {
#pragma clang fp contract(off)
    return 1.0f / (1.0f + expf(-(o - bias)));
}

// Sigma3D = R diag(s)^2 R^T = M^T M with R = R(q) (q = (r, x, y, z), not normalised) and M[k][a] = s_k R[a][k]
struct Cov3 {
    float R[3][3], M[3][3], S[3][3];
};
__device__ __forceinline__ Cov3 cov3d(float r, float x, float y, float z, float s0, float s1, float s2) {
#pragma clang fp contract(off)
    Cov3 c = {{{1.f - 2.f * (y * y + z * z), 2.f * (x * y - r * z), 2.f * (x * z + r * y)},
               {2.f * (x * y + r * z), 1.f - 2.f * (x * x + z * z), 2.f * (y * z - r * x)},
               {2.f * (x * z - r * y), 2.f * (y * z + r * x), 1.f - 2.f * (x * x + y * y)}},
              {},
              {}};
    const float sv[3] = {s0, s1, s2};
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int a = 0; a < 3; ++a) c.M[k][a] = sv[k] * c.R[a][k];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) c.S[a][b] = c.M[0][a] * c.M[0][b] + c.M[1][a] * c.M[1][b] + c.M[2][a] * c.M[2][b];
    return c;
}

// cov2D = (J W) Sigma (J W)^T = [[ca, cb], [cb, cc]] from the rows T0, T1 of J W, before the +0.3 dilation (the
// callers add it); ST0 = Sigma T0, ST1 = Sigma T1
struct Cov2 {
    float ST0[3], ST1[3], ca, cb, cc;
};
__device__ __forceinline__ Cov2 cov2d(const float (&S)[3][3], const float (&T0)[3], const float (&T1)[3]) {
#pragma clang fp contract(off)
    Cov2 c;
#pragma unroll
    for (int a = 0; a < 3; ++a) c.ST0[a] = S[a][0] * T0[0] + S[a][1] * T0[1] + S[a][2] * T0[2];
#pragma unroll
    for (int a = 0; a < 3; ++a) c.ST1[a] = S[a][0] * T1[0] + S[a][1] * T1[1] + S[a][2] * T1[2];
    c.ca = T0[0] * c.ST0[0] + T0[1] * c.ST0[1] + T0[2] * c.ST0[2];
    c.cb = T0[0] * c.ST1[0] + T0[1] * c.ST1[1] + T0[2] * c.ST1[2];
    c.cc = T1[0] * c.ST1[0] + T1[1] * c.ST1[1] + T1[2] * c.ST1[2];
    return c;
}

// The blend record's quadratic form from the dilated 2D covariance (ca, cb, cc) and det_inv = 1 / (ca cc - cb^2),
// det > 0.  The blend needs log2(alpha) = log2(op) + log2(e) * power, power = -1/2 (A dx^2 + C dy^2) - B dx dy with the
// conic (A, B, C) = (cc, -cb, ca) / det.  It is stored as its Cholesky factor: with k = log2(e) / 2,
//     -log2(e) * power = (a dx + b dy)^2 + (c dy)^2,   a = sqrt(k A), b = k B / a, c = sqrt(k (C - B^2 / A)) = sqrt(k / cc)
// (A C - B^2 = 1 / det).  A sum of squares is >= 0 in floating point too, so upstream's "power > 0 -> skip" guard
// (which only ever fires on rounding noise of ITS three-term form) has nothing left to catch, and the blend kernel
// evaluates log2(alpha) in five fused multiply-adds (blend_px).
struct Conic {
    float A, qa, qb, qc;
};
__device__ __forceinline__ Conic conic(float cb, float cc, float det_inv) {
#pragma clang fp contract(off)
    const float kk = 0.5f * kLog2e;
    Conic q;
    q.A = cc * det_inv;
    q.qa = sqrtf(kk * q.A);
    q.qb = -(kk * (cb * det_inv)) / q.qa;
    q.qc = sqrtf(kk / cc);
    return q;
}

// A blend record {x, y, qa, qb} {qc, ...} moved into the frame of the tile whose first pixel is (X0, Y0):
// u = qa (x - px) + qb (y - py) = k0 - qa lx - qb ly with k0 = qa (x - X0) + qb (y - Y0) (one fma); v = k1 - qc ly
// with k1 = qc (y - Y0)
__device__ __forceinline__ float2 tile_k(const float4 &g0, const float4 &g1, float X0f, float Y0f) {
#pragma clang fp contract(off)
    const float rx = g0.x - X0f, ry = g0.y - Y0f;
    return make_float2(fmaf(g0.z, rx, g0.w * ry), g1.x * ry);
}

// The 8x8 quadrants of that tile (bit = quadrant x | y << 1) that the record's alpha >= 1/255 box {.., bx, by} (g2.z,
// g2.w: half extents around (x, y)) reaches
__device__ __forceinline__ int quad_mask(const float4 &g0, const float4 &g2, float X0f, float Y0f) {
#pragma clang fp contract(off)
    const bool hx0 = (g0.x + g2.z >= X0f) & (g0.x - g2.z <= X0f + 7.f);
    const bool hx1 = (g0.x + g2.z >= X0f + 8.f) & (g0.x - g2.z <= X0f + 15.f);
    const bool hy0 = (g0.y + g2.w >= Y0f) & (g0.y - g2.w <= Y0f + 7.f);
    const bool hy1 = (g0.y + g2.w >= Y0f + 8.f) & (g0.y - g2.w <= Y0f + 15.f);
    return (int)(hx0 & hy0) | ((int)(hx1 & hy0) << 1) | ((int)(hx0 & hy1) << 2) | ((int)(hx1 & hy1) << 3);
}

}  // namespace raster
}  // namespace amav
