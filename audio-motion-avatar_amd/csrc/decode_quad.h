// Triplane decode of one point by a quad of lanes (4 lanes per point, lane q owns projected channels 4q..4q+3), shared
// by triplane.hip's sample_decode_kernel and rasterizer.hip's decoding binning block (bin_kernel<., ., true>); its
// per-plane taps and per-group pieces are also what triplane_backward.hip recomputes the forward with.
//
// The arithmetic is pinned: contraction is off and every fused multiply-add is written out, in the places where the
// compiler fused them when this code lived inside sample_decode_kernel alone (triplane.o, SLP on).  Inlined into another
// kernel -- rasterizer.o is built without SLP packing -- the compiler would otherwise contract differently (the
// rotation's sum of squares, for one, is four separate products in the packed build and becomes a chain of FMAs in the scalar
// one), and the two paths could no longer produce the same packed records bit for bit.
#pragma once
#include <hip/hip_runtime.h>

namespace amav {
namespace decode {

// value of lane K of this lane's quad
template <int K>
__device__ __forceinline__ float quad_bcast(float v) {
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), K * 0x55, 0xf, 0xf, true));
}
template <int K>
__device__ __forceinline__ int quad_bcast_i(int v) {
    return __builtin_amdgcn_mov_dpp(v, K * 0x55, 0xf, 0xf, true);
}

// The point from its four base vertices, one per lane of the quad (the lane's own vertex in v0..v2):
// 1/2 (1/2 (v[a0]+v[b0]) + 1/2 (v[a1]+v[b1])), the operation order of lbs.hip's gather_kernel
__device__ __forceinline__ void quad_point(float v0, float v1, float v2, float &p0, float &p1, float &p2) {
#pragma clang fp contract(off)
    p0 = fmaf(quad_bcast<0>(v0) + quad_bcast<1>(v0), 0.5f, (quad_bcast<2>(v0) + quad_bcast<3>(v0)) * 0.5f) * 0.5f;
    p1 = fmaf(quad_bcast<0>(v1) + quad_bcast<1>(v1), 0.5f, (quad_bcast<2>(v1) + quad_bcast<3>(v1)) * 0.5f) * 0.5f;
    p2 = ((quad_bcast<0>(v2) + quad_bcast<1>(v2)) * 0.5f + (quad_bcast<2>(v2) + quad_bcast<3>(v2)) * 0.5f) * 0.5f;
}

// Bilinear taps, torch grid_sampler, bilinear, align_corners=False, zero padding: pixel = ((g + 1) * R - 1) / 2; an
// out-of-range texel is a clamped address with weight 0.  clamp_unit is the grid coordinate of a point coordinate;
// plane 0 <- (x, y), plane 1 <- (x, z), plane 2 <- (y, z); grid x indexes W, grid y indexes H.
__device__ __forceinline__ float clamp_unit(float p, float radius) {
#pragma clang fp contract(off)
    return fminf(fmaxf(p / radius, -1.0f), 1.0f);  // IEEE division, as torch: the taps depend on it
}

// One plane's taps: tap (dy, dx) is texel (ix0 + dx, iy0 + dy), weight wx[dx] * wy[dy]; per tap k = dy * 2 + dx, its
// offset in float4 units from the plane's first texel (clamped address), its weight (0 outside) and whether it is inside
struct PlaneTaps {
    int ix0, iy0;
    float wx0, wx1, wy0, wy1;
    int off[4];
    float w[4];
    bool in[4];
};
__device__ __forceinline__ PlaneTaps plane_taps(float gx, float gy, int R) {
#pragma clang fp contract(off)
    const float sx = fmaf(gx + 1.0f, (float)R, -1.0f), sy = fmaf(gy + 1.0f, (float)R, -1.0f);  // 2 * pixel
    const float fx = floorf(sx * 0.5f), fy = floorf(sy * 0.5f);
    PlaneTaps t;
    t.ix0 = (int)fx, t.iy0 = (int)fy;
    t.wx1 = fmaf(sx, 0.5f, -fx), t.wx0 = fmaf(-sx, 0.5f, fx + 1.0f);
    t.wy1 = fmaf(sy, 0.5f, -fy), t.wy0 = fmaf(-sy, 0.5f, fy + 1.0f);
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
            const int x = t.ix0 + dx, y = t.iy0 + dy;
            const bool in = x >= 0 && x < R && y >= 0 && y < R;
            const int cx = min(max(x, 0), R - 1), cy = min(max(y, 0), R - 1);
            t.in[dy * 2 + dx] = in;
            t.w[dy * 2 + dx] = in ? (dx ? t.wx1 : t.wx0) * (dy ? t.wy1 : t.wy0) : 0.0f;
            t.off[dy * 2 + dx] = (cy * R + cx) * 4;
        }
    return t;
}

// The twelve taps of a point (plane, then dy, then dx): texel offsets in float4 units from the frame's plane 0 and
// bilinear weights.  Lane q < 3 works out plane q's four pairs and the quad trades them by DPP (every lane of the quad
// ends up with all twelve).
struct QuadTaps {
    int off[12];
    float w[12];
};
__device__ __forceinline__ QuadTaps quad_taps(float p0, float p1, float p2, float radius, int R, int q) {
#pragma clang fp contract(off)
    const float u0 = clamp_unit(p0, radius), u1 = clamp_unit(p1, radius), u2 = clamp_unit(p2, radius);
    const PlaneTaps pt = plane_taps(q == 2 ? u1 : u0, q == 0 ? u1 : u2, R);
    QuadTaps t;
    const int RR4 = R * R * 4;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        t.w[k] = quad_bcast<0>(pt.w[k]), t.w[4 + k] = quad_bcast<1>(pt.w[k]), t.w[8 + k] = quad_bcast<2>(pt.w[k]);
        t.off[k] = quad_bcast_i<0>(pt.off[k]);
        t.off[4 + k] = RR4 + quad_bcast_i<1>(pt.off[k]);
        t.off[8 + k] = 2 * RR4 + quad_bcast_i<2>(pt.off[k]);
    }
    return t;
}

// Raw head outputs of one group of four channels (quad lane q of the decode: channels 4q..4q+3) from its twelve tap
// values, the point and the group's head weights wp[0..3] (wpoint [16][4]: 3 xyz weights, bias, per channel):
// sum_k w_k tap_k + W_xyz p + bias
__device__ __forceinline__ float4 group_raw(const float4 (&tv)[12], const float (&tw)[12], const float4 (&wp)[4],
                                            float p0, float p1, float p2) {
#pragma clang fp contract(off)
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        const float w = tw[k];
        const float4 v = tv[k];
        acc.x = fmaf(v.x, w, acc.x), acc.y = fmaf(v.y, w, acc.y), acc.z = fmaf(v.z, w, acc.z), acc.w = fmaf(v.w, w, acc.w);
    }
    const float4 w0 = wp[0], w1 = wp[1], w2 = wp[2], w3 = wp[3];
    acc.x += fmaf(w0.z, p2, fmaf(w0.y, p1, w0.x * p0)) + w0.w;
    acc.y += fmaf(w1.z, p2, fmaf(w1.x, p0, w1.y * p1)) + w1.w;
    acc.z += fmaf(w2.z, p2, fmaf(w2.y, p1, w2.x * p0)) + w2.w;
    acc.w += fmaf(w3.z, p2, fmaf(w3.x, p0, w3.y * p1)) + w3.w;
    return acc;
}

// F.normalize(dim=-1) of the rotation group: v / max(||v||, 1e-12); nrm = ||v|| before the clamp, inv = the factor
__device__ __forceinline__ float4 normalize4(float4 a, float &nrm, float &inv) {
#pragma clang fp contract(off)
    nrm = __fsqrt_rn(a.x * a.x + a.y * a.y + a.z * a.z + a.w * a.w);
    inv = __frcp_rn(fmaxf(nrm, 1e-12f));
    return make_float4(a.x * inv, a.y * inv, a.z * inv, a.w * inv);
}

__device__ __forceinline__ float sigmoid(float x) {
#pragma clang fp contract(off)
    return __frcp_rn(1.0f + __expf(-x));
}

// The lane's record quarter from its twelve tap values, the point and its head weights:
//   q0 = (xyz + offset + transl, opacity), q1 = normalised rotation, q2 = (scaling, 0), q3 = (sigmoid(shs), 0)
__device__ __forceinline__ float4 quad_record(const float4 (&tv)[12], const float (&tw)[12], const float4 (&wp)[4],
                                              float p0, float p1, float p2, float tx, float ty, float tz, int q) {
#pragma clang fp contract(off)
    const float4 acc = group_raw(tv, tw, wp, p0, p1, p2);
    if (q == 0) return make_float4(p0 + acc.x + tx, p1 + acc.y + ty, p2 + acc.z + tz, acc.w);
    if (q == 1) {
        float nrm, inv;
        return normalize4(acc, nrm, inv);
    }
    if (q == 2) return make_float4(acc.x, acc.y, acc.z, 0.0f);
    return make_float4(sigmoid(acc.x), sigmoid(acc.y), sigmoid(acc.z), 0.0f);
}

}  // namespace decode
}  // namespace amav
