// View-dependent colour from spherical-harmonic coefficients, the SH branch of the reference's render_one
// (src/models/renderer.py:540-545 with eval_sh, src/utils/graphic_utils.py:707-762):
//
//     d      = (p - campos) / |p - campos|                      (a plain division, no epsilon)
//     colour = max(sum_k B_k(d) * sh[k][c] + 0.5, 0)            (no clamp at 1)
//
// and its backward.  One source for sh_color.hip (forward and backward kernels) and for tools/sh_eval_host.cpp, which a
// plain host compiler builds: no HIP header is needed here.  The backward replays the forward's statements (direction,
// basis, pre-clamp sum) from this file, so its gate `pre > 0` is the forward's clamp bit for bit and no mask is stored.
// Contraction is off in every body (the pragma covers the body it is written in): the bits must not depend on which
// kernel a helper was inlined into.
//
// The real SH basis up to degree 4, in the order and signs of the reference (and of the 3D Gaussian splatting code it
// descends from): k = l*l + l + m, odd m carry the Condon-Shortley sign.  On the unit sphere (r = 1):
//   l = 0   1/(2 sqrt(pi))
//   l = 1   sqrt(3/(4 pi)) * (-y, z, -x)
//   l = 2   sqrt(15/pi)/2 * (xy, -yz, ., -xz, .),  m = 0: sqrt(5/pi)/4 (2zz - xx - yy),  m = 2: sqrt(15/pi)/4 (xx - yy)
//   l = 3   -sqrt(35/(2 pi))/4 y(3xx - yy),  sqrt(105/pi)/2 xyz,  -sqrt(21/(2 pi))/4 y(4zz - xx - yy),
//           sqrt(7/pi)/4 z(2zz - 3xx - 3yy),  -sqrt(21/(2 pi))/4 x(4zz - xx - yy),  sqrt(105/pi)/4 z(xx - yy),
//           -sqrt(35/(2 pi))/4 x(xx - 3yy)
//   l = 4   3 sqrt(35/pi)/4 xy(xx - yy),  -3 sqrt(35/(2 pi))/4 yz(3xx - yy),  3 sqrt(5/pi)/4 xy(7zz - 1),
//           -3 sqrt(5/(2 pi))/4 yz(7zz - 3),  3/(16 sqrt(pi)) (35 z^4 - 30 zz + 3),  -3 sqrt(5/(2 pi))/4 xz(7zz - 3),
//           3 sqrt(5/pi)/8 (xx - yy)(7zz - 1),  -3 sqrt(35/(2 pi))/4 xz(xx - 3yy),
//           3 sqrt(35/pi)/16 (xx(xx - 3yy) - yy(3xx - yy))
// The derivatives treat x, y, z as independent variables of these polynomials; which extension off the sphere is
// chosen does not matter to a caller, because d(d)/d(p) = (I - d d^T) / |p - campos| removes the radial part.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define AMAV_SH_FN __host__ __device__ __forceinline__
#else
#define AMAV_SH_FN inline
#endif
#if defined(__clang__)
#define AMAV_SH_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define AMAV_SH_NO_CONTRACT  // a host compiler without FMA code generation has nothing to contract
#endif

namespace amav {
namespace sh {

constexpr int kMaxDegree = 4;
constexpr int num_coeffs(int degree) { return (degree + 1) * (degree + 1); }

constexpr float kC0 = 0.28209479177387814f;   // 1 / (2 sqrt(pi))
constexpr float kC1 = 0.4886025119029199f;    // sqrt(3 / (4 pi))
constexpr float kC2a = 1.0925484305920792f;   // sqrt(15 / pi) / 2
constexpr float kC2b = 0.31539156525252005f;  // sqrt(5 / pi) / 4
constexpr float kC2c = 0.5462742152960396f;   // sqrt(15 / pi) / 4
constexpr float kC3a = 0.5900435899266435f;   // sqrt(35 / (2 pi)) / 4
constexpr float kC3b = 2.890611442640554f;    // sqrt(105 / pi) / 2
constexpr float kC3c = 0.4570457994644658f;   // sqrt(21 / (2 pi)) / 4
constexpr float kC3d = 0.3731763325901154f;   // sqrt(7 / pi) / 4
constexpr float kC3e = 1.445305721320277f;    // sqrt(105 / pi) / 4
constexpr float kC4a = 2.5033429417967046f;   // 3 sqrt(35 / pi) / 4
constexpr float kC4b = 1.7701307697799304f;   // 3 sqrt(35 / (2 pi)) / 4
constexpr float kC4c = 0.9461746957575601f;   // 3 sqrt(5 / pi) / 4
constexpr float kC4d = 0.6690465435572892f;   // 3 sqrt(5 / (2 pi)) / 4
constexpr float kC4e = 0.10578554691520431f;  // 3 / (16 sqrt(pi))
constexpr float kC4f = 0.47308734787878004f;  // 3 sqrt(5 / pi) / 8
constexpr float kC4g = 0.6258357354491761f;   // 3 sqrt(35 / pi) / 16

// B[0 .. (D+1)^2) at the direction (x, y, z)
template <int D>
AMAV_SH_FN void basis(float x, float y, float z, float *B) {
    AMAV_SH_NO_CONTRACT
    B[0] = kC0;
    if (D < 1) return;
    B[1] = -kC1 * y;
    B[2] = kC1 * z;
    B[3] = -kC1 * x;
    if (D < 2) return;
    const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
    B[4] = kC2a * xy;
    B[5] = -kC2a * yz;
    B[6] = kC2b * (2.0f * zz - xx - yy);
    B[7] = -kC2a * xz;
    B[8] = kC2c * (xx - yy);
    if (D < 3) return;
    B[9] = -kC3a * y * (3.0f * xx - yy);
    B[10] = kC3b * xy * z;
    B[11] = -kC3c * y * (4.0f * zz - xx - yy);
    B[12] = kC3d * z * (2.0f * zz - 3.0f * xx - 3.0f * yy);
    B[13] = -kC3c * x * (4.0f * zz - xx - yy);
    B[14] = kC3e * z * (xx - yy);
    B[15] = -kC3a * x * (xx - 3.0f * yy);
    if (D < 4) return;
    B[16] = kC4a * xy * (xx - yy);
    B[17] = -kC4b * yz * (3.0f * xx - yy);
    B[18] = kC4c * xy * (7.0f * zz - 1.0f);
    B[19] = -kC4d * yz * (7.0f * zz - 3.0f);
    B[20] = kC4e * (zz * (35.0f * zz - 30.0f) + 3.0f);
    B[21] = -kC4d * xz * (7.0f * zz - 3.0f);
    B[22] = kC4f * (xx - yy) * (7.0f * zz - 1.0f);
    B[23] = -kC4b * xz * (xx - 3.0f * yy);
    B[24] = kC4g * (xx * (xx - 3.0f * yy) - yy * (3.0f * xx - yy));
}

// The partial derivatives of basis<D> with respect to x, y and z (the polynomials above, term by term)
template <int D>
AMAV_SH_FN void basis_grad(float x, float y, float z, float *Bx, float *By, float *Bz) {
    AMAV_SH_NO_CONTRACT
    Bx[0] = 0.0f, By[0] = 0.0f, Bz[0] = 0.0f;
    if (D < 1) return;
    Bx[1] = 0.0f, By[1] = -kC1, Bz[1] = 0.0f;
    Bx[2] = 0.0f, By[2] = 0.0f, Bz[2] = kC1;
    Bx[3] = -kC1, By[3] = 0.0f, Bz[3] = 0.0f;
    if (D < 2) return;
    const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
    Bx[4] = kC2a * y, By[4] = kC2a * x, Bz[4] = 0.0f;
    Bx[5] = 0.0f, By[5] = -kC2a * z, Bz[5] = -kC2a * y;
    Bx[6] = kC2b * (-2.0f * x), By[6] = kC2b * (-2.0f * y), Bz[6] = kC2b * (4.0f * z);
    Bx[7] = -kC2a * z, By[7] = 0.0f, Bz[7] = -kC2a * x;
    Bx[8] = kC2c * (2.0f * x), By[8] = kC2c * (-2.0f * y), Bz[8] = 0.0f;
    if (D < 3) return;
    // y (3xx - yy)
    Bx[9] = -kC3a * (6.0f * xy), By[9] = -kC3a * (3.0f * xx - 3.0f * yy), Bz[9] = 0.0f;
    // xyz
    Bx[10] = kC3b * yz, By[10] = kC3b * xz, Bz[10] = kC3b * xy;
    // y (4zz - xx - yy)
    Bx[11] = -kC3c * (-2.0f * xy), By[11] = -kC3c * (4.0f * zz - xx - 3.0f * yy), Bz[11] = -kC3c * (8.0f * yz);
    // z (2zz - 3xx - 3yy)
    Bx[12] = kC3d * (-6.0f * xz), By[12] = kC3d * (-6.0f * yz), Bz[12] = kC3d * (6.0f * zz - 3.0f * xx - 3.0f * yy);
    // x (4zz - xx - yy)
    Bx[13] = -kC3c * (4.0f * zz - 3.0f * xx - yy), By[13] = -kC3c * (-2.0f * xy), Bz[13] = -kC3c * (8.0f * xz);
    // z (xx - yy)
    Bx[14] = kC3e * (2.0f * xz), By[14] = kC3e * (-2.0f * yz), Bz[14] = kC3e * (xx - yy);
    // x (xx - 3yy)
    Bx[15] = -kC3a * (3.0f * xx - 3.0f * yy), By[15] = -kC3a * (-6.0f * xy), Bz[15] = 0.0f;
    if (D < 4) return;
    const float s1 = 7.0f * zz - 1.0f, s3 = 7.0f * zz - 3.0f;
    // xy (xx - yy) = x^3 y - x y^3
    Bx[16] = kC4a * (y * (3.0f * xx - yy)), By[16] = kC4a * (x * (xx - 3.0f * yy)), Bz[16] = 0.0f;
    // yz (3xx - yy)
    Bx[17] = -kC4b * (6.0f * xy * z), By[17] = -kC4b * (z * (3.0f * xx - 3.0f * yy)), Bz[17] = -kC4b * (y * (3.0f * xx - yy));
    // xy (7zz - 1)
    Bx[18] = kC4c * (y * s1), By[18] = kC4c * (x * s1), Bz[18] = kC4c * (14.0f * xy * z);
    // yz (7zz - 3) = 7 y z^3 - 3 y z
    Bx[19] = 0.0f, By[19] = -kC4d * (z * s3), Bz[19] = -kC4d * (y * (21.0f * zz - 3.0f));
    // 35 z^4 - 30 zz + 3
    Bx[20] = 0.0f, By[20] = 0.0f, Bz[20] = kC4e * (z * (140.0f * zz - 60.0f));
    // xz (7zz - 3)
    Bx[21] = -kC4d * (z * s3), By[21] = 0.0f, Bz[21] = -kC4d * (x * (21.0f * zz - 3.0f));
    // (xx - yy)(7zz - 1)
    Bx[22] = kC4f * (2.0f * x * s1), By[22] = kC4f * (-2.0f * y * s1), Bz[22] = kC4f * (14.0f * z * (xx - yy));
    // xz (xx - 3yy) = x^3 z - 3 x yy z
    Bx[23] = -kC4b * (z * (3.0f * xx - 3.0f * yy)), By[23] = -kC4b * (-6.0f * xy * z), Bz[23] = -kC4b * (x * (xx - 3.0f * yy));
    // x^4 - 6 xx yy + y^4
    Bx[24] = kC4g * (4.0f * x * (xx - 3.0f * yy)), By[24] = kC4g * (4.0f * y * (yy - 3.0f * xx)), Bz[24] = 0.0f;
}

// d = (p - campos) / |p - campos| and 1 / |p - campos| (the backward's factor).  A point at the camera centre gives NaN,
// as in the reference; the rasterizer culls such a Gaussian at the near plane.
struct Direction {
    float x, y, z, inv_len;
};
AMAV_SH_FN Direction direction(const float *p, const float *campos) {
    AMAV_SH_NO_CONTRACT
    const float dx = p[0] - campos[0], dy = p[1] - campos[1], dz = p[2] - campos[2];
    const float len = sqrtf(dx * dx + dy * dy + dz * dz);
    return {dx / len, dy / len, dz / len, 1.0f / len};
}

// sum_k B_k * sh[k][c] + 0.5 of channel c; `rec` is one Gaussian's record, coefficient k of channel c at rec[k * 3 + c]
template <int D>
AMAV_SH_FN float pre_clamp(const float *B, const float *rec, int c) {
    AMAV_SH_NO_CONTRACT
    float acc = B[0] * rec[c];
#if defined(__clang__)
#pragma unroll
#endif
    for (int k = 1; k < num_coeffs(D); ++k) acc = acc + B[k] * rec[k * 3 + c];
    return acc + 0.5f;
}

// clamp_min(., 0): NaN stays NaN, as torch's
AMAV_SH_FN float clamp_colour(float pre) { return pre < 0.0f ? 0.0f : pre; }

// Forward of one Gaussian: colour[3]
template <int D>
AMAV_SH_FN void colour(const float *p, const float *campos, const float *rec, float *out) {
    const Direction d = direction(p, campos);
    float B[num_coeffs(D)];
    basis<D>(d.x, d.y, d.z, B);
    for (int c = 0; c < 3; ++c) out[c] = clamp_colour(pre_clamp<D>(B, rec, c));
}

// Backward of one Gaussian for the colour gradient g[3]: grad_rec[k * 3 + c] = gate_c g_c B_k for k < (D+1)^2 (the
// caller zeroes the coefficients beyond; grad_rec may be `rec` itself: every coefficient is read before it is written)
// and, with want_p, grad_p[3] = (I - d d^T) / |p - campos| * sum_k grad B_k(d) sum_c gate_c g_c sh[k][c].
template <int D>
AMAV_SH_FN void colour_backward(const float *p, const float *campos, const float *rec, const float *g, float *grad_rec,
                                float *grad_p, bool want_p) {
    AMAV_SH_NO_CONTRACT
    const Direction d = direction(p, campos);
    float B[num_coeffs(D)];
    basis<D>(d.x, d.y, d.z, B);
    float gg[3];
    for (int c = 0; c < 3; ++c) gg[c] = pre_clamp<D>(B, rec, c) > 0.0f ? g[c] : 0.0f;  // the forward's clamp, replayed
    float gx = 0.0f, gy = 0.0f, gz = 0.0f;
    if (want_p) {
        float Bx[num_coeffs(D)], By[num_coeffs(D)], Bz[num_coeffs(D)];
        basis_grad<D>(d.x, d.y, d.z, Bx, By, Bz);
#if defined(__clang__)
#pragma unroll
#endif
        for (int k = 1; k < num_coeffs(D); ++k) {
            const float v = gg[0] * rec[k * 3] + gg[1] * rec[k * 3 + 1] + gg[2] * rec[k * 3 + 2];
            gx = gx + v * Bx[k], gy = gy + v * By[k], gz = gz + v * Bz[k];
        }
    }
#if defined(__clang__)
#pragma unroll
#endif
    for (int k = 0; k < num_coeffs(D); ++k)
        for (int c = 0; c < 3; ++c) grad_rec[k * 3 + c] = gg[c] * B[k];
    if (want_p) {
        const float radial = d.x * gx + d.y * gy + d.z * gz;
        grad_p[0] = (gx - d.x * radial) * d.inv_len;
        grad_p[1] = (gy - d.y * radial) * d.inv_len;
        grad_p[2] = (gz - d.z * radial) * d.inv_len;
    }
}

}  // namespace sh
}  // namespace amav
