// Rotation arithmetic of the SMPL-X parameter term (device code), shared by the forward and the backward kernels of
// smplx_params.hip.  Every forward function returns a record of what it computed, branch choices included; the backward
// functions take that record, so a backward can only replay the branches its forward took (the single-source rule of
// the other backwards here).
//
//   rot6d_forward / rot6d_backward         smplx_decoder.py: matrix_to_axis_angle(rotation_6d_to_matrix(d6)), per row
//   rodrigues                              losses.batch_rodrigues, per row
//   geodesic_forward / geodesic_backward   losses.rotation_geodesic_loss, per pair of rows
#pragma once
#include <hip/hip_runtime.h>

namespace amav {
namespace smplx {

// The arithmetic runs in double.  These kernels are bound by their launch, not by their few thousand operations per
// lane, and in double the results are the float64 statement rounded once to fp32: no row of a nearly singular
// conversion (w near 0, cos near the clamp) is left to the order of a few dozen fp32 roundings.  Inputs, outputs and
// the constants are the fp32 interface's; the constants compare as the float64 evaluation of the Python compares them.
using real = double;

constexpr real kNormalizeEps = 1e-12;  // F.normalize: x / max(||x||, eps)
constexpr real kQuatDenomMin = 0.1;    // cand / (2 * q_abs.clamp_min(0.1))
constexpr real kSmallAngle = 1e-6;     // |angle| < 1e-6: the series of sin(angle / 2) / angle
constexpr real kRodriguesEps = 1e-8;   // angle = ||r + 1e-8||
constexpr real kCosClamp = 0.999;      // acos(clamp(cos, -0.999, 0.999))

__device__ __forceinline__ real dot3(const real *a, const real *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
__device__ __forceinline__ void cross3(const real *a, const real *b, real *c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// x / max(||x||, eps) and its gates: `above` is clamp_min's (norm >= eps passes the gradient to the norm), a norm of
// exactly 0 gives the norm no gradient (torch.norm's rule)
struct Normalized {
    real v[3], norm, denom;
    bool above;
};
__device__ __forceinline__ Normalized normalize3(const real *x) {
    Normalized n;
    n.norm = sqrt(dot3(x, x));
    n.above = n.norm >= kNormalizeEps;
    n.denom = fmax(n.norm, kNormalizeEps);
#pragma unroll
    for (int a = 0; a < 3; ++a) n.v[a] = x[a] / n.denom;
    return n;
}
// gx += the gradient of normalize3(x) for the gradient gv of its value
__device__ __forceinline__ void normalize3_backward(const real *x, const Normalized &n, const real *gv, real *gx) {
    const real gdenom = -dot3(gv, x) / (n.denom * n.denom);
    const real gnorm = n.above ? gdenom : 0.0;
    const real along = n.norm == 0.0 ? 0.0 : gnorm / n.norm;
#pragma unroll
    for (int a = 0; a < 3; ++a) gx[a] += gv[a] / n.denom + along * x[a];
}

// The four quaternion candidates' numerators (row `pick` of the Python `cand`, before the division); m row-major.
__device__ __forceinline__ void quat_candidate(int pick, const real *m, real qq, real *c) {
    const real m01 = m[1], m02 = m[2], m10 = m[3], m12 = m[5], m20 = m[6], m21 = m[7];
    switch (pick) {
        case 0: c[0] = qq, c[1] = m21 - m12, c[2] = m02 - m20, c[3] = m10 - m01; break;
        case 1: c[0] = m21 - m12, c[1] = qq, c[2] = m10 + m01, c[3] = m02 + m20; break;
        case 2: c[0] = m02 - m20, c[1] = m10 + m01, c[2] = qq, c[3] = m12 + m21; break;
        default: c[0] = m10 - m01, c[1] = m20 + m02, c[2] = m21 + m12, c[3] = qq; break;
    }
}

struct Rot6d {
    Normalized b1, b2;
    real dot, u[3];     // b2 = normalize(u), u = a2 - dot b1
    real m[9];          // rows b1, b2, b1 x b2
    real q2, q_abs;     // of the picked candidate
    int pick;            // the largest q_abs (the first of equal ones, as argmax)
    bool positive;       // q2 > 0: sqrt has a derivative
    bool above;          // q_abs >= 0.1: clamp_min passes the gradient
    bool flip;           // w < 0
    real cand[4], denom, quat[4];  // quat after the flip
    real norms, half, angle;
    bool small;          // |angle| < 1e-6
    real ratio;         // sin(half) / angle, or its series
    real aa[3];
};

__device__ __forceinline__ Rot6d rot6d_forward(const real *d6) {
    Rot6d r;
    const real *a1 = d6, *a2 = d6 + 3;
    r.b1 = normalize3(a1);
    r.dot = dot3(r.b1.v, a2);
#pragma unroll
    for (int a = 0; a < 3; ++a) r.u[a] = a2[a] - r.dot * r.b1.v[a];
    r.b2 = normalize3(r.u);
#pragma unroll
    for (int a = 0; a < 3; ++a) r.m[a] = r.b1.v[a], r.m[3 + a] = r.b2.v[a];
    cross3(r.b1.v, r.b2.v, r.m + 6);
    const real m00 = r.m[0], m11 = r.m[4], m22 = r.m[8];
    const real q2[4] = {1.0 + m00 + m11 + m22, 1.0 + m00 - m11 - m22, 1.0 - m00 + m11 - m22, 1.0 - m00 - m11 + m22};
    r.pick = 0;
    r.q2 = q2[0];
    r.q_abs = q2[0] > 0.0 ? sqrt(q2[0]) : 0.0;
#pragma unroll
    for (int i = 1; i < 4; ++i) {
        const real qa = q2[i] > 0.0 ? sqrt(q2[i]) : 0.0;
        if (qa > r.q_abs) r.pick = i, r.q2 = q2[i], r.q_abs = qa;
    }
    r.positive = r.q2 > 0.0;
    r.above = r.q_abs >= kQuatDenomMin;
    r.denom = 2.0 * fmax(r.q_abs, kQuatDenomMin);
    quat_candidate(r.pick, r.m, r.q_abs * r.q_abs, r.cand);
    real q[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] = r.cand[i] / r.denom;
    r.flip = q[0] < 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) r.quat[i] = r.flip ? -q[i] : q[i];
    r.norms = sqrt(dot3(r.quat + 1, r.quat + 1));
    r.half = atan2(r.norms, r.quat[0]);
    r.angle = 2.0 * r.half;
    r.small = fabs(r.angle) < kSmallAngle;
    r.ratio = r.small ? 0.5 - r.angle * r.angle / 48.0 : sin(r.half) / r.angle;
#pragma unroll
    for (int a = 0; a < 3; ++a) r.aa[a] = r.quat[1 + a] / r.ratio;
    return r;
}

// grad_d6 [6] for grad_aa [3], through the branches `r` recorded
__device__ __forceinline__ void rot6d_backward(const real *d6, const Rot6d &r, const real *gaa, real *gd6) {
    // aa = xyz / ratio
    real gquat[4];
    real gratio = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        gquat[1 + a] = gaa[a] / r.ratio;
        gratio -= gaa[a] * r.quat[1 + a];
    }
    gratio /= r.ratio * r.ratio;
    // ratio: the series in angle, or sin(half) / angle; angle = 2 half
    real gangle, ghalf = 0.0;
    if (r.small) {
        gangle = -gratio * r.angle / 24.0;
    } else {
        ghalf = gratio * cos(r.half) / r.angle;
        gangle = -gratio * sin(r.half) / (r.angle * r.angle);
    }
    ghalf += 2.0 * gangle;
    // half = atan2(norms, w); norms = ||xyz|| (no gradient at exactly 0)
    const real hyp2 = r.norms * r.norms + r.quat[0] * r.quat[0];
    const real gnorms = ghalf * r.quat[0] / hyp2;
    gquat[0] = -ghalf * r.norms / hyp2;
    const real along = r.norms == 0.0 ? 0.0 : gnorms / r.norms;
#pragma unroll
    for (int a = 0; a < 3; ++a) gquat[1 + a] += along * r.quat[1 + a];
    // the flip, then quat = cand / denom with denom = 2 max(q_abs, 0.1)
    real gcand[4], gdenom = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const real g = r.flip ? -gquat[i] : gquat[i];
        gcand[i] = g / r.denom;
        gdenom -= g * r.cand[i];
    }
    gdenom /= r.denom * r.denom;
    real gq_abs = r.above ? 2.0 * gdenom : 0.0;
    // the picked row of cand: q_abs^2 on the diagonal, sums and differences of m elsewhere
    real gm[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    gq_abs += 2.0 * r.q_abs * gcand[r.pick];
    switch (r.pick) {
        case 0:
            gm[7] += gcand[1], gm[5] -= gcand[1], gm[2] += gcand[2], gm[6] -= gcand[2], gm[3] += gcand[3], gm[1] -= gcand[3];
            break;
        case 1:
            gm[7] += gcand[0], gm[5] -= gcand[0], gm[3] += gcand[2], gm[1] += gcand[2], gm[2] += gcand[3], gm[6] += gcand[3];
            break;
        case 2:
            gm[2] += gcand[0], gm[6] -= gcand[0], gm[3] += gcand[1], gm[1] += gcand[1], gm[5] += gcand[3], gm[7] += gcand[3];
            break;
        default:
            gm[3] += gcand[0], gm[1] -= gcand[0], gm[6] += gcand[1], gm[2] += gcand[1], gm[7] += gcand[2], gm[5] += gcand[2];
            break;
    }
    // q_abs = sqrt(q2) where q2 > 0 (zero derivative elsewhere); q2 = 1 +- m00 +- m11 +- m22
    const real gq2 = r.positive ? gq_abs / (2.0 * r.q_abs) : 0.0;
    gm[0] += (r.pick == 0 || r.pick == 1) ? gq2 : -gq2;
    gm[4] += (r.pick == 0 || r.pick == 2) ? gq2 : -gq2;
    gm[8] += (r.pick == 0 || r.pick == 3) ? gq2 : -gq2;
    // m = rows b1, b2, b1 x b2
    real gb1[3], gb2[3], t[3];
    cross3(r.b2.v, gm + 6, gb1);
    cross3(gm + 6, r.b1.v, gb2);
#pragma unroll
    for (int a = 0; a < 3; ++a) gb1[a] += gm[a], gb2[a] += gm[3 + a];
    // b2 = normalize(u), u = a2 - dot b1, dot = b1 . a2
    real gu[3] = {0.0, 0.0, 0.0};
    normalize3_backward(r.u, r.b2, gb2, gu);
    const real gdot = -dot3(gu, r.b1.v);
    const real *a2 = d6 + 3;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        gd6[3 + a] = gu[a] + gdot * r.b1.v[a];
        gb1[a] += gdot * a2[a] - r.dot * gu[a];
        t[a] = 0.0;
    }
    normalize3_backward(d6, r.b1, gb1, t);
#pragma unroll
    for (int a = 0; a < 3; ++a) gd6[a] = t[a];
}

// losses.batch_rodrigues: R = I + sin K + (1 - cos) K K with K the cross matrix of k = r / angle, angle = ||r + 1e-8||.
// 1 - cos is taken as 2 sin^2(angle / 2): the same function without the cancellation (as csrc/lbs_backward.hip).
struct Rodrigues {
    real e[3], angle, k[3], sn, cs, c1, R[9];
};
__device__ __forceinline__ Rodrigues rodrigues(const real *rv) {
    Rodrigues o;
#pragma unroll
    for (int a = 0; a < 3; ++a) o.e[a] = rv[a] + kRodriguesEps;
    o.angle = sqrt(dot3(o.e, o.e));
#pragma unroll
    for (int a = 0; a < 3; ++a) o.k[a] = rv[a] / o.angle;
    o.sn = sin(o.angle);
    o.cs = cos(o.angle);
    const real sh = sin(0.5 * o.angle);
    o.c1 = 2.0 * sh * sh;
    const real x = o.k[0], y = o.k[1], z = o.k[2];
    // K K = k k^T - |k|^2 I (k is r / ||r + 1e-8||, not exactly a unit vector)
    o.R[0] = 1.0 - o.c1 * (y * y + z * z);
    o.R[4] = 1.0 - o.c1 * (x * x + z * z);
    o.R[8] = 1.0 - o.c1 * (x * x + y * y);
    o.R[1] = o.c1 * x * y - o.sn * z;
    o.R[3] = o.c1 * x * y + o.sn * z;
    o.R[2] = o.c1 * x * z + o.sn * y;
    o.R[6] = o.c1 * x * z - o.sn * y;
    o.R[5] = o.c1 * y * z - o.sn * x;
    o.R[7] = o.c1 * y * z + o.sn * x;
    return o;
}

// acos(clamp((tr(Rp^T Rg) - 1) / 2, -0.999, 0.999)); `inside` is the clamp's gate, -0.999 <= cos <= 0.999
struct Geodesic {
    Rodrigues p, g;
    real cos_raw, cos_used, value;
    bool inside;
};
__device__ __forceinline__ Geodesic geodesic_forward(const real *rp, const real *rg) {
    Geodesic o;
    o.p = rodrigues(rp);
    o.g = rodrigues(rg);
    real tr = 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) tr += o.p.R[i] * o.g.R[i];
    o.cos_raw = (tr - 1.0) / 2.0;
    o.inside = o.cos_raw >= -kCosClamp && o.cos_raw <= kCosClamp;
    o.cos_used = fmin(fmax(o.cos_raw, -kCosClamp), kCosClamp);
    o.value = acos(o.cos_used);
    return o;
}
// grad_rp [3] for the gradient gvalue of the angle; the target gets none
__device__ __forceinline__ void geodesic_backward(const real *rp, const Geodesic &o, real gvalue, real *grp) {
    const real gcos = o.inside ? -gvalue / sqrt(1.0 - o.cos_used * o.cos_used) : 0.0;
    real G[9];  // dL / dRp = gcos / 2 * Rg
#pragma unroll
    for (int i = 0; i < 9; ++i) G[i] = 0.5 * gcos * o.g.R[i];
    const Rodrigues &p = o.p;
    const real x = p.k[0], y = p.k[1], z = p.k[2];
    const real s13 = G[1] + G[3], s26 = G[2] + G[6], s57 = G[5] + G[7];
    const real gsn = x * (G[7] - G[5]) + y * (G[2] - G[6]) + z * (G[3] - G[1]);
    const real gc1 = -(y * y + z * z) * G[0] - (x * x + z * z) * G[4] - (x * x + y * y) * G[8] + x * y * s13 +
                      x * z * s26 + y * z * s57;
    real gk[3];
    gk[0] = p.sn * (G[7] - G[5]) + p.c1 * (y * s13 + z * s26 - 2.0 * x * (G[4] + G[8]));
    gk[1] = p.sn * (G[2] - G[6]) + p.c1 * (x * s13 + z * s57 - 2.0 * y * (G[0] + G[8]));
    gk[2] = p.sn * (G[3] - G[1]) + p.c1 * (x * s26 + y * s57 - 2.0 * z * (G[0] + G[4]));
    // k = r / angle: gr = gk / angle, gangle -= (gk . k) / angle;  angle = ||e||: gr += gangle e / angle
    const real gangle = gsn * p.cs + gc1 * p.sn - dot3(gk, p.k) / p.angle;
#pragma unroll
    for (int a = 0; a < 3; ++a) grp[a] = gk[a] / p.angle + gangle * (p.e[a] / p.angle);
}

}  // namespace smplx
}  // namespace amav
