// SMPL-X forward + LBS, backward, for gfx950: dL/d vertices [F,V,3] -> dL/d full_pose [F,J*3], dL/d coeffs [F,NC].
//
// Forward (lbs.hip, oracle.lbs.lbs): feat = [c; vec(R_j - I)] (KB rows), v_posed = v_template + blend^T feat,
// J = j_template + j_dirs c, G_j = G_parent [R_j | J_j - J_parent], A_j = G_j with the rest pose removed
// (t_A = t_j - M_j J_j), T_v = sum_j w_vj A_j, out_v = T_v [v_posed; 1].  Backward, five launches:
//
//   joint_chain_kernel<false>  (lbs.hip, as it is) featT and A into scratch.
//   vposed_kernel      skin_mfma_kernel's decomposition and k-loop (block = 128 frames x one 32-vertex tile, the tile's
//                      blend slab streamed once through LDS on v_mfma_f32_32x32x2_f32): v_posed is recomputed (the
//                      forward never stores it) and written out; the epilogue forms T_v as the forward does and
//                      dv_posed = M_v^T dOut_v, stored [Fpad][tile][3][32] -- the k order of the blend slab's rows.
//   dfeat_kernel       dfeat = dv_posed [Fpad, 96 ntiles] x blend [96 ntiles, KB] on the same MFMA, split over S =
//                      ceil(ntiles / 8) groups of 8 tiles (S depends on V only): wave = 32 frames x 32 table rows x one
//                      group, both operands K-contiguous (float4 loads, no LDS), partial sums [S][Fpad][KP].
//   joint_grad_kernel  one wave per (frame, joint): dA_j = sum_v w_vj dOut_v [v_posed_v; 1]^T over the joint's vertices
//                      (transposed skin table, ascending), a fixed butterfly at the end.
//   chain_backward_kernel  one 64-lane block per frame (joint_chain_kernel's shape): sums the S partials in order,
//                      recomputes Rodrigues / joints / chain, runs the chain backward level by level from the deepest
//                      level (a parent sums its children in ascending joint order), Rodrigues backward, and
//                      dc = dfeat[:NC] + j_dirs^T dJ.
//   gather_backward_kernel  amav_points_gather's transpose over the vertex-major table (one thread per (frame, vertex)).
//
// No float atomics, no hipMemsetAsync (featT's padding is cleared by zero_async, a kernel), no host synchronisation:
// every sum has an order fixed by V, J and the tables, and a
// frame's values never depend on another frame (MFMA rows are independent fma chains), so results are bitwise
// reproducible and independent of how the frames are split into calls.
#include <algorithm>
#include <cmath>

#include "lbs_common.h"
#include "wave_ops.h"

namespace amav {
namespace lbs {

constexpr int kTileGroup = 8;  // 32-vertex tiles per dfeat partial

static int frame_pad32(int F) { return (F + 31) / 32 * 32; }
static int rows_pad(int KB) { return (KB + 127) / 128 * 128; }  // partial row length: whole 128-row wave groups
static int tile_groups(int V) { return ((V + 31) / 32 + kTileGroup - 1) / kTileGroup; }

// grid and block decomposition of skin_mfma_kernel; featT has kMfmaKPad zero rows and zero columns past F
__global__ __launch_bounds__(64 * kMfmaWaves, 3) void vposed_kernel(Tables t, int F, int Fpad, int ntiles,
                                                                 const float *__restrict__ featT,
                                                                 const float *__restrict__ A,
                                                                 const float *__restrict__ grad_v,
                                                                 float *__restrict__ vposed, float *__restrict__ dvp) {
    __shared__ float4 Bs[2][kMfmaChunk4];
    const int ngroups = (Fpad / 32 + kMfmaWaves - 1) / kMfmaWaves;
    const int xcd = blockIdx.x & 7, bj = blockIdx.x >> 3;
    const int tile = (bj / ngroups) * 8 + xcd, fg = bj % ngroups;
    if (tile >= ntiles) return;  // block-uniform
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ftile = fg * kMfmaWaves + wave;
    const bool active = ftile * 32 < Fpad;
    const int f0 = active ? ftile * 32 : 0;
    const int c = lane & 31, hh = lane >> 5;
    const int v = tile * 32 + c;

    f32x16 X, Y, Z;
    {
        const int vl = min(v, t.V - 1);
        const float x = t.v_template[vl * 3], y = t.v_template[vl * 3 + 1], z = t.v_template[vl * 3 + 2];
#pragma unroll
        for (int r = 0; r < 16; ++r) X[r] = x, Y[r] = y, Z[r] = z;
    }
    const float4 *bt4 = reinterpret_cast<const float4 *>(t.blend + (size_t)tile * t.KB * 96);
    const int total4 = t.KB * 24;
    const int nchunks = (t.KB + kMfmaKC - 1) / kMfmaKC;
    const unsigned lane_a = (unsigned)(hh * Fpad + f0 + c);
    float4 breg[3];
    float a_cur[kMfmaKC / 2], a_nxt[kMfmaKC / 2];
    auto gload = [&](int ch) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int idx = ch * kMfmaChunk4 + (int)threadIdx.x + 256 * i;
            breg[i] = idx < total4 ? bt4[idx] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    auto aload = [&](float (&a)[kMfmaKC / 2], int ch) {
        const float *pa = featT + (size_t)(ch * kMfmaKC) * Fpad;
#pragma unroll
        for (int s = 0; s < kMfmaKC / 2; ++s) a[s] = pa[(size_t)(2 * s) * Fpad + lane_a];
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 3; ++i) Bs[buf][threadIdx.x + 256 * i] = breg[i];
    };
    gload(0);
    aload(a_cur, 0);
    stage(0);
    __syncthreads();
    for (int ch = 0; ch < nchunks; ++ch) {
        const int buf = ch & 1;
        const int nxt = min(ch + 1, nchunks - 1);
        gload(nxt);
        aload(a_nxt, nxt);
        __builtin_amdgcn_sched_barrier(0);
        if (active) {
            const float *bs = reinterpret_cast<const float *>(Bs[buf]) + hh * 96 + c;
            float q0 = bs[0], q1 = bs[32], q2 = bs[64];
#pragma unroll
            for (int s = 0; s < kMfmaKC / 2; ++s) {
                const float p0 = q0, p1 = q1, p2 = q2;
                if (s + 1 < kMfmaKC / 2) q0 = bs[(s + 1) * 192], q1 = bs[(s + 1) * 192 + 32], q2 = bs[(s + 1) * 192 + 64];
                X = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur[s], p0, X, 0, 0, 0);
                Y = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur[s], p1, Y, 0, 0, 0);
                Z = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur[s], p2, Z, 0, 0, 0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        stage(buf ^ 1);
#pragma unroll
        for (int s = 0; s < kMfmaKC / 2; ++s) a_cur[s] = a_nxt[s];
        __syncthreads();
    }
    if (!active) return;
    // dv_posed [Fpad][ntiles][3][32]: zero for padded frames and for the padded vertices of the last tile (their table
    // columns are zero, but 0 x an unwritten value could be NaN)
    const size_t Kd = (size_t)ntiles * 96;
    float *dv = dvp + (size_t)tile * 96 + c;
    if (v >= t.V) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float *d = dv + (size_t)(f0 + 8 * (r >> 2) + 4 * hh + (r & 3)) * Kd;
            d[0] = 0.f, d[32] = 0.f, d[64] = 0.f;
        }
        return;
    }
    int jidx[8];
    float jw[8];
    const int kw = t.KW;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        jidx[k] = k < kw ? t.skin_idx[(size_t)v * kw + k] : 0;
        jw[k] = k < kw ? t.skin_w[(size_t)v * kw + k] : 0.0f;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int f = f0 + 8 * (r >> 2) + 4 * hh + (r & 3);
        float *d = dv + (size_t)f * Kd;
        if (f >= F) {
            d[0] = 0.f, d[32] = 0.f, d[64] = 0.f;
            continue;
        }
        float Tm[12];
#pragma unroll
        for (int e = 0; e < 12; ++e) Tm[e] = 0.0f;
        const float *Af = A + (size_t)f * t.J * 12;
        auto add = [&](int ji, float w) {
            const float4 *a4 = reinterpret_cast<const float4 *>(Af + ji * 12);
            const float4 r0 = a4[0], r1 = a4[1], r2 = a4[2];
            Tm[0] += w * r0.x, Tm[1] += w * r0.y, Tm[2] += w * r0.z;
            Tm[4] += w * r1.x, Tm[5] += w * r1.y, Tm[6] += w * r1.z;
            Tm[8] += w * r2.x, Tm[9] += w * r2.y, Tm[10] += w * r2.z;
        };
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (k < kw) add(jidx[k], jw[k]);
        for (int k = 8; k < kw; ++k) add(t.skin_idx[(size_t)v * kw + k], t.skin_w[(size_t)v * kw + k]);
        const size_t o = ((size_t)f * t.V + v) * 3;
        vposed[o] = X[r], vposed[o + 1] = Y[r], vposed[o + 2] = Z[r];
        const float g0 = grad_v[o], g1 = grad_v[o + 1], g2 = grad_v[o + 2];
        d[0] = Tm[0] * g0 + Tm[4] * g1 + Tm[8] * g2;
        d[32] = Tm[1] * g0 + Tm[5] * g1 + Tm[9] * g2;
        d[64] = Tm[2] * g0 + Tm[6] * g1 + Tm[10] * g2;
    }
}

// grid: (Fpad / 32) x (KP / 128) x S blocks of 4 waves; wave w of block (fg, kg, s): frames fg*32.., table rows
// kg*128 + 32w.., tiles [8s, 8s + 8).  MFMA step: lane (i, hh) gives A[i][hh] = dvp[frame i][k-slot] and
// B[hh][i] = blend[row i][k-slot] for the same k-slot (8g + 4hh + e, e = 0..3 of one float4), so D[frame][row] sums
// over the tile's 96 (component, vertex) slots in a fixed order.
__global__ __launch_bounds__(256) void dfeat_kernel(Tables t, int Fpad, int ntiles, int S, int KP,
                                                    const float *__restrict__ dvp, float *__restrict__ part) {
    const int nfg = Fpad / 32, nkg = KP / 128;
    const int fg = blockIdx.x % nfg, kg = (blockIdx.x / nfg) % nkg, s = blockIdx.x / (nfg * nkg);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 31, hh = lane >> 5;
    const int f0 = fg * 32, k0 = kg * 128 + wave * 32;
    if (k0 >= t.KB || s >= S) return;  // wave-uniform
    const int tile0 = s * kTileGroup, tile1 = min(tile0 + kTileGroup, ntiles);
    const size_t Kd = (size_t)ntiles * 96;
    const int k = k0 + c;
    const bool krow = k < t.KB;
    const float *pa = dvp + (size_t)(f0 + c) * Kd + 4 * hh;
    const float *pb = t.blend + (size_t)min(k, t.KB - 1) * 96 + 4 * hh;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int tile = tile0; tile < tile1; ++tile) {
        const float4 *a4 = reinterpret_cast<const float4 *>(pa + (size_t)tile * 96);
        const float4 *b4 = reinterpret_cast<const float4 *>(pb + (size_t)tile * t.KB * 96);
#pragma unroll
        for (int g = 0; g < 12; ++g) {
            const float4 a = a4[2 * g];
            float4 b = b4[2 * g];
            if (!krow) b = make_float4(0.f, 0.f, 0.f, 0.f);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
        }
    }
    float *dst = part + ((size_t)s * Fpad + f0) * KP + k0 + c;
#pragma unroll
    for (int r = 0; r < 16; ++r) dst[(size_t)(8 * (r >> 2) + 4 * hh + (r & 3)) * KP] = acc[r];
}

// grid F * J waves: dA [F][J][12] (rows of the 3x4 gradient of A_j)
__global__ __launch_bounds__(64) void joint_grad_kernel(int V, int J, const int *__restrict__ off,
                                                        const int *__restrict__ verts, const float *__restrict__ wts,
                                                        const float *__restrict__ vposed,
                                                        const float *__restrict__ grad_v, float *__restrict__ dA) {
    const int f = blockIdx.x / J, j = blockIdx.x % J, lane = threadIdx.x;
    const float *vp = vposed + (size_t)f * V * 3, *gv = grad_v + (size_t)f * V * 3;
    float acc[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) acc[e] = 0.f;
    const int e1 = off[j + 1];
    for (int e = off[j] + lane; e < e1; e += 64) {
        const int v = verts[e];
        if ((unsigned)v >= (unsigned)V) continue;
        const float w = wts[e];
        const float x = vp[v * 3], y = vp[v * 3 + 1], z = vp[v * 3 + 2];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const float gw = w * gv[v * 3 + d];
            acc[d * 4] += gw * x, acc[d * 4 + 1] += gw * y, acc[d * 4 + 2] += gw * z, acc[d * 4 + 3] += gw;
        }
    }
#pragma unroll
    for (int e = 0; e < 12; ++e) acc[e] = wave_sum(acc[e]);
    if (lane == 0) {
        float *dst = dA + ((size_t)f * J + j) * 12;
#pragma unroll
        for (int e = 0; e < 12; ++e) dst[e] = acc[e];
    }
}

__global__ __launch_bounds__(64) void chain_backward_kernel(Tables t, int Fpad, int S, int KP, PoseSource src,
                                                            const float *__restrict__ part,
                                                            const float *__restrict__ dA,
                                                            float *__restrict__ grad_pose,
                                                            float *__restrict__ grad_coeffs) {
    __shared__ float coef[64];
    __shared__ float dfeat[kMaxFeatures];
    __shared__ float G[kMaxJoints][12];
    __shared__ float Jl[kMaxJoints][3];
    __shared__ float up[kMaxJoints][12];    // a joint's contribution to its parent: dM (9), dt (3)
    __shared__ float drel_s[kMaxJoints][3];
    __shared__ float dJ_s[kMaxJoints][3];
    __shared__ int depth_s[kMaxJoints];
    const int f = blockIdx.x, j = threadIdx.x;
    const int J = t.J, NC = t.NC, KB = t.KB;

    if (j < NC) {
        const float *base = src.cpart[0];
        long long st = src.cstride[0];
        int fj = 0;
        for (int q = 1; q < src.ncparts; ++q)
            if (j >= src.cfirst[q]) base = src.cpart[q], st = src.cstride[q], fj = src.cfirst[q];
        coef[j] = base[(size_t)f * st + (j - fj)];
    }
    for (int k = j; k < KB; k += 64) {  // the partials in group order
        float sum = 0.f;
        for (int q = 0; q < S; ++q) sum += part[((size_t)q * Fpad + f) * KP + k];
        dfeat[k] = sum;
    }
    __syncthreads();

    // forward recompute (joint_chain_kernel's arithmetic)
    float r[3] = {0, 0, 0}, e3[3] = {0, 0, 0}, kk[3] = {0, 0, 0}, angle = 1.f, sn = 0.f, cs = 1.f;
    float R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, Jp[3] = {0, 0, 0}, rel[3] = {0, 0, 0};
    int parent = -1, depth = 0;
    if (j < J) {
        const float *base = src.part[0];
        long long st = src.stride[0];
        int fj = 0;
        for (int q = 1; q < src.nparts; ++q)
            if (j >= src.first[q]) base = src.part[q], st = src.stride[q], fj = src.first[q];
        base += (size_t)f * st + (j - fj) * 3;
#pragma unroll
        for (int d = 0; d < 3; ++d) r[d] = base[d] + (src.mean ? src.mean[j * 3 + d] : 0.f);
#pragma unroll
        for (int d = 0; d < 3; ++d) e3[d] = r[d] + 1e-8f;
        angle = sqrtf(e3[0] * e3[0] + e3[1] * e3[1] + e3[2] * e3[2]);
#pragma unroll
        for (int d = 0; d < 3; ++d) kk[d] = r[d] / angle;
        sn = sinf(angle), cs = cosf(angle);
        const float c1 = 1.0f - cs, kx = kk[0], ky = kk[1], kz = kk[2];
        R[0] = 1.0f + c1 * (-kz * kz - ky * ky);
        R[1] = -sn * kz + c1 * (kx * ky);
        R[2] = sn * ky + c1 * (kx * kz);
        R[3] = sn * kz + c1 * (kx * ky);
        R[4] = 1.0f + c1 * (-kz * kz - kx * kx);
        R[5] = -sn * kx + c1 * (ky * kz);
        R[6] = -sn * ky + c1 * (kx * kz);
        R[7] = sn * kx + c1 * (ky * kz);
        R[8] = 1.0f + c1 * (-ky * ky - kx * kx);
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            float acc = t.j_template[j * 3 + d];
            const float *row = t.j_dirs + (size_t)(j * 3 + d) * NC;
            for (int l = 0; l < NC; ++l) acc += row[l] * coef[l];
            Jp[d] = acc;
            Jl[j][d] = acc;
        }
        parent = t.parents[j];
        for (int a = parent; a >= 0; a = t.parents[a]) ++depth;
        depth_s[j] = depth;
    }
    __syncthreads();
    int max_depth = 0;
    for (int q = 0; q < J; ++q) max_depth = max(max_depth, depth_s[q]);
#pragma unroll
    for (int d = 0; d < 3; ++d) rel[d] = Jp[d] - (j < J && parent >= 0 ? Jl[parent][d] : 0.f);
    for (int lv = 0; lv <= max_depth; ++lv) {
        if (j < J && depth == lv) {
            float Gj[12];
            if (parent < 0) {
#pragma unroll
                for (int a = 0; a < 3; ++a)
                    Gj[a * 4] = R[a * 3], Gj[a * 4 + 1] = R[a * 3 + 1], Gj[a * 4 + 2] = R[a * 3 + 2], Gj[a * 4 + 3] = rel[a];
            } else {
                const float *P = G[parent];
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const float p0 = P[a * 4], p1 = P[a * 4 + 1], p2 = P[a * 4 + 2], p3 = P[a * 4 + 3];
                    Gj[a * 4 + 0] = p0 * R[0] + p1 * R[3] + p2 * R[6];
                    Gj[a * 4 + 1] = p0 * R[1] + p1 * R[4] + p2 * R[7];
                    Gj[a * 4 + 2] = p0 * R[2] + p1 * R[5] + p2 * R[8];
                    Gj[a * 4 + 3] = p0 * rel[0] + p1 * rel[1] + p2 * rel[2] + p3;
                }
            }
#pragma unroll
            for (int e = 0; e < 12; ++e) G[j][e] = Gj[e];
        }
        __syncthreads();
    }

    // A_j = [M_j | t_j - M_j J_j]:  dM_j = dA_M - dA_t J_j^T,  dt_j = dA_t,  dJ_j = -M_j^T dA_t
    float dM[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, dt[3] = {0, 0, 0}, dJ[3] = {0, 0, 0};
    if (j < J) {
        const float *g = dA + ((size_t)f * J + j) * 12;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            dt[a] = g[a * 4 + 3];
#pragma unroll
            for (int b = 0; b < 3; ++b) dM[a * 3 + b] = g[a * 4 + b] - dt[a] * Jp[b];
        }
#pragma unroll
        for (int b = 0; b < 3; ++b) dJ[b] = -(G[j][b] * dt[0] + G[j][4 + b] * dt[1] + G[j][8 + b] * dt[2]);
    }
    // chain backward, deepest level first: G_j = G_p [R_j | rel_j]
    float dR[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, drel[3] = {0, 0, 0};
    for (int lv = max_depth; lv >= 0; --lv) {
        if (j < J && depth == lv) {
            for (int q = 0; q < J; ++q) {  // children, ascending
                if (t.parents[q] != j) continue;
#pragma unroll
                for (int e = 0; e < 9; ++e) dM[e] += up[q][e];
#pragma unroll
                for (int a = 0; a < 3; ++a) dt[a] += up[q][9 + a];
            }
            if (parent < 0) {
#pragma unroll
                for (int e = 0; e < 9; ++e) dR[e] = dM[e];
#pragma unroll
                for (int a = 0; a < 3; ++a) drel[a] = dt[a];
            } else {
                const float *P = G[parent];  // M_p rows at P[a * 4 + b]
#pragma unroll
                for (int a = 0; a < 3; ++a) {
#pragma unroll
                    for (int b = 0; b < 3; ++b) dR[a * 3 + b] = P[a] * dM[b] + P[4 + a] * dM[3 + b] + P[8 + a] * dM[6 + b];
                    drel[a] = P[a] * dt[0] + P[4 + a] * dt[1] + P[8 + a] * dt[2];
                }
#pragma unroll
                for (int a = 0; a < 3; ++a) {
#pragma unroll
                    for (int b = 0; b < 3; ++b)
                        up[j][a * 3 + b] = dM[a * 3] * R[b * 3] + dM[a * 3 + 1] * R[b * 3 + 1] + dM[a * 3 + 2] * R[b * 3 + 2] +
                                           dt[a] * rel[b];
                    up[j][9 + a] = dt[a];
                }
            }
#pragma unroll
            for (int a = 0; a < 3; ++a) drel_s[j][a] = drel[a];
        }
        __syncthreads();
    }
    if (j < J) {
        // rel_j = J_j - J_parent: dJ_j += drel_j - sum over children drel_child (ascending)
#pragma unroll
        for (int a = 0; a < 3; ++a) dJ[a] += drel[a];
        for (int q = 0; q < J; ++q) {
            if (t.parents[q] != j) continue;
#pragma unroll
            for (int a = 0; a < 3; ++a) dJ[a] -= drel_s[q][a];
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) dJ_s[j][a] = dJ[a];
        if (j >= 1) {
#pragma unroll
            for (int e = 0; e < 9; ++e) dR[e] += dfeat[NC + (j - 1) * 9 + e];
        }
        // Rodrigues backward: R = I + s K + c1 K K, k = r / angle, angle = ||r + 1e-8||.  c1 as 2 sin^2(angle / 2)
        // (no cancellation; the forward's 1 - cos is the same function)
        const float *Gd = dR;
        const float kx = kk[0], ky = kk[1], kz = kk[2];
        const float sh = sinf(0.5f * angle), c1 = 2.0f * sh * sh;
        const float s13 = Gd[1] + Gd[3], s26 = Gd[2] + Gd[6], s57 = Gd[5] + Gd[7];
        const float ds = kx * (Gd[7] - Gd[5]) + ky * (Gd[2] - Gd[6]) + kz * (Gd[3] - Gd[1]);
        const float dc1 = -(ky * ky + kz * kz) * Gd[0] - (kx * kx + kz * kz) * Gd[4] - (kx * kx + ky * ky) * Gd[8] +
                          kx * ky * s13 + kx * kz * s26 + ky * kz * s57;
        float dk[3];
        dk[0] = sn * (Gd[7] - Gd[5]) + c1 * (ky * s13 + kz * s26 - 2.0f * kx * (Gd[4] + Gd[8]));
        dk[1] = sn * (Gd[2] - Gd[6]) + c1 * (kx * s13 + kz * s57 - 2.0f * ky * (Gd[0] + Gd[8]));
        dk[2] = sn * (Gd[3] - Gd[1]) + c1 * (kx * s26 + ky * s57 - 2.0f * kz * (Gd[0] + Gd[4]));
        // k = r / angle: dr = dk / angle, dangle -= (dk . k) / angle;  angle = ||e||: dr += dangle e / angle
        const float dangle = ds * cs + dc1 * sn - (dk[0] * kx + dk[1] * ky + dk[2] * kz) / angle;
        float *gp = grad_pose + ((size_t)f * J + j) * 3;
#pragma unroll
        for (int d = 0; d < 3; ++d) gp[d] = dk[d] / angle + dangle * (e3[d] / angle);
    }
    __syncthreads();
    if (j < NC) {
        // J = j_template + j_dirs c: dc = dfeat[:NC] + j_dirs^T dJ (joints, then components, ascending)
        float acc = dfeat[j];
        for (int q = 0; q < J; ++q)
#pragma unroll
            for (int d = 0; d < 3; ++d) acc += t.j_dirs[(size_t)(q * 3 + d) * NC + j] * dJ_s[q][d];
        grad_coeffs[(size_t)f * NC + j] = acc;
    }
}

__global__ __launch_bounds__(256) void gather_backward_kernel(int F, int V, int N, const float *__restrict__ gp,
                                                              const int *__restrict__ off, const int *__restrict__ ent,
                                                              float *__restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)F * V) return;
    const int f = (int)(i / V), v = (int)(i % V);
    const float *g = gp + (size_t)f * N * 3;
    float x = 0.f, y = 0.f, z = 0.f;
    const int e1 = off[v + 1];
    for (int e = off[v]; e < e1; ++e) {
        const int n = ent[e];
        if ((unsigned)n >= (unsigned)N) continue;
        x += 0.25f * g[n * 3], y += 0.25f * g[n * 3 + 1], z += 0.25f * g[n * 3 + 2];
    }
    float *o = out + (size_t)i * 3;
    o[0] = x, o[1] = y, o[2] = z;
}

struct BackwardScratch {
    float *featT, *A, *vposed, *dvp, *part, *dA;
};

static size_t backward_ws(int F, const amav_body_tables *tb, void *base, BackwardScratch *p) {
    const int KB = tb->num_coeffs + (tb->num_joints - 1) * 9, Fpad = frame_pad32(F);
    const size_t ntiles = ((size_t)tb->num_verts + 31) / 32;
    Carver c(base);
    BackwardScratch s;
    s.featT = c.take<float>((size_t)(KB + kMfmaKPad) * Fpad);
    s.A = c.take<float>((size_t)Fpad * tb->num_joints * 12);
    s.vposed = c.take<float>((size_t)F * tb->num_verts * 3);
    s.dvp = c.take<float>((size_t)Fpad * ntiles * 96);
    s.part = c.take<float>((size_t)tile_groups(tb->num_verts) * Fpad * rows_pad(KB));
    s.dA = c.take<float>((size_t)F * tb->num_joints * 12);
    if (p) *p = s;
    return c.total();
}

}  // namespace lbs
}  // namespace amav

using namespace amav;
using namespace amav::lbs;

extern "C" size_t amav_lbs_backward_bytes(int F, const amav_body_tables *t) {
    if (F <= 0 || validate_tables(t, "amav_lbs_backward_bytes") != AMAV_OK) return 0;
    return backward_ws(F, t, nullptr, nullptr);
}

extern "C" int amav_lbs_backward(const amav_lbs_backward_args *a, void *stream_) {
    AMAV_REQUIRE(a != nullptr, "amav_lbs_backward: args is NULL");
    const int F = a->num_frames;
    AMAV_REQUIRE(F > 0, "amav_lbs_backward: F=%d", F);
    const amav_body_tables *tb = a->tables;
    if (int rc = validate_tables(tb, "amav_lbs_backward")) return rc;
    AMAV_REQUIRE(a->parts && a->grad_vertices && a->grad_full_pose && a->grad_coeffs && a->skin_offsets &&
                     a->skin_verts && a->skin_weights && a->scratch,
                 "amav_lbs_backward: NULL pointer");
    PoseSource src;
    if (int rc = pose_source(a->parts, tb, &src, "amav_lbs_backward")) return rc;
    AMAV_REQUIRE((reinterpret_cast<uintptr_t>(a->scratch) & 15) == 0, "amav_lbs_backward: scratch not 16-byte aligned");
    BackwardScratch s;
    const size_t need = backward_ws(F, tb, a->scratch, &s);
    if (a->scratch_bytes < need)
        return fail(AMAV_ERR_WORKSPACE, "amav_lbs_backward: scratch %zu < required %zu", a->scratch_bytes, need);
    const Tables t = make_tables(tb);
    const int Fpad = frame_pad32(F), ntiles = (t.V + 31) / 32, S = tile_groups(t.V), KP = rows_pad(t.KB);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    // featT's padded frame columns and the kMfmaKPad rows past the table must be zero (they feed the MFMA product)
    if (zero_async(s.featT, (size_t)(t.KB + kMfmaKPad) * Fpad * sizeof(float), stream) != hipSuccess)
        return fail(AMAV_ERR_LAUNCH, "amav_lbs_backward: padding clear failed");
    launch_joint_chain(t, F, Fpad, src, s.featT, s.A, stream);
    const int ngroups = (Fpad / 32 + kMfmaWaves - 1) / kMfmaWaves;
    const unsigned mgrid = (unsigned)(((ntiles + 7) / 8) * 8 * ngroups);
    vposed_kernel<<<mgrid, 64 * kMfmaWaves, 0, stream>>>(t, F, Fpad, ntiles, s.featT, s.A, a->grad_vertices, s.vposed,
                                                         s.dvp);
    dfeat_kernel<<<(unsigned)((Fpad / 32) * (KP / 128) * S), 256, 0, stream>>>(t, Fpad, ntiles, S, KP, s.dvp, s.part);
    joint_grad_kernel<<<(unsigned)((size_t)F * t.J), 64, 0, stream>>>(t.V, t.J, a->skin_offsets, a->skin_verts,
                                                                      a->skin_weights, s.vposed, a->grad_vertices, s.dA);
    chain_backward_kernel<<<F, 64, 0, stream>>>(t, Fpad, S, KP, src, s.part, s.dA, a->grad_full_pose, a->grad_coeffs);
    return check_launch("amav_lbs_backward");
}

extern "C" int amav_points_gather_backward(int F, int V, int N, const float *grad_points, const int32_t *csr_offsets,
                                           const int32_t *csr_entries, float *grad_vertices, void *stream) {
    AMAV_REQUIRE(F > 0 && V > 0 && N > 0, "amav_points_gather_backward: bad sizes F=%d V=%d N=%d", F, V, N);
    AMAV_REQUIRE(grad_points && grad_vertices, "amav_points_gather_backward: NULL pointer");
    AMAV_REQUIRE(csr_offsets && csr_entries, "amav_points_gather_backward: NULL gather table");
    AMAV_REQUIRE((reinterpret_cast<uintptr_t>(csr_offsets) & 3) == 0 && (reinterpret_cast<uintptr_t>(csr_entries) & 3) == 0,
                 "amav_points_gather_backward: gather table not 4-byte aligned");
    const long long items = (long long)F * V;
    gather_backward_kernel<<<(unsigned)((items + 255) / 256), 256, 0, static_cast<hipStream_t>(stream)>>>(
        F, V, N, grad_points, csr_offsets, csr_entries, grad_vertices);
    return check_launch("amav_points_gather_backward");
}
