// The flash-attention-2 backward that the audio transformer's self-attention, the stage-1 encoder's cross-attention
// (attention_backward.hip) and the point refiner's patch attention (cloud_backward.hip) share; DESIGN.md section 4.10.  Given the forward's inputs, its output
// O, the row log-sum-exp L and dO = dLoss/dO, the gradients
//     P = exp(scale Q K^T - L),  dP = dO V^T,  delta_i = rowsum(dO_i * O_i),  dS = P * (dP - delta)
//     dV = P^T dO,  dK = scale dS^T Q,  dQ = scale dS K
// never materialising the queries x keys matrices, in three passes:
//   delta_kernel   delta_i, one pass over O and dO;
//   dkdv_kernel    key-major: a wave owns 32 keys (K, V rows in registers) and sweeps every query tile, recomputing P
//                  and dS and accumulating dV^T and dK^T in its accumulator registers -- no cross-workgroup sum;
//   dq_kernel      query-major: a wave owns 32 queries (Q, dO rows in registers) and sweeps every key tile, recomputing
//                  S and dP, accumulating dQ^T.  Seven products instead of the five of a slab-summed dQ, but no slabs.
// Every sum runs in a fixed order with no atomics, so a call is deterministic bit for bit, and each (blockIdx.y,
// blockIdx.z) is computed alone.  The products run on v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 sums).
//
// Layouts (v_mfma_f32_32x32x2_f32): A lane (i, hh) holds A[i][hh], B lane (j, hh) holds B[hh][j], accumulator register t
// of lane (j, hh) holds C[r(t) + 4 hh][j] with r(t) = (t & 3) + 8 (t >> 2).  A product whose contraction index is the
// row index of an accumulator takes that accumulator as its B operand directly: k-step t pairs rows r(t) and r(t) + 4.
// The key-major kernel computes S = Q K^T (queries on the rows) for that reason, and the dQ kernel S^T = K Q^T.
//
// The kernels are templated on the head dim D (16, 32 or 64) and on a trivially copyable `Rows`, passed by value, that
// says where a row comes from and where a gradient goes -- the only things on which the callers differ:
//     long long delta_rows()                   (row, head) pairs of the delta pass
//     void delta_io(r, out, dout, delta)       the D floats of O and dO of pair r and where its delta is written
//     void bind(blockIdx.y, blockIdx.z)        narrows the struct to one workgroup's head and batch item / patch; the
//                                              calls below follow it and take a slot of that item
//     int keys(), queries()                    key slots and query slots (patch attention: query slot i is also key slot
//                                              i; cross-attention: two row sets of any two sizes)
//     const float *q_row(i), dout_row(i), k_row(j), v_row(j)     the D floats of the bound head
//     float lse_at(i), delta_at(i)
//     float *dk_row(j), dv_row(j), dq_row(i)   destinations
#pragma once
#include "amav_common.h"

namespace amav {
namespace attn_bwd {

constexpr int kBW = 128;        // keys (dkdv_kernel) or queries (dq_kernel) per workgroup: 4 waves x 32
constexpr int kBT = 32;         // rows of the swept operand per LDS tile
constexpr int kLd = kBT + 1;    // padded row of a transposed [d][row] tile
constexpr float kLog2e = 1.4426950408889634f;

__device__ __forceinline__ int acc_row(int t, int hh) { return (t & 3) + 8 * (t >> 2) + 4 * hh; }

// PER consecutive floats of a row: 16-byte loads where a thread's share is a multiple of 4 floats, 8-byte loads at
// D = 16, where its 2 floats are only 8-byte aligned
template <int PER>
__device__ __forceinline__ void load_floats(const float *__restrict__ p, float (&r)[PER]) {
    if constexpr (PER % 4 == 0) {
#pragma unroll
        for (int e = 0; e < PER; e += 4) {
            const float4 t = *reinterpret_cast<const float4 *>(p + e);
            r[e] = t.x, r[e + 1] = t.y, r[e + 2] = t.z, r[e + 3] = t.w;
        }
    } else {
#pragma unroll
        for (int e = 0; e < PER; e += 2) {
            const float2 t = *reinterpret_cast<const float2 *>(p + e);
            r[e] = t.x, r[e + 1] = t.y;
        }
    }
}

// D / 4 threads per (row, head) pair, 4 consecutive d each
template <int D, class Rows>
__global__ __launch_bounds__(256) void delta_kernel(Rows rows) {
    constexpr int G = D / 4;
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long r = gid / G;
    const int d4 = (int)(gid % G);
    const bool live = r < rows.delta_rows();
    float acc = 0.f;
    float *dst = nullptr;
    if (live) {
        const float *op, *gp;
        rows.delta_io(r, op, gp, dst);
        const float4 o = *reinterpret_cast<const float4 *>(op + 4 * d4);
        const float4 g = *reinterpret_cast<const float4 *>(gp + 4 * d4);
        acc = (o.x * g.x + o.y * g.y) + (o.z * g.z + o.w * g.w);
    }
    // written out, not group_sum<G> (wave_ops.h): with the call the compiler fuses one of the products above into an
    // fma, which changes the low bits of delta and with them of every gradient
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o, G);
    if (live && d4 == 0) *dst = acc;
}

// grid (key slot blocks of 128, blockIdx.y, blockIdx.z), 256 threads.  Wave w owns key slots blockIdx.x * 128 + 32 w +
// (lane & 31) and sweeps every query slot.
template <int D, class Rows>
__global__ __launch_bounds__(256) void dkdv_kernel(Rows rows, float scale) {
    constexpr int DV = D < 32 ? 32 : D, NB = DV / 32, PER = D / 8;
    __shared__ float Qt[DV * kLd];  // [d][query] of the current query tile (rows D.. stay zero)
    __shared__ float Gt[DV * kLd];  // [d][query] of dO
    __shared__ float Ls[kBT], Ds[kBT];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int c = lane & 31, hh = lane >> 5;
    rows.bind(blockIdx.y, blockIdx.z);
    const int nk = rows.keys(), nq = rows.queries();
    if ((int)blockIdx.x * kBW >= nk) return;  // uniform over the workgroup
    const int key = blockIdx.x * kBW + wave * 32 + c;
    const float sl2 = scale * kLog2e;

    // B operands of S = Q K^T (K pre-scaled to the log2 domain) and dP = dO V^T: lane (key, hh) holds row[2 s + hh].
    // A lane past the last key works on the last key's row; its result is dropped
    const int kc = min(key, nk - 1);
    float Kr[D / 2], Vr[D / 2];
    {
        const float *kp = rows.k_row(kc), *vp = rows.v_row(kc);
#pragma unroll
        for (int s = 0; s < D / 2; ++s) {
            const float2 kt = *reinterpret_cast<const float2 *>(kp + 2 * s);
            const float2 vt = *reinterpret_cast<const float2 *>(vp + 2 * s);
            Kr[s] = (hh ? kt.y : kt.x) * sl2;
            Vr[s] = hh ? vt.y : vt.x;
        }
    }
    if (D < 32) {
        for (int t = tid; t < (DV - D) * kLd; t += 256) Qt[D * kLd + t] = 0.f, Gt[D * kLd + t] = 0.f;
    }
    // the destinations, looked up before the sweep: looked up after it, the D = 64 patch kernel gets 32 fewer AGPRs and
    // copies 32 values per tile through them (4 % slower)
    float *const krow = rows.dk_row(kc), *const vrow = rows.dv_row(kc);
    f32x16 dV[NB], dK[NB];  // dV^T, dK^T: rows d (32 a ..), column = this lane's key
#pragma unroll
    for (int a = 0; a < NB; ++a)
#pragma unroll
        for (int t = 0; t < 16; ++t) dV[a][t] = 0.f, dK[a][t] = 0.f;

    // staging map: thread -> query tid / 8 of the tile, PER consecutive d at (tid % 8) * PER.  Queries past the end are
    // staged as zeros with L = delta = 0: their P is 1 and their dS 0, and both meet a zero dO / Q row, so they add
    // exact zeros.
    const int sq = tid >> 3, sd = (tid & 7) * PER;
    const int ntiles = (nq + kBT - 1) / kBT;
    for (int qt = 0; qt < ntiles; ++qt) {
        const int qi = qt * kBT + sq;
        float av[PER], gv[PER];
#pragma unroll
        for (int e = 0; e < PER; ++e) av[e] = 0.f, gv[e] = 0.f;
        if (qi < nq) {
            load_floats(rows.q_row(qi) + sd, av);
            load_floats(rows.dout_row(qi) + sd, gv);
        }
#pragma unroll
        for (int e = 0; e < PER; ++e) Qt[(sd + e) * kLd + sq] = av[e], Gt[(sd + e) * kLd + sq] = gv[e];
        if (tid < kBT) {
            const int qq = qt * kBT + tid;
            Ls[tid] = qq < nq ? rows.lse_at(qq) * kLog2e : 0.f;
            Ds[tid] = qq < nq ? rows.delta_at(qq) : 0.f;
        }
        __syncthreads();

        f32x16 Sa, dP;  // rows = queries r(t) + 4 hh of the tile, column = this lane's key
#pragma unroll
        for (int t = 0; t < 16; ++t) Sa[t] = 0.f, dP[t] = 0.f;
#pragma unroll
        for (int s = 0; s < D / 2; ++s) {
            Sa = __builtin_amdgcn_mfma_f32_32x32x2f32(Qt[(2 * s + hh) * kLd + c], Kr[s], Sa, 0, 0, 0);
            dP = __builtin_amdgcn_mfma_f32_32x32x2f32(Gt[(2 * s + hh) * kLd + c], Vr[s], dP, 0, 0, 0);
        }
        f32x16 P, dS;
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const int qq = acc_row(t, hh);
            P[t] = exp2f(Sa[t] - Ls[qq]);
            dS[t] = P[t] * (dP[t] - Ds[qq]);
        }
        // dV^T += dO^T P, dK^T += Q^T dS: k-step t contracts over queries r(t), r(t) + 4
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const int qq = acc_row(t, hh);
#pragma unroll
            for (int a = 0; a < NB; ++a)
                dV[a] = __builtin_amdgcn_mfma_f32_32x32x2f32(Gt[(c + 32 * a) * kLd + qq], P[t], dV[a], 0, 0, 0);
#pragma unroll
            for (int a = 0; a < NB; ++a)
                dK[a] = __builtin_amdgcn_mfma_f32_32x32x2f32(Qt[(c + 32 * a) * kLd + qq], dS[t], dK[a], 0, 0, 0);
        }
        __syncthreads();  // every wave is done with this tile before it is overwritten
    }

    if (key < nk) {
#pragma unroll
        for (int g = 0; g < 4; ++g)  // registers 4g..4g+3 are 4 consecutive d: 32 a + 8 g + 4 hh + (0..3)
#pragma unroll
            for (int a = 0; a < NB; ++a) {
                const int d = 32 * a + 8 * g + 4 * hh;
                if (d < D) {
                    *reinterpret_cast<float4 *>(vrow + d) =
                        make_float4(dV[a][4 * g], dV[a][4 * g + 1], dV[a][4 * g + 2], dV[a][4 * g + 3]);
                    *reinterpret_cast<float4 *>(krow + d) = make_float4(dK[a][4 * g] * scale, dK[a][4 * g + 1] * scale,
                                                                        dK[a][4 * g + 2] * scale, dK[a][4 * g + 3] * scale);
                }
            }
    }
}

// grid (query slot blocks of 128, blockIdx.y, blockIdx.z), 256 threads.  Wave w owns query slots blockIdx.x * 128 +
// 32 w + (lane & 31) and sweeps every key slot.
template <int D, class Rows>
__global__ __launch_bounds__(256) void dq_kernel(Rows rows, float scale) {
    constexpr int DV = D < 32 ? 32 : D, NB = DV / 32, PER = D / 8;
    __shared__ float Kt[DV * kLd];  // [d][key] of the current key tile (rows D.. stay zero)
    __shared__ float Vt[D * kLd];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int c = lane & 31, hh = lane >> 5;
    rows.bind(blockIdx.y, blockIdx.z);
    const int nk = rows.keys(), nq = rows.queries();
    if ((int)blockIdx.x * kBW >= nq) return;  // uniform over the workgroup
    const int query = blockIdx.x * kBW + wave * 32 + c;
    const int qc = min(query, nq - 1);  // a lane past the last query works on the last query's row; its result is dropped

    // B operands of S^T = K Q^T (Q pre-scaled to the log2 domain) and dP^T = V dO^T
    float Qr[D / 2], Gr[D / 2];
    {
        const float *qp = rows.q_row(qc), *gp = rows.dout_row(qc);
        const float sl2 = scale * kLog2e;
#pragma unroll
        for (int s = 0; s < D / 2; ++s) {
            const float2 qt = *reinterpret_cast<const float2 *>(qp + 2 * s);
            const float2 gt = *reinterpret_cast<const float2 *>(gp + 2 * s);
            Qr[s] = (hh ? qt.y : qt.x) * sl2;
            Gr[s] = hh ? gt.y : gt.x;
        }
    }
    // a lane past the last query is computed and dropped: L = 1e30 makes its probabilities zero
    const float Lq = query < nq ? rows.lse_at(qc) * kLog2e : 1e30f, Dq = rows.delta_at(qc);
    if (D < 32) {
        for (int t = tid; t < (DV - D) * kLd; t += 256) Kt[D * kLd + t] = 0.f;
    }
    f32x16 dQ[NB];  // dQ^T: rows d, column = this lane's query
#pragma unroll
    for (int a = 0; a < NB; ++a)
#pragma unroll
        for (int t = 0; t < 16; ++t) dQ[a][t] = 0.f;

    const int sk = tid >> 3, sd = (tid & 7) * PER;
    const int ntiles = (nk + kBT - 1) / kBT;
    for (int kt = 0; kt < ntiles; ++kt) {
        const int kj = kt * kBT + sk;
        float av[PER], bv[PER];
#pragma unroll
        for (int e = 0; e < PER; ++e) av[e] = 0.f, bv[e] = 0.f;
        if (kj < nk) {
            load_floats(rows.k_row(kj) + sd, av);
            load_floats(rows.v_row(kj) + sd, bv);
        }
#pragma unroll
        for (int e = 0; e < PER; ++e) Kt[(sd + e) * kLd + sk] = av[e], Vt[(sd + e) * kLd + sk] = bv[e];
        __syncthreads();

        f32x16 St, dPt;  // rows = keys r(t) + 4 hh of the tile, column = this lane's query
#pragma unroll
        for (int t = 0; t < 16; ++t) St[t] = 0.f, dPt[t] = 0.f;
#pragma unroll
        for (int s = 0; s < D / 2; ++s) {
            St = __builtin_amdgcn_mfma_f32_32x32x2f32(Kt[(2 * s + hh) * kLd + c], Qr[s], St, 0, 0, 0);
            dPt = __builtin_amdgcn_mfma_f32_32x32x2f32(Vt[(2 * s + hh) * kLd + c], Gr[s], dPt, 0, 0, 0);
        }
        f32x16 dS;
        const bool tail = (kt + 1) * kBT > nk;
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const float p = tail && kt * kBT + acc_row(t, hh) >= nk ? 0.f : exp2f(St[t] - Lq);  // keys past the end: P = 0
            dS[t] = p * (dPt[t] - Dq);
        }
        // dQ^T += K^T dS^T: k-step t contracts over keys r(t), r(t) + 4
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const int kk = acc_row(t, hh);
#pragma unroll
            for (int a = 0; a < NB; ++a)
                dQ[a] = __builtin_amdgcn_mfma_f32_32x32x2f32(Kt[(c + 32 * a) * kLd + kk], dS[t], dQ[a], 0, 0, 0);
        }
        __syncthreads();
    }

    if (query < nq) {
        float *row = rows.dq_row(query);
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int a = 0; a < NB; ++a) {
                const int d = 32 * a + 8 * g + 4 * hh;
                if (d < D)
                    *reinterpret_cast<float4 *>(row + d) = make_float4(dQ[a][4 * g] * scale, dQ[a][4 * g + 1] * scale,
                                                                       dQ[a][4 * g + 2] * scale, dQ[a][4 * g + 3] * scale);
            }
    }
}

}  // namespace attn_bwd
}  // namespace amav
