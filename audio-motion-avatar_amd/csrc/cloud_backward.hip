// Backward of the point refiner's sparse / serialised operators (csrc/cloud.hip).
//
//   amav_subm_pair_sum_csr        the transposed ordered sum of the submanifold convolution: dfeat[j] = sum over the pairs
//                                 whose SOURCE row is j (CSR by source row, ascending pair index) of the per-pair
//                                 products g[dst(p)] W[tap(p)]^T, which amav_subm_pair_gemm computes with pair_dst as its
//                                 gather index and the per-tap transposed weights
//   amav_subm_pair_wgrad          dW[t] = sum over the pairs p of tap t of feat[src(p)]^T (x) g[dst(p)]: both operands
//                                 gathered into LDS, the reduction dimension is the tap's pairs, split over chunks of
//                                 pairs whose partial matrices a second pass adds in slice order
//   amav_patch_attention_backward flash-attention-2 form through `order` / `patch_desc`: delta = rowsum(dO * O), a key-major
//                                 pass for dK / dV and a query-major pass for dQ, probabilities recomputed from the row
//                                 log-sum-exp of amav_patch_attention_lse.  A row is a query of exactly one patch (dQ is
//                                 written once); it can be a key of two (its own and, as a borrowed slot, the cloud's last
//                                 incomplete patch): the borrowed part is staged and added after the own part by a fixed pass
//   amav_cluster_max_backward     gelu(max * scale + shift): the whole gradient to the first member, in segment order, that
//                                 attains the maximum; every row of dx written once
//   amav_cluster_sum              out[j] = sum of x[members[r]] over segment j in segment order: the backward of the
//                                 up[cluster] gather of amav_unpool_merge
// No atomics, every sum in a fixed order: a call is deterministic bit for bit.  Products on v_mfma_f32_32x32x2_f32 (exact
// fp32 products, fp32 sums).  MFMA layouts: csrc/attention_backward.hip.
#include <climits>
#include <cmath>

#include "amav_common.h"

namespace amav {
namespace cloud_bwd {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr float kLog2e = 1.4426950408889634f;
constexpr int kWgradChunk = 128;  // granularity of a split-K slice of amav_subm_pair_wgrad, in pairs

__device__ __forceinline__ int acc_row(int t, int hh) { return (t & 3) + 8 * (t >> 2) + 4 * hh; }

// ---- submanifold convolution ----------------------------------------------------------------------------------------
// out[i] (+)= sum over r in [src_start[i], src_start[i+1]) with pair_lo <= src_pairs[r] < pair_hi of
// products[src_pairs[r] - pair_lo]; one thread per (row, 4 channels).  src_pairs ascends inside a row, so a sweep of
// consecutive pair ranges with accumulate = 1 adds in the order of one call over all pairs.
__global__ __launch_bounds__(256) void pair_sum_csr_kernel(long long n, int c4n, const float4 *__restrict__ products,
                                                           long long pair_lo, long long pair_hi,
                                                           const int *__restrict__ src_start,
                                                           const int *__restrict__ src_pairs, int accumulate,
                                                           float4 *__restrict__ out) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= n * c4n) return;
    const long long i = gid / c4n;
    const int c = (int)(gid - i * c4n);
    float4 acc = accumulate ? out[gid] : make_float4(0.f, 0.f, 0.f, 0.f);
    const int beg = src_start[i], end = src_start[i + 1];
    for (int r = beg; r < end; ++r) {
        const long long p = src_pairs[r];
        if (p >= pair_lo && p < pair_hi) {
            const float4 y = products[(p - pair_lo) * c4n + c];
            acc.x += y.x, acc.y += y.y, acc.z += y.z, acc.w += y.w;
        }
    }
    out[gid] = acc;
}

// grid (slices, cin / TM, cout / TN); a slice is `chunk` consecutive pairs of one tap (slice_start [taps + 1] = prefix sum
// of ceil(pairs of tap / chunk)).  One wave per 32 x 32 block of the [TM, TN] tile; 32 pairs per LDS stage, pairs past the
// slice's end staged as zeros.  partial [slices, cin, cout].
template <int TM, int TN>
__global__ __launch_bounds__(64 * (TM / 32) * (TN / 32)) void pair_wgrad_kernel(
    const float *__restrict__ feat, const float *__restrict__ g, const int *__restrict__ pair_src,
    const int *__restrict__ pair_dst, const int *__restrict__ tap_start, const int *__restrict__ slice_start, int taps,
    int chunk, float *__restrict__ partial, int Cin, int Cout) {
    constexpr int WM = TM / 32, NTHREADS = 64 * WM * (TN / 32), KP = 32, LDF = TM + 4, LDG = TN + 4;
    __shared__ float Fs[KP * LDF];  // [pair][c_in]
    __shared__ float Gs[KP * LDG];  // [pair][c_out]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 31, hh = lane >> 5;
    const int wm = wave % WM, wn = wave / WM;
    int lo = 0, hi = taps;
    while (hi - lo > 1) {  // last tap with slice_start[tap] <= blockIdx.x
        const int mid = (lo + hi) >> 1;
        if (slice_start[mid] <= (int)blockIdx.x) lo = mid; else hi = mid;
    }
    const int tap = lo;
    const int p0 = tap_start[tap] + ((int)blockIdx.x - slice_start[tap]) * chunk;
    const int p_end = min(p0 + chunk, tap_start[tap + 1]);
    const int ci0 = blockIdx.y * TM, co0 = blockIdx.z * TN;

    f32x16 acc;
#pragma unroll
    for (int t = 0; t < 16; ++t) acc[t] = 0.f;
    for (int pb = p0; pb < p_end; pb += KP) {
        for (int t = tid; t < KP * (TM / 4); t += NTHREADS) {
            const int pr = t / (TM / 4), q = (t % (TM / 4)) * 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (pb + pr < p_end) v = *reinterpret_cast<const float4 *>(feat + (size_t)pair_src[pb + pr] * Cin + ci0 + q);
            *reinterpret_cast<float4 *>(&Fs[pr * LDF + q]) = v;
        }
        for (int t = tid; t < KP * (TN / 4); t += NTHREADS) {
            const int pr = t / (TN / 4), q = (t % (TN / 4)) * 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (pb + pr < p_end) v = *reinterpret_cast<const float4 *>(g + (size_t)pair_dst[pb + pr] * Cout + co0 + q);
            *reinterpret_cast<float4 *>(&Gs[pr * LDG + q]) = v;
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < KP / 2; ++s)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(Fs[(2 * s + hh) * LDF + wm * 32 + c],
                                                       Gs[(2 * s + hh) * LDG + wn * 32 + c], acc, 0, 0, 0);
        __syncthreads();
    }
    float *dst = partial + (size_t)blockIdx.x * Cin * Cout + (size_t)(ci0 + wm * 32) * Cout + co0 + wn * 32 + c;
#pragma unroll
    for (int t = 0; t < 16; ++t) dst[(size_t)acc_row(t, hh) * Cout] = acc[t];
}

// dW[tap] = sum of the tap's slices in slice order (zeros for a tap without pairs); one thread per 4 entries
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(int taps, long long mat4, const int *__restrict__ slice_start,
                                                           const float4 *__restrict__ partial, float4 *__restrict__ out) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= taps * mat4) return;
    const long long t = gid / mat4, e = gid - t * mat4;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int s = slice_start[t]; s < slice_start[t + 1]; ++s) {
        const float4 y = partial[(long long)s * mat4 + e];
        acc.x += y.x, acc.y += y.y, acc.z += y.z, acc.w += y.w;
    }
    out[gid] = acc;
}

// ---- patch attention ------------------------------------------------------------------------------------------------
// Slots, patch_desc and the borrowed tail: cloud.hip, patch_attention_kernel.  lse / delta are [n, heads] in point order.
constexpr int kBT = 32;        // rows of the swept operand per LDS tile
constexpr int kLd = kBT + 1;   // padded row of a transposed [d][row] tile

__device__ __forceinline__ long long slot_row(const long long *__restrict__ order, int first, int K, int own, int j) {
    j = min(j, K - 1);
    return order[first + j - (j >= own ? K : 0)];
}

// D / 4 threads per (row, head): out and dout are [n, heads * D] contiguous, so (row, head) number r starts at r * D
template <int D>
__global__ __launch_bounds__(256) void pa_delta_kernel(long long row_heads, const float *__restrict__ out,
                                                       const float *__restrict__ dout, float *__restrict__ delta) {
    constexpr int G = D / 4;
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long r = gid / G;
    const int d4 = (int)(gid % G);
    const bool live = r < row_heads;
    float acc = 0.f;
    if (live) {
        const float4 o = *reinterpret_cast<const float4 *>(out + r * D + 4 * d4);
        const float4 gg = *reinterpret_cast<const float4 *>(dout + r * D + 4 * d4);
        acc = (o.x * gg.x + o.y * gg.y) + (o.z * gg.z + o.w * gg.w);
    }
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o, G);
    if (live && d4 == 0) delta[r] = acc;
}

// grid (key slot blocks of 128, heads, patches).  Wave w owns key slots blockIdx.x * 128 + 32 w + (lane & 31) and sweeps
// the patch's own queries (a borrowed slot's query result is dropped by the forward, so it has no gradient).
template <int D>
__global__ __launch_bounds__(256) void pa_dkdv_kernel(const float *__restrict__ qkv, const long long *__restrict__ order,
                                                      const int4 *__restrict__ desc, const float *__restrict__ dout,
                                                      const float *__restrict__ lse, const float *__restrict__ delta,
                                                      float *__restrict__ dqkv, float *__restrict__ stage, int C, int heads,
                                                      float scale) {
    constexpr int DV = D < 32 ? 32 : D, NB = DV / 32, PER = D / 8;
    __shared__ float Qt[DV * kLd];  // [d][query] of the current query tile (rows D.. stay zero)
    __shared__ float Gt[DV * kLd];  // [d][query] of dO
    __shared__ float Ls[kBT], Ds[kBT];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 31, hh = lane >> 5;
    const int head = blockIdx.y;
    const int4 pd = desc[blockIdx.z];
    const int first = pd.x, K = pd.y, own = pd.z;
    if ((int)blockIdx.x * 128 >= K) return;  // uniform over the workgroup
    const int slot = blockIdx.x * 128 + wave * 32 + c;
    const long long krow = slot_row(order, first, K, own, slot);
    const long long rs = 3LL * C;
    const float sl2 = scale * kLog2e;

    float Kr[D / 2], Vr[D / 2];
    {
        const float *kp = qkv + krow * rs + C + head * D;
#pragma unroll
        for (int s = 0; s < D / 2; ++s) {
            const float2 kt = *reinterpret_cast<const float2 *>(kp + 2 * s);
            const float2 vt = *reinterpret_cast<const float2 *>(kp + C + 2 * s);
            Kr[s] = (hh ? kt.y : kt.x) * sl2;
            Vr[s] = hh ? vt.y : vt.x;
        }
    }
    if (D < 32) {
        for (int t = tid; t < (DV - D) * kLd; t += 256) Qt[D * kLd + t] = 0.f, Gt[D * kLd + t] = 0.f;
    }
    f32x16 dV[NB], dK[NB];  // dV^T, dK^T: rows d, column = this lane's key slot
#pragma unroll
    for (int a = 0; a < NB; ++a)
#pragma unroll
        for (int t = 0; t < 16; ++t) dV[a][t] = 0.f, dK[a][t] = 0.f;

    // staging: thread -> query tid / 8 of the tile, PER consecutive d at (tid % 8) * PER.  Queries past `own` are staged
    // as zeros with L = delta = 0: P = 1 and dS = 0 meet a zero dO / Q row and add exact zeros
    const int sq = tid >> 3, sd = (tid & 7) * PER;
    const int ntiles = (own + kBT - 1) / kBT;
    for (int qt = 0; qt < ntiles; ++qt) {
        const int qi = qt * kBT + sq;
        float av[PER], gv[PER];
#pragma unroll
        for (int e = 0; e < PER; ++e) av[e] = 0.f, gv[e] = 0.f;
        if (qi < own) {
            const long long r = slot_row(order, first, K, own, qi);
            const float *qp = qkv + r * rs + head * D + sd;
            const float *gp = dout + r * C + head * D + sd;
#pragma unroll
            for (int e = 0; e < PER; e += 2) {
                const float2 a = *reinterpret_cast<const float2 *>(qp + e);
                const float2 b = *reinterpret_cast<const float2 *>(gp + e);
                av[e] = a.x, av[e + 1] = a.y, gv[e] = b.x, gv[e + 1] = b.y;
            }
        }
#pragma unroll
        for (int e = 0; e < PER; ++e) Qt[(sd + e) * kLd + sq] = av[e], Gt[(sd + e) * kLd + sq] = gv[e];
        if (tid < kBT) {
            const int qq = qt * kBT + tid;
            float l = 0.f, d = 0.f;
            if (qq < own) {
                const long long r = slot_row(order, first, K, own, qq);
                l = lse[r * heads + head] * kLog2e, d = delta[r * heads + head];
            }
            Ls[tid] = l, Ds[tid] = d;
        }
        __syncthreads();

        f32x16 Sa, dP;  // rows = queries r(t) + 4 hh of the tile, column = this lane's key slot
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
            for (int a = 0; a < NB; ++a) {
                dV[a] = __builtin_amdgcn_mfma_f32_32x32x2f32(Gt[(c + 32 * a) * kLd + qq], P[t], dV[a], 0, 0, 0);
                dK[a] = __builtin_amdgcn_mfma_f32_32x32x2f32(Qt[(c + 32 * a) * kLd + qq], dS[t], dK[a], 0, 0, 0);
            }
        }
        __syncthreads();  // every wave is done with this tile before it is overwritten
    }

    if (slot < K) {  // an own slot writes the gradient row, a borrowed slot the staging row of the same point
        float *kdst = slot < own ? dqkv + krow * rs + C + head * D : stage + krow * 2LL * C + head * D;
        float *vdst = kdst + C;
#pragma unroll
        for (int a = 0; a < NB; ++a)
#pragma unroll
            for (int g = 0; g < 4; ++g) {  // registers 4g..4g+3 are 4 consecutive d: 32 a + 8 g + 4 hh + (0..3)
                const int d = 32 * a + 8 * g + 4 * hh;
                if (d < D) {
                    *reinterpret_cast<float4 *>(vdst + d) =
                        make_float4(dV[a][4 * g], dV[a][4 * g + 1], dV[a][4 * g + 2], dV[a][4 * g + 3]);
                    *reinterpret_cast<float4 *>(kdst + d) = make_float4(dK[a][4 * g] * scale, dK[a][4 * g + 1] * scale,
                                                                        dK[a][4 * g + 2] * scale, dK[a][4 * g + 3] * scale);
                }
            }
    }
}

// grid (query slot blocks of 128, heads, patches).  Wave w owns query slots blockIdx.x * 128 + 32 w + (lane & 31) and
// sweeps every key slot of the patch, borrowed ones included.
template <int D>
__global__ __launch_bounds__(256) void pa_dq_kernel(const float *__restrict__ qkv, const long long *__restrict__ order,
                                                    const int4 *__restrict__ desc, const float *__restrict__ dout,
                                                    const float *__restrict__ lse, const float *__restrict__ delta,
                                                    float *__restrict__ dqkv, int C, int heads, float scale) {
    constexpr int DV = D < 32 ? 32 : D, NB = DV / 32, PER = D / 8;
    __shared__ float Kt[DV * kLd];  // [d][key] of the current key tile (rows D.. stay zero)
    __shared__ float Vt[D * kLd];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 31, hh = lane >> 5;
    const int head = blockIdx.y;
    const int4 pd = desc[blockIdx.z];
    const int first = pd.x, K = pd.y, own = pd.z;
    if ((int)blockIdx.x * 128 >= K) return;
    const int slot = blockIdx.x * 128 + wave * 32 + c;
    const long long qrow = slot_row(order, first, K, own, slot);
    const long long rs = 3LL * C;

    float Qr[D / 2], Gr[D / 2];
    {
        const float *qp = qkv + qrow * rs + head * D;
        const float *gp = dout + qrow * C + head * D;
        const float sl2 = scale * kLog2e;
#pragma unroll
        for (int s = 0; s < D / 2; ++s) {
            const float2 qt = *reinterpret_cast<const float2 *>(qp + 2 * s);
            const float2 gt = *reinterpret_cast<const float2 *>(gp + 2 * s);
            Qr[s] = (hh ? qt.y : qt.x) * sl2;
            Gr[s] = hh ? gt.y : gt.x;
        }
    }
    // a slot that is not an own query is computed and dropped: L = 1e30 makes its probabilities zero
    const float Lq = slot < own ? lse[qrow * heads + head] * kLog2e : 1e30f, Dq = delta[qrow * heads + head];
    if (D < 32) {
        for (int t = tid; t < (DV - D) * kLd; t += 256) Kt[D * kLd + t] = 0.f;
    }
    f32x16 dQ[NB];  // dQ^T: rows d, column = this lane's query slot
#pragma unroll
    for (int a = 0; a < NB; ++a)
#pragma unroll
        for (int t = 0; t < 16; ++t) dQ[a][t] = 0.f;

    const int sk = tid >> 3, sd = (tid & 7) * PER;
    const int ntiles = (K + kBT - 1) / kBT;
    for (int kt = 0; kt < ntiles; ++kt) {
        const int kj = kt * kBT + sk;
        float av[PER], bv[PER];
#pragma unroll
        for (int e = 0; e < PER; ++e) av[e] = 0.f, bv[e] = 0.f;
        if (kj < K) {
            const float *kp = qkv + slot_row(order, first, K, own, kj) * rs + C + head * D + sd;
#pragma unroll
            for (int e = 0; e < PER; e += 2) {
                const float2 a = *reinterpret_cast<const float2 *>(kp + e);
                const float2 b = *reinterpret_cast<const float2 *>(kp + C + e);
                av[e] = a.x, av[e + 1] = a.y, bv[e] = b.x, bv[e + 1] = b.y;
            }
        }
#pragma unroll
        for (int e = 0; e < PER; ++e) Kt[(sd + e) * kLd + sk] = av[e], Vt[(sd + e) * kLd + sk] = bv[e];
        __syncthreads();

        f32x16 St, dPt;  // rows = keys r(t) + 4 hh of the tile, column = this lane's query slot
#pragma unroll
        for (int t = 0; t < 16; ++t) St[t] = 0.f, dPt[t] = 0.f;
#pragma unroll
        for (int s = 0; s < D / 2; ++s) {
            St = __builtin_amdgcn_mfma_f32_32x32x2f32(Kt[(2 * s + hh) * kLd + c], Qr[s], St, 0, 0, 0);
            dPt = __builtin_amdgcn_mfma_f32_32x32x2f32(Vt[(2 * s + hh) * kLd + c], Gr[s], dPt, 0, 0, 0);
        }
        f32x16 dS;
        const bool tail = (kt + 1) * kBT > K;
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const float p = tail && kt * kBT + acc_row(t, hh) >= K ? 0.f : exp2f(St[t] - Lq);  // slots past K: P = 0
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

    if (slot < own) {
        float *row = dqkv + qrow * rs + head * D;
#pragma unroll
        for (int a = 0; a < NB; ++a)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int d = 32 * a + 8 * g + 4 * hh;
                if (d < D)
                    *reinterpret_cast<float4 *>(row + d) = make_float4(dQ[a][4 * g] * scale, dQ[a][4 * g + 1] * scale,
                                                                       dQ[a][4 * g + 2] * scale, dQ[a][4 * g + 3] * scale);
            }
    }
}

// dK | dV of every borrowed slot: own part (already in dqkv) + borrowed part (stage), in that order.  One thread per
// (patch, slot, 4 floats of the 2 C); a point is borrowed by at most one patch, so no two threads meet.
__global__ __launch_bounds__(256) void pa_borrow_add_kernel(long long threads, int max_patch, int q2c,
                                                            const long long *__restrict__ order,
                                                            const int4 *__restrict__ desc, const float4 *__restrict__ stage,
                                                            float *__restrict__ dqkv, int C) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= threads) return;
    const int e = (int)(gid % q2c);
    const int j = (int)((gid / q2c) % max_patch);
    const int4 pd = desc[gid / ((long long)q2c * max_patch)];
    if (j < pd.z || j >= pd.y) return;
    const long long row = order[pd.x + j - pd.y];
    const float4 s = stage[row * q2c + e];
    float4 *d = reinterpret_cast<float4 *>(dqkv + row * 3LL * C + C) + e;
    const float4 o = *d;
    *d = make_float4(o.x + s.x, o.y + s.y, o.z + s.z, o.w + s.w);
}

// ---- segment kernels --------------------------------------------------------------------------------------------------
__device__ __forceinline__ float gelu_grad(float z) {
    return 0.5f * (1.0f + erff(z * 0.70710678118654752440f)) + z * 0.39894228040143267794f * expf(-0.5f * z * z);
}

// one wave per cluster, as cluster_max_kernel: recompute the maximum and the first member (in segment order) that attains
// it, dz = dout * gelu'(max * scale + shift); dx = dz * scale on that member's row and zero on the others
__global__ __launch_bounds__(256) void cluster_max_backward_kernel(long long clusters, int C4, const float4 *__restrict__ x,
                                                                   const long long *__restrict__ members,
                                                                   const long long *__restrict__ seg,
                                                                   const float4 *__restrict__ scale,
                                                                   const float4 *__restrict__ shift,
                                                                   const float4 *__restrict__ dout, float4 *__restrict__ dx,
                                                                   float4 *__restrict__ dz, float4 *__restrict__ xmax) {
    const long long j = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= clusters) return;
    const int lane = threadIdx.x & 63;
    const long long beg = seg[j], end = seg[j + 1];
    for (int c = lane; c < C4; c += 64) {
        float4 m = x[members[beg] * C4 + c];
        int ax = 0, ay = 0, az = 0, aw = 0;
        for (long long r = beg + 1; r < end; ++r) {
            const float4 v = x[members[r] * C4 + c];
            const int k = (int)(r - beg);
            if (v.x > m.x) m.x = v.x, ax = k;  // strictly larger: a tie stays with the earlier member
            if (v.y > m.y) m.y = v.y, ay = k;
            if (v.z > m.z) m.z = v.z, az = k;
            if (v.w > m.w) m.w = v.w, aw = k;
        }
        const float4 s = scale[c], b = shift[c], d = dout[j * C4 + c];
        const float4 g = make_float4(d.x * gelu_grad(m.x * s.x + b.x), d.y * gelu_grad(m.y * s.y + b.y),
                                     d.z * gelu_grad(m.z * s.z + b.z), d.w * gelu_grad(m.w * s.w + b.w));
        dz[j * C4 + c] = g;
        xmax[j * C4 + c] = m;
        const float4 gs = make_float4(g.x * s.x, g.y * s.y, g.z * s.z, g.w * s.w);
        for (long long r = beg; r < end; ++r) {
            const int k = (int)(r - beg);
            dx[members[r] * C4 + c] = make_float4(k == ax ? gs.x : 0.f, k == ay ? gs.y : 0.f, k == az ? gs.z : 0.f,
                                                  k == aw ? gs.w : 0.f);
        }
    }
}

__global__ __launch_bounds__(256) void cluster_sum_kernel(long long clusters, int C4, const float4 *__restrict__ x,
                                                          const long long *__restrict__ members,
                                                          const long long *__restrict__ seg, float4 *__restrict__ out) {
    const long long j = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= clusters) return;
    const int lane = threadIdx.x & 63;
    const long long beg = seg[j], end = seg[j + 1];
    for (int c = lane; c < C4; c += 64) {
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        if (beg < end) acc = x[members[beg] * C4 + c];
        for (long long r = beg + 1; r < end; ++r) {
            const float4 v = x[members[r] * C4 + c];
            acc.x += v.x, acc.y += v.y, acc.z += v.z, acc.w += v.w;
        }
        out[j * C4 + c] = acc;
    }
}

}  // namespace cloud_bwd
}  // namespace amav

using namespace amav;

static inline unsigned blocks_for(long long threads) { return (unsigned)((threads + 255) / 256); }
static inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

extern "C" int amav_subm_pair_sum_csr(int64_t n, int channels, const float *products, int64_t pair_lo, int64_t pair_count,
                                      const int32_t *src_start, const int32_t *src_pairs, int accumulate, float *out,
                                      void *stream) {
    AMAV_REQUIRE(n > 0 && n < INT_MAX && channels > 0 && channels % 4 == 0 && pair_lo >= 0 && pair_count > 0 &&
                     pair_lo + pair_count < INT_MAX,
                 "amav_subm_pair_sum_csr: bad sizes n=%lld channels=%d pair_lo=%lld pair_count=%lld", (long long)n, channels,
                 (long long)pair_lo, (long long)pair_count);
    AMAV_REQUIRE(products && src_start && src_pairs && out, "amav_subm_pair_sum_csr: NULL pointer");
    AMAV_REQUIRE(aligned16(products) && aligned16(out), "amav_subm_pair_sum_csr: buffers must be 16-byte aligned");
    cloud_bwd::pair_sum_csr_kernel<<<blocks_for((long long)n * (channels / 4)), 256, 0, static_cast<hipStream_t>(stream)>>>(
        n, channels / 4, reinterpret_cast<const float4 *>(products), pair_lo, pair_lo + pair_count, src_start, src_pairs,
        accumulate, reinterpret_cast<float4 *>(out));
    return check_launch("amav_subm_pair_sum_csr");
}

extern "C" size_t amav_subm_pair_wgrad_workspace_bytes(int slices, int cin, int cout) {
    if (slices <= 0 || cin <= 0 || cin % 32 || cout <= 0 || cout % 32) return 0;
    return align_up((size_t)slices * cin * cout * sizeof(float), 256);
}

extern "C" int amav_subm_pair_wgrad(int64_t pairs, int slices, int chunk, int taps, int cin, int cout, const float *feat,
                                    const float *grad_out, const int32_t *pair_src, const int32_t *pair_dst,
                                    const int32_t *tap_start, const int32_t *slice_start, float *grad_weights,
                                    void *workspace, size_t workspace_bytes, void *stream_) {
    AMAV_REQUIRE(pairs > 0 && pairs < INT_MAX && slices > 0 && taps > 0 && chunk > 0 && chunk % cloud_bwd::kWgradChunk == 0,
                 "amav_subm_pair_wgrad: bad sizes pairs=%lld slices=%d taps=%d chunk=%d (a multiple of %d)", (long long)pairs,
                 slices, taps, chunk, cloud_bwd::kWgradChunk);
    AMAV_REQUIRE(cin > 0 && cin % 32 == 0 && cout > 0 && cout % 32 == 0 && cin / 32 <= 65535 && cout / 32 <= 65535,
                 "amav_subm_pair_wgrad: channels must be multiples of 32 (C_in %d, C_out %d)", cin, cout);
    AMAV_REQUIRE(feat && grad_out && pair_src && pair_dst && tap_start && slice_start && grad_weights,
                 "amav_subm_pair_wgrad: NULL pointer");
    AMAV_REQUIRE(aligned16(feat) && aligned16(grad_out) && aligned16(grad_weights) && aligned16(workspace),
                 "amav_subm_pair_wgrad: buffers must be 16-byte aligned");
    const size_t need = amav_subm_pair_wgrad_workspace_bytes(slices, cin, cout);
    if (workspace == nullptr || workspace_bytes < need)
        return fail(AMAV_ERR_WORKSPACE, "amav_subm_pair_wgrad: workspace %zu < required %zu", workspace_bytes, need);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    float *partial = static_cast<float *>(workspace);
    const int tm = cin % 64 == 0 ? 64 : 32, tn = cout % 64 == 0 ? 64 : 32;
    const dim3 grid((unsigned)slices, (unsigned)(cin / tm), (unsigned)(cout / tn));
#define AMAV_WGRAD(TM_, TN_)                                                                                          \
    cloud_bwd::pair_wgrad_kernel<TM_, TN_><<<grid, 64 * (TM_ / 32) * (TN_ / 32), 0, stream>>>(                         \
        feat, grad_out, pair_src, pair_dst, tap_start, slice_start, taps, chunk, partial, cin, cout)
    if (tm == 64 && tn == 64) AMAV_WGRAD(64, 64);
    else if (tm == 64) AMAV_WGRAD(64, 32);
    else if (tn == 64) AMAV_WGRAD(32, 64);
    else AMAV_WGRAD(32, 32);
#undef AMAV_WGRAD
    const long long mat4 = (long long)cin * cout / 4;
    cloud_bwd::wgrad_reduce_kernel<<<blocks_for(taps * mat4), 256, 0, stream>>>(
        taps, mat4, slice_start, reinterpret_cast<const float4 *>(partial), reinterpret_cast<float4 *>(grad_weights));
    return check_launch("amav_subm_pair_wgrad");
}

extern "C" size_t amav_patch_attention_backward_workspace_bytes(int64_t n, int heads, int head_dim) {
    if (n <= 0 || heads <= 0 || (head_dim != 16 && head_dim != 32 && head_dim != 64)) return 0;
    Carver cv(nullptr);
    cv.take<float>((size_t)n * heads);                 // delta [n, heads]
    cv.take<float>((size_t)n * 2 * heads * head_dim);  // borrowed dK | dV [n, 2 C]
    return cv.total();
}

extern "C" int amav_patch_attention_backward(int64_t n, int patches, int max_patch, int heads, int head_dim,
                                             const float *qkv, const int64_t *order, const int32_t *patch_desc,
                                             const float *out, const float *lse, const float *grad_out, float *grad_qkv,
                                             float scale, void *workspace, size_t workspace_bytes, void *stream_) {
    AMAV_REQUIRE(n > 0 && n < INT_MAX && patches > 0 && patches <= 65535 && heads > 0 && heads <= 65535 && max_patch > 0,
                 "amav_patch_attention_backward: bad sizes n=%lld patches=%d heads=%d max_patch=%d", (long long)n, patches,
                 heads, max_patch);
    AMAV_REQUIRE(head_dim == 16 || head_dim == 32 || head_dim == 64,
                 "amav_patch_attention_backward: head_dim %d (16, 32, 64 are built)", head_dim);
    AMAV_REQUIRE(qkv && order && patch_desc && out && lse && grad_out && grad_qkv, "amav_patch_attention_backward: NULL pointer");
    AMAV_REQUIRE(aligned16(qkv) && aligned16(out) && aligned16(patch_desc) && aligned16(grad_out) && aligned16(grad_qkv) &&
                     (reinterpret_cast<uintptr_t>(lse) & 3) == 0 && aligned16(workspace),
                 "amav_patch_attention_backward: buffers must be 16-byte aligned (lse: 4)");
    AMAV_REQUIRE(std::isfinite(scale), "amav_patch_attention_backward: scale must be finite");
    const size_t need = amav_patch_attention_backward_workspace_bytes(n, heads, head_dim);
    if (workspace == nullptr || workspace_bytes < need)
        return fail(AMAV_ERR_WORKSPACE, "amav_patch_attention_backward: workspace %zu < required %zu", workspace_bytes, need);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int C = heads * head_dim;
    Carver cv(workspace);
    float *delta = cv.take<float>((size_t)n * heads);
    float *stage = cv.take<float>((size_t)n * 2 * C);
    const long long *ord = reinterpret_cast<const long long *>(order);
    const int4 *pd = reinterpret_cast<const int4 *>(patch_desc);
    const dim3 grid((unsigned)((max_patch + 127) / 128), (unsigned)heads, (unsigned)patches);
    const long long row_heads = (long long)n * heads;
#define AMAV_PA_BWD(D_)                                                                                              \
    {                                                                                                                \
        cloud_bwd::pa_delta_kernel<D_><<<blocks_for(row_heads * (D_ / 4)), 256, 0, stream>>>(row_heads, out, grad_out, delta); \
        cloud_bwd::pa_dkdv_kernel<D_><<<grid, 256, 0, stream>>>(qkv, ord, pd, grad_out, lse, delta, grad_qkv, stage, C,    \
                                                               heads, scale);                                       \
        cloud_bwd::pa_dq_kernel<D_><<<grid, 256, 0, stream>>>(qkv, ord, pd, grad_out, lse, delta, grad_qkv, C, heads, scale); \
    }
    if (head_dim == 16) AMAV_PA_BWD(16)
    else if (head_dim == 32) AMAV_PA_BWD(32)
    else AMAV_PA_BWD(64)
#undef AMAV_PA_BWD
    const long long threads = (long long)patches * max_patch * (C / 2);
    cloud_bwd::pa_borrow_add_kernel<<<blocks_for(threads), 256, 0, stream>>>(threads, max_patch, C / 2, ord, pd,
                                                                          reinterpret_cast<const float4 *>(stage), grad_qkv, C);
    return check_launch("amav_patch_attention_backward");
}

extern "C" int amav_cluster_max_backward(int64_t clusters, int channels, const float *x, const int64_t *members,
                                         const int64_t *seg, const float *scale, const float *shift, const float *grad_out,
                                         float *grad_x, float *grad_z, float *x_max, void *stream) {
    AMAV_REQUIRE(clusters > 0 && channels > 0 && channels % 4 == 0, "amav_cluster_max_backward: bad sizes clusters=%lld channels=%d",
                 (long long)clusters, channels);
    AMAV_REQUIRE(x && members && seg && scale && shift && grad_out && grad_x && grad_z && x_max,
                 "amav_cluster_max_backward: NULL pointer");
    AMAV_REQUIRE(aligned16(x) && aligned16(scale) && aligned16(shift) && aligned16(grad_out) && aligned16(grad_x) &&
                     aligned16(grad_z) && aligned16(x_max),
                 "amav_cluster_max_backward: buffers must be 16-byte aligned");
    auto f4 = [](const float *p) { return reinterpret_cast<const float4 *>(p); };
    cloud_bwd::cluster_max_backward_kernel<<<(unsigned)((clusters + 3) / 4), 256, 0, static_cast<hipStream_t>(stream)>>>(
        clusters, channels / 4, f4(x), reinterpret_cast<const long long *>(members), reinterpret_cast<const long long *>(seg),
        f4(scale), f4(shift), f4(grad_out), reinterpret_cast<float4 *>(grad_x), reinterpret_cast<float4 *>(grad_z),
        reinterpret_cast<float4 *>(x_max));
    return check_launch("amav_cluster_max_backward");
}

extern "C" int amav_cluster_sum(int64_t clusters, int channels, const float *x, const int64_t *members, const int64_t *seg,
                                float *out, void *stream) {
    AMAV_REQUIRE(clusters > 0 && channels > 0 && channels % 4 == 0, "amav_cluster_sum: bad sizes clusters=%lld channels=%d",
                 (long long)clusters, channels);
    AMAV_REQUIRE(x && members && seg && out, "amav_cluster_sum: NULL pointer");
    AMAV_REQUIRE(aligned16(x) && aligned16(out), "amav_cluster_sum: buffers must be 16-byte aligned");
    cloud_bwd::cluster_sum_kernel<<<(unsigned)((clusters + 3) / 4), 256, 0, static_cast<hipStream_t>(stream)>>>(
        clusters, channels / 4, reinterpret_cast<const float4 *>(x), reinterpret_cast<const long long *>(members),
        reinterpret_cast<const long long *>(seg), reinterpret_cast<float4 *>(out));
    return check_launch("amav_cluster_sum");
}
