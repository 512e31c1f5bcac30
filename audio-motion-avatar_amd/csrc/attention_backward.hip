// Backward of the audio transformer's self-attention (csrc/attention.hip): given the forward's
// inputs, its output O, the row log-sum-exp L (amav_selfattn_forward_lse) and dO = dLoss/dO, the gradients
//     P = exp(scale Q K^T - L),  dP = dO V^T,  delta_i = rowsum(dO_i * O_i),  dS = P * (dP - delta)
//     dV = P^T dO,  dK = scale dS^T Q,  dQ = scale dS K
// flash-attention-2 style, never materialising the S x S matrices, in three passes:
//   delta_kernel   delta_i, one pass over O and dO;
//   dkdv_kernel    key-major: a wave owns 32 keys (K, V rows in registers) and sweeps every query tile, recomputing P
//                  and dS and accumulating dV^T and dK^T in its accumulator registers -- no cross-workgroup sum;
//   dq_kernel      query-major: a wave owns 32 queries (Q, dO rows in registers) and sweeps every key tile, recomputing
//                  S and dP, accumulating dQ^T.  Seven products instead of the five of a slab-summed dQ, but no slabs.
// Every sum runs in a fixed order with no atomics, so a call is deterministic bit for bit, and each (batch, head) is
// computed alone, so a batch of B equals B single calls.  The products run on v_mfma_f32_32x32x2_f32 (exact fp32
// products, fp32 sums), as the AMAV_ATTN=f32 forward does; DESIGN.md section 4.10 has the accuracy and the reasons.
//
// Layouts (v_mfma_f32_32x32x2_f32): A lane (i, hh) holds A[i][hh], B lane (j, hh) holds B[hh][j], accumulator register t
// of lane (j, hh) holds C[r(t) + 4 hh][j] with r(t) = (t & 3) + 8 (t >> 2).  A product whose contraction index is the
// row index of an accumulator takes that accumulator as its B operand directly: k-step t pairs rows r(t) and r(t) + 4.
// The key-major kernel computes S = Q K^T (queries on the rows) for that reason, and the dQ kernel S^T = K Q^T.
#include <cmath>

#include "amav_common.h"

namespace amav {
namespace attn_bwd {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kD = 64;          // head dim
constexpr int kBW = 128;        // keys (dkdv_kernel) or queries (dq_kernel) per workgroup: 4 waves x 32
constexpr int kBT = 32;         // rows of the swept operand per LDS tile
constexpr int kLd = kBT + 1;    // padded row of a transposed [d][row] tile
constexpr float kLog2e = 1.4426950408889634f;

__device__ __forceinline__ int acc_row(int t, int hh) { return (t & 3) + 8 * (t >> 2) + 4 * hh; }

// 16 threads per (b, query, head) row, 4 consecutive d each (rows in memory order, so the reads are contiguous)
__global__ __launch_bounds__(256) void delta_kernel(const float *__restrict__ out, long long out_rs,
                                                    const float *__restrict__ dout, long long dout_rs, int B, int H,
                                                    int S, float *__restrict__ delta) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long row = gid >> 4;  // (b * S + i) * H + head
    const int d4 = (int)(gid & 15);
    const bool live = row < (long long)B * S * H;
    float acc = 0.f;
    int head = 0, i = 0, b = 0;
    if (live) {
        head = (int)(row % H), i = (int)((row / H) % S), b = (int)(row / ((long long)H * S));
        const float4 o = *reinterpret_cast<const float4 *>(out + ((size_t)b * S + i) * out_rs + head * kD + 4 * d4);
        const float4 g = *reinterpret_cast<const float4 *>(dout + ((size_t)b * S + i) * dout_rs + head * kD + 4 * d4);
        acc = (o.x * g.x + o.y * g.y) + (o.z * g.z + o.w * g.w);
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 16);
    if (live && d4 == 0) delta[((size_t)b * H + head) * S + i] = acc;
}

// grid (key blocks of 128, H, B), 256 threads.  Wave w owns keys blockIdx.x * 128 + 32 w + (lane & 31).
__global__ __launch_bounds__(256) void dkdv_kernel(const float *__restrict__ q, const float *__restrict__ k,
                                                   const float *__restrict__ v, long long rs,
                                                   const float *__restrict__ dout, long long dout_rs,
                                                   const float *__restrict__ lse, const float *__restrict__ delta,
                                                   float *__restrict__ dk, float *__restrict__ dv, long long g_rs, int S,
                                                   int H, float scale) {
    __shared__ float Qt[kD * kLd];  // [d][query] of the current query tile
    __shared__ float Gt[kD * kLd];  // [d][query] of dO
    __shared__ float Ls[kBT], Ds[kBT];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int c = lane & 31, hh = lane >> 5;
    const int head = blockIdx.y, b = blockIdx.z;
    const int key = blockIdx.x * kBW + wave * 32 + c;
    const size_t base = (size_t)b * S, bh = (size_t)b * H + head;
    const float sl2 = scale * kLog2e;

    // B operands of S = Q K^T (K pre-scaled to the log2 domain) and dP = dO V^T: lane (key, hh) holds row[2 s + hh]
    float Kr[32], Vr[32];
    {
        const size_t off = (base + min(key, S - 1)) * rs + head * kD;
#pragma unroll
        for (int s = 0; s < 32; ++s) {
            const float2 kt = *reinterpret_cast<const float2 *>(k + off + 2 * s);
            const float2 vt = *reinterpret_cast<const float2 *>(v + off + 2 * s);
            Kr[s] = (hh ? kt.y : kt.x) * sl2;
            Vr[s] = hh ? vt.y : vt.x;
        }
    }
    f32x16 dV0, dV1, dK0, dK1;  // dV^T, dK^T: rows d (0..31 / 32..63), column = this lane's key
#pragma unroll
    for (int t = 0; t < 16; ++t) dV0[t] = 0.f, dV1[t] = 0.f, dK0[t] = 0.f, dK1[t] = 0.f;

    // staging map: thread -> query tid / 8 of the tile, 8 consecutive d at (tid % 8) * 8.  Queries past S are staged as
    // zeros with L = delta = 0: their P is 1 and their dS 0, and both meet a zero dO / Q row, so they add exact zeros.
    const int sq = tid >> 3, sd = (tid & 7) * 8;
    const int ntiles = (S + kBT - 1) / kBT;
    for (int qt = 0; qt < ntiles; ++qt) {
        const int qi = qt * kBT + sq;
        float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0, g0 = a0, g1 = a0;
        if (qi < S) {
            const float *qrow = q + (base + qi) * rs + head * kD + sd;
            const float *grow = dout + (base + qi) * dout_rs + head * kD + sd;
            a0 = *reinterpret_cast<const float4 *>(qrow), a1 = *reinterpret_cast<const float4 *>(qrow + 4);
            g0 = *reinterpret_cast<const float4 *>(grow), g1 = *reinterpret_cast<const float4 *>(grow + 4);
        }
        const float av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
        const float gv[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) Qt[(sd + e) * kLd + sq] = av[e], Gt[(sd + e) * kLd + sq] = gv[e];
        if (tid < kBT) {
            const int qq = qt * kBT + tid;
            Ls[tid] = qq < S ? lse[bh * S + qq] * kLog2e : 0.f;
            Ds[tid] = qq < S ? delta[bh * S + qq] : 0.f;
        }
        __syncthreads();

        f32x16 Sa, dP;  // rows = queries r(t) + 4 hh of the tile, column = this lane's key
#pragma unroll
        for (int t = 0; t < 16; ++t) Sa[t] = 0.f, dP[t] = 0.f;
#pragma unroll
        for (int s = 0; s < 32; ++s) {
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
            dV0 = __builtin_amdgcn_mfma_f32_32x32x2f32(Gt[c * kLd + qq], P[t], dV0, 0, 0, 0);
            dV1 = __builtin_amdgcn_mfma_f32_32x32x2f32(Gt[(c + 32) * kLd + qq], P[t], dV1, 0, 0, 0);
            dK0 = __builtin_amdgcn_mfma_f32_32x32x2f32(Qt[c * kLd + qq], dS[t], dK0, 0, 0, 0);
            dK1 = __builtin_amdgcn_mfma_f32_32x32x2f32(Qt[(c + 32) * kLd + qq], dS[t], dK1, 0, 0, 0);
        }
        __syncthreads();  // every wave is done with this tile before it is overwritten
    }

    if (key < S) {
        float *krow = dk + (base + key) * g_rs + head * kD;
        float *vrow = dv + (base + key) * g_rs + head * kD;
#pragma unroll
        for (int g = 0; g < 4; ++g) {  // registers 4g..4g+3 are 4 consecutive d: 8g + 4hh + (0..3)
            const int d = 8 * g + 4 * hh;
            *reinterpret_cast<float4 *>(vrow + d) = make_float4(dV0[4 * g], dV0[4 * g + 1], dV0[4 * g + 2], dV0[4 * g + 3]);
            *reinterpret_cast<float4 *>(vrow + 32 + d) =
                make_float4(dV1[4 * g], dV1[4 * g + 1], dV1[4 * g + 2], dV1[4 * g + 3]);
            *reinterpret_cast<float4 *>(krow + d) = make_float4(dK0[4 * g] * scale, dK0[4 * g + 1] * scale,
                                                                dK0[4 * g + 2] * scale, dK0[4 * g + 3] * scale);
            *reinterpret_cast<float4 *>(krow + 32 + d) = make_float4(dK1[4 * g] * scale, dK1[4 * g + 1] * scale,
                                                                     dK1[4 * g + 2] * scale, dK1[4 * g + 3] * scale);
        }
    }
}

// grid (query blocks of 128, H, B), 256 threads.  Wave w owns queries blockIdx.x * 128 + 32 w + (lane & 31).
__global__ __launch_bounds__(256) void dq_kernel(const float *__restrict__ q, const float *__restrict__ k,
                                                 const float *__restrict__ v, long long rs,
                                                 const float *__restrict__ dout, long long dout_rs,
                                                 const float *__restrict__ lse, const float *__restrict__ delta,
                                                 float *__restrict__ dq, long long g_rs, int S, int H, float scale) {
    __shared__ float Kt[kD * kLd];  // [d][key] of the current key tile
    __shared__ float Vt[kD * kLd];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int c = lane & 31, hh = lane >> 5;
    const int head = blockIdx.y, b = blockIdx.z;
    const int query = blockIdx.x * kBW + wave * 32 + c;
    const size_t base = (size_t)b * S, bh = (size_t)b * H + head;
    const int qc = min(query, S - 1);

    // B operands of S^T = K Q^T (Q pre-scaled to the log2 domain) and dP^T = V dO^T
    float Qr[32], Gr[32];
    {
        const float *qrow = q + (base + qc) * rs + head * kD;
        const float *grow = dout + (base + qc) * dout_rs + head * kD;
        const float sl2 = scale * kLog2e;
#pragma unroll
        for (int s = 0; s < 32; ++s) {
            const float2 qt = *reinterpret_cast<const float2 *>(qrow + 2 * s);
            const float2 gt = *reinterpret_cast<const float2 *>(grow + 2 * s);
            Qr[s] = (hh ? qt.y : qt.x) * sl2;
            Gr[s] = hh ? gt.y : gt.x;
        }
    }
    const float Lq = lse[bh * S + qc] * kLog2e, Dq = delta[bh * S + qc];
    f32x16 dQ0, dQ1;  // dQ^T: rows d, column = this lane's query
#pragma unroll
    for (int t = 0; t < 16; ++t) dQ0[t] = 0.f, dQ1[t] = 0.f;

    const int sk = tid >> 3, sd = (tid & 7) * 8;
    const int ntiles = (S + kBT - 1) / kBT;
    for (int kt = 0; kt < ntiles; ++kt) {
        const int kj = kt * kBT + sk;
        float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0, b0 = a0, b1 = a0;
        if (kj < S) {
            const float *krow = k + (base + kj) * rs + head * kD + sd;
            const float *vrow = v + (base + kj) * rs + head * kD + sd;
            a0 = *reinterpret_cast<const float4 *>(krow), a1 = *reinterpret_cast<const float4 *>(krow + 4);
            b0 = *reinterpret_cast<const float4 *>(vrow), b1 = *reinterpret_cast<const float4 *>(vrow + 4);
        }
        const float av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
        const float bv[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) Kt[(sd + e) * kLd + sk] = av[e], Vt[(sd + e) * kLd + sk] = bv[e];
        __syncthreads();

        f32x16 St, dPt;  // rows = keys r(t) + 4 hh of the tile, column = this lane's query
#pragma unroll
        for (int t = 0; t < 16; ++t) St[t] = 0.f, dPt[t] = 0.f;
#pragma unroll
        for (int s = 0; s < 32; ++s) {
            St = __builtin_amdgcn_mfma_f32_32x32x2f32(Kt[(2 * s + hh) * kLd + c], Qr[s], St, 0, 0, 0);
            dPt = __builtin_amdgcn_mfma_f32_32x32x2f32(Vt[(2 * s + hh) * kLd + c], Gr[s], dPt, 0, 0, 0);
        }
        f32x16 dS;
        const bool tail = (kt + 1) * kBT > S;
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const float p = tail && kt * kBT + acc_row(t, hh) >= S ? 0.f : exp2f(St[t] - Lq);  // keys past S: P = 0
            dS[t] = p * (dPt[t] - Dq);
        }
        // dQ^T += K^T dS^T: k-step t contracts over keys r(t), r(t) + 4
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const int kk = acc_row(t, hh);
            dQ0 = __builtin_amdgcn_mfma_f32_32x32x2f32(Kt[c * kLd + kk], dS[t], dQ0, 0, 0, 0);
            dQ1 = __builtin_amdgcn_mfma_f32_32x32x2f32(Kt[(c + 32) * kLd + kk], dS[t], dQ1, 0, 0, 0);
        }
        __syncthreads();
    }

    if (query < S) {
        float *row = dq + (base + query) * g_rs + head * kD;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int d = 8 * g + 4 * hh;
            *reinterpret_cast<float4 *>(row + d) = make_float4(dQ0[4 * g] * scale, dQ0[4 * g + 1] * scale,
                                                               dQ0[4 * g + 2] * scale, dQ0[4 * g + 3] * scale);
            *reinterpret_cast<float4 *>(row + 32 + d) = make_float4(dQ1[4 * g] * scale, dQ1[4 * g + 1] * scale,
                                                                    dQ1[4 * g + 2] * scale, dQ1[4 * g + 3] * scale);
        }
    }
}

}  // namespace attn_bwd
}  // namespace amav

using namespace amav;

extern "C" size_t amav_selfattn_backward_workspace_bytes(int B, int S, int H, int D) {
    if (B <= 0 || S <= 0 || H <= 0 || D != attn_bwd::kD) return 0;
    return align_up((size_t)B * H * S * sizeof(float), 256);  // delta [B, H, S]
}

extern "C" int amav_selfattn_backward(int B, int S, int H, int D, const float *q, const float *k, const float *v,
                                      int64_t row_stride, const float *out, int64_t out_row_stride, const float *lse,
                                      const float *dout, int64_t dout_row_stride, float *dqkv, int64_t dqkv_row_stride,
                                      float scale, void *workspace, size_t workspace_bytes, void *stream_) {
    AMAV_REQUIRE(B > 0 && S > 0 && H > 0, "amav_selfattn_backward: bad sizes B=%d S=%d H=%d", B, S, H);
    AMAV_REQUIRE(D == attn_bwd::kD, "amav_selfattn_backward: head_dim %d (only %d is built)", D, attn_bwd::kD);
    AMAV_REQUIRE(q && k && v && out && lse && dout && dqkv, "amav_selfattn_backward: NULL pointer");
    const int64_t hd = (int64_t)H * D;
    AMAV_REQUIRE(row_stride >= hd && out_row_stride >= hd && dout_row_stride >= hd && row_stride % 4 == 0 &&
                     out_row_stride % 4 == 0 && dout_row_stride % 4 == 0,
                 "amav_selfattn_backward: q/k/v, out and dout row strides must be multiples of 4 floats and >= H*D");
    AMAV_REQUIRE(dqkv_row_stride >= 3 * hd && dqkv_row_stride % 4 == 0,
                 "amav_selfattn_backward: dqkv row stride must be a multiple of 4 floats and >= 3*H*D");
    AMAV_REQUIRE(((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(v) |
                   reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(dout) |
                   reinterpret_cast<uintptr_t>(dqkv)) & 15) == 0 &&
                     (reinterpret_cast<uintptr_t>(lse) & 3) == 0,
                 "amav_selfattn_backward: q/k/v/out/dout/dqkv must be 16-byte aligned, lse 4-byte aligned");
    AMAV_REQUIRE(std::isfinite(scale), "amav_selfattn_backward: scale must be finite");
    AMAV_REQUIRE(H <= 65535 && B <= 65535, "amav_selfattn_backward: grid too large");
    const size_t need = amav_selfattn_backward_workspace_bytes(B, S, H, D);
    if (workspace == nullptr || workspace_bytes < need)
        return fail(AMAV_ERR_WORKSPACE, "amav_selfattn_backward: workspace %zu < required %zu", workspace_bytes, need);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    float *delta = static_cast<float *>(workspace);
    const long long threads = (long long)B * S * H * 16;
    attn_bwd::delta_kernel<<<(unsigned)((threads + 255) / 256), 256, 0, stream>>>(out, out_row_stride, dout,
                                                                                 dout_row_stride, B, H, S, delta);
    const dim3 grid((unsigned)((S + attn_bwd::kBW - 1) / attn_bwd::kBW), H, B);
    attn_bwd::dkdv_kernel<<<grid, 256, 0, stream>>>(q, k, v, row_stride, dout, dout_row_stride, lse, delta, dqkv + hd,
                                                    dqkv + 2 * hd, dqkv_row_stride, S, H, scale);
    attn_bwd::dq_kernel<<<grid, 256, 0, stream>>>(q, k, v, row_stride, dout, dout_row_stride, lse, delta, dqkv,
                                                  dqkv_row_stride, S, H, scale);
    return check_launch("amav_selfattn_backward");
}
