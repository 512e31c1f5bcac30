// Attention backward on fp16 x 2 split products ("split arithmetic"): the flash-attention-2
// backward of attention_backward_core.h -- delta pre-pass, key-major dK | dV kernel, query-major dQ kernel, every sum in
// a fixed order, no float atomics -- specialised to head dim 64 and dense rows, with all seven products on
// v_mfma_f32_32x32x16_f16.  An operand scaled by an exact power of two becomes h1 + h2 (split_f16.h) and a product is
// h2 g1 + h1 g2 + h1 g1 with fp32 accumulation, small terms first, as in selfattn_f16_kernel (attention.hip).
//
// Scales (all exact powers of two, all taken on the device from a header the pre-pass fills):
//   Q 2^eq, K 2^ek, V 2^ev, dO 2^eg     the call-wide max |.| lands in [2^14, 2^15); the side of S = Q K^T that a wave
//                                       holds in registers carries scale * log2 e, folded in fp32 before the split
//   P 2^14                              P = exp2(S - L log2 e) in [0, 1]
//   dS 2^es, es = 14 - ilogb(2 Ng Nv)   Ng = max_i |dO_i|_2, Nv = max_j |v_j|_2 per head row: |dS_ij| <= 2 Ng Nv
// The header is filled by integer atomicMax on the bit patterns of non-negative floats (order-independent, hence
// deterministic), as absmax_kernel of attention.hip does.
//
// Layouts (v_mfma_f32_32x32x16_f16): A lane (i, hh) holds A[i][8 hh + 0..7], B lane (j, hh) holds B[8 hh + 0..7][j],
// accumulator register t of lane (j, hh) holds C[(t & 3) + 8 (t >> 2) + 4 hh][j].  A product that contracts over the rows
// of an accumulator takes registers 8 u .. 8 u + 7 as the B operand of k-step u: lane half hh then holds rows
// 16 u + {0..3, 8..11} + 4 hh, so the transposed [d][row] tiles in LDS store every group of 16 rows in that order
// (tile_pos: bits 2 and 3 of the row index swapped) and the A operand is one 16-byte read.
#include "attention_dense_rows.h"
#include "split_f16.h"
#include "wave_ops.h"

namespace amav {
namespace attn_bwd_split {

constexpr int kD = 64;          // head dim
constexpr int kBW = 128;        // keys (dkdv) or queries (dq) per workgroup: 4 waves x 32
constexpr int kBT = 32;         // rows of the swept operand per LDS tile
constexpr int kLdR = kD + 8;    // fp16 per row of a [row][d] tile (144 B: 16-byte reads of 8 consecutive lanes cover all banks)
constexpr int kLdT = kBT + 8;   // fp16 per row of a transposed [d][row] tile (80 B, keeps 16-byte reads aligned)
constexpr float kLog2e = 1.4426950408889634f;
constexpr size_t kHeaderBytes = 256;  // six words: max |q|, |k|, |v|, |dO|, Ng, Nv
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

using attn_bwd::DenseRows;  // the split kernels use its fields and bind only

struct Scales {
    int eq, ek, ev, eg, es;  // exponents of the unfolded operands and of dS
    float mq, mk;            // max |q|, |k| (the folded side takes its exponent from max * |scale log2 e|)
};
__device__ __forceinline__ Scales read_scales(const unsigned *__restrict__ hdr) {
    Scales s;
    s.mq = __uint_as_float(hdr[0]), s.mk = __uint_as_float(hdr[1]);
    s.eq = f16_scale_exp(s.mq), s.ek = f16_scale_exp(s.mk);
    s.ev = f16_scale_exp(__uint_as_float(hdr[2])), s.eg = f16_scale_exp(__uint_as_float(hdr[3]));
    s.es = f16_scale_exp(2.0f * __uint_as_float(hdr[4]) * __uint_as_float(hdr[5]));  // Ng Nv = 0 -> 0
    return s;
}

__device__ __forceinline__ int tile_pos(int row) {  // column of a row in a transposed tile
    return (row & 0x13) | ((row & 4) << 1) | ((row & 8) >> 1);
}
__device__ __forceinline__ float sumsq4(const float4 a) { return (a.x * a.x + a.y * a.y) + (a.z * a.z + a.w * a.w); }

// 16 threads per (row, head) pair, 4 consecutive d each: delta_i as delta_kernel of the fp32 core computes it, and the
// six maxima of the header.  A thread serves query pair r and key pair r where they exist.
__global__ __launch_bounds__(256) void prepass_kernel(DenseRows rows, unsigned *__restrict__ hdr) {
    constexpr int G = kD / 4;
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long r = gid / G;
    const int d4 = (int)(gid % G);
    const long long q_pairs = (long long)rows.B * rows.Sq * rows.H, k_pairs = (long long)rows.B * rows.Sk * rows.H;
    float m[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float acc = 0.f, gg = 0.f, vv = 0.f;
    float *dst = nullptr;
    if (r < q_pairs) {
        const int head = (int)(r % rows.H), i = (int)((r / rows.H) % rows.Sq), b = (int)(r / ((long long)rows.H * rows.Sq));
        const size_t row = (size_t)b * rows.Sq + i;
        const float4 o = *reinterpret_cast<const float4 *>(rows.out + row * rows.out_rs + head * kD + 4 * d4);
        const float4 g = *reinterpret_cast<const float4 *>(rows.dout + row * rows.dout_rs + head * kD + 4 * d4);
        const float4 qv = *reinterpret_cast<const float4 *>(rows.q + row * rows.q_rs + head * kD + 4 * d4);
        dst = rows.delta + ((size_t)b * rows.H + head) * rows.Sq + i;
        acc = (o.x * g.x + o.y * g.y) + (o.z * g.z + o.w * g.w);
        gg = sumsq4(g);
        m[0] = absmax4(0.f, qv), m[3] = absmax4(0.f, g);
    }
    if (r < k_pairs) {
        const int head = (int)(r % rows.H);
        const size_t row = (size_t)(r / rows.H);  // b * Sk + j
        const float4 kx = *reinterpret_cast<const float4 *>(rows.k + row * rows.kv_rs + head * kD + 4 * d4);
        const float4 vx = *reinterpret_cast<const float4 *>(rows.v + row * rows.kv_rs + head * kD + 4 * d4);
        vv = sumsq4(vx);
        m[1] = absmax4(0.f, kx), m[2] = absmax4(0.f, vx);
    }
    acc = group_sum<G>(acc), gg = group_sum<G>(gg), vv = group_sum<G>(vv);
    if (dst && d4 == 0) *dst = acc;
    m[4] = sqrtf(gg), m[5] = sqrtf(vv);
    block_absmax_publish(m, hdr);  // one atomic per block and word
}

// One thread's share of a 32-row tile: rows 2 pi and 2 pi + 1, 4 consecutive d at d4, scaled by `mul`, split, and
// written to the [part][row][d] tile and (kT) to the transposed [part][d][tile_pos(row)] tile -- the two rows are
// neighbours there too, so a transposed store is one 32-bit word.
template <bool kT>
__device__ __forceinline__ void stage_pair(const float4 x0, const float4 x1, float mul, int pi, int d4,
                                           _Float16 (*rm)[kBT * kLdR], _Float16 (*tr)[kD * kLdT]) {
    const float a[2][4] = {{x0.x, x0.y, x0.z, x0.w}, {x1.x, x1.y, x1.z, x1.w}};
    f16x4 h[2][2];  // [row][part]
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            _Float16 p1, p2;
            split2(a[r][e] * mul, p1, p2);
            h[r][0][e] = p1, h[r][1][e] = p2;
        }
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int p = 0; p < 2; ++p) *reinterpret_cast<f16x4 *>(&rm[p][(2 * pi + r) * kLdR + d4]) = h[r][p];
    if (kT) {
        const int pos = tile_pos(2 * pi);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                f16x2 w;
                w[0] = h[0][p][e], w[1] = h[1][p][e];
                *reinterpret_cast<f16x2 *>(&tr[p][(d4 + e) * kLdT + pos]) = w;
            }
    }
}

// A row's 64 floats, times `mul`, as the B operand of a contraction over d: lane half hh holds d 16 s + 8 hh + 0..7
__device__ __forceinline__ void load_b_operand(const float *__restrict__ row, int hh, float mul, f16x8 (&X1)[4],
                                               f16x8 (&X2)[4]) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const float4 lo = *reinterpret_cast<const float4 *>(row + 16 * s + 8 * hh);
        const float4 hi = *reinterpret_cast<const float4 *>(row + 16 * s + 8 * hh + 4);
        const float x[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) {
            _Float16 a, b;
            split2(x[jj] * mul, a, b);
            X1[s][jj] = a, X2[s][jj] = b;
        }
    }
}

// acc += A B over d for a [row][d] tile in LDS (A, rows on the accumulator's rows) and a register operand
__device__ __forceinline__ f32x16 product_over_d(const _Float16 (*rm)[kBT * kLdR], int c, int hh, const f16x8 (&X1)[4],
                                                 const f16x8 (&X2)[4]) {
    f32x16 acc;
#pragma unroll
    for (int t = 0; t < 16; ++t) acc[t] = 0.f;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int off = c * kLdR + 16 * s + 8 * hh;
        const f16x8 a1 = *reinterpret_cast<const f16x8 *>(&rm[0][off]);
        const f16x8 a2 = *reinterpret_cast<const f16x8 *>(&rm[1][off]);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a2, X1[s], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, X2[s], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, X1[s], acc, 0, 0, 0);
    }
    return acc;
}

// out[a] += T^T X over the tile's 32 rows: T^T the transposed tile (d 32 a + c on the accumulator's rows), X the two
// parts of an accumulator-shaped matrix, k-step u = its registers 8 u .. 8 u + 7
__device__ __forceinline__ void product_over_rows(const _Float16 (*tr)[kD * kLdT], int c, int hh, const f16x8 (&X1)[2],
                                                  const f16x8 (&X2)[2], f32x16 (&out)[2]) {
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const int off = (c + 32 * a) * kLdT + 16 * u + 8 * hh;
            const f16x8 t1 = *reinterpret_cast<const f16x8 *>(&tr[0][off]);
            const f16x8 t2 = *reinterpret_cast<const f16x8 *>(&tr[1][off]);
            out[a] = __builtin_amdgcn_mfma_f32_32x32x16_f16(t2, X1[u], out[a], 0, 0, 0);
            out[a] = __builtin_amdgcn_mfma_f32_32x32x16_f16(t1, X2[u], out[a], 0, 0, 0);
            out[a] = __builtin_amdgcn_mfma_f32_32x32x16_f16(t1, X1[u], out[a], 0, 0, 0);
        }
}

__device__ __forceinline__ void split_acc(const f32x16 &x, f16x8 (&X1)[2], f16x8 (&X2)[2]) {
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        _Float16 a, b;
        split2(x[t], a, b);
        X1[t >> 3][t & 7] = a, X2[t >> 3][t & 7] = b;
    }
}

// registers 4 g .. 4 g + 3 of an accumulator pair are 4 consecutive d: 32 a + 8 g + 4 hh + (0..3)
__device__ __forceinline__ void store_row(float *__restrict__ row, const f32x16 (&acc)[2], int hh, float f1, float f2) {
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int a = 0; a < 2; ++a)
            *reinterpret_cast<float4 *>(row + 32 * a + 8 * g + 4 * hh) =
                make_float4(acc[a][4 * g] * f1 * f2, acc[a][4 * g + 1] * f1 * f2, acc[a][4 * g + 2] * f1 * f2,
                            acc[a][4 * g + 3] * f1 * f2);
}

// grid (key blocks of 128, H, B), 256 threads.  Wave w owns keys blockIdx.x * 128 + 32 w + (lane & 31): K' (softmax
// scale and log2 e folded in) and V' stay in registers as B operands, and the wave sweeps every query tile, recomputing
// P and dS and accumulating dV^T and dK^T -- no cross-workgroup sum.
__global__ __launch_bounds__(256, 2) void dkdv_kernel(DenseRows rows, float scale, const unsigned *__restrict__ hdr) {
    __shared__ __attribute__((aligned(16))) _Float16 Qr[2][kBT * kLdR], Gr[2][kBT * kLdR];  // [part][query][d]
    __shared__ __attribute__((aligned(16))) _Float16 Qt[2][kD * kLdT], Gt[2][kD * kLdT];    // [part][d][tile_pos(query)]
    __shared__ __attribute__((aligned(16))) float Ls[kBT], Ds[kBT];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int c = lane & 31, hh = lane >> 5;
    rows.bind(blockIdx.y, blockIdx.z);
    const int nk = rows.Sk, nq = rows.Sq;
    if ((int)blockIdx.x * kBW >= nk) return;  // uniform over the workgroup
    const int key = blockIdx.x * kBW + wave * 32 + c;
    const int kc = min(key, nk - 1);  // a lane past the last key works on the last key's row; its result is dropped
    const Scales sc = read_scales(hdr);
    const float sl2 = scale * kLog2e;
    const int ekf = f16_scale_exp(sc.mk * fabsf(sl2));
    const float cs = ldexpf(1.0f, -(sc.eq + ekf));      // raw S accumulator -> log2-domain score
    const float cdp = ldexpf(1.0f, -(sc.eg + sc.ev));   // raw dP accumulator -> dP
    const float fs = ldexpf(1.0f, sc.es - 14);          // P 2^14 (dP - delta) -> dS 2^es
    const float q_mul = ldexpf(1.0f, sc.eq), g_mul = ldexpf(1.0f, sc.eg);

    f16x8 K1[4], K2[4], V1[4], V2[4];
    load_b_operand(rows.k + (size_t)kc * rows.kv_rs, hh, sl2 * ldexpf(1.0f, ekf), K1, K2);
    load_b_operand(rows.v + (size_t)kc * rows.kv_rs, hh, ldexpf(1.0f, sc.ev), V1, V2);
    float *const krow = rows.dk + (size_t)kc * rows.dkv_rs, *const vrow = rows.dv + (size_t)kc * rows.dkv_rs;
    f32x16 dV[2], dK[2];  // dV^T, dK^T: rows d (32 a ..), column = this lane's key
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int t = 0; t < 16; ++t) dV[a][t] = 0.f, dK[a][t] = 0.f;

    // Queries past the end are staged as zeros with L = delta = 0: their P is 2^14 and their dS 0, and both meet a zero
    // dO / Q row, so they add exact zeros.
    const int pi = tid >> 4, d4 = (tid & 15) * 4;
    const int ntiles = (nq + kBT - 1) / kBT;
    // the next tile's rows are loaded into registers under this tile's MFMAs
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 qa, qb, ga, gb;
    float lv, dv;
    auto load_tile = [&](int qt) {
        const int q0 = qt * kBT + 2 * pi, qq = qt * kBT + tid;
        qa = qb = ga = gb = zero;
        if (q0 < nq) {
            qa = *reinterpret_cast<const float4 *>(rows.q + (size_t)q0 * rows.q_rs + d4);
            ga = *reinterpret_cast<const float4 *>(rows.dout + (size_t)q0 * rows.dout_rs + d4);
        }
        if (q0 + 1 < nq) {
            qb = *reinterpret_cast<const float4 *>(rows.q + (size_t)(q0 + 1) * rows.q_rs + d4);
            gb = *reinterpret_cast<const float4 *>(rows.dout + (size_t)(q0 + 1) * rows.dout_rs + d4);
        }
        lv = tid < kBT && qq < nq ? rows.lse[qq] * kLog2e : 0.f;
        dv = tid < kBT && qq < nq ? rows.delta[qq] : 0.f;
    };
    load_tile(0);
    for (int qt = 0; qt < ntiles; ++qt) {
        stage_pair<true>(qa, qb, q_mul, pi, d4, Qr, Qt);
        stage_pair<true>(ga, gb, g_mul, pi, d4, Gr, Gt);
        if (tid < kBT) Ls[tid] = lv, Ds[tid] = dv;
        __syncthreads();
        if (qt + 1 < ntiles) load_tile(qt + 1);

        // rows = queries (t & 3) + 8 (t >> 2) + 4 hh of the tile, column = this lane's key
        const f32x16 Sa = product_over_d(Qr, c, hh, K1, K2);
        const f32x16 dP = product_over_d(Gr, c, hh, V1, V2);
        f32x16 P, dS;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 l4 = *reinterpret_cast<const float4 *>(&Ls[8 * g + 4 * hh]);
            const float4 d4v = *reinterpret_cast<const float4 *>(&Ds[8 * g + 4 * hh]);
            const float lq[4] = {l4.x, l4.y, l4.z, l4.w}, dl[4] = {d4v.x, d4v.y, d4v.z, d4v.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int t = 4 * g + e;
                P[t] = __builtin_amdgcn_exp2f(fmaf(Sa[t], cs, -lq[e])) * 16384.0f;
                dS[t] = P[t] * fmaf(dP[t], cdp, -dl[e]) * fs;
            }
        }
        f16x8 P1[2], P2[2], S1[2], S2[2];
        split_acc(P, P1, P2);
        split_acc(dS, S1, S2);
        product_over_rows(Gt, c, hh, P1, P2, dV);  // dV^T += dO^T P
        product_over_rows(Qt, c, hh, S1, S2, dK);  // dK^T += Q^T dS
        __syncthreads();  // every wave is done with this tile before it is overwritten
    }

    if (key < nk) {
        store_row(vrow, dV, hh, ldexpf(1.0f, -14 - sc.eg), 1.0f);
        store_row(krow, dK, hh, ldexpf(1.0f, -sc.eq) * scale, ldexpf(1.0f, -sc.es));
    }
}

// grid (query blocks of 128, H, B), 256 threads.  Wave w owns queries blockIdx.x * 128 + 32 w + (lane & 31): Q' (scale
// and log2 e folded in) and dO' stay in registers, and the wave sweeps every key tile, recomputing S^T and dP^T and
// accumulating dQ^T.
__global__ __launch_bounds__(256, 2) void dq_kernel(DenseRows rows, float scale, const unsigned *__restrict__ hdr) {
    __shared__ __attribute__((aligned(16))) _Float16 Kr[2][kBT * kLdR], Vr[2][kBT * kLdR];  // [part][key][d]
    __shared__ __attribute__((aligned(16))) _Float16 Kt[2][kD * kLdT];                      // [part][d][tile_pos(key)]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int c = lane & 31, hh = lane >> 5;
    rows.bind(blockIdx.y, blockIdx.z);
    const int nk = rows.Sk, nq = rows.Sq;
    if ((int)blockIdx.x * kBW >= nq) return;  // uniform over the workgroup
    const int query = blockIdx.x * kBW + wave * 32 + c;
    const int qc = min(query, nq - 1);  // a lane past the last query works on the last query's row; its result is dropped
    const Scales sc = read_scales(hdr);
    const float sl2 = scale * kLog2e;
    const int eqf = f16_scale_exp(sc.mq * fabsf(sl2));
    const float cs = ldexpf(1.0f, -(sc.ek + eqf));
    const float cdp = ldexpf(1.0f, -(sc.eg + sc.ev));
    const float fs = ldexpf(1.0f, sc.es - 14);
    const float k_mul = ldexpf(1.0f, sc.ek), v_mul = ldexpf(1.0f, sc.ev);

    f16x8 Q1[4], Q2[4], G1[4], G2[4];
    load_b_operand(rows.q + (size_t)qc * rows.q_rs, hh, sl2 * ldexpf(1.0f, eqf), Q1, Q2);
    load_b_operand(rows.dout + (size_t)qc * rows.dout_rs, hh, ldexpf(1.0f, sc.eg), G1, G2);
    // a lane past the last query is computed and dropped: L = 1e30 makes its probabilities zero
    const float Lq = query < nq ? rows.lse[qc] * kLog2e : 1e30f, Dq = rows.delta[qc];
    f32x16 dQ[2];  // dQ^T: rows d, column = this lane's query
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int t = 0; t < 16; ++t) dQ[a][t] = 0.f;

    const int pi = tid >> 4, d4 = (tid & 15) * 4;
    const int ntiles = (nk + kBT - 1) / kBT;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 ka, kb, va, vb;  // the next tile's rows, loaded under this tile's MFMAs
    auto load_tile = [&](int kt) {
        const int k0 = kt * kBT + 2 * pi;
        ka = kb = va = vb = zero;
        if (k0 < nk) {
            ka = *reinterpret_cast<const float4 *>(rows.k + (size_t)k0 * rows.kv_rs + d4);
            va = *reinterpret_cast<const float4 *>(rows.v + (size_t)k0 * rows.kv_rs + d4);
        }
        if (k0 + 1 < nk) {
            kb = *reinterpret_cast<const float4 *>(rows.k + (size_t)(k0 + 1) * rows.kv_rs + d4);
            vb = *reinterpret_cast<const float4 *>(rows.v + (size_t)(k0 + 1) * rows.kv_rs + d4);
        }
    };
    load_tile(0);
    for (int kt = 0; kt < ntiles; ++kt) {
        stage_pair<true>(ka, kb, k_mul, pi, d4, Kr, Kt);
        stage_pair<false>(va, vb, v_mul, pi, d4, Vr, nullptr);
        __syncthreads();
        if (kt + 1 < ntiles) load_tile(kt + 1);

        // rows = keys (t & 3) + 8 (t >> 2) + 4 hh of the tile, column = this lane's query
        const f32x16 St = product_over_d(Kr, c, hh, Q1, Q2);
        const f32x16 dPt = product_over_d(Vr, c, hh, G1, G2);
        f32x16 dS;
        const bool tail = (kt + 1) * kBT > nk;
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const int kk = kt * kBT + (t & 3) + 8 * (t >> 2) + 4 * hh;
            const float p = tail && kk >= nk ? 0.f  // keys past the end: P = 0
                                             : __builtin_amdgcn_exp2f(fmaf(St[t], cs, -Lq)) * 16384.0f;
            dS[t] = p * fmaf(dPt[t], cdp, -Dq) * fs;
        }
        f16x8 S1[2], S2[2];
        split_acc(dS, S1, S2);
        product_over_rows(Kt, c, hh, S1, S2, dQ);  // dQ^T += K^T dS^T
        __syncthreads();
    }

    if (query < nq) store_row(rows.dq + (size_t)query * rows.dq_rs, dQ, hh, ldexpf(1.0f, -sc.ek) * scale, ldexpf(1.0f, -sc.es));
}

static size_t workspace_bytes(int B, int Sq, int H) {
    return kHeaderBytes + align_up((size_t)B * H * Sq * sizeof(float), 256);  // header, delta [B, H, Sq]
}

// `rows.delta` is set here; three kernels and the header's zero fill, no host synchronisation
static int launch(DenseRows rows, float scale, void *workspace, hipStream_t stream, const char *what) {
    unsigned *hdr = static_cast<unsigned *>(workspace);
    rows.delta = reinterpret_cast<float *>(static_cast<char *>(workspace) + kHeaderBytes);
    if (zero_async(hdr, 32, stream) != hipSuccess) return check_launch(what);
    const long long pairs = (long long)rows.B * (rows.Sq > rows.Sk ? rows.Sq : rows.Sk) * rows.H;
    prepass_kernel<<<blocks_for(pairs * (kD / 4)), 256, 0, stream>>>(rows, hdr);
    const dim3 key_grid((unsigned)((rows.Sk + kBW - 1) / kBW), rows.H, rows.B);
    const dim3 query_grid((unsigned)((rows.Sq + kBW - 1) / kBW), rows.H, rows.B);
    dkdv_kernel<<<key_grid, 256, 0, stream>>>(rows, scale, hdr);
    dq_kernel<<<query_grid, 256, 0, stream>>>(rows, scale, hdr);
    return check_launch(what);
}

}  // namespace attn_bwd_split
}  // namespace amav

using namespace amav;

extern "C" size_t amav_selfattn_backward_split_workspace_bytes(int B, int S, int H, int D) {
    if (B <= 0 || S <= 0 || H <= 0 || D != attn_bwd_split::kD) return 0;
    return attn_bwd_split::workspace_bytes(B, S, H);
}

extern "C" int amav_selfattn_backward_split(int B, int S, int H, int D, const float *q, const float *k, const float *v,
                                            int64_t row_stride, const float *out, int64_t out_row_stride,
                                            const float *lse, const float *dout, int64_t dout_row_stride, float *dqkv,
                                            int64_t dqkv_row_stride, float scale, void *workspace,
                                            size_t workspace_bytes, void *stream_) {
    const char *what = "amav_selfattn_backward_split";
    const int64_t hd = (int64_t)H * attn_bwd_split::kD;  // D itself is checked with the rest
    AMAV_REQUIRE(dqkv_row_stride >= 3 * hd && dqkv_row_stride % 4 == 0,
                 "%s: dqkv row stride must be a multiple of 4 floats and >= 3*H*D", what);
    attn_bwd::DenseRows rows = {q, row_stride, k, v, row_stride, out, dout, out_row_stride, dout_row_stride, lse, nullptr,
                                dqkv, dqkv_row_stride, dqkv, nullptr, dqkv_row_stride, B, S, S, H};
    if (int rc = attn_bwd::check_dense_backward(what, rows, D, scale, amav_selfattn_backward_split_workspace_bytes(B, S, H, D),
                                                workspace, workspace_bytes))
        return rc;
    rows.dk = dqkv + hd, rows.dv = dqkv + 2 * hd;
    return attn_bwd_split::launch(rows, scale, workspace, static_cast<hipStream_t>(stream_), what);
}

extern "C" size_t amav_crossattn_backward_split_workspace_bytes(int B, int Sq, int H, int D) {
    if (B <= 0 || Sq <= 0 || H <= 0 || D != attn_bwd_split::kD) return 0;
    return attn_bwd_split::workspace_bytes(B, Sq, H);
}

extern "C" int amav_crossattn_backward_split(int B, int Sq, int Sk, int H, int D, const float *q, int64_t q_row_stride,
                                             const float *k, const float *v, int64_t kv_row_stride, const float *out,
                                             int64_t out_row_stride, const float *lse, const float *dout,
                                             int64_t dout_row_stride, float *dq, int64_t dq_row_stride, float *dkv,
                                             int64_t dkv_row_stride, float scale, void *workspace,
                                             size_t workspace_bytes, void *stream_) {
    const char *what = "amav_crossattn_backward_split";
    const int64_t hd = (int64_t)H * attn_bwd_split::kD;  // D itself is checked with the rest
    AMAV_REQUIRE(dkv_row_stride >= 2 * hd && dkv_row_stride % 4 == 0,
                 "%s: dkv row stride must be a multiple of 4 floats and >= 2*H*D", what);
    attn_bwd::DenseRows rows = {q, q_row_stride, k, v, kv_row_stride, out, dout, out_row_stride, dout_row_stride, lse, nullptr,
                                dq, dq_row_stride, dkv, nullptr, dkv_row_stride, B, Sq, Sk, H};
    if (int rc = attn_bwd::check_dense_backward(what, rows, D, scale, amav_crossattn_backward_split_workspace_bytes(B, Sq, H, D),
                                                workspace, workspace_bytes))
        return rc;
    rows.dv = dkv + hd;
    return attn_bwd_split::launch(rows, scale, workspace, static_cast<hipStream_t>(stream_), what);
}
