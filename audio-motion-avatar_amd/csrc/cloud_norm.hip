// Train-mode BatchNorm of the point refiner: batch statistics of [rows, C] rows, the backward of
// gelu(BatchNorm(x)) through those statistics, and the pooling maximum / its gradient routing on their own.
//
//   amav_bn_batch_stats           mean and biased variance of every column
//   amav_bn_gelu_train_backward   grad_bias = sum g, grad_weight = sum g xhat, grad_x = w rstd (g - mean g - xhat mean(g xhat));
//                                 its column sums in fp64
//   amav_cluster_max_raw          segment maxima (amav_cluster_max without scale, shift and GELU)
//   amav_cluster_max_route        a gradient of those maxima to the first member that attains each
//
// Memory-bound passes: float4 accesses, 64-bit row offsets, no atomics, kernel launches only (capturable).
//
// Layout of every column reduction here.  Rows are cut into consecutive chunks of kChunkRows = 64 (the last may be
// shorter); one wave owns a chunk.  L = min(64, C / 4 rounded up to a power of two) lanes lie along the channel quads and
// the wave's S = 64 / L lane groups ("sub-rows") take the chunk's rows s, s + S, s + 2 S, ... in ascending order, so a
// narrow level (C = 32: L = 8, S = 8) still issues 1 KiB per load instruction.  Order of a sum:
//   stage 1  each sub-row adds its rows in ascending order from +0; the S sub-row partials are then added by an xor
//            butterfly over the lane groups (strides L, 2 L, ... 32; both partners compute the same a + b);
//   stage 2  one wave per channel quad: lane j folds the chunk partials j, j + 64, j + 128, ... in ascending order, then
//            the 64 lanes are folded by a shuffle-down tree (strides 1, 2, ... 32) whose result lane 0 stores.
// The order depends on (rows, C) alone, so two calls are bit-identical.
//
// Statistics.  sum x^2 - (sum x)^2 / n in fp32 loses every digit of the variance of a column whose mean is large against
// its spread.  A chunk is therefore summed about a pivot, its own first row: s1 = sum (x - p), s2 = sum (x - p)^2 ->
// (count, mean = p + s1 / count, M2 = s2 - s1^2 / count, clamped at 0), where p is within the column's spread of the
// chunk's mean; stage 2 merges (count, mean, M2) triples with the update of Chan, Golub & LeVeque (1979):
//   d = mean_b - mean_a, n = n_a + n_b, mean = mean_a + d n_b / n, M2 = M2_a + M2_b + d^2 n_a n_b / n.
// A constant column gives x - p = 0 and d = 0 everywhere: var = 0 exactly.
#include <cmath>

#include "amav_common.h"
#include "gelu.h"

namespace amav {
namespace cloud_norm {

constexpr int kChunkRows = 64;

__device__ __forceinline__ float4 add4(const float4 &a, const float4 &b) {
    return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}
__device__ __forceinline__ float4 shfl_xor4(const float4 &a, int o) {
    return make_float4(__shfl_xor(a.x, o, 64), __shfl_xor(a.y, o, 64), __shfl_xor(a.z, o, 64), __shfl_xor(a.w, o, 64));
}
__device__ __forceinline__ float4 shfl_down4(const float4 &a, int o) {
    return make_float4(__shfl_down(a.x, o, 64), __shfl_down(a.y, o, 64), __shfl_down(a.z, o, 64), __shfl_down(a.w, o, 64));
}

// The wave's place in the layout above.  `live` is false for lanes past the last channel quad of a column pass; they
// carry zeros, so every lane runs every shuffle.
struct Place {
    long long chunk, first;
    int count, sub, ql, S;
    __device__ Place(long long rows, int L) {
        chunk = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
        first = chunk * kChunkRows;
        const long long left = rows - first;
        count = left < kChunkRows ? (int)left : kChunkRows;
        const int lane = threadIdx.x & 63;
        sub = lane / L, ql = lane % L, S = 64 / L;
    }
};

// stage 1 of the statistics: parts [chunks, 2, C4] = (mean, M2) of every chunk (its count follows from its index)
__global__ __launch_bounds__(256) void stats_chunks_kernel(long long rows, long long chunks, int C4, int L,
                                                           const float4 *__restrict__ x, float4 *__restrict__ parts) {
    const Place at(rows, L);
    if (at.chunk >= chunks) return;  // wave-uniform
    const float inv = 1.0f / (float)at.count;
    for (int q0 = 0; q0 < C4; q0 += L) {
        const int q = q0 + at.ql;
        const bool live = q < C4;
        const float4 *src = x + at.first * C4 + (live ? q : 0);
        const float4 p = src[0];
        float4 s1 = make_float4(0.f, 0.f, 0.f, 0.f), s2 = s1;
        if (live) {
#pragma unroll 4
            for (int r = at.sub; r < at.count; r += at.S) {
                const float4 v = src[(long long)r * C4];
                const float dx = v.x - p.x, dy = v.y - p.y, dz = v.z - p.z, dw = v.w - p.w;
                s1.x += dx, s1.y += dy, s1.z += dz, s1.w += dw;
                s2.x += dx * dx, s2.y += dy * dy, s2.z += dz * dz, s2.w += dw * dw;
            }
        }
        for (int o = L; o < 64; o <<= 1) {
            s1 = add4(s1, shfl_xor4(s1, o));
            s2 = add4(s2, shfl_xor4(s2, o));
        }
        if (live && at.sub == 0) {
            const float4 m = make_float4(s1.x * inv, s1.y * inv, s1.z * inv, s1.w * inv);
            parts[(at.chunk * 2 + 0) * C4 + q] = make_float4(p.x + m.x, p.y + m.y, p.z + m.z, p.w + m.w);
            parts[(at.chunk * 2 + 1) * C4 + q] = make_float4(fmaxf(s2.x - s1.x * m.x, 0.f), fmaxf(s2.y - s1.y * m.y, 0.f),
                                                             fmaxf(s2.z - s1.z * m.z, 0.f), fmaxf(s2.w - s1.w * m.w, 0.f));
        }
    }
}

// (n, mean, M2) <- (n, mean, M2) merged with (nb, mb, Mb); either side may be empty (count 0, M2 0)
__device__ __forceinline__ void merge(float &n, float4 &mean, float4 &M2, float nb, const float4 &mb, const float4 &Mb) {
    const float na = n;
    n = na + nb;
    if (na == 0.f) {
        mean = mb, M2 = Mb;
        return;
    }
    const float f = nb / n, w = na * f;  // nb == 0: f = 0 and Mb = 0, the left side is kept
    const float dx = mb.x - mean.x, dy = mb.y - mean.y, dz = mb.z - mean.z, dw = mb.w - mean.w;
    mean = make_float4(mean.x + dx * f, mean.y + dy * f, mean.z + dz * f, mean.w + dw * f);
    M2 = make_float4(M2.x + Mb.x + dx * dx * w, M2.y + Mb.y + dy * dy * w, M2.z + Mb.z + dz * dz * w,
                     M2.w + Mb.w + dw * dw * w);
}

// stage 2 of the statistics: one wave per channel quad
__global__ __launch_bounds__(256) void stats_merge_kernel(long long rows, long long chunks, int C4,
                                                          const float4 *__restrict__ parts, float4 *__restrict__ mean_out,
                                                          float4 *__restrict__ var_out) {
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= C4) return;  // wave-uniform
    const int lane = threadIdx.x & 63;
    float n = 0.f;
    float4 mean = make_float4(0.f, 0.f, 0.f, 0.f), M2 = mean;
    for (long long k = lane; k < chunks; k += 64) {
        const long long left = rows - k * kChunkRows;
        merge(n, mean, M2, left < kChunkRows ? (float)left : (float)kChunkRows, parts[(k * 2 + 0) * C4 + q],
              parts[(k * 2 + 1) * C4 + q]);
    }
    for (int o = 1; o < 64; o <<= 1) {
        const float nb = __shfl_down(n, o, 64);
        const float4 mb = shfl_down4(mean, o), Mb = shfl_down4(M2, o);
        merge(n, mean, M2, nb, mb, Mb);  // lanes whose partner is past the wave fold themselves; lane 0 never reads them
    }
    if (lane == 0) {
        const float inv = 1.0f / (float)rows;
        mean_out[q] = mean;
        var_out[q] = make_float4(M2.x * inv, M2.y * inv, M2.z * inv, M2.w * inv);
    }
}

// ---- backward through the batch statistics ---------------------------------------------------------------------------
// grad_x of a batch-normalised layer sums to zero down every column; at few rows grad_x is itself a small residue of g
// (two rows: 2 d ~ eps / var of it), so that zero has to come out of the arithmetic, not out of luck with fp32 roundings.
// Three things make it so:
//   * xhat and g of an element are the same bits in the sum pass and in the grad_x pass: every operation that the
//     compiler could contract differently in the two kernels is a rounding intrinsic, gelu' is one function (not inlined);
//   * the column sums sum g, sum g xhat and sum xhat are accumulated and kept in fp64 (the partials and a [3, C] block of
//     totals in the workspace); grad_bias and grad_weight are their fp32 roundings;
//   * grad_x = w rstd ((g - mean g) - (xhat - mean xhat) mean(g xhat)) in fp64, rounded once: both brackets sum to zero
//     over a column to fp64 accuracy whatever mean and rstd were rounded to, so |sum grad_x| <= 2^-24 sum |grad_x|.
//     mean xhat is zero up to the fp32 rounding of `mean`; subtracting it is what keeps the zero exact.
__device__ __noinline__ float gelu_grad_pinned(float z) { return gelu_grad(z); }

struct Affine {
    float4 mean, rstd, w, b;
    __device__ Affine(const float4 *mean_, const float4 *rstd_, const float4 *w_, const float4 *b_, int q)
        : mean(mean_[q]), rstd(rstd_[q]), w(w_[q]), b(b_[q]) {}
    __device__ static void one(float v, float d, float mean, float rstd, float w, float b, float &xhat, float &g) {
        xhat = __fmul_rn(__fsub_rn(v, mean), rstd);
        g = __fmul_rn(d, gelu_grad_pinned(__fmaf_rn(xhat, w, b)));
    }
    // xhat of v, and g = d * gelu'(xhat * w + b)
    __device__ void at(const float4 &v, const float4 &d, float4 &xhat, float4 &g) const {
        one(v.x, d.x, mean.x, rstd.x, w.x, b.x, xhat.x, g.x);
        one(v.y, d.y, mean.y, rstd.y, w.y, b.y, xhat.y, g.y);
        one(v.z, d.z, mean.z, rstd.z, w.z, b.z, xhat.z, g.z);
        one(v.w, d.w, mean.w, rstd.w, w.w, b.w, xhat.w, g.w);
    }
};

struct Sums {  // of one channel quad: sum g, sum g xhat, sum xhat
    double g[4], gx[4], x[4];
    __device__ Sums() {
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] = gx[k] = x[k] = 0.0;
    }
    __device__ void add(const float4 &xhat, const float4 &gv) {
        const float xs[4] = {xhat.x, xhat.y, xhat.z, xhat.w}, gs[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] += (double)gs[k], gx[k] += (double)gs[k] * (double)xs[k], x[k] += (double)xs[k];
    }
    __device__ void add(const Sums &o) {
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] += o.g[k], gx[k] += o.gx[k], x[k] += o.x[k];
    }
    template <bool kXor>
    __device__ Sums shuffled(int o) const {
        Sums r;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            r.g[k] = kXor ? __shfl_xor(g[k], o, 64) : __shfl_down(g[k], o, 64);
            r.gx[k] = kXor ? __shfl_xor(gx[k], o, 64) : __shfl_down(gx[k], o, 64);
            r.x[k] = kXor ? __shfl_xor(x[k], o, 64) : __shfl_down(x[k], o, 64);
        }
        return r;
    }
    // block [3, C] of doubles at `to`: row 0 sum g, row 1 sum g xhat, row 2 sum xhat
    __device__ void store(double *to, int C, int q) const {
#pragma unroll
        for (int k = 0; k < 4; ++k) to[4 * q + k] = g[k], to[C + 4 * q + k] = gx[k], to[2 * C + 4 * q + k] = x[k];
    }
    __device__ void load(const double *from, int C, int q) {
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] = from[4 * q + k], gx[k] = from[C + 4 * q + k], x[k] = from[2 * C + 4 * q + k];
    }
};

// stage 1 of the backward's column sums: parts [chunks, 3, C] fp64
__global__ __launch_bounds__(256) void train_backward_chunks_kernel(long long rows, long long chunks, int C4, int L,
                                                                    const float4 *__restrict__ x,
                                                                    const float4 *__restrict__ mean,
                                                                    const float4 *__restrict__ rstd,
                                                                    const float4 *__restrict__ w, const float4 *__restrict__ b,
                                                                    const float4 *__restrict__ dout,
                                                                    double *__restrict__ parts) {
    const Place at(rows, L);
    if (at.chunk >= chunks) return;  // wave-uniform
    for (int q0 = 0; q0 < C4; q0 += L) {
        const int q = q0 + at.ql;
        const bool live = q < C4;
        Sums s;
        if (live) {
            const Affine bn(mean, rstd, w, b, q);
            const long long base = at.first * C4 + q;
#pragma unroll 2
            for (int r = at.sub; r < at.count; r += at.S) {
                float4 xhat, g;
                bn.at(x[base + (long long)r * C4], dout[base + (long long)r * C4], xhat, g);
                s.add(xhat, g);
            }
        }
        for (int o = L; o < 64; o <<= 1) s.add(s.shuffled<true>(o));
        if (live && at.sub == 0) s.store(parts + at.chunk * 12 * C4, 4 * C4, q);
    }
}

// stage 2 of the backward's column sums: one wave per channel quad -> totals [3, C] fp64, grad_bias, grad_weight
__global__ __launch_bounds__(256) void train_backward_sums_kernel(long long chunks, int C4, const double *__restrict__ parts,
                                                                  double *__restrict__ totals,
                                                                  float4 *__restrict__ grad_bias,
                                                                  float4 *__restrict__ grad_weight) {
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= C4) return;  // wave-uniform
    const int lane = threadIdx.x & 63;
    Sums s;
    for (long long k = lane; k < chunks; k += 64) {
        Sums p;
        p.load(parts + k * 12 * C4, 4 * C4, q);
        s.add(p);
    }
    for (int o = 1; o < 64; o <<= 1) s.add(s.shuffled<false>(o));  // lane 0 never reads a lane past the wave
    if (lane == 0) {
        s.store(totals, 4 * C4, q);
        grad_bias[q] = make_float4((float)s.g[0], (float)s.g[1], (float)s.g[2], (float)s.g[3]);
        grad_weight[q] = make_float4((float)s.gx[0], (float)s.gx[1], (float)s.gx[2], (float)s.gx[3]);
    }
}

// grad_x, one thread per (row, channel quad): g and xhat recomputed to the bit, the rest in fp64
__global__ __launch_bounds__(256) void train_backward_dx_kernel(long long quads, int C4, double inv_rows,
                                                                const float4 *__restrict__ x, const float4 *__restrict__ mean,
                                                                const float4 *__restrict__ rstd, const float4 *__restrict__ w,
                                                                const float4 *__restrict__ b, const float4 *__restrict__ dout,
                                                                const double *__restrict__ totals, float4 *__restrict__ dx) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= quads) return;
    const int q = (int)(i % C4);
    const Affine bn(mean, rstd, w, b, q);
    float4 xhat, g;
    bn.at(x[i], dout[i], xhat, g);
    Sums t;
    t.load(totals, 4 * C4, q);
    const float xs[4] = {xhat.x, xhat.y, xhat.z, xhat.w}, gs[4] = {g.x, g.y, g.z, g.w};
    const float ws[4] = {bn.w.x, bn.w.y, bn.w.z, bn.w.w}, rs[4] = {bn.rstd.x, bn.rstd.y, bn.rstd.z, bn.rstd.w};
    float out[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double u = ((double)gs[k] - t.g[k] * inv_rows) - ((double)xs[k] - t.x[k] * inv_rows) * (t.gx[k] * inv_rows);
        out[k] = (float)((double)ws[k] * (double)rs[k] * u);
    }
    dx[i] = make_float4(out[0], out[1], out[2], out[3]);
}

// one wave per cluster, as cluster_max_kernel (csrc/cloud.hip) without its epilogue
__global__ __launch_bounds__(256) void cluster_max_raw_kernel(long long clusters, int C4, const float4 *__restrict__ x,
                                                              const long long *__restrict__ members,
                                                              const long long *__restrict__ seg, float4 *__restrict__ out) {
    const long long j = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= clusters) return;
    const int lane = threadIdx.x & 63;
    const long long beg = seg[j], end = seg[j + 1];
    for (int c = lane; c < C4; c += 64) {
        float4 m = x[members[beg] * C4 + c];
        for (long long r = beg + 1; r < end; ++r) {
            const float4 v = x[members[r] * C4 + c];
            m.x = fmaxf(m.x, v.x), m.y = fmaxf(m.y, v.y), m.z = fmaxf(m.z, v.z), m.w = fmaxf(m.w, v.w);
        }
        out[j * C4 + c] = m;
    }
}

// one wave per cluster, as cluster_max_backward_kernel (csrc/cloud_backward.hip): find the first member (in segment
// order) that attains each maximum, write the cluster's gradient on its row and +0 on the segment's other rows
__global__ __launch_bounds__(256) void cluster_max_route_kernel(long long clusters, int C4, const float4 *__restrict__ x,
                                                                const long long *__restrict__ members,
                                                                const long long *__restrict__ seg,
                                                                const float4 *__restrict__ dmax, float4 *__restrict__ dx) {
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
        const float4 g = dmax[j * C4 + c];
        for (long long r = beg; r < end; ++r) {
            const int k = (int)(r - beg);
            dx[members[r] * C4 + c] = make_float4(k == ax ? g.x : 0.f, k == ay ? g.y : 0.f, k == az ? g.z : 0.f,
                                                  k == aw ? g.w : 0.f);
        }
    }
}

inline long long chunks_of(long long rows) { return (rows + kChunkRows - 1) / kChunkRows; }

inline int lanes_for(int C4) {
    int L = 1;
    while (L < C4 && L < 64) L <<= 1;
    return L;
}

}  // namespace cloud_norm
}  // namespace amav

using namespace amav;

// the larger of the two users: the statistics keep [chunks, 2, C] floats, the backward [chunks + 1, 3, C] doubles
extern "C" size_t amav_bn_batch_stats_workspace_bytes(int64_t rows, int channels) {
    if (rows < 2 || channels <= 0 || channels % 4) return 0;
    return align_up((size_t)(cloud_norm::chunks_of(rows) + 1) * 3 * channels * sizeof(double), 256);
}

extern "C" int amav_bn_batch_stats(int64_t rows, int channels, const float *x, float *mean, float *var, void *workspace,
                                   size_t workspace_bytes, void *stream_) {
    AMAV_REQUIRE(channels > 0 && channels % 4 == 0, "amav_bn_batch_stats: bad sizes rows=%lld channels=%d (a multiple of 4)",
                 (long long)rows, channels);
    AMAV_REQUIRE(rows >= 2, "amav_bn_batch_stats: rows=%lld: batch statistics need at least 2 rows", (long long)rows);
    AMAV_REQUIRE(x && mean && var, "amav_bn_batch_stats: NULL pointer");
    AMAV_REQUIRE(aligned16(x, mean, var, workspace), "amav_bn_batch_stats: buffers must be 16-byte aligned");
    const size_t need = amav_bn_batch_stats_workspace_bytes(rows, channels);
    if (workspace == nullptr || workspace_bytes < need)
        return fail(AMAV_ERR_WORKSPACE, "amav_bn_batch_stats: workspace %zu < required %zu", workspace_bytes, need);
    const long long chunks = cloud_norm::chunks_of(rows);
    AMAV_REQUIRE((chunks + 3) / 4 <= 0x7fffffffLL, "amav_bn_batch_stats: grid too large");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int C4 = channels / 4;
    float4 *parts = static_cast<float4 *>(workspace);
    cloud_norm::stats_chunks_kernel<<<(unsigned)((chunks + 3) / 4), 256, 0, stream>>>(
        rows, chunks, C4, cloud_norm::lanes_for(C4), reinterpret_cast<const float4 *>(x), parts);
    cloud_norm::stats_merge_kernel<<<(unsigned)((C4 + 3) / 4), 256, 0, stream>>>(
        rows, chunks, C4, parts, reinterpret_cast<float4 *>(mean), reinterpret_cast<float4 *>(var));
    return check_launch("amav_bn_batch_stats");
}

extern "C" int amav_bn_gelu_train_backward(int64_t rows, int channels, const float *x, const float *mean, const float *rstd,
                                           const float *weight, const float *bias, const float *grad_out, float *grad_x,
                                           float *grad_weight, float *grad_bias, void *workspace, size_t workspace_bytes,
                                           void *stream_) {
    AMAV_REQUIRE(channels > 0 && channels % 4 == 0,
                 "amav_bn_gelu_train_backward: bad sizes rows=%lld channels=%d (a multiple of 4)", (long long)rows, channels);
    AMAV_REQUIRE(rows >= 2, "amav_bn_gelu_train_backward: rows=%lld: batch statistics need at least 2 rows", (long long)rows);
    AMAV_REQUIRE(x && mean && rstd && weight && bias && grad_out && grad_x && grad_weight && grad_bias,
                 "amav_bn_gelu_train_backward: NULL pointer");
    AMAV_REQUIRE(aligned16(x, mean, rstd, weight, bias, grad_out, grad_x, grad_weight, grad_bias, workspace),
                 "amav_bn_gelu_train_backward: buffers must be 16-byte aligned");
    const size_t need = amav_bn_batch_stats_workspace_bytes(rows, channels);
    if (workspace == nullptr || workspace_bytes < need)
        return fail(AMAV_ERR_WORKSPACE, "amav_bn_gelu_train_backward: workspace %zu < required %zu", workspace_bytes, need);
    const long long chunks = cloud_norm::chunks_of(rows);
    const int C4 = channels / 4;
    const long long quads = (long long)rows * C4;
    AMAV_REQUIRE((quads + 255) / 256 <= 0x7fffffffLL, "amav_bn_gelu_train_backward: grid too large");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    auto p4 = [](const float *p) { return reinterpret_cast<const float4 *>(p); };
    double *parts = static_cast<double *>(workspace), *totals = parts + (size_t)chunks * 3 * channels;
    float4 *db = reinterpret_cast<float4 *>(grad_bias), *dw = reinterpret_cast<float4 *>(grad_weight);
    cloud_norm::train_backward_chunks_kernel<<<(unsigned)((chunks + 3) / 4), 256, 0, stream>>>(
        rows, chunks, C4, cloud_norm::lanes_for(C4), p4(x), p4(mean), p4(rstd), p4(weight), p4(bias), p4(grad_out), parts);
    cloud_norm::train_backward_sums_kernel<<<(unsigned)((C4 + 3) / 4), 256, 0, stream>>>(chunks, C4, parts, totals, db, dw);
    cloud_norm::train_backward_dx_kernel<<<blocks_for(quads), 256, 0, stream>>>(
        quads, C4, 1.0 / (double)rows, p4(x), p4(mean), p4(rstd), p4(weight), p4(bias), p4(grad_out), totals,
        reinterpret_cast<float4 *>(grad_x));
    return check_launch("amav_bn_gelu_train_backward");
}

extern "C" int amav_cluster_max_raw(int64_t clusters, int channels, const float *x, const int64_t *members, const int64_t *seg,
                                    float *out, void *stream) {
    AMAV_REQUIRE(clusters > 0 && channels > 0 && channels % 4 == 0, "amav_cluster_max_raw: bad sizes clusters=%lld channels=%d",
                 (long long)clusters, channels);
    AMAV_REQUIRE(x && members && seg && out, "amav_cluster_max_raw: NULL pointer");
    AMAV_REQUIRE(aligned16(x) && aligned16(out), "amav_cluster_max_raw: buffers must be 16-byte aligned");
    AMAV_REQUIRE((clusters + 3) / 4 <= 0x7fffffffLL, "amav_cluster_max_raw: grid too large");
    cloud_norm::cluster_max_raw_kernel<<<(unsigned)((clusters + 3) / 4), 256, 0, static_cast<hipStream_t>(stream)>>>(
        clusters, channels / 4, reinterpret_cast<const float4 *>(x), reinterpret_cast<const long long *>(members),
        reinterpret_cast<const long long *>(seg), reinterpret_cast<float4 *>(out));
    return check_launch("amav_cluster_max_raw");
}

extern "C" int amav_cluster_max_route(int64_t clusters, int channels, const float *x, const int64_t *members,
                                      const int64_t *seg, const float *grad_max, float *grad_x, void *stream) {
    AMAV_REQUIRE(clusters > 0 && channels > 0 && channels % 4 == 0, "amav_cluster_max_route: bad sizes clusters=%lld channels=%d",
                 (long long)clusters, channels);
    AMAV_REQUIRE(x && members && seg && grad_max && grad_x, "amav_cluster_max_route: NULL pointer");
    AMAV_REQUIRE(aligned16(x) && aligned16(grad_max) && aligned16(grad_x),
                 "amav_cluster_max_route: buffers must be 16-byte aligned");
    AMAV_REQUIRE((clusters + 3) / 4 <= 0x7fffffffLL, "amav_cluster_max_route: grid too large");
    cloud_norm::cluster_max_route_kernel<<<(unsigned)((clusters + 3) / 4), 256, 0, static_cast<hipStream_t>(stream)>>>(
        clusters, channels / 4, reinterpret_cast<const float4 *>(x), reinterpret_cast<const long long *>(members),
        reinterpret_cast<const long long *>(seg), reinterpret_cast<const float4 *>(grad_max),
        reinterpret_cast<float4 *>(grad_x));
    return check_launch("amav_cluster_max_route");
}
