// Backward of the point refiner's sparse / serialised operators (csrc/cloud.hip).
//
//   amav_subm_pair_sum_csr        the transposed ordered sum of the submanifold convolution: dfeat[j] = sum over the pairs
//                                 whose SOURCE row is j (CSR by source row, ascending pair index) of the per-pair
//                                 products g[dst(p)] W[tap(p)]^T, which amav_subm_pair_gemm computes with pair_dst as its
//                                 gather index and the per-tap transposed weights
//   amav_subm_pair_wgrad          dW[t] = sum over the pairs p of tap t of feat[src(p)]^T (x) g[dst(p)]: both operands
//                                 gathered into LDS, the reduction dimension is the tap's pairs, split over chunks of
//                                 pairs whose partial matrices a second pass adds in slice order
//   amav_patch_attention_backward the flash-attention-2 backward of attention_backward_core.h through `order` /
//                                 `patch_desc`, probabilities recomputed from the row log-sum-exp of
//                                 amav_patch_attention_lse.  A row is a query of exactly one patch (dQ is written once);
//                                 it can be a key of two (its own and, as a borrowed slot, the cloud's last incomplete
//                                 patch): the borrowed part is staged and added after the own part by a fixed pass
//   amav_cluster_max_backward     gelu(max * scale + shift): the whole gradient to the first member, in segment order, that
//                                 attains the maximum; every row of dx written once
//   amav_cluster_sum              out[j] = sum of x[members[r]] over segment j in segment order: the backward of the
//                                 up[cluster] gather of amav_unpool_merge
// No atomics, every sum in a fixed order: a call is deterministic bit for bit.  Products on v_mfma_f32_32x32x2_f32 (exact
// fp32 products, fp32 sums).  MFMA layouts: csrc/attention_backward_core.h.
#include <climits>
#include <cmath>

#include "attention_backward_core.h"
#include "gelu.h"

namespace amav {
namespace cloud_bwd {

using attn_bwd::acc_row;

constexpr int kWgradChunk = 128;  // granularity of a split-K slice of amav_subm_pair_wgrad, in pairs

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
// The kernels of attention_backward_core.h through `order` / `patch_desc` (slots and the borrowed tail: cloud.hip,
// patch_attention_kernel).  A patch has K key slots, of which the first `own` are its queries; slot j >= own is borrowed:
// row order[first + j - K] of the patch before.  Rows are [n, 3 C] of qkv / dqkv and [n, C] of out / dout, lse and delta
// are [n, heads], all in point order.
struct PatchRows {
    const float *qkv;
    const long long *order;
    const int4 *desc;
    const float *out, *dout, *lse;
    float *delta, *dqkv, *stage;  // stage [n, 2 C]: dK | dV that a borrowed slot adds to its point
    long long row_heads;          // n * heads
    int C, heads, D;
    int first, K, own;            // of the bound patch (bind)

    __device__ long long delta_rows() const { return row_heads; }
    // out and dout are contiguous, so pair r = row * heads + head starts at r * D
    __device__ void delta_io(long long r, const float *&o, const float *&g, float *&d) const {
        o = out + r * D, g = dout + r * D, d = delta + r;
    }
    __device__ void bind(int head, int patch) {
        const int4 pd = desc[patch];
        first = pd.x, K = pd.y, own = pd.z;
        qkv += head * D, dout += head * D, dqkv += head * D, stage += head * D;
        lse += head, delta += head;
    }
    __device__ int keys() const { return K; }
    __device__ int queries() const { return own; }
    __device__ long long slot_row(int j) const { return order[first + j - (j >= own ? K : 0)]; }
    __device__ const float *q_row(int i) const { return qkv + slot_row(i) * 3 * C; }
    __device__ const float *k_row(int j) const { return q_row(j) + C; }
    __device__ const float *v_row(int j) const { return q_row(j) + 2 * C; }
    __device__ const float *dout_row(int i) const { return dout + slot_row(i) * C; }
    __device__ float lse_at(int i) const { return lse[slot_row(i) * heads]; }
    __device__ float delta_at(int i) const { return delta[slot_row(i) * heads]; }
    __device__ float *dq_row(int i) const { return dqkv + slot_row(i) * 3 * C; }
    // an own slot writes the gradient row, a borrowed slot the staging row of the same point
    __device__ float *dk_row(int j) const {
        const long long row = slot_row(j);
        return j < own ? dqkv + row * 3 * C + C : stage + row * 2 * C;
    }
    __device__ float *dv_row(int j) const { return dk_row(j) + C; }
};

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
    const cloud_bwd::PatchRows rows = {qkv, ord, pd, out, grad_out, lse, delta, grad_qkv, stage, (long long)n * heads,
                                       C, heads, head_dim, 0, 0, 0};
#define AMAV_PA_BWD(D_)                                                                                          \
    {                                                                                                            \
        attn_bwd::delta_kernel<D_><<<blocks_for(rows.row_heads * (D_ / 4)), 256, 0, stream>>>(rows);             \
        attn_bwd::dkdv_kernel<D_><<<grid, 256, 0, stream>>>(rows, scale);                                        \
        attn_bwd::dq_kernel<D_><<<grid, 256, 0, stream>>>(rows, scale);                                          \
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
