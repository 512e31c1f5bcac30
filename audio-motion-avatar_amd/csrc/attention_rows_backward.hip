// Backwards of the transformer step's row kernels (csrc/attention_rows.hip: geglu_kernel, add_layernorm_kernel) and the
// column sum their bias-like gradients need.  Memory-bound passes: float4 accesses, 64-bit row
// offsets, no atomics, no hidden allocation or synchronisation, kernel launches only (capturable).
//
// Summation order of every column sum here (amav_rows_colsum, and dweight / dbias of amav_add_layernorm_backward):
//   stage 1  the rows of a group are cut into consecutive chunks of kRowChunk = 16 rows (the last chunk of a group may be
//            shorter; a chunk never straddles a group); a chunk is summed in ascending row order, starting from its
//            first row (the LayerNorm backward's lanes start from +0, which differs for a sum of -0 alone);
//   stage 2  the chunk partials of a group are added in ascending chunk order, starting from the first partial.
// The order depends on (rows, rows_per_group) alone -- not on the grid, the clock or the batch around a group -- so two
// calls are bit-identical and a batch of groups equals the groups one by one.
#include <cmath>

#include "amav_common.h"
#include "wave_ops.h"

namespace amav {
namespace rows_bwd {

constexpr int kRowChunk = 16;

__device__ __forceinline__ float4 add4(const float4 &a, const float4 &b) {
    return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}

// stage 1: one thread per (chunk, column quad).  blockIdx.y = chunk over all groups, chunk = group * chunks_per_group + k.
__global__ __launch_bounds__(64) void colsum_chunks_kernel(long long rows_per_group, long long chunks_per_group, int cols4,
                                                           const float4 *__restrict__ x, long long x_row4,
                                                           float4 *__restrict__ parts) {
    const int q = blockIdx.x * 64 + threadIdx.x;
    if (q >= cols4) return;
    const long long chunk = blockIdx.y;
    const long long group = chunk / chunks_per_group, k = chunk - group * chunks_per_group;
    const long long first = k * kRowChunk;
    const long long left = rows_per_group - first;
    const int count = left < kRowChunk ? (int)left : kRowChunk;
    const float4 *src = x + (group * rows_per_group + first) * x_row4 + q;
    float4 acc;
    if (count == kRowChunk) {
        float4 v[kRowChunk];
#pragma unroll
        for (int r = 0; r < kRowChunk; ++r) v[r] = src[r * x_row4];
        acc = v[0];
#pragma unroll
        for (int r = 1; r < kRowChunk; ++r) acc = add4(acc, v[r]);
    } else {
        acc = src[0];
        for (int r = 1; r < count; ++r) acc = add4(acc, src[r * x_row4]);
    }
    parts[chunk * cols4 + q] = acc;
}

// stage 2: one thread per (group, column quad) of parts [groups, chunks_per_group, cols4].  Quads below `split4` go to
// out_a [groups, split4], the others to out_b [groups, cols4 - split4] (dweight | dbias of the LayerNorm backward).
__global__ __launch_bounds__(64) void colsum_parts_kernel(long long chunks_per_group, int cols4, int split4,
                                                          const float4 *__restrict__ parts, float4 *__restrict__ out_a,
                                                          float4 *__restrict__ out_b) {
    const int q = blockIdx.x * 64 + threadIdx.x;
    if (q >= cols4) return;
    const long long group = blockIdx.y;
    const float4 *src = parts + group * chunks_per_group * cols4 + q;
    float4 acc = src[0];
    long long k = 1;
    for (; k + 8 <= chunks_per_group; k += 8) {
        float4 v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = src[(k + j) * cols4];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc = add4(acc, v[j]);
    }
    for (; k < chunks_per_group; ++k) acc = add4(acc, src[k * cols4]);
    if (q < split4)
        out_a[group * split4 + q] = acc;
    else
        out_b[group * (cols4 - split4) + (q - split4)] = acc;
}

// With h = proj_h + b_h, g = proj_g + b_g:  d proj_h = dout gelu(g),  d proj_g = dout h (Phi(g) + g phi(g)); exact erf,
// gelu(g) by geglu_kernel's expression.  A saturated gate gives exp(-g^2 / 2) = 0 and Phi = 0 or 1: finite results.
__global__ __launch_bounds__(256) void geglu_backward_kernel(long long quads, int inner4, const float4 *__restrict__ in,
                                                             long long in_row4, const float4 *__restrict__ bias,
                                                             const float4 *__restrict__ dout, float4 *__restrict__ dproj,
                                                             long long dproj_row4) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= quads) return;
    const long long row = i / inner4;
    const int col = (int)(i - row * inner4);
    float4 h = in[row * in_row4 + col], g = in[row * in_row4 + inner4 + col];
    if (bias) {
        h = add4(h, bias[col]);
        g = add4(g, bias[inner4 + col]);
    }
    const float4 d = dout[i];
    float dh[4], dg[4];
    const float hv[4] = {h.x, h.y, h.z, h.w}, gv[4] = {g.x, g.y, g.z, g.w}, dv[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float x = gv[j];
        const float e = erff(x * 0.70710678118654752440f);
        const float gelu = 0.5f * x * (1.0f + e);
        const float cdf = 0.5f * (1.0f + e);
        const float pdf = expf(-0.5f * x * x) * 0.39894228040143267794f;
        dh[j] = dv[j] * gelu;
        dg[j] = dv[j] * hv[j] * (cdf + x * pdf);
    }
    dproj[row * dproj_row4 + col] = make_float4(dh[0], dh[1], dh[2], dh[3]);
    dproj[row * dproj_row4 + inner4 + col] = make_float4(dg[0], dg[1], dg[2], dg[3]);
}

// One wave per chunk of kRowChunk rows, a row in registers (as add_layernorm_kernel: lane l holds float4 l + 64 v).  mean
// and rstd are recomputed with the forward's two-pass expressions, in its operation order.  With xhat = (h - mean) rstd
// and t = dnorm * weight:
//   dh = dhidden_out + rstd (t - mean_c(t) - xhat mean_c(t xhat))
// and the lane adds dnorm * xhat and dnorm of its columns over the chunk's rows in ascending order (stage 1 of the
// column sums) into parts [chunks, 2, dim]: dweight's partial, then dbias's.
template <int kVec>
__global__ __launch_bounds__(256) void add_layernorm_backward_kernel(long long rows, const float4 *__restrict__ h,
                                                                     const float4 *__restrict__ w, float eps,
                                                                     const float4 *__restrict__ dnorm,
                                                                     const float4 *__restrict__ dh_out,
                                                                     float4 *__restrict__ dh, float4 *__restrict__ parts) {
    const long long chunk = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const long long first = chunk * kRowChunk;
    if (first >= rows) return;
    const long long last = first + kRowChunk < rows ? first + kRowChunk : rows;
    constexpr int kRow4 = 64 * kVec;
    constexpr float kInv = 1.0f / (256.0f * kVec);
    float4 wv[kVec], dw[kVec], db[kVec];
#pragma unroll
    for (int v = 0; v < kVec; ++v) {
        wv[v] = w[lane + 64 * v];
        dw[v] = db[v] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (long long row = first; row < last; ++row) {
        float4 x[kVec], dn[kVec], up[kVec];
        float sum = 0.f;
#pragma unroll
        for (int v = 0; v < kVec; ++v) {
            const long long at = row * kRow4 + lane + 64 * v;
            x[v] = h[at];
            dn[v] = dnorm ? dnorm[at] : make_float4(0.f, 0.f, 0.f, 0.f);
            up[v] = dh_out ? dh_out[at] : make_float4(0.f, 0.f, 0.f, 0.f);
            sum += (x[v].x + x[v].y) + (x[v].z + x[v].w);
        }
        const float mean = wave_sum(sum) * kInv;
        float var = 0.f;
#pragma unroll
        for (int v = 0; v < kVec; ++v) {
            const float dx = x[v].x - mean, dy = x[v].y - mean, dz = x[v].z - mean, dw_ = x[v].w - mean;
            var += (dx * dx + dy * dy) + (dz * dz + dw_ * dw_);
        }
        const float rstd = 1.0f / sqrtf(wave_sum(var) * kInv + eps);
        if (!dnorm) {  // wave-uniform: the LayerNorm part is zero, dweight / dbias partials stay +0
#pragma unroll
            for (int v = 0; v < kVec; ++v) dh[row * kRow4 + lane + 64 * v] = up[v];
            continue;
        }
        float4 t[kVec];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int v = 0; v < kVec; ++v) {
            x[v] = make_float4((x[v].x - mean) * rstd, (x[v].y - mean) * rstd, (x[v].z - mean) * rstd,
                               (x[v].w - mean) * rstd);  // xhat
            t[v] = make_float4(dn[v].x * wv[v].x, dn[v].y * wv[v].y, dn[v].z * wv[v].z, dn[v].w * wv[v].w);
            s1 += (t[v].x + t[v].y) + (t[v].z + t[v].w);
            s2 += (t[v].x * x[v].x + t[v].y * x[v].y) + (t[v].z * x[v].z + t[v].w * x[v].w);
            dw[v] = make_float4(dw[v].x + dn[v].x * x[v].x, dw[v].y + dn[v].y * x[v].y, dw[v].z + dn[v].z * x[v].z,
                                dw[v].w + dn[v].w * x[v].w);
            db[v] = add4(db[v], dn[v]);
        }
        const float m1 = wave_sum(s1) * kInv, m2 = wave_sum(s2) * kInv;
#pragma unroll
        for (int v = 0; v < kVec; ++v) {
            dh[row * kRow4 + lane + 64 * v] =
                make_float4(up[v].x + rstd * (t[v].x - m1 - x[v].x * m2), up[v].y + rstd * (t[v].y - m1 - x[v].y * m2),
                            up[v].z + rstd * (t[v].z - m1 - x[v].z * m2), up[v].w + rstd * (t[v].w - m1 - x[v].w * m2));
        }
    }
#pragma unroll
    for (int v = 0; v < kVec; ++v) {
        parts[(chunk * 2 + 0) * kRow4 + lane + 64 * v] = dw[v];
        parts[(chunk * 2 + 1) * kRow4 + lane + 64 * v] = db[v];
    }
}

inline long long chunks_of(long long rows) { return (rows + kRowChunk - 1) / kRowChunk; }

}  // namespace rows_bwd
}  // namespace amav

using namespace amav;

extern "C" size_t amav_rows_colsum_workspace_bytes(int64_t rows, int cols, int64_t rows_per_group) {
    if (rows <= 0 || cols <= 0 || cols % 4 || rows_per_group <= 0 || rows % rows_per_group) return 0;
    const long long chunks = (rows / rows_per_group) * rows_bwd::chunks_of(rows_per_group);
    return align_up((size_t)chunks * cols * sizeof(float), 256);
}

extern "C" int amav_rows_colsum(int64_t rows, int cols, const float *x, int64_t x_row_stride, int64_t rows_per_group,
                                float *out, void *workspace, size_t workspace_bytes, void *stream_) {
    AMAV_REQUIRE(rows > 0 && cols > 0 && cols % 4 == 0, "amav_rows_colsum: rows=%lld cols=%d (cols must be a multiple of 4)",
                 (long long)rows, cols);
    AMAV_REQUIRE(rows_per_group > 0 && rows % rows_per_group == 0,
                 "amav_rows_colsum: rows=%lld is not a multiple of rows_per_group=%lld", (long long)rows,
                 (long long)rows_per_group);
    AMAV_REQUIRE(x && out, "amav_rows_colsum: NULL pointer");
    AMAV_REQUIRE(x_row_stride >= cols && x_row_stride % 4 == 0, "amav_rows_colsum: bad row stride");
    AMAV_REQUIRE(aligned16(x, out, workspace), "amav_rows_colsum: buffers must be 16-byte aligned");
    const long long groups = rows / rows_per_group, per_group = rows_bwd::chunks_of(rows_per_group);
    AMAV_REQUIRE(groups <= 65535 && groups * per_group <= 65535, "amav_rows_colsum: grid too large");
    const size_t need = amav_rows_colsum_workspace_bytes(rows, cols, rows_per_group);
    if (workspace == nullptr || workspace_bytes < need)
        return fail(AMAV_ERR_WORKSPACE, "amav_rows_colsum: workspace %zu < required %zu", workspace_bytes, need);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int cols4 = cols / 4;
    const unsigned gx = (unsigned)((cols4 + 63) / 64);
    float4 *parts = static_cast<float4 *>(workspace);
    rows_bwd::colsum_chunks_kernel<<<dim3(gx, (unsigned)(groups * per_group)), 64, 0, stream>>>(
        rows_per_group, per_group, cols4, reinterpret_cast<const float4 *>(x), x_row_stride / 4, parts);
    rows_bwd::colsum_parts_kernel<<<dim3(gx, (unsigned)groups), 64, 0, stream>>>(per_group, cols4, cols4, parts,
                                                                               reinterpret_cast<float4 *>(out), nullptr);
    return check_launch("amav_rows_colsum");
}

extern "C" int amav_geglu_backward(int64_t rows, int inner, const float *proj, int64_t proj_row_stride, const float *bias,
                                   const float *dout, float *dproj, int64_t dproj_row_stride, void *stream) {
    AMAV_REQUIRE(rows > 0 && inner > 0 && inner % 4 == 0, "amav_geglu_backward: bad sizes rows=%lld inner=%d",
                 (long long)rows, inner);
    AMAV_REQUIRE(proj && dout && dproj, "amav_geglu_backward: NULL pointer");
    AMAV_REQUIRE(proj_row_stride >= 2LL * inner && proj_row_stride % 4 == 0 && dproj_row_stride >= 2LL * inner &&
                     dproj_row_stride % 4 == 0,
                 "amav_geglu_backward: bad row stride");
    AMAV_REQUIRE(aligned16(proj, bias, dout, dproj), "amav_geglu_backward: buffers must be 16-byte aligned");
    const long long quads = rows * (inner / 4);
    AMAV_REQUIRE((quads + 255) / 256 <= 0x7fffffffLL, "amav_geglu_backward: grid too large");
    rows_bwd::geglu_backward_kernel<<<(unsigned)((quads + 255) / 256), 256, 0, static_cast<hipStream_t>(stream)>>>(
        quads, inner / 4, reinterpret_cast<const float4 *>(proj), proj_row_stride / 4,
        reinterpret_cast<const float4 *>(bias), reinterpret_cast<const float4 *>(dout), reinterpret_cast<float4 *>(dproj),
        dproj_row_stride / 4);
    return check_launch("amav_geglu_backward");
}

extern "C" size_t amav_add_layernorm_backward_workspace_bytes(int64_t rows, int dim) {
    if (rows <= 0 || !(dim == 256 || dim == 512 || dim == 768 || dim == 1024)) return 0;
    return align_up((size_t)rows_bwd::chunks_of(rows) * 2 * dim * sizeof(float), 256);
}

extern "C" int amav_add_layernorm_backward(int64_t rows, int dim, const float *h, const float *weight, float eps,
                                           const float *dnorm, const float *dhidden_out, float *dh, float *dweight,
                                           float *dbias, void *workspace, size_t workspace_bytes, void *stream_) {
    AMAV_REQUIRE(rows > 0 && (dim == 256 || dim == 512 || dim == 768 || dim == 1024),
                 "amav_add_layernorm_backward: rows=%lld dim=%d (dim must be 256, 512, 768 or 1024)", (long long)rows, dim);
    AMAV_REQUIRE(h && weight && dh && dweight && dbias, "amav_add_layernorm_backward: NULL pointer");
    AMAV_REQUIRE(aligned16(h, weight, dnorm, dhidden_out, dh, dweight, dbias, workspace),
                 "amav_add_layernorm_backward: buffers must be 16-byte aligned");
    const size_t need = amav_add_layernorm_backward_workspace_bytes(rows, dim);
    if (workspace == nullptr || workspace_bytes < need)
        return fail(AMAV_ERR_WORKSPACE, "amav_add_layernorm_backward: workspace %zu < required %zu", workspace_bytes, need);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const long long chunks = rows_bwd::chunks_of(rows);
    AMAV_REQUIRE((chunks + 3) / 4 <= 0x7fffffffLL, "amav_add_layernorm_backward: grid too large");
    const unsigned grid = (unsigned)((chunks + 3) / 4);
    auto p4 = [](const float *p) { return reinterpret_cast<const float4 *>(p); };
    float4 *parts = static_cast<float4 *>(workspace);
#define AMAV_LNB_LAUNCH(V)                                                                                              \
    rows_bwd::add_layernorm_backward_kernel<V><<<grid, 256, 0, stream>>>(rows, p4(h), p4(weight), eps, p4(dnorm),        \
                                                                         p4(dhidden_out), reinterpret_cast<float4 *>(dh), \
                                                                         parts)
    if (dim == 256) AMAV_LNB_LAUNCH(1);
    else if (dim == 512) AMAV_LNB_LAUNCH(2);
    else if (dim == 768) AMAV_LNB_LAUNCH(3);
    else AMAV_LNB_LAUNCH(4);
#undef AMAV_LNB_LAUNCH
    // stage 2 over parts [1 group, chunks, 2 * dim]: the first dim columns are dweight's partials, the rest dbias's
    const int cols4 = 2 * dim / 4;
    rows_bwd::colsum_parts_kernel<<<dim3((unsigned)((cols4 + 63) / 64), 1), 64, 0, stream>>>(
        chunks, cols4, dim / 4, parts, reinterpret_cast<float4 *>(dweight), reinterpret_cast<float4 *>(dbias));
    return check_launch("amav_add_layernorm_backward");
}
