// The tail of a training step for gfx950: the global L2 norm of all gradients with clip_grad_norm_'s coefficient, and
// torch.optim.Adam's update with that coefficient folded in (trainer_factory.py:44-45, lightning_model_wrapper.py:366-382,
// 642-658; include/amav.h has the contract, DESIGN.md section 4.20 the measurements).
//
// Multi-tensor by a device-resident table: the host cuts every tensor into chunks of at most `chunk` elements (a chunk
// never spans two tensors) and a work-group of 256 threads handles one chunk.  The grid is min(chunks, 2048) -- 8
// work-groups, 32 waves per CU, the guide's cap for a memory-bound kernel -- and work-group b takes chunks b, b + grid,
// ...: a fixed assignment, so the order of every sum depends on the tables alone.
//
//   sumsq_kernel        partial[c] = the sum of g^2 over chunk c.  A lane squares and adds in fp64 (the square of an fp32
//                       value is exact there), four running sums per lane (one per element of its 16 bytes), then a
//                       shuffle tree inside the wave and the 4 waves in order.  With n elements the relative error of
//                       the sum is below (n / 1024 + 11) 2^-53: nothing next to the 2^-24 of the final rounding, at any
//                       chunk size.  The fp64 work is 2 instructions per 4 bytes read and stays under the memory time.
//   norm_finish_kernel  one work-group: lane l adds partials l, l + 256, ... in order (fp64), the same tree, and lane 0
//                       writes norm and coefficient with ordinary vector stores.
//   adam_kernel         one pass: reads p, g, m, v, writes p, m, v (28 B per element); with `zero` also g (32 B).
//   pack_kernel         the data-parallel step's fourth launch: scale * g of every tensor into one bucket, which the
//                       collective then averages in place and the two kernels above read through a second table.
//   fingerprint_kernel  a wrap-around sum of the bit patterns of one of the four arrays (replicas still in step?), with
//                       fingerprint_finish_kernel in the two stages of the norm.
//
// 16-byte path: when the chunk's first element is 16-byte aligned in every array the kernel touches, lanes move float4;
// the up to 3 elements left over, and every chunk of a tensor that is not aligned (a view at an odd offset), go one
// float per lane.  Loads in flight: the Adam pass has 4 x 16 B per lane outstanding per iteration, 4 KiB per wave and
// 128 KiB per CU at its 8 waves per SIMD; the norm pass has one load per iteration and is unrolled by 4 for the same reason.
#include <climits>
#include <cmath>

#include "amav_common.h"

namespace amav {
namespace optimizer {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / kWave;
constexpr unsigned kGridMax = 2048;

// The tables hand the kernels addresses out of memory, which the compiler can only treat as generic (flat_load / flat_store,
// counted on two wait counters).  They are device memory by contract: say so, and the loops use global_load / global_store.
#define AMAV_GLOBAL __attribute__((address_space(1)))
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef AMAV_GLOBAL float *gfloat_p;
typedef AMAV_GLOBAL f32x4 *gfloat4_p;

struct Groups {
    amav_optim_group g[AMAV_OPTIM_MAX_GROUPS];
};

struct Piece {
    amav_optim_tensor t;
    int64_t start;
    int count;  // 0: nothing to do (a chunk that points outside its tensor is skipped)
};

__device__ __forceinline__ Piece piece_of(const amav_optim_tensor *__restrict__ tensors, int num_tensors,
                                          const amav_optim_chunk *__restrict__ chunks, int c, int chunk) {
    Piece p;
    const amav_optim_chunk ch = chunks[c];
    p.start = ch.start;
    p.count = 0;
    if (ch.tensor < 0 || ch.tensor >= num_tensors) return p;
    p.t = tensors[ch.tensor];
    if (ch.start < 0 || ch.start >= p.t.numel) return p;
    const int64_t left = p.t.numel - ch.start;
    p.count = left < chunk ? (int)left : chunk;
    return p;
}

template <typename... P>
__device__ __forceinline__ bool lanes_aligned16(const P *...p) {
    return ((... | reinterpret_cast<uintptr_t>(p)) & 15) == 0;
}

// the sum over the work-group in a fixed order, returned to every thread; `wave_sums` is free again on return
__device__ __forceinline__ double block_sum(double v, double *wave_sums) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
    if (threadIdx.x % kWave == 0) wave_sums[threadIdx.x / kWave] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) s += wave_sums[w];
    __syncthreads();
    return s;
}

__global__ __launch_bounds__(kBlock) void sumsq_kernel(const amav_optim_tensor *__restrict__ tensors, int num_tensors,
                                                       const amav_optim_chunk *__restrict__ chunks, int num_chunks,
                                                       int chunk, double *__restrict__ partial) {
    __shared__ double wave_sums[kWaves];
    for (int c = blockIdx.x; c < num_chunks; c += gridDim.x) {
        const Piece pc = piece_of(tensors, num_tensors, chunks, c, chunk);
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        if (pc.count > 0) {
            const gfloat_p g = (gfloat_p)(pc.t.grad + pc.start);
            int done = 0;
            if (lanes_aligned16(pc.t.grad + pc.start)) {
                const gfloat4_p g4 = (gfloat4_p)g;
                const int n4 = pc.count / 4;
#pragma unroll 4
                for (int i = threadIdx.x; i < n4; i += kBlock) {
                    const f32x4 x = g4[i];
                    a0 = fma((double)x.x, (double)x.x, a0);
                    a1 = fma((double)x.y, (double)x.y, a1);
                    a2 = fma((double)x.z, (double)x.z, a2);
                    a3 = fma((double)x.w, (double)x.w, a3);
                }
                done = n4 * 4;
            }
#pragma unroll 4
            for (int i = done + threadIdx.x; i < pc.count; i += kBlock) a0 = fma((double)g[i], (double)g[i], a0);
        }
        const double s = block_sum((a0 + a1) + (a2 + a3), wave_sums);
        if (threadIdx.x == 0) partial[c] = s;
    }
}

// one work-group; norm[0] = the norm, norm[1] = clip_grad_norm_'s coefficient
__global__ __launch_bounds__(kBlock) void norm_finish_kernel(int num_chunks, const double *__restrict__ partial,
                                                             float max_norm, float *__restrict__ norm) {
    __shared__ double wave_sums[kWaves];
    double a = 0.0;
    for (int c = threadIdx.x; c < num_chunks; c += kBlock) a += partial[c];
    const double s = block_sum(a, wave_sums);
    if (threadIdx.x == 0) {
        const float n = (float)sqrt(s);
        const float c = max_norm / (n + 1e-6f);
        norm[0] = n;
        norm[1] = c > 1.0f ? 1.0f : c;  // torch.clamp(max=1): a NaN stays a NaN
    }
}

__device__ __forceinline__ void adam_element(float &p, float g, float &m, float &v, float c, const amav_optim_group &h) {
    g *= c;
    if (h.weight_decay != 0.0f) g = fmaf(h.weight_decay, p, g);
    m = fmaf(h.one_minus_beta1, g - m, m);
    v = fmaf(h.one_minus_beta2 * g, g, h.beta2 * v);
    const float denom = fmaf(sqrtf(v), h.inv_sqrt_bc2, h.eps);
    p = fmaf(-h.step_size, m / denom, p);
}

template <bool kZero>
__global__ __launch_bounds__(kBlock) void adam_kernel(const amav_optim_tensor *__restrict__ tensors, int num_tensors,
                                                      const amav_optim_chunk *__restrict__ chunks, int num_chunks,
                                                      int chunk, Groups groups, int num_groups,
                                                      const float *__restrict__ coef) {
    const float c = coef ? *coef : 1.0f;
    for (int ci = blockIdx.x; ci < num_chunks; ci += gridDim.x) {
        const Piece pc = piece_of(tensors, num_tensors, chunks, ci, chunk);
        if (pc.count == 0 || pc.t.group < 0 || pc.t.group >= num_groups) continue;
        const amav_optim_group h = groups.g[pc.t.group];
        // the four arrays of a tensor never overlap (include/amav.h): loads of the next iteration may pass this one's stores
        const gfloat_p __restrict__ p = (gfloat_p)(pc.t.param + pc.start);
        const gfloat_p __restrict__ g = (gfloat_p)(pc.t.grad + pc.start);
        const gfloat_p __restrict__ m = (gfloat_p)(pc.t.exp_avg + pc.start);
        const gfloat_p __restrict__ v = (gfloat_p)(pc.t.exp_avg_sq + pc.start);
        int done = 0;
        if (lanes_aligned16(pc.t.param + pc.start, pc.t.grad + pc.start, pc.t.exp_avg + pc.start, pc.t.exp_avg_sq + pc.start)) {
            const gfloat4_p __restrict__ p4 = (gfloat4_p)p;
            const gfloat4_p __restrict__ g4 = (gfloat4_p)g;
            const gfloat4_p __restrict__ m4 = (gfloat4_p)m;
            const gfloat4_p __restrict__ v4 = (gfloat4_p)v;
            const int n4 = pc.count / 4;
            for (int i = threadIdx.x; i < n4; i += kBlock) {
                f32x4 pp = p4[i], mm = m4[i], vv = v4[i];
                const f32x4 gg = g4[i];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float pk = pp[k], mk = mm[k], vk = vv[k];
                    adam_element(pk, gg[k], mk, vk, c, h);
                    pp[k] = pk;
                    mm[k] = mk;
                    vv[k] = vk;
                }
                p4[i] = pp;
                m4[i] = mm;
                v4[i] = vv;
                if (kZero) g4[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            }
            done = n4 * 4;
        }
        for (int i = done + threadIdx.x; i < pc.count; i += kBlock) {
            float pp = p[i], mm = m[i], vv = v[i];
            adam_element(pp, g[i], mm, vv, c, h);
            p[i] = pp;
            m[i] = mm;
            v[i] = vv;
            if (kZero) g[i] = 0.0f;
        }
    }
}

// Data-parallel step: every gradient times `scale` into one bucket (the buffer the all-reduce runs on), tensor t at
// bucket[offsets[t]].  8 B per element (a read and a write), 12 with kZero; a tensor without a gradient costs the write.
// Only [offsets[t], offsets[t] + numel) is ever written: the gaps between tensors belong to the caller.
__device__ __forceinline__ f32x4 scaled(f32x4 x, float s) {  // one rounding per element, contracted with nothing
    return f32x4{__fmul_rn(x.x, s), __fmul_rn(x.y, s), __fmul_rn(x.z, s), __fmul_rn(x.w, s)};
}

template <bool kZero>
__global__ __launch_bounds__(kBlock) void pack_kernel(const amav_optim_tensor *__restrict__ tensors, int num_tensors,
                                                      const amav_optim_chunk *__restrict__ chunks, int num_chunks,
                                                      int chunk, const int64_t *__restrict__ offsets,
                                                      float *__restrict__ bucket, int64_t bucket_numel, float scale) {
    for (int ci = blockIdx.x; ci < num_chunks; ci += gridDim.x) {
        const Piece pc = piece_of(tensors, num_tensors, chunks, ci, chunk);
        if (pc.count == 0) continue;
        const int64_t off = offsets[chunks[ci].tensor];
        if (off < 0 || off > bucket_numel || pc.t.numel > bucket_numel - off) continue;
        float *dst = bucket + off + pc.start;
        const gfloat_p __restrict__ out = (gfloat_p)dst;
        const gfloat4_p __restrict__ out4 = (gfloat4_p)out;
        const int n4 = pc.count / 4;
        int done = 0;
        if (pc.t.grad == nullptr) {  // not used on this rank: zeros travel
            if (lanes_aligned16(dst)) {
                for (int i = threadIdx.x; i < n4; i += kBlock) out4[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                done = n4 * 4;
            }
            for (int i = done + threadIdx.x; i < pc.count; i += kBlock) out[i] = 0.0f;
            continue;
        }
        // source and destination never overlap (include/amav.h)
        const gfloat_p __restrict__ g = (gfloat_p)(pc.t.grad + pc.start);
        if (lanes_aligned16(pc.t.grad + pc.start, dst)) {
            const gfloat4_p __restrict__ g4 = (gfloat4_p)g;
            const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
            int i = threadIdx.x;
            // four loads per lane in flight before the first store: written out, since the compiler's own unrolling
            // keeps every load behind the store in front of it
            for (; i + 3 * kBlock < n4; i += 4 * kBlock) {
                const f32x4 x0 = g4[i], x1 = g4[i + kBlock], x2 = g4[i + 2 * kBlock], x3 = g4[i + 3 * kBlock];
                out4[i] = scaled(x0, scale);
                out4[i + kBlock] = scaled(x1, scale);
                out4[i + 2 * kBlock] = scaled(x2, scale);
                out4[i + 3 * kBlock] = scaled(x3, scale);
                if (kZero) g4[i] = g4[i + kBlock] = g4[i + 2 * kBlock] = g4[i + 3 * kBlock] = zero;
            }
            for (; i < n4; i += kBlock) {
                out4[i] = scaled(g4[i], scale);
                if (kZero) g4[i] = zero;
            }
            done = n4 * 4;
        }
#pragma unroll 4
        for (int i = done + threadIdx.x; i < pc.count; i += kBlock) {
            out[i] = __fmul_rn(g[i], scale);
            if (kZero) g[i] = 0.0f;
        }
    }
}

// the sum over the work-group, returned to every thread; modulo 2^64, so the order does not matter
__device__ __forceinline__ unsigned long long block_sum_u64(unsigned long long v, unsigned long long *wave_sums) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
    if (threadIdx.x % kWave == 0) wave_sums[threadIdx.x / kWave] = v;
    __syncthreads();
    unsigned long long s = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) s += wave_sums[w];
    __syncthreads();
    return s;
}

// partial[c] = the sum of the 32-bit patterns of chunk c's elements in array `which`, modulo 2^64
__global__ __launch_bounds__(kBlock) void fingerprint_kernel(const amav_optim_tensor *__restrict__ tensors, int num_tensors,
                                                             const amav_optim_chunk *__restrict__ chunks, int num_chunks,
                                                             int chunk, int which,
                                                             unsigned long long *__restrict__ partial) {
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    __shared__ unsigned long long wave_sums[kWaves];
    for (int c = blockIdx.x; c < num_chunks; c += gridDim.x) {
        const Piece pc = piece_of(tensors, num_tensors, chunks, c, chunk);
        unsigned long long a = 0;
        if (pc.count > 0) {
            const float *base = which == 0 ? pc.t.param : which == 1 ? pc.t.grad : which == 2 ? pc.t.exp_avg : pc.t.exp_avg_sq;
            if (base != nullptr) {
                const AMAV_GLOBAL unsigned *x = (const AMAV_GLOBAL unsigned *)(base + pc.start);
                int done = 0;
                if (lanes_aligned16(base + pc.start)) {
                    const AMAV_GLOBAL u32x4 *x4 = (const AMAV_GLOBAL u32x4 *)x;
                    const int n4 = pc.count / 4;
#pragma unroll 4
                    for (int i = threadIdx.x; i < n4; i += kBlock) {
                        const u32x4 q = x4[i];
                        a += ((unsigned long long)q.x + q.y) + ((unsigned long long)q.z + q.w);
                    }
                    done = n4 * 4;
                }
#pragma unroll 4
                for (int i = done + threadIdx.x; i < pc.count; i += kBlock) a += x[i];
            }
        }
        const unsigned long long s = block_sum_u64(a, wave_sums);
        if (threadIdx.x == 0) partial[c] = s;
    }
}

// one work-group; out[0] = the sum of the partials
__global__ __launch_bounds__(kBlock) void fingerprint_finish_kernel(int num_chunks,
                                                                    const unsigned long long *__restrict__ partial,
                                                                    unsigned long long *__restrict__ out) {
    __shared__ unsigned long long wave_sums[kWaves];
    unsigned long long a = 0;
    for (int c = threadIdx.x; c < num_chunks; c += kBlock) a += partial[c];
    const unsigned long long s = block_sum_u64(a, wave_sums);
    if (threadIdx.x == 0) out[0] = s;
}

// the checks the entry points share; `what` names the entry point.  *empty: nothing to launch over
inline int check_tables(const char *what, const void *tensors, int num_tensors, const void *chunks, int num_chunks,
                        int chunk, bool *empty) {
    AMAV_REQUIRE(num_tensors >= 0 && num_chunks >= 0, "%s: negative count num_tensors=%d num_chunks=%d", what, num_tensors,
                 num_chunks);
    AMAV_REQUIRE(chunk > 0, "%s: chunk=%d, expected a positive element count", what, chunk);
    *empty = num_tensors == 0 || num_chunks == 0;
    if (!*empty) AMAV_REQUIRE(tensors && chunks, "%s: NULL table (tensors / chunks)", what);
    return AMAV_OK;
}

inline unsigned grid_for(int num_chunks) { return (unsigned)num_chunks < kGridMax ? (unsigned)num_chunks : kGridMax; }

}  // namespace optimizer
}  // namespace amav

using namespace amav;
using namespace amav::optimizer;

extern "C" int amav_grad_norm_clip(const void *tensors_dev, int num_tensors, const void *chunks_dev, int num_chunks,
                                   int chunk, float max_norm, void *partial_dev, float *norm_dev, void *stream_) {
    bool empty;
    if (int rc = check_tables("amav_grad_norm_clip", tensors_dev, num_tensors, chunks_dev, num_chunks, chunk, &empty))
        return rc;
    AMAV_REQUIRE(norm_dev, "amav_grad_norm_clip: NULL pointer (norm)");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!empty) {
        AMAV_REQUIRE(partial_dev, "amav_grad_norm_clip: NULL pointer (partial)");
        sumsq_kernel<<<grid_for(num_chunks), kBlock, 0, stream>>>(static_cast<const amav_optim_tensor *>(tensors_dev),
                                                                  num_tensors,
                                                                  static_cast<const amav_optim_chunk *>(chunks_dev),
                                                                  num_chunks, chunk, static_cast<double *>(partial_dev));
        if (int rc = check_launch("amav_grad_norm_clip: sumsq_kernel")) return rc;
    }
    norm_finish_kernel<<<1, kBlock, 0, stream>>>(empty ? 0 : num_chunks, static_cast<const double *>(partial_dev), max_norm,
                                                 norm_dev);
    return check_launch("amav_grad_norm_clip: norm_finish_kernel");
}

extern "C" int amav_adam_step(const void *tensors_dev, int num_tensors, const void *chunks_dev, int num_chunks, int chunk,
                              const amav_optim_group *groups, int num_groups, const float *coef_dev, int zero_grad,
                              void *stream_) {
    bool empty;
    if (int rc = check_tables("amav_adam_step", tensors_dev, num_tensors, chunks_dev, num_chunks, chunk, &empty)) return rc;
    AMAV_REQUIRE(num_groups >= 0 && num_groups <= AMAV_OPTIM_MAX_GROUPS, "amav_adam_step: num_groups=%d outside 0..%d",
                 num_groups, AMAV_OPTIM_MAX_GROUPS);
    if (empty) return AMAV_OK;
    AMAV_REQUIRE(groups && num_groups > 0, "amav_adam_step: NULL or empty group array");
    Groups by_value = {};
    for (int i = 0; i < num_groups; ++i) by_value.g[i] = groups[i];
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const amav_optim_tensor *tensors = static_cast<const amav_optim_tensor *>(tensors_dev);
    const amav_optim_chunk *chunks = static_cast<const amav_optim_chunk *>(chunks_dev);
    if (zero_grad)
        adam_kernel<true><<<grid_for(num_chunks), kBlock, 0, stream>>>(tensors, num_tensors, chunks, num_chunks, chunk,
                                                                       by_value, num_groups, coef_dev);
    else
        adam_kernel<false><<<grid_for(num_chunks), kBlock, 0, stream>>>(tensors, num_tensors, chunks, num_chunks, chunk,
                                                                        by_value, num_groups, coef_dev);
    return check_launch("amav_adam_step: adam_kernel");
}

extern "C" int amav_grads_pack(const void *tensors_dev, int num_tensors, const void *chunks_dev, int num_chunks, int chunk,
                               const int64_t *offsets_dev, float *bucket_dev, int64_t bucket_numel, float scale,
                               int zero_source, void *stream_) {
    bool empty;
    if (int rc = check_tables("amav_grads_pack", tensors_dev, num_tensors, chunks_dev, num_chunks, chunk, &empty)) return rc;
    AMAV_REQUIRE(bucket_numel >= 0, "amav_grads_pack: bucket_numel=%lld is negative", (long long)bucket_numel);
    AMAV_REQUIRE(std::isfinite(scale), "amav_grads_pack: scale=%g is not finite", (double)scale);
    if (empty) return AMAV_OK;
    AMAV_REQUIRE(offsets_dev && bucket_dev, "amav_grads_pack: NULL pointer (offsets / bucket)");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const amav_optim_tensor *tensors = static_cast<const amav_optim_tensor *>(tensors_dev);
    const amav_optim_chunk *chunks = static_cast<const amav_optim_chunk *>(chunks_dev);
    if (zero_source)
        pack_kernel<true><<<grid_for(num_chunks), kBlock, 0, stream>>>(tensors, num_tensors, chunks, num_chunks, chunk,
                                                                       offsets_dev, bucket_dev, bucket_numel, scale);
    else
        pack_kernel<false><<<grid_for(num_chunks), kBlock, 0, stream>>>(tensors, num_tensors, chunks, num_chunks, chunk,
                                                                        offsets_dev, bucket_dev, bucket_numel, scale);
    return check_launch("amav_grads_pack: pack_kernel");
}

extern "C" int amav_tensors_fingerprint(const void *tensors_dev, int num_tensors, const void *chunks_dev, int num_chunks,
                                        int chunk, int which, void *partial_dev, void *out_dev, void *stream_) {
    bool empty;
    if (int rc = check_tables("amav_tensors_fingerprint", tensors_dev, num_tensors, chunks_dev, num_chunks, chunk, &empty))
        return rc;
    AMAV_REQUIRE(which >= 0 && which <= 3, "amav_tensors_fingerprint: which=%d outside 0..3", which);
    AMAV_REQUIRE(out_dev, "amav_tensors_fingerprint: NULL pointer (out)");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!empty) {
        AMAV_REQUIRE(partial_dev, "amav_tensors_fingerprint: NULL pointer (partial)");
        fingerprint_kernel<<<grid_for(num_chunks), kBlock, 0, stream>>>(
            static_cast<const amav_optim_tensor *>(tensors_dev), num_tensors, static_cast<const amav_optim_chunk *>(chunks_dev),
            num_chunks, chunk, which, static_cast<unsigned long long *>(partial_dev));
        if (int rc = check_launch("amav_tensors_fingerprint: fingerprint_kernel")) return rc;
    }
    fingerprint_finish_kernel<<<1, kBlock, 0, stream>>>(empty ? 0 : num_chunks,
                                                        static_cast<const unsigned long long *>(partial_dev),
                                                        static_cast<unsigned long long *>(out_dev));
    return check_launch("amav_tensors_fingerprint: fingerprint_finish_kernel");
}
