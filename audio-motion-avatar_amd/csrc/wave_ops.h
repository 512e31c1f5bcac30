// Wave-level reductions and scans of the kernels (device code only; 64-lane waves, all lanes active unless said
// otherwise).  Two families that must not be mistaken for each other, because float sums differ in their low bits:
//   wave_sum / wave_max / wave_min / group_sum / wave_inclusive_sum   on __shfl_xor / __shfl_up (ds_bpermute)
//   wave_sum_rows / wave_min_u32 / wave_max_u32 / wave_inclusive_sum_u32   on DPP row operations, no address registers
#pragma once
#include <hip/hip_runtime.h>

#include "amav_common.h"

namespace amav {

// Orders this wave's LDS traffic.  LDS operations of one wave execute in order; this only stops the compiler from
// moving them.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- xor butterfly: partner distances 32, 16, 8, 4, 2, 1, in that order; EVERY lane receives the result ----------
// (float, double, int, unsigned, 64-bit integers.)  A float sum is v + partner at every step, so all lanes also hold
// the same bits.
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}
template <typename T>  // integers
__device__ __forceinline__ T wave_max(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}
template <typename T>  // integers
__device__ __forceinline__ T wave_min(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}
// Sum over every aligned group of G lanes (G a power of two): distances G / 2, .., 1; every lane of a group receives
// its group's sum.
template <int G, typename T>
__device__ __forceinline__ T group_sum(T v) {
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Inclusive prefix sum over the wave (int, long long): lane i receives v_0 + .. + v_i; distances 1, 2, .., 32.
template <typename T>
__device__ __forceinline__ T wave_inclusive_sum(T v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T up = __shfl_up(v, o, 64);
        if (lane >= o) v += up;
    }
    return v;
}

// ---- the same WITHOUT ds_bpermute -----------------------------------------------------------------------------------
// Wave-wide min / max / sum / inclusive sum on DPP: __shfl_xor / __shfl_up keep one address register per
// distance alive (the compiler hoists (lane ^ o) << 2 out of the rasterizer's tile loop: thirteen registers), and what
// did not fit was spilled -- reloaded per tile as scratch loads, i.e. vector-memory operations whose s_waitcnt vmcnt(0)
// also drains every background store issued before them.  DPP permutes inside rows of 16 lanes need no address; the
// four rows are combined on the scalar unit (the results are wave-uniform anyway).
template <int kCtrl>
__device__ __forceinline__ unsigned dpp_permute(unsigned v) {  // every lane has a source for these controls
    return (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, kCtrl, 0xf, 0xf, false);
}
__device__ __forceinline__ unsigned wave_min_u32(unsigned v) {  // all 64 lanes active
    v = min(v, dpp_permute<0xB1>(v));   // quad_perm [1,0,3,2]
    v = min(v, dpp_permute<0x4E>(v));   // quad_perm [2,3,0,1]
    v = min(v, dpp_permute<0x141>(v));  // row_half_mirror
    v = min(v, dpp_permute<0x140>(v));  // row_mirror: every lane of a row holds the row's minimum
    const unsigned a = __builtin_amdgcn_readlane((int)v, 0), b = __builtin_amdgcn_readlane((int)v, 16);
    const unsigned c = __builtin_amdgcn_readlane((int)v, 32), d = __builtin_amdgcn_readlane((int)v, 48);
    return min(min(a, b), min(c, d));
}
__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
    v = max(v, dpp_permute<0xB1>(v));
    v = max(v, dpp_permute<0x4E>(v));
    v = max(v, dpp_permute<0x141>(v));
    v = max(v, dpp_permute<0x140>(v));
    const unsigned a = __builtin_amdgcn_readlane((int)v, 0), b = __builtin_amdgcn_readlane((int)v, 16);
    const unsigned c = __builtin_amdgcn_readlane((int)v, 32), d = __builtin_amdgcn_readlane((int)v, 48);
    return max(max(a, b), max(c, d));
}
template <int kShift>
__device__ __forceinline__ unsigned dpp_row_shr(unsigned v) {  // lane i of a row <- lane i - kShift, 0 at the row's start
    return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x110 + kShift, 0xf, 0xf, false);
}
__device__ __forceinline__ unsigned wave_inclusive_sum_u32(unsigned v, int lane) {  // all 64 lanes active
    v += dpp_row_shr<1>(v);
    v += dpp_row_shr<2>(v);
    v += dpp_row_shr<4>(v);
    v += dpp_row_shr<8>(v);  // inclusive sums inside every row of 16
    const unsigned r0 = __builtin_amdgcn_readlane((int)v, 15), r1 = __builtin_amdgcn_readlane((int)v, 31);
    const unsigned r2 = __builtin_amdgcn_readlane((int)v, 47);
    return v + (lane >= 16 ? r0 : 0u) + (lane >= 32 ? r1 : 0u) + (lane >= 48 ? r2 : 0u);
}
// Float wave sum in ITS OWN fixed order, not wave_sum's (all 64 lanes active): row_shr 1, 2, 4, 8 inside each row of
// 16, then the four row totals as (r0 + r1) + (r2 + r3).  Wave-uniform.
template <int kShift>
__device__ __forceinline__ float row_shr_add(float v) {
    return v + __uint_as_float(dpp_row_shr<kShift>(__float_as_uint(v)));
}
__device__ __forceinline__ float wave_sum_rows(float v) {
    v = row_shr_add<1>(v);
    v = row_shr_add<2>(v);
    v = row_shr_add<4>(v);
    v = row_shr_add<8>(v);  // lane 15 of every row holds the row's sum
    const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 15));
    const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 31));
    const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 47));
    const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
    return (r0 + r1) + (r2 + r3);
}

// ---- tail of a magnitude sweep (blocks of 256 threads = 4 waves, every thread calls it once) ----------------------
// Per value x: the block's largest m[x] -> atomicMax(out + x), one atomic per block and word (same-address atomics
// serialise in L2: ~10 ns each).  The values are non-negative floats, which order like their bit patterns: an integer
// maximum, order-independent.
template <int N>
__device__ __forceinline__ void block_absmax_publish(const float (&m)[N], unsigned *out) {
    __shared__ float wm[4][N];
    float r[N];
#pragma unroll
    for (int x = 0; x < N; ++x) r[x] = wave_max(m[x]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int x = 0; x < N; ++x) wm[threadIdx.x >> 6][x] = r[x];
    }
    __syncthreads();
    if (threadIdx.x < N)
        atomicMax(out + threadIdx.x, __float_as_uint(fmaxf(fmaxf(wm[0][threadIdx.x], wm[1][threadIdx.x]),
                                                           fmaxf(wm[2][threadIdx.x], wm[3][threadIdx.x]))));
}
__device__ __forceinline__ void block_absmax_publish(float m, unsigned *out) {
    const float one[1] = {m};
    block_absmax_publish<1>(one, out);
}

}  // namespace amav
