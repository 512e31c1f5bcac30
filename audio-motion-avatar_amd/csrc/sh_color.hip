// amav_sh_colors / amav_sh_colors_backward: view-dependent colours from spherical-harmonic coefficients, the SH branch of
// the reference's render_one (src/models/renderer.py:540-545) for all frames of a shard in one launch.  The arithmetic
// is sh_eval.h's; this file is the data movement.
//
// Lanes run along the Gaussians, one wave per block, one frame row per block-row.  A lane needs its own record of
// rec = 3 * num_coeffs floats (192 B at 16 coefficients): read lane by lane that is a gather of `rec` dwords at a stride
// of `rec` dwords.  Where the records of a block are one contiguous run (element stride = rec) the wave instead copies
// the run of 64 records into LDS with 16-byte loads (dword loads when the run does not start on a 16-byte boundary) and
// each lane reads its record from there; the backward writes grad_sh the same way in reverse.
//
// LDS stride: record r lives at tile[r * S], S = rec | 1 (rec itself when it is odd, rec + 1 otherwise).  The lanes read
// coefficient j of their records with one ds_read_b32, whose 32 banks serve each 32-lane half: lane l touches bank
// (l * S + j) mod 32, and an odd S makes l -> l * S a bijection mod 32, so no two lanes of a half meet on a bank.  An
// even S = 2^t * odd would be a 2^t-way conflict (48 dwords, the degree-3 record: 16-way).  The copy side writes dwords
// at a lane stride of 4, a 4-way conflict on ds_write_b32 (2x its conflict-free cost); with rec odd the tile equals the
// global run and the copy is ds_write_b128.  Both are far from what limits the kernel, the memory traffic.
//
// A block whose records are not contiguous (a padded element stride), or whose tile would not fit into 64 KiB, reads
// and writes lane by lane; the results are the same bits either way (the same sh_eval.h calls on the same values).
// No workspace, no atomics, no host synchronisation: every output element is written once by one lane.
#include <climits>
#include <type_traits>

#include "amav_common.h"
#include "sh_eval.h"

namespace amav {
namespace sh {

constexpr int kLdsBytes = 64 * 1024;
constexpr unsigned kGridMax = 65535;

// how the 64-record tile of a block is laid out; stride = 0: no tile (lane-by-lane accesses only)
struct Tile {
    int rec;     // floats per record = 3 * num_coeffs
    int stride;  // floats between records in LDS: rec | 1
    int q, m;    // 256 / rec, 256 % rec: how (record, offset) advance when a lane steps 64 float4 ahead
};

__device__ __forceinline__ const float *at(const amav_attr &a, int f, int i) {
    return a.ptr + (long long)f * a.frame_stride + (long long)i * a.elem_stride;
}

__device__ __forceinline__ bool aligned16_dev(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// tile <- run[0 .. total): total = (records of this block) * rec floats, contiguous in global memory
__device__ __forceinline__ void stage_in(float *tile, const float *run, int total, const Tile &t, int lane) {
    const int pad = t.stride - t.rec;
    if (!aligned16_dev(run)) {  // dword loads, still coalesced
        int idx = lane, r = idx / t.rec, k = idx - r * t.rec;
        const int q = 64 / t.rec, m = 64 - q * t.rec;
        for (; idx < total; idx += 64) {
            tile[idx + pad * r] = run[idx];
            r += q, k += m;
            if (k >= t.rec) k -= t.rec, ++r;
        }
        return;
    }
    const int vec = total >> 2;
    const float4 *run4 = reinterpret_cast<const float4 *>(run);
    // kAhead loads are issued before the first of them is waited for: with one load per trip a wave has 1 KiB in flight
    // and the CU's dozen waves together too little to cover the memory latency
    constexpr int kAhead = 4;
    float4 *tile4 = reinterpret_cast<float4 *>(tile);
    int idx = 4 * lane, r = idx / t.rec, k = idx - r * t.rec;
    for (int i = lane; i < vec; i += 64 * kAhead) {
        float4 v[kAhead];
#pragma unroll
        for (int u = 0; u < kAhead; ++u)
            if (i + 64 * u < vec) v[u] = run4[i + 64 * u];
#pragma unroll
        for (int u = 0; u < kAhead; ++u) {
            if (i + 64 * u < vec) {
                if (pad == 0) {
                    tile4[i + 64 * u] = v[u];
                } else {
                    const float e[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
                    for (int j = 0; j < 4; ++j) tile[idx + j + r + (k + j >= t.rec)] = e[j];  // rec >= 3: at most one wrap
                }
            }
            idx += 256, r += t.q, k += t.m;
            if (k >= t.rec) k -= t.rec, ++r;
        }
    }
    idx = (vec << 2) + lane;  // the last total % 4 floats
    if (lane < 4 && idx < total) tile[idx + pad * (idx / t.rec)] = run[idx];
}

// run[0 .. total) <- tile, the reverse of stage_in
__device__ __forceinline__ void stage_out(const float *tile, float *run, int total, const Tile &t, int lane) {
    const int pad = t.stride - t.rec;
    if (!aligned16_dev(run)) {
        int idx = lane, r = idx / t.rec, k = idx - r * t.rec;
        const int q = 64 / t.rec, m = 64 - q * t.rec;
        for (; idx < total; idx += 64) {
            run[idx] = tile[idx + pad * r];
            r += q, k += m;
            if (k >= t.rec) k -= t.rec, ++r;
        }
        return;
    }
    const int vec = total >> 2;
    float4 *run4 = reinterpret_cast<float4 *>(run);
    if (pad == 0) {
        const float4 *tile4 = reinterpret_cast<const float4 *>(tile);
        for (int i = lane; i < vec; i += 64) run4[i] = tile4[i];
    } else {
        int idx = 4 * lane, r = idx / t.rec, k = idx - r * t.rec;
        for (int i = lane; i < vec; i += 64) {
            float e[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) e[j] = tile[idx + j + r + (k + j >= t.rec)];
            run4[i] = make_float4(e[0], e[1], e[2], e[3]);
            idx += 256, r += t.q, k += t.m;
            if (k >= t.rec) k -= t.rec, ++r;
        }
    }
    const int idx = (vec << 2) + lane;
    if (lane < 4 && idx < total) run[idx] = tile[idx + pad * (idx / t.rec)];
}

template <int D>
__global__ __launch_bounds__(kWave) void sh_colors_kernel(int F, int N, amav_attr means3d, amav_attr sh, const float *campos,
                                                         Tile t, float *colors) {
    extern __shared__ __attribute__((aligned(16))) float tile[];
    const int lane = (int)threadIdx.x, n0 = (int)blockIdx.x * kWave, n = n0 + lane;
    const int count = N - n0 < kWave ? N - n0 : kWave;
    for (int f = (int)blockIdx.y; f < F; f += (int)gridDim.y) {
        float p[3], cam[3], out[3];
        if (n < N) {
            const float *pp = at(means3d, f, n);
            p[0] = pp[0], p[1] = pp[1], p[2] = pp[2];
        }
        cam[0] = campos[(long long)f * 3], cam[1] = campos[(long long)f * 3 + 1], cam[2] = campos[(long long)f * 3 + 2];
        if (t.stride) {
            stage_in(tile, at(sh, f, n0), count * t.rec, t, lane);
            __syncthreads();
            if (n < N) colour<D>(p, cam, tile + lane * t.stride, out);
            __syncthreads();  // the tile is free for the next frame
        } else if (n < N) {
            colour<D>(p, cam, at(sh, f, n), out);
        }
        if (n < N) {
            float *o = colors + ((long long)f * N + n) * 3;
            o[0] = out[0], o[1] = out[1], o[2] = out[2];
        }
    }
}

// stage_input: the records come through the tile (contiguous input); the gradients, dense rows, always leave through it
// when there is one
template <int D>
__global__ __launch_bounds__(kWave) void sh_colors_backward_kernel(int F, int N, amav_attr means3d, amav_attr sh,
                                                                  const float *campos, Tile t, int stage_input,
                                                                  const float *grad_colors, float *grad_sh,
                                                                  float *grad_means3d) {
    extern __shared__ __attribute__((aligned(16))) float tile[];
    constexpr int kUsed = 3 * num_coeffs(D);
    const int lane = (int)threadIdx.x, n0 = (int)blockIdx.x * kWave, n = n0 + lane;
    const int count = N - n0 < kWave ? N - n0 : kWave;
    for (int f = (int)blockIdx.y; f < F; f += (int)gridDim.y) {
        float p[3], cam[3], g[3], gp[3];
        const long long row = (long long)f * N + n;
        if (n < N) {
            const float *pp = at(means3d, f, n), *gc = grad_colors + row * 3;
            p[0] = pp[0], p[1] = pp[1], p[2] = pp[2];
            g[0] = gc[0], g[1] = gc[1], g[2] = gc[2];
        }
        cam[0] = campos[(long long)f * 3], cam[1] = campos[(long long)f * 3 + 1], cam[2] = campos[(long long)f * 3 + 2];
        const bool want_p = grad_means3d != nullptr;
        if (t.stride) {
            float *mine = tile + lane * t.stride;
            if (stage_input) {
                stage_in(tile, at(sh, f, n0), count * t.rec, t, lane);
                __syncthreads();
                if (n < N) colour_backward<D>(p, cam, mine, g, mine, gp, want_p);  // in place: a lane owns its record
            } else if (n < N) {
                colour_backward<D>(p, cam, at(sh, f, n), g, mine, gp, want_p);
            }
            if (n < N)
                for (int j = kUsed; j < t.rec; ++j) mine[j] = 0.0f;  // coefficients the degree does not use
            __syncthreads();
            stage_out(tile, grad_sh + ((long long)f * N + n0) * t.rec, count * t.rec, t, lane);
            __syncthreads();  // the tile is free for the next frame
        } else if (n < N) {
            float *mine = grad_sh + row * t.rec;
            colour_backward<D>(p, cam, at(sh, f, n), g, mine, gp, want_p);
            for (int j = kUsed; j < t.rec; ++j) mine[j] = 0.0f;
        }
        if (grad_means3d && n < N) {
            float *o = grad_means3d + row * 3;
            o[0] = gp[0], o[1] = gp[1], o[2] = gp[2];
        }
    }
}

// f(std::integral_constant<int, D>) for the degree the kernels are instantiated for
template <typename Fn>
inline void for_degree(int degree, Fn &&f) {
    switch (degree) {
        case 0: f(std::integral_constant<int, 0>{}); break;
        case 1: f(std::integral_constant<int, 1>{}); break;
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 3: f(std::integral_constant<int, 3>{}); break;
        default: f(std::integral_constant<int, 4>{}); break;
    }
}

// the checks the two entry points share; `what` names the entry point.  *empty: nothing to do
inline int check_args(const char *what, const amav_sh_args *a, bool *empty) {
    AMAV_REQUIRE(a, "%s: NULL pointer (args)", what);
    AMAV_REQUIRE(a->num_frames >= 0 && a->num_gaussians >= 0, "%s: negative count F=%d N=%d", what, a->num_frames,
                 a->num_gaussians);
    AMAV_REQUIRE(a->degree >= 0 && a->degree <= kMaxDegree, "%s: degree=%d outside 0..%d", what, a->degree, kMaxDegree);
    AMAV_REQUIRE(a->num_coeffs >= num_coeffs(a->degree), "%s: num_coeffs=%d, degree %d needs (degree+1)^2 = %d", what,
                 a->num_coeffs, a->degree, num_coeffs(a->degree));
    AMAV_REQUIRE(a->num_coeffs <= INT_MAX / 3 / kWave, "%s: num_coeffs=%d is too large", what, a->num_coeffs);
    *empty = a->num_frames == 0 || a->num_gaussians == 0;
    if (*empty) return AMAV_OK;
    AMAV_REQUIRE(a->means3d.ptr && a->sh.ptr && a->campos, "%s: NULL pointer (means3d / sh / campos)", what);
    AMAV_REQUIRE(a->means3d.elem_stride >= 3, "%s: means3d element stride %d below its width 3", what,
                 a->means3d.elem_stride);
    AMAV_REQUIRE(a->sh.elem_stride >= 3 * a->num_coeffs, "%s: sh element stride %d below its width 3 * num_coeffs = %d",
                 what, a->sh.elem_stride, 3 * a->num_coeffs);
    return AMAV_OK;
}

// the tile of a problem: none when 64 records at the padded stride exceed the LDS a block may ask for
inline Tile tile_of(int num_coeffs_) {
    const int rec = 3 * num_coeffs_, stride = rec | 1;
    if ((long long)stride * kWave * (long long)sizeof(float) > kLdsBytes) return {rec, 0, 0, 0};
    return {rec, stride, 256 / rec, 256 % rec};
}

inline dim3 grid_of(const amav_sh_args *a) {
    const unsigned F = (unsigned)a->num_frames;
    return dim3((unsigned)((a->num_gaussians + kWave - 1) / kWave), F < kGridMax ? F : kGridMax);
}

}  // namespace sh
}  // namespace amav

using namespace amav;
using namespace amav::sh;

extern "C" int amav_sh_colors(const amav_sh_args *a, float *colors_dev, void *stream_) {
    bool empty = false;
    if (int rc = check_args("amav_sh_colors", a, &empty)) return rc;
    if (empty) return AMAV_OK;
    AMAV_REQUIRE(colors_dev, "amav_sh_colors: NULL pointer (colors)");
    Tile t = tile_of(a->num_coeffs);
    if (a->sh.elem_stride != t.rec) t.stride = 0;  // records apart from each other: lane by lane
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const size_t lds = (size_t)t.stride * kWave * sizeof(float);
    for_degree(a->degree, [&](auto d) {
        sh_colors_kernel<decltype(d)::value><<<grid_of(a), kWave, lds, stream>>>(
            a->num_frames, a->num_gaussians, a->means3d, a->sh, a->campos, t, colors_dev);
    });
    return check_launch("amav_sh_colors: sh_colors_kernel");
}

extern "C" int amav_sh_colors_backward(const amav_sh_args *a, const float *grad_colors_dev, float *grad_sh_dev,
                                       float *grad_means3d_dev, void *stream_) {
    bool empty = false;
    if (int rc = check_args("amav_sh_colors_backward", a, &empty)) return rc;
    if (empty) return AMAV_OK;
    AMAV_REQUIRE(grad_colors_dev && grad_sh_dev, "amav_sh_colors_backward: NULL pointer (grad_colors / grad_sh)");
    const Tile t = tile_of(a->num_coeffs);
    const int stage_input = a->sh.elem_stride == t.rec;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const size_t lds = (size_t)t.stride * kWave * sizeof(float);
    for_degree(a->degree, [&](auto d) {
        sh_colors_backward_kernel<decltype(d)::value><<<grid_of(a), kWave, lds, stream>>>(
            a->num_frames, a->num_gaussians, a->means3d, a->sh, a->campos, t, stage_input, grad_colors_dev, grad_sh_dev,
            grad_means3d_dev);
    });
    return check_launch("amav_sh_colors_backward: sh_colors_backward_kernel");
}
