// Operand staging of the 3x3 cell convolution (upsample_conv.hip), shared by conv3x3_cells_kernel and the weight-gradient
// kernel that replays it: which source texel a patch texel reads (nearest x2, the cell's zero padding, the plane rule),
// the prologue, the optional gate of the backward's operand, and the fp16 x 2 split.  One 10 x 18 patch (an 8 x 16 tile
// and its halo) per 32-channel chunk; only the LDS layout the two parts are stored in differs between the kernels.
#pragma once
#include "amav_common.h"
#include "split_f16.h"

namespace amav {
namespace upconv {

constexpr int kTileH = 8, kTileW = 16;
constexpr int kPatchW = kTileW + 2, kPatch = (kTileH + 2) * kPatchW;  // 180 texels
constexpr int kKC = 32, kLDA = kKC + 8;
constexpr int kAItems = (kPatch * (kKC / 4) + 255) / 256;  // float4 reads per thread and chunk: 6

struct Params {
    const float *x;
    const void *wsplit;
    const unsigned *amax;
    const float *in_scale, *in_shift, *bias, *residual;
    const float *gate;  // the backward's operand: x is a gradient and counts where gate > 0 (same layout as x), or NULL
    const int *origin;
    float *out;
    int H, W, Cin, Cout, extent, upsample, relu_out, tiles_x, tiles_per_cell;
};

__device__ __forceinline__ float prologue(float x, float s, float b) { return fmaxf(__builtin_fmaf(s, x, b), 0.f); }

// g where the saved output is positive: the backward of an output ReLU, applied while the operand is read
__device__ __forceinline__ float4 gated(float4 g, float4 o) {
    return make_float4(o.x > 0.f ? g.x : 0.f, o.y > 0.f ? g.y : 0.f, o.z > 0.f ? g.z : 0.f, o.w > 0.f ? g.w : 0.f);
}

// The patch texels one thread of 256 stages: item i = tid + 256 j is (texel i / 8, channels 4 (i % 8) .. + 3) of the chunk.
struct PatchStage {
    long long aoff[kAItems];  // float offset of the source texel's channel ak, or -1: a zero of the operand
    float4 av[kAItems], sc, sh;
    int ak;

    __device__ __forceinline__ void locate(const Params &p, long long cell, int ty0, int tx0, int tid) {
        ak = (tid & 7) * 4;
        sc = sh = make_float4(0.f, 0.f, 0.f, 0.f);
        const int H = p.H, W = p.W;
        const int h_in = p.upsample ? H >> 1 : H, w_in = p.upsample ? W >> 1 : W;
        int oy = 0, ox = 0;
        if (p.origin) oy = p.origin[2 * cell], ox = p.origin[2 * cell + 1];
#pragma unroll
        for (int j = 0; j < kAItems; ++j) {
            const int texel = (tid >> 3) + 32 * j;
            const int y = ty0 + texel / kPatchW - 1, x = tx0 + texel % kPatchW - 1;
            bool ok = texel < kPatch && y >= 0 && y < H && x >= 0 && x < W;  // zero padding at the output's resolution
            if (p.origin) ok = ok && oy + y >= 0 && oy + y < p.extent && ox + x >= 0 && ox + x < p.extent;
            const int sy = p.upsample ? y >> 1 : y, sx = p.upsample ? x >> 1 : x;
            aoff[j] = ok ? ((cell * h_in + sy) * w_in + sx) * (long long)p.Cin + ak : -1;
        }
    }

    // global reads of the chunk that starts at channel k0
    template <bool GATE>
    __device__ __forceinline__ void load(const Params &p, int k0) {
#pragma unroll
        for (int j = 0; j < kAItems; ++j) {
            av[j] = aoff[j] >= 0 ? *reinterpret_cast<const float4 *>(p.x + aoff[j] + k0) : make_float4(0.f, 0.f, 0.f, 0.f);
            if (GATE && aoff[j] >= 0) av[j] = gated(av[j], *reinterpret_cast<const float4 *>(p.gate + aoff[j] + k0));
        }
        if (p.in_scale) {
            sc = *reinterpret_cast<const float4 *>(p.in_scale + k0 + ak);
            sh = *reinterpret_cast<const float4 *>(p.in_shift + k0 + ak);
        }
    }

    // prologue -> zeroing -> scaling -> split of what load() read; store(texel, ak, h1, h2) puts the parts into LDS
    template <typename Store>
    __device__ __forceinline__ void stage(const Params &p, float a_scale, int tid, Store store) const {
#pragma unroll
        for (int j = 0; j < kAItems; ++j) {
            const int texel = (tid >> 3) + 32 * j;
            if (texel < kPatch) {
                float x_[4] = {av[j].x, av[j].y, av[j].z, av[j].w};
                if (p.in_scale) {  // zeros of the operand stay zeros: the prologue applies to texels that exist
                    const float s_[4] = {sc.x, sc.y, sc.z, sc.w}, b_[4] = {sh.x, sh.y, sh.z, sh.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) x_[e] = aoff[j] >= 0 ? prologue(x_[e], s_[e], b_[e]) : 0.f;
                }
                f16x4 h1, h2;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    _Float16 u, l;
                    split2(x_[e] * a_scale, u, l);
                    h1[e] = u, h2[e] = l;
                }
                store(texel, ak, h1, h2);
            }
        }
    }
};

}  // namespace upconv
}  // namespace amav
