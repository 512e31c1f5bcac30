// Stage-1 TriplaneDownsampler (src/models/triplane_net.py:411-451): the kernels of ConvNeXtBlock and of the 4x4 strided
// convolution that are not matrix products.  fp32, planes channels-last [K, H, W, C] with K =
// frames x 3 planes; no float atomics, every sum in an order fixed by the sizes alone; kernel launches only.
//
//   dwconv7_layernorm        y = depthwise 7x7 (padding 3, zero outside the plane) + bias; LayerNorm over C of y
//   ..._backward             LayerNorm backward over the stored y, then the flipped-kernel stencil for dx and the weight /
//                            bias gradients from the same staged halo
//   gelu_bias (+ backward)   exact-erf GELU of proj + bias
//   patch4_gather (+ backward)  the im2col of Conv2d(C, C, 4, stride s, padding 1), tap-major, and its transpose
//
// Lanes run along the channels everywhere: lane l of a wave holds channel 64 v + l of chunk v, so every global access of a
// wave is 256 contiguous bytes and every LDS access is conflict-free (consecutive dwords; the per-lane weight rows have
// the odd stride 49).  The stencils work on 8 x 8 pixel tiles of one plane: the 14 x 14 halo of a 64-channel chunk is
// staged once in LDS (50 176 B) and read by all 49 taps; coordinates outside the plane are written as zero, never loaded,
// so planes cannot bleed into each other.
//
// Summation orders.  Convolution: the taps in (ky, kx) order from +0, one fma each, then the bias -- added last, as the
// library does: with the bias first, a bias far above the tap sum costs every one of the 49 roundings the bias's ulp (found
// at a bias of 8: 5.6e-7 of max |y| against the library's 1e-7).  LayerNorm statistics: the lane's
// chunks ascending, then the xor butterfly (32, 16, .., 1) -- add_layernorm_kernel's two-pass form.  Parameter gradients:
// two stages, amav_rows_colsum's scheme with another first-stage unit: LayerNorm's dweight / dbias over chunks of 16 rows
// (ascending rows, then ascending chunks); the depthwise dweight / dbias over the 8 x 8 tiles (inside a tile: the wave's
// two rows top to bottom and left to right, then waves 0..3; then tiles ascending over (plane, tile row, tile column)).
#include <cmath>

#include "amav_common.h"
#include "gelu.h"
#include "split_bf16.h"
#include "split_f16.h"
#include "wave_ops.h"

namespace amav {
namespace convnext {

constexpr int kTile = 8;                     // output pixels per tile edge
constexpr int kHalo = kTile + 6;             // 14
constexpr int kHaloPix = kHalo * kHalo;      // 196
constexpr int kTaps = 49;
constexpr int kTilePart = kTaps + 1;         // per-tile partials: 49 weight taps + the bias
constexpr int kRowChunk = 16;                // rows per first-stage partial of LayerNorm's dweight / dbias
constexpr int kLds = kHaloPix * 64 + 64 * kTaps;  // floats: halo | weights of the chunk (>= 4 * kTilePart * 64)

// The splits of amav_split_operand (csrc/attention_rows.hip), part for part: split3 of split_bf16.h, and split2 with
// + 0 on the residual (not split_f16.h's split2).
__device__ __forceinline__ void split2_plus0(float x, _Float16 &a, _Float16 &b) {
    a = (_Float16)x;
    b = (_Float16)(__builtin_fmaf((float)a, -1.0f, x) + 0.0f);  // + 0: an exactly-zero residual is +0 (geglu_kernel's note)
}

// One value of row `row`, column `col` of a [rows, K] result: fp32 (kind 0), or the activation operand of
// amav_split_operand -- bf16 x 3 [x3 x2 x1 x2 x1 x1] (kind 1), fp16 x 2 of x * prescale [h2 h1 h1] (kind 2).
__device__ __forceinline__ void store1(int kind, float *out, void *out_split, float prescale, long long row, int K, int col,
                                       float v) {
    if (kind == 0) {
        out[row * K + col] = v;
    } else if (kind == 1) {
        __bf16 p1, p2, p3;
        split3(v, p1, p2, p3);
        __bf16 *dst = static_cast<__bf16 *>(out_split) + row * 6 * K + col;
        dst[0] = p3, dst[K] = p2, dst[2 * K] = p1, dst[3 * K] = p2, dst[4 * K] = p1, dst[5 * (long long)K] = p1;
    } else {
        _Float16 h1, h2;
        split2_plus0(v * prescale, h1, h2);
        _Float16 *dst = static_cast<_Float16 *>(out_split) + row * 3 * K + col;
        dst[0] = h2, dst[K] = h1, dst[2 * K] = h1;
    }
}

// The same for four consecutive columns (col a multiple of 4).
__device__ __forceinline__ void store4(int kind, float *out, void *out_split, float prescale, long long row, int K, int col,
                                       const float4 &v) {
    if (kind == 0) {
        *reinterpret_cast<float4 *>(out + row * K + col) = v;
        return;
    }
    const float x[4] = {v.x, v.y, v.z, v.w};
    if (kind == 1) {
        bf16x4 p1, p2, p3;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            __bf16 a, b, c;
            split3(x[j], a, b, c);
            p1[j] = a, p2[j] = b, p3[j] = c;
        }
        __bf16 *dst = static_cast<__bf16 *>(out_split) + row * 6 * K + col;
        auto put = [&](int block, const bf16x4 &p) { *reinterpret_cast<bf16x4 *>(dst + (long long)block * K) = p; };
        put(0, p3), put(1, p2), put(2, p1), put(3, p2), put(4, p1), put(5, p1);
    } else {
        f16x4 p1, p2;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            _Float16 a, b;
            split2_plus0(x[j] * prescale, a, b);
            p1[j] = a, p2[j] = b;
        }
        _Float16 *dst = static_cast<_Float16 *>(out_split) + row * 3 * K + col;
        *reinterpret_cast<f16x4 *>(dst) = p2;
        *reinterpret_cast<f16x4 *>(dst + K) = p1;
        *reinterpret_cast<f16x4 *>(dst + 2 * (long long)K) = p1;
    }
}

// The 14 x 14 halo of the tile at (ty0, tx0) of one plane, channels [c0, c0 + 64), and the 64 x 49 depthwise weights of
// those channels ([C, 49]: contiguous), into LDS.  Outside the plane: +0, without a load.
__device__ __forceinline__ void stage_chunk(float *lds, const float *__restrict__ plane, int H, int W, int C, int ty0,
                                            int tx0, int c0, const float *__restrict__ dw_w) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // a wave takes the halo pixels wave, wave + 4, ...: 49 each, seven loads in flight at a time.  Every load is issued at
    // coordinates clamped into the plane (no branch between the loads) and a pixel outside the plane is SELECTED to +0
    // afterwards, so what is loaded there never reaches the LDS.
    const float *src = plane + c0 + lane;
    for (int i0 = 0; i0 < kHaloPix / 4; i0 += 7) {
        float v[7];
#pragma unroll
        for (int u = 0; u < 7; ++u) {
            const int p = wave + 4 * (i0 + u);
            const int hy = p / kHalo, hx = p - hy * kHalo;
            const int gy = ty0 + hy - 3, gx = tx0 + hx - 3;
            const bool inside = gy >= 0 && gy < H && gx >= 0 && gx < W;
            const int cy = min(max(gy, 0), H - 1), cx = min(max(gx, 0), W - 1);
            const float t = src[((long long)cy * W + cx) * C];
            v[u] = inside ? t : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < 7; ++u) lds[(wave + 4 * (i0 + u)) * 64 + lane] = v[u];
    }
    const float *w = dw_w + (long long)c0 * kTaps;
    static_assert(64 * kTaps == 12 * 256 + 64, "weight staging below");
    float wv[13];
#pragma unroll
    for (int j = 0; j < 12; ++j) wv[j] = w[tid + 256 * j];
    wv[12] = tid < 64 ? w[tid + 256 * 12] : 0.0f;
#pragma unroll
    for (int j = 0; j < 12; ++j) lds[kHaloPix * 64 + tid + 256 * j] = wv[j];
    if (tid < 64) lds[kHaloPix * 64 + tid + 256 * 12] = wv[12];
}

// grid: one block per tile over (plane, tile row, tile column); 256 threads, wave w owns the tile's rows 2w and 2w + 1.
template <int kVec>
__global__ __launch_bounds__(256) void dwconv7_layernorm_kernel(int H, int W, int tiles_x, int tiles_per_plane,
                                                                const float *__restrict__ x, const float *__restrict__ dw_w,
                                                                const float *__restrict__ dw_b,
                                                                const float *__restrict__ ln_w,
                                                                const float *__restrict__ ln_b, float eps,
                                                                float *__restrict__ y_out, float *__restrict__ out,
                                                                void *__restrict__ out_split, int kind, float prescale) {
    constexpr int C = 64 * kVec;
    constexpr float kInv = 1.0f / C;
    __shared__ float lds[kLds];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int plane = blockIdx.x / tiles_per_plane, tile = blockIdx.x - plane * tiles_per_plane;
    const int ty0 = (tile / tiles_x) * kTile, tx0 = (tile % tiles_x) * kTile;
    const float *xp = x + (long long)plane * H * W * C;
    float acc[2][kTile][kVec];
#pragma unroll
    for (int v = 0; v < kVec; ++v) {
        __syncthreads();  // the previous chunk's readers are done
        stage_chunk(lds, xp, H, W, C, ty0, tx0, 64 * v, dw_w);
        __syncthreads();
        float wr[kTaps];
#pragma unroll
        for (int t = 0; t < kTaps; ++t) wr[t] = lds[kHaloPix * 64 + lane * kTaps + t];
        const float bias = dw_b[64 * v + lane];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int row = 2 * wave + r;
            float a[kTile];
#pragma unroll
            for (int o = 0; o < kTile; ++o) a[o] = 0.f;
#pragma unroll
            for (int ky = 0; ky < 7; ++ky) {
                float in[kHalo];
#pragma unroll
                for (int j = 0; j < kHalo; ++j) in[j] = lds[((row + ky) * kHalo + j) * 64 + lane];
#pragma unroll
                for (int kx = 0; kx < 7; ++kx)
#pragma unroll
                    for (int o = 0; o < kTile; ++o) a[o] = fmaf(wr[ky * 7 + kx], in[o + kx], a[o]);
            }
#pragma unroll
            for (int o = 0; o < kTile; ++o) acc[r][o][v] = a[o] + bias;
        }
    }
    float lw[kVec], lb[kVec];
#pragma unroll
    for (int v = 0; v < kVec; ++v) lw[v] = ln_w[64 * v + lane], lb[v] = ln_b[64 * v + lane];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int gy = ty0 + 2 * wave + r;
        if (gy >= H) continue;  // wave-uniform
#pragma unroll
        for (int o = 0; o < kTile; ++o) {
            const int gx = tx0 + o;
            if (gx >= W) continue;
            const long long pix = ((long long)plane * H + gy) * W + gx;
            float sum = 0.f;
#pragma unroll
            for (int v = 0; v < kVec; ++v) sum += acc[r][o][v];
            const float mean = wave_sum(sum) * kInv;
            float var = 0.f;
#pragma unroll
            for (int v = 0; v < kVec; ++v) {
                const float d = acc[r][o][v] - mean;
                var += d * d;
            }
            const float rstd = 1.0f / sqrtf(wave_sum(var) * kInv + eps);
#pragma unroll
            for (int v = 0; v < kVec; ++v) {
                const int c = 64 * v + lane;
                if (y_out) y_out[pix * C + c] = acc[r][o][v];
                store1(kind, out, out_split, prescale, pix, C, c, (acc[r][o][v] - mean) * rstd * lw[v] + lb[v]);
            }
        }
    }
}

// LayerNorm backward over the rows of y [rows, 64 kVec]: one wave per chunk of kRowChunk rows.  mean and rstd as the forward
// computes them; with xhat = (y - mean) rstd and t = dnorm * w:  dy = rstd (t - mean_c(t) - xhat mean_c(t xhat)).  The lane
// adds dnorm * xhat and dnorm of its channels over the chunk's rows, ascending, into parts [chunks, 2, C].
template <int kVec>
__global__ __launch_bounds__(256) void layernorm_backward_kernel(long long rows, const float *__restrict__ y,
                                                                 const float *__restrict__ ln_w, float eps,
                                                                 const float *__restrict__ dnorm, float *__restrict__ dy,
                                                                 float *__restrict__ parts) {
    constexpr int C = 64 * kVec;
    constexpr float kInv = 1.0f / C;
    const long long chunk = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const long long first = chunk * kRowChunk;
    if (first >= rows) return;
    const long long last = first + kRowChunk < rows ? first + kRowChunk : rows;
    float w[kVec], dw[kVec], db[kVec];
#pragma unroll
    for (int v = 0; v < kVec; ++v) w[v] = ln_w[64 * v + lane], dw[v] = 0.f, db[v] = 0.f;
    for (long long row = first; row < last; ++row) {
        float xv[kVec], dn[kVec], t[kVec];
        float sum = 0.f;
#pragma unroll
        for (int v = 0; v < kVec; ++v) {
            xv[v] = y[row * C + 64 * v + lane];
            dn[v] = dnorm[row * C + 64 * v + lane];
            sum += xv[v];
        }
        const float mean = wave_sum(sum) * kInv;
        float var = 0.f;
#pragma unroll
        for (int v = 0; v < kVec; ++v) {
            const float d = xv[v] - mean;
            var += d * d;
        }
        const float rstd = 1.0f / sqrtf(wave_sum(var) * kInv + eps);
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int v = 0; v < kVec; ++v) {
            xv[v] = (xv[v] - mean) * rstd;  // xhat
            t[v] = dn[v] * w[v];
            s1 += t[v];
            s2 += t[v] * xv[v];
            dw[v] += dn[v] * xv[v];
            db[v] += dn[v];
        }
        const float m1 = wave_sum(s1) * kInv, m2 = wave_sum(s2) * kInv;
#pragma unroll
        for (int v = 0; v < kVec; ++v) dy[row * C + 64 * v + lane] = rstd * (t[v] - m1 - xv[v] * m2);
    }
#pragma unroll
    for (int v = 0; v < kVec; ++v) {
        parts[(chunk * 2 + 0) * C + 64 * v + lane] = dw[v];
        parts[(chunk * 2 + 1) * C + 64 * v + lane] = db[v];
    }
}

// Depthwise backward on one tile and one 64-channel chunk (blockIdx.y): with off(ky, kx) = (ky - 3, kx - 3),
//   dx[q] = sum_(ky,kx) w[ky,kx] dy[q - off],   dw[ky,kx] += x[q] dy[q - off],   db += dy[q]        for q in the tile,
// all three from the staged halo of dy.  parts [tiles, 50, C]: the tile's dw taps, then its db.
__global__ __launch_bounds__(256) void dwconv7_backward_kernel(int H, int W, int C, int tiles_x, int tiles_per_plane,
                                                               const float *__restrict__ x, const float *__restrict__ dy,
                                                               const float *__restrict__ dw_w, float *__restrict__ dx,
                                                               float *__restrict__ parts) {
    __shared__ float lds[kLds];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int plane = blockIdx.x / tiles_per_plane, tile = blockIdx.x - plane * tiles_per_plane;
    const int ty0 = (tile / tiles_x) * kTile, tx0 = (tile % tiles_x) * kTile;
    const int c = 64 * blockIdx.y + lane;
    const long long plane_at = (long long)plane * H * W * C;
    stage_chunk(lds, dy + plane_at, H, W, C, ty0, tx0, 64 * blockIdx.y, dw_w);
    __syncthreads();
    float wr[kTaps], dwacc[kTaps];
#pragma unroll
    for (int t = 0; t < kTaps; ++t) wr[t] = lds[kHaloPix * 64 + lane * kTaps + t], dwacc[t] = 0.f;
    float dbacc = 0.f;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int row = 2 * wave + r, gy = ty0 + row;
        float xc[kTile], a[kTile];
#pragma unroll
        for (int o = 0; o < kTile; ++o) {
            const int gx = tx0 + o;
            xc[o] = (gy < H && gx < W) ? x[plane_at + ((long long)gy * W + gx) * C + c] : 0.0f;
            a[o] = 0.f;
            dbacc += lds[((row + 3) * kHalo + o + 3) * 64 + lane];  // +0 outside the plane
        }
#pragma unroll
        for (int ky = 0; ky < 7; ++ky) {
            float in[kHalo];
#pragma unroll
            for (int j = 0; j < kHalo; ++j) in[j] = lds[((row + 6 - ky) * kHalo + j) * 64 + lane];
#pragma unroll
            for (int kx = 0; kx < 7; ++kx)
#pragma unroll
                for (int o = 0; o < kTile; ++o) {
                    const float g = in[o + 6 - kx];
                    a[o] = fmaf(wr[ky * 7 + kx], g, a[o]);
                    dwacc[ky * 7 + kx] = fmaf(xc[o], g, dwacc[ky * 7 + kx]);
                }
        }
        if (gy < H) {
#pragma unroll
            for (int o = 0; o < kTile; ++o)
                if (tx0 + o < W) dx[plane_at + ((long long)gy * W + tx0 + o) * C + c] = a[o];
        }
    }
    __syncthreads();  // every wave has read its halo rows and weights: the LDS becomes [4 waves][50][64]
#pragma unroll
    for (int t = 0; t < kTaps; ++t) lds[(wave * kTilePart + t) * 64 + lane] = dwacc[t];
    lds[(wave * kTilePart + kTaps) * 64 + lane] = dbacc;
    __syncthreads();
    float *dst = parts + (long long)blockIdx.x * kTilePart * C + 64 * blockIdx.y;
    for (int i = threadIdx.x; i < kTilePart * 64; i += 256) {
        const int t = i >> 6, l = i & 63;
        float s = lds[(0 * kTilePart + t) * 64 + l];
        s += lds[(1 * kTilePart + t) * 64 + l];
        s += lds[(2 * kTilePart + t) * 64 + l];
        s += lds[(3 * kTilePart + t) * 64 + l];
        dst[(long long)t * C + l] = s;
    }
}

// Stage 2 of the parameter gradients: parts [count, cols] summed over `count` in ascending order, one thread per column.
// kind 0: columns [0, C) -> out_a [C], [C, 2C) -> out_b [C] (LayerNorm's dweight | dbias);
// kind 1: cols = 50 C, column t * C + c -> out_a [C, 49] at [c, t] for t < 49, out_b [c] for t = 49 (depthwise).
__global__ __launch_bounds__(64) void sum_parts_kernel(long long count, int cols, int C, int kind,
                                                       const float *__restrict__ parts, float *__restrict__ out_a,
                                                       float *__restrict__ out_b) {
    const int col = blockIdx.x * 64 + threadIdx.x;
    if (col >= cols) return;
    const float *src = parts + col;
    float acc = src[0];
    long long k = 1;
    for (; k + 8 <= count; k += 8) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = src[(k + j) * cols];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc += v[j];
    }
    for (; k < count; ++k) acc += src[k * cols];
    const int t = col / C, c = col - t * C;
    if (kind == 0) {
        (t == 0 ? out_a : out_b)[c] = acc;
    } else if (t < kTaps) {
        out_a[c * kTaps + t] = acc;
    } else {
        out_b[c] = acc;
    }
}

// out[row, :] = gelu(proj[row, :] + bias), one thread per column quad (geglu_kernel's expression for gelu)
__global__ __launch_bounds__(256) void gelu_bias_kernel(long long quads, int inner4, const float4 *__restrict__ in,
                                                        long long in_row4, const float4 *__restrict__ bias,
                                                        float *__restrict__ out, void *__restrict__ out_split, int kind,
                                                        float prescale) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= quads) return;
    const long long row = i / inner4;
    const int col = (int)(i - row * inner4);
    float4 g = in[row * in_row4 + col];
    if (bias) {
        const float4 b = bias[col];
        g = make_float4(g.x + b.x, g.y + b.y, g.z + b.z, g.w + b.w);
    }
    store4(kind, out, out_split, prescale, row, 4 * inner4, 4 * col,
           make_float4(gelu(g.x), gelu(g.y), gelu(g.z), gelu(g.w)));
}

// dproj = dout (Phi(g) + g phi(g)) with g = proj + bias recomputed (geglu_backward_kernel's expressions)
__global__ __launch_bounds__(256) void gelu_bias_backward_kernel(long long quads, int inner4, const float4 *__restrict__ in,
                                                                 long long in_row4, const float4 *__restrict__ bias,
                                                                 const float4 *__restrict__ dout, float4 *__restrict__ dproj,
                                                                 long long dproj_row4) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= quads) return;
    const long long row = i / inner4;
    const int col = (int)(i - row * inner4);
    float4 g = in[row * in_row4 + col];
    if (bias) {
        const float4 b = bias[col];
        g = make_float4(g.x + b.x, g.y + b.y, g.z + b.z, g.w + b.w);
    }
    const float4 d = dout[i];
    const float gv[4] = {g.x, g.y, g.z, g.w}, dv[4] = {d.x, d.y, d.z, d.w};
    float r[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float xx = gv[j];
        const float cdf = 0.5f * (1.0f + erff(xx * 0.70710678118654752440f));
        const float pdf = expf(-0.5f * xx * xx) * 0.39894228040143267794f;
        r[j] = dv[j] * (cdf + xx * pdf);
    }
    dproj[row * dproj_row4 + col] = make_float4(r[0], r[1], r[2], r[3]);
}

// cols [K Ho Wo, 16 C]: column (4 ky + kx) C + c of window (k, oy, ox) = x[k, oy s - 1 + ky, ox s - 1 + kx, c], +0 outside
// the plane.  One thread per (window, tap, channel quad).
__global__ __launch_bounds__(256) void patch4_gather_kernel(long long quads, int H, int W, int C4, int Ho, int Wo, int s,
                                                            const float4 *__restrict__ x, float *__restrict__ out,
                                                            void *__restrict__ out_split, int kind, float prescale) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= quads) return;
    const int c4 = (int)(i % C4);
    const long long rest = i / C4;
    const int tap = (int)(rest & 15);
    const long long win = rest >> 4;
    const int ox = (int)(win % Wo);
    const int oy = (int)((win / Wo) % Ho);
    const long long k = win / ((long long)Wo * Ho);
    const int y = oy * s - 1 + (tap >> 2), xx = ox * s - 1 + (tap & 3);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (y >= 0 && y < H && xx >= 0 && xx < W) v = x[((k * H + y) * W + xx) * C4 + c4];
    store4(kind, out, out_split, prescale, win, 16 * 4 * C4, 4 * (tap * C4 + c4), v);
}

// The transpose: dx[k, y, x, c] = the windows that cover the pixel, in ascending window index (oy, then ox): at most
// ceil(4 / s)^2 terms, none (+0) for a pixel no window reads.  One thread per (pixel, channel quad).
__global__ __launch_bounds__(256) void patch4_gather_backward_kernel(long long quads, int H, int W, int C4, int Ho, int Wo,
                                                                     int s, const float4 *__restrict__ dcols,
                                                                     float4 *__restrict__ dx) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= quads) return;
    const int c4 = (int)(i % C4);
    const long long pix = i / C4;
    const int xx = (int)(pix % W);
    const int y = (int)((pix / W) % H);
    const long long k = pix / ((long long)W * H);
    // window oy reads row y with ky = y + 1 - oy s in [0, 3]
    const int oy_lo = y >= 2 ? (y - 2 + s - 1) / s : 0, oy_hi = min((y + 1) / s, Ho - 1);
    const int ox_lo = xx >= 2 ? (xx - 2 + s - 1) / s : 0, ox_hi = min((xx + 1) / s, Wo - 1);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int oy = oy_lo; oy <= oy_hi; ++oy)
        for (int ox = ox_lo; ox <= ox_hi; ++ox) {
            const int tap = 4 * (y + 1 - oy * s) + (xx + 1 - ox * s);
            const float4 g = dcols[(((k * Ho + oy) * Wo + ox) * 16 + tap) * C4 + c4];
            acc = make_float4(acc.x + g.x, acc.y + g.y, acc.z + g.z, acc.w + g.w);
        }
    dx[i] = acc;
}

inline bool channels_ok(int C) { return C >= 64 && C <= 512 && C % 64 == 0; }
inline long long tiles_of(int n) { return (n + kTile - 1) / kTile; }
inline long long chunks_of(long long rows) { return (rows + kRowChunk - 1) / kRowChunk; }
inline bool split_ok(const void *out_split, int format, int scale_exp) {
    return !out_split || format == AMAV_SPLIT_BF16X3 || (format == AMAV_SPLIT_FP16X2 && scale_exp >= -126 && scale_exp <= 126);
}
inline int kind_of(const void *out_split, int format) { return !out_split ? 0 : format == AMAV_SPLIT_FP16X2 ? 2 : 1; }
inline float prescale_of(const void *out_split, int format, int scale_exp) {
    return ldexpf(1.0f, out_split && format == AMAV_SPLIT_FP16X2 ? scale_exp : 0);
}
// planes, height and width of a call, with every product the kernels form inside 63 / 31 bits
inline bool plane_sizes_ok(int planes, int H, int W) {
    return planes > 0 && H > 0 && W > 0 && H <= 32768 && W <= 32768 && (long long)planes * H * W <= (1LL << 40) &&
           (long long)planes * tiles_of(H) * tiles_of(W) <= 0x7fffffffLL;
}

struct BackwardWorkspace {
    float *dy, *ln_parts, *tile_parts;
    size_t bytes;
};
inline BackwardWorkspace carve_backward(void *base, int planes, int H, int W, int C) {
    const long long rows = (long long)planes * H * W, tiles = (long long)planes * tiles_of(H) * tiles_of(W);
    Carver carve(base);
    BackwardWorkspace ws;
    ws.dy = carve.take<float>((size_t)rows * C);
    ws.ln_parts = carve.take<float>((size_t)chunks_of(rows) * 2 * C);
    ws.tile_parts = carve.take<float>((size_t)tiles * kTilePart * C);
    ws.bytes = carve.total();
    return ws;
}

}  // namespace convnext
}  // namespace amav

using namespace amav;

extern "C" int amav_dwconv7_layernorm(int planes, int height, int width, int channels, const float *x, const float *dw_weight,
                                      const float *dw_bias, const float *ln_weight, const float *ln_bias, float eps,
                                      float *y, float *out, void *out_split, int split_format, int split_scale_exp,
                                      void *stream_) {
    AMAV_REQUIRE(convnext::plane_sizes_ok(planes, height, width) && convnext::channels_ok(channels),
                 "amav_dwconv7_layernorm: planes=%d height=%d width=%d channels=%d (channels: a multiple of 64 in [64, 512])",
                 planes, height, width, channels);
    AMAV_REQUIRE(x && dw_weight && dw_bias && ln_weight && ln_bias, "amav_dwconv7_layernorm: NULL pointer");
    AMAV_REQUIRE((out != nullptr) != (out_split != nullptr),
                 "amav_dwconv7_layernorm: give exactly one of out (fp32) and out_split (split operand)");
    AMAV_REQUIRE(convnext::split_ok(out_split, split_format, split_scale_exp),
                 "amav_dwconv7_layernorm: split format %d / scale exponent %d", split_format, split_scale_exp);
    AMAV_REQUIRE(eps >= 0.0f && std::isfinite(eps), "amav_dwconv7_layernorm: eps must be finite and >= 0");
    AMAV_REQUIRE(aligned16(x, dw_weight, dw_bias, ln_weight, ln_bias, y, out) && aligned16(out_split),
                 "amav_dwconv7_layernorm: buffers must be 16-byte aligned");
    const int tiles_x = (int)convnext::tiles_of(width), tiles_per_plane = tiles_x * (int)convnext::tiles_of(height);
    const unsigned grid = (unsigned)((long long)planes * tiles_per_plane);
    const int kind = convnext::kind_of(out_split, split_format);
    const float prescale = convnext::prescale_of(out_split, split_format, split_scale_exp);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
#define AMAV_DW_LAUNCH(V)                                                                                              \
    case V:                                                                                                            \
        convnext::dwconv7_layernorm_kernel<V><<<grid, 256, 0, stream>>>(height, width, tiles_x, tiles_per_plane, x,     \
                                                                        dw_weight, dw_bias, ln_weight, ln_bias, eps, y, \
                                                                        out, out_split, kind, prescale);                \
        break
    switch (channels / 64) {
        AMAV_DW_LAUNCH(1);
        AMAV_DW_LAUNCH(2);
        AMAV_DW_LAUNCH(3);
        AMAV_DW_LAUNCH(4);
        AMAV_DW_LAUNCH(5);
        AMAV_DW_LAUNCH(6);
        AMAV_DW_LAUNCH(7);
        AMAV_DW_LAUNCH(8);
    }
#undef AMAV_DW_LAUNCH
    return check_launch("amav_dwconv7_layernorm");
}

extern "C" size_t amav_dwconv7_layernorm_backward_workspace_bytes(int planes, int height, int width, int channels) {
    if (!convnext::plane_sizes_ok(planes, height, width) || !convnext::channels_ok(channels)) return 0;
    return convnext::carve_backward(nullptr, planes, height, width, channels).bytes;
}

extern "C" int amav_dwconv7_layernorm_backward(int planes, int height, int width, int channels, const float *x,
                                               const float *y, const float *dw_weight, const float *ln_weight, float eps,
                                               const float *dnorm, float *dx, float *d_dw_weight, float *d_dw_bias,
                                               float *d_ln_weight, float *d_ln_bias, void *workspace, size_t workspace_bytes,
                                               void *stream_) {
    AMAV_REQUIRE(convnext::plane_sizes_ok(planes, height, width) && convnext::channels_ok(channels),
                 "amav_dwconv7_layernorm_backward: planes=%d height=%d width=%d channels=%d (channels: a multiple of 64 in "
                 "[64, 512])", planes, height, width, channels);
    AMAV_REQUIRE(x && y && dw_weight && ln_weight && dnorm && dx && d_dw_weight && d_dw_bias && d_ln_weight && d_ln_bias,
                 "amav_dwconv7_layernorm_backward: NULL pointer");
    AMAV_REQUIRE(eps >= 0.0f && std::isfinite(eps), "amav_dwconv7_layernorm_backward: eps must be finite and >= 0");
    AMAV_REQUIRE(aligned16(x, y, dw_weight, ln_weight, dnorm, dx, d_dw_weight, d_dw_bias, d_ln_weight, d_ln_bias) &&
                     aligned16(workspace),
                 "amav_dwconv7_layernorm_backward: buffers must be 16-byte aligned");
    const size_t need = amav_dwconv7_layernorm_backward_workspace_bytes(planes, height, width, channels);
    if (workspace == nullptr || workspace_bytes < need)
        return fail(AMAV_ERR_WORKSPACE, "amav_dwconv7_layernorm_backward: workspace %zu < required %zu", workspace_bytes, need);
    const convnext::BackwardWorkspace ws = convnext::carve_backward(workspace, planes, height, width, channels);
    const long long rows = (long long)planes * height * width, chunks = convnext::chunks_of(rows);
    const int tiles_x = (int)convnext::tiles_of(width), tiles_per_plane = tiles_x * (int)convnext::tiles_of(height);
    const long long tiles = (long long)planes * tiles_per_plane;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const unsigned ln_grid = (unsigned)((chunks + 3) / 4);
#define AMAV_LNB_LAUNCH(V)                                                                                             \
    case V:                                                                                                            \
        convnext::layernorm_backward_kernel<V><<<ln_grid, 256, 0, stream>>>(rows, y, ln_weight, eps, dnorm, ws.dy,       \
                                                                            ws.ln_parts);                               \
        break
    switch (channels / 64) {
        AMAV_LNB_LAUNCH(1);
        AMAV_LNB_LAUNCH(2);
        AMAV_LNB_LAUNCH(3);
        AMAV_LNB_LAUNCH(4);
        AMAV_LNB_LAUNCH(5);
        AMAV_LNB_LAUNCH(6);
        AMAV_LNB_LAUNCH(7);
        AMAV_LNB_LAUNCH(8);
    }
#undef AMAV_LNB_LAUNCH
    convnext::sum_parts_kernel<<<(unsigned)((2 * channels + 63) / 64), 64, 0, stream>>>(chunks, 2 * channels, channels, 0,
                                                                                      ws.ln_parts, d_ln_weight, d_ln_bias);
    convnext::dwconv7_backward_kernel<<<dim3((unsigned)tiles, (unsigned)(channels / 64)), 256, 0, stream>>>(
        height, width, channels, tiles_x, tiles_per_plane, x, ws.dy, dw_weight, dx, ws.tile_parts);
    const int cols = convnext::kTilePart * channels;
    convnext::sum_parts_kernel<<<(unsigned)((cols + 63) / 64), 64, 0, stream>>>(tiles, cols, channels, 1, ws.tile_parts,
                                                                              d_dw_weight, d_dw_bias);
    return check_launch("amav_dwconv7_layernorm_backward");
}

extern "C" int amav_gelu_bias(int64_t rows, int inner, const float *proj, int64_t proj_row_stride, const float *bias,
                              float *out, void *out_split, int split_format, int split_scale_exp, void *stream) {
    AMAV_REQUIRE(rows > 0 && inner > 0 && inner % 4 == 0 && (!out_split || inner % 8 == 0),
                 "amav_gelu_bias: bad sizes rows=%lld inner=%d (inner: a multiple of 4; of 8 for a split operand)",
                 (long long)rows, inner);
    AMAV_REQUIRE(proj && ((out != nullptr) != (out_split != nullptr)),
                 "amav_gelu_bias: NULL projection, or not exactly one of out (fp32) and out_split (split operand)");
    AMAV_REQUIRE(convnext::split_ok(out_split, split_format, split_scale_exp),
                 "amav_gelu_bias: split format %d / scale exponent %d", split_format, split_scale_exp);
    AMAV_REQUIRE(proj_row_stride >= inner && proj_row_stride % 4 == 0, "amav_gelu_bias: bad row stride");
    AMAV_REQUIRE(aligned16(proj, bias, out) && aligned16(out_split), "amav_gelu_bias: buffers must be 16-byte aligned");
    const long long quads = rows * (inner / 4);
    AMAV_REQUIRE((quads + 255) / 256 <= 0x7fffffffLL, "amav_gelu_bias: grid too large");
    convnext::gelu_bias_kernel<<<(unsigned)((quads + 255) / 256), 256, 0, static_cast<hipStream_t>(stream)>>>(
        quads, inner / 4, reinterpret_cast<const float4 *>(proj), proj_row_stride / 4, reinterpret_cast<const float4 *>(bias),
        out, out_split, convnext::kind_of(out_split, split_format),
        convnext::prescale_of(out_split, split_format, split_scale_exp));
    return check_launch("amav_gelu_bias");
}

extern "C" int amav_gelu_bias_backward(int64_t rows, int inner, const float *proj, int64_t proj_row_stride, const float *bias,
                                       const float *dout, float *dproj, int64_t dproj_row_stride, void *stream) {
    AMAV_REQUIRE(rows > 0 && inner > 0 && inner % 4 == 0, "amav_gelu_bias_backward: bad sizes rows=%lld inner=%d",
                 (long long)rows, inner);
    AMAV_REQUIRE(proj && dout && dproj, "amav_gelu_bias_backward: NULL pointer");
    AMAV_REQUIRE(proj_row_stride >= inner && proj_row_stride % 4 == 0 && dproj_row_stride >= inner && dproj_row_stride % 4 == 0,
                 "amav_gelu_bias_backward: bad row stride");
    AMAV_REQUIRE(aligned16(proj, bias, dout, dproj), "amav_gelu_bias_backward: buffers must be 16-byte aligned");
    const long long quads = rows * (inner / 4);
    AMAV_REQUIRE((quads + 255) / 256 <= 0x7fffffffLL, "amav_gelu_bias_backward: grid too large");
    convnext::gelu_bias_backward_kernel<<<(unsigned)((quads + 255) / 256), 256, 0, static_cast<hipStream_t>(stream)>>>(
        quads, inner / 4, reinterpret_cast<const float4 *>(proj), proj_row_stride / 4, reinterpret_cast<const float4 *>(bias),
        reinterpret_cast<const float4 *>(dout), reinterpret_cast<float4 *>(dproj), dproj_row_stride / 4);
    return check_launch("amav_gelu_bias_backward");
}

// Output size of Conv2d(kernel 4, stride s, padding 1) along one axis; 0 = no window fits
static int patch4_out(int n, int stride) { return n >= 2 ? (n - 2) / stride + 1 : 0; }

extern "C" int amav_patch4_gather(int planes, int height, int width, int channels, int stride, const float *x, float *out,
                                  void *out_split, int split_format, int split_scale_exp, void *stream) {
    AMAV_REQUIRE(convnext::plane_sizes_ok(planes, height, width) && height >= 2 && width >= 2 && channels > 0 &&
                     channels % 4 == 0 && channels <= 65536 && (!out_split || channels % 8 == 0) && stride >= 2,
                 "amav_patch4_gather: planes=%d height=%d width=%d channels=%d stride=%d (height, width >= 2; channels a "
                 "multiple of 4, of 8 for a split operand; stride >= 2)", planes, height, width, channels, stride);
    AMAV_REQUIRE(x && ((out != nullptr) != (out_split != nullptr)),
                 "amav_patch4_gather: NULL input, or not exactly one of out (fp32) and out_split (split operand)");
    AMAV_REQUIRE(convnext::split_ok(out_split, split_format, split_scale_exp),
                 "amav_patch4_gather: split format %d / scale exponent %d", split_format, split_scale_exp);
    AMAV_REQUIRE(aligned16(x, out) && aligned16(out_split), "amav_patch4_gather: buffers must be 16-byte aligned");
    const int Ho = patch4_out(height, stride), Wo = patch4_out(width, stride);
    const long long quads = (long long)planes * Ho * Wo * 16 * (channels / 4);
    AMAV_REQUIRE((quads + 255) / 256 <= 0x7fffffffLL, "amav_patch4_gather: grid too large");
    convnext::patch4_gather_kernel<<<(unsigned)((quads + 255) / 256), 256, 0, static_cast<hipStream_t>(stream)>>>(
        quads, height, width, channels / 4, Ho, Wo, stride, reinterpret_cast<const float4 *>(x), out, out_split,
        convnext::kind_of(out_split, split_format), convnext::prescale_of(out_split, split_format, split_scale_exp));
    return check_launch("amav_patch4_gather");
}

extern "C" int amav_patch4_gather_backward(int planes, int height, int width, int channels, int stride, const float *dcols,
                                           float *dx, void *stream) {
    AMAV_REQUIRE(convnext::plane_sizes_ok(planes, height, width) && height >= 2 && width >= 2 && channels > 0 &&
                     channels % 4 == 0 && channels <= 65536 && stride >= 2,
                 "amav_patch4_gather_backward: planes=%d height=%d width=%d channels=%d stride=%d (height, width >= 2; "
                 "channels a multiple of 4; stride >= 2)", planes, height, width, channels, stride);
    AMAV_REQUIRE(dcols && dx, "amav_patch4_gather_backward: NULL pointer");
    AMAV_REQUIRE(aligned16(dcols, dx), "amav_patch4_gather_backward: buffers must be 16-byte aligned");
    const int Ho = patch4_out(height, stride), Wo = patch4_out(width, stride);
    const long long quads = (long long)planes * height * width * (channels / 4);
    AMAV_REQUIRE((quads + 255) / 256 <= 0x7fffffffLL, "amav_patch4_gather_backward: grid too large");
    convnext::patch4_gather_backward_kernel<<<(unsigned)((quads + 255) / 256), 256, 0, static_cast<hipStream_t>(stream)>>>(
        quads, height, width, channels / 4, Ho, Wo, stride, reinterpret_cast<const float4 *>(dcols),
        reinterpret_cast<float4 *>(dx));
    return check_launch("amav_patch4_gather_backward");
}
