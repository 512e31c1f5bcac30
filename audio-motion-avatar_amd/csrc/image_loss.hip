// The image loss of the two training steps, for gfx950: per-image sums of |x - y| and of the SSIM map
// (src/utils/loss_utils.py:18-19, 24-84; losses.l1_loss / losses.ssim), and the gradient with respect to x.
// N images of H x W x C, C = 1..4; separable 11-tap window, zero padding of 5 (not renormalised), C1 = 0.01^2,
// C2 = 0.03^2.
//
//   forward_kernel   workgroup = one 16 x 16 pixel tile of one image, all C channels.  It stages the 26 x 26 pixel
//                    neighbourhood of x and y in LDS (padding: see the pivot below), runs the horizontal pass of the
//                    five moments (mu1, mu2, E[x^2], E[y^2], E[xy]) over 26 rows into a second LDS buffer, the vertical pass
//                    over 16 rows in registers, and forms the SSIM value and |x - y| per element; with `maps` it also
//                    writes dS/dE[x^2], dS/dE[xy] and dS/dmu1 per element (12 B) for the backward.  The block's two
//                    sums (shuffle tree inside a wave, then the 4 waves in order) go to the workspace slot of the tile.
//                    The moments are taken about a pivot per tile and channel (p for x, q for y: the tile's centre
//                    pixel): on the renderer's frames -- flat white with a figure -- E[x^2] - mu^2 of the raw values
//                    cancels to the last bits and the error of the sums is all that is left of the variance.  With
//                    x' = x - p inside the image (the padding stays 0), w = the window weight that falls inside the
//                    image and d = 1 - w:
//                        mu1     = mu1' + p w
//                        sigma1^2 = (E[x'^2] - mu1'^2) + d (2 p mu1' + p^2 w)
//                        sigma12  = (E[x'y'] - mu1' mu2') + d (q mu1' + p mu2' + p q w)
//                    d is formed without cancellation, per axis: 1 - sum of the 11 taps (host, double) plus the taps
//                    that fall outside the image, and d = dy + dx - dy dx.  Outside the image the pivot itself is
//                    staged: an exact zero once the pivot is subtracted, and the centre values stay raw for |x - y|.
//   finalize_kernel  wave = one image: lane l adds slots l, l + 64, ... in ascending order, then a fixed xor tree.
//   backward_kernel  same tiling over the three maps (zeros outside the image); grad_x = g_l1 sign(x - y) + g_ssim
//                    (conv(d_m1) + 2 x conv(d_e11) + y conv(d_e12)), every element written once: a gather, no atomics.
//
// Layout.  Channels stay interleaved in LDS, as they are in the renderer's frames: a tile row is 16 C consecutive floats
// ("float columns"), the horizontal taps sit C floats apart, and a thread owns one float column of one row.  Lanes walk
// (row, float column) with the column fastest, so every LDS access of a wave is a run of consecutive floats per row and
// all lanes move by the same tap offset: the tap stride C never enters the banking.  A ds_read_b32 / ds_write_b32 is
// served per 32-lane half over 32 banks.  C = 2 and C = 4 put 32 or 64 float columns in a row, so a half reads 32
// consecutive floats of one row: conflict-free at any row stride.  C = 1 and C = 3 put 16 or 48 in a row, so a half
// straddles two rows; the staged rows are padded from 26 C to a stride = 16 C (mod 32) floats (48 for C = 1, 80 for
// C = 3), which makes the half's addresses consecutive modulo 32 again.  The moment buffer has rows of exactly 16 C floats and
// is indexed by the linear work index: consecutive as well.
//
// Tile and occupancy.  16 x 16 pixels x C floats = 256 C outputs on 256 threads (4 waves), C per thread.  LDS per
// workgroup, C = 3: 2 x 26 x 80 x 4 B staged + 5 x 26 x 48 x 4 B moments = 16.3 + 24.4 = 40.6 KiB, three workgroups
// (12 waves) per CU out of 160 KiB; C = 4: 21.1 + 32.5 = 53.6 KiB, two workgroups.  A 32 x 32 tile would cut the halo
// overfetch from 2.64 x to 1.72 x but needs 123 KiB at C = 3, one workgroup per CU with nothing to overlap its
// barriers; the overfetch is served by the L2, which holds a frame's rows between neighbouring tiles.  The kernel issues
// about 90 ds_read_b32 per output element against 20 B of memory traffic, so it is bound by LDS issue and not by
// bandwidth (measured: DESIGN.md section 4.17).
#include <climits>
#include <cstddef>
#include <type_traits>

#include "amav_common.h"

namespace amav {
namespace image_loss {

constexpr int kTaps = 11;
constexpr int kHalo = kTaps / 2;
constexpr int kTile = 16;
constexpr int kSpan = kTile + 2 * kHalo;  // 26
constexpr int kBlock = 256;
constexpr int kWaves = kBlock / kWave;
constexpr unsigned kGridMax = 65535;
constexpr float kC1 = (float)(0.01 * 0.01), kC2 = (float)(0.03 * 0.03);

// floats per staged row: 26 C, padded so that rows of 16 C lanes stay consecutive modulo the 32 banks
constexpr int stage_stride(int C) {
    int s = kSpan * C;
    if ((kTile * C) % 32 != 0)
        while ((s - kTile * C) % 32 != 0) ++s;
    return s;
}

struct Tile {
    int y0, x0;
};

__device__ __forceinline__ Tile tile_origin(int tiles_x) {
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    return {ty * kTile, tx * kTile};
}

__device__ __forceinline__ int64_t view_offset(const amav_image_view &v, int n, int y, int x, int c) {
    return (int64_t)n * v.image_stride + (int64_t)y * v.row_stride + (int64_t)x * v.pixel_stride +
           (int64_t)c * v.channel_stride;
}

// grid (tiles of one image, min(N, 65535)); partial [N, tiles, 2]; maps NULL or [3, N, H, W, C]; deficit = 1 - the sum
// of the 11 taps
template <int C>
__global__ __launch_bounds__(kBlock) void forward_kernel(int N, int H, int W, amav_image_view x, amav_image_view y,
                                                         amav_image_loss_window win, float deficit, int tiles_x,
                                                         float *__restrict__ partial, float *__restrict__ maps) {
    constexpr int kCols = kTile * C, kSpanCols = kSpan * C, kStride = stage_stride(C);
    __shared__ float sx[kSpan * kStride], sy[kSpan * kStride];
    __shared__ float moments[5][kSpan * kCols];
    __shared__ float wave_sums[2][kWaves], pivots[2][4];
    const Tile t = tile_origin(tiles_x);
    const int64_t plane = (int64_t)N * H * W * C;

    for (int n = blockIdx.y; n < N; n += gridDim.y) {
        // the tile's pivots: its centre pixel (any value would do; one near the tile's values is what helps)
        const int cy = min(t.y0 + kTile / 2, H - 1), cx = min(t.x0 + kTile / 2, W - 1);
        if (threadIdx.x < C) {
            pivots[0][threadIdx.x] = x.ptr[view_offset(x, n, cy, cx, threadIdx.x)];
            pivots[1][threadIdx.x] = y.ptr[view_offset(y, n, cy, cx, threadIdx.x)];
        }
        // outside the image the pivot is staged, so that the padding is an exact zero once the pivot is subtracted
        for (int i = threadIdx.x; i < kSpan * kSpanCols; i += kBlock) {
            const int r = i / kSpanCols, j = i - r * kSpanCols, px = j / C, c = j - px * C;
            const int gy = t.y0 + r - kHalo, gx = t.x0 + px - kHalo;
            const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
            const int ly = in ? gy : cy, lx = in ? gx : cx;
            sx[r * kStride + j] = x.ptr[view_offset(x, n, ly, lx, c)];
            sy[r * kStride + j] = y.ptr[view_offset(y, n, ly, lx, c)];
        }
        __syncthreads();

        for (int i = threadIdx.x; i < kSpan * kCols; i += kBlock) {
            const int r = i / kCols, j = i - r * kCols, c = j % C;
            const float *px = sx + r * kStride + j, *py = sy + r * kStride + j;
            const float p = pivots[0][c], q = pivots[1][c];
            float m1 = 0.0f, m2 = 0.0f, e11 = 0.0f, e22 = 0.0f, e12 = 0.0f;
#pragma unroll
            for (int k = 0; k < kTaps; ++k) {
                const float a = px[k * C] - p, b = py[k * C] - q, w = win.taps[k];
                const float aa = a * a, bb = b * b, ab = a * b;
                m1 = fmaf(w, a, m1);
                m2 = fmaf(w, b, m2);
                e11 = fmaf(w, aa, e11);
                e22 = fmaf(w, bb, e22);
                e12 = fmaf(w, ab, e12);
            }
            moments[0][i] = m1;
            moments[1][i] = m2;
            moments[2][i] = e11;
            moments[3][i] = e22;
            moments[4][i] = e12;
        }
        __syncthreads();

        float l1_sum = 0.0f, ssim_sum = 0.0f;
#pragma unroll
        for (int i = threadIdx.x; i < kTile * kCols; i += kBlock) {  // C rounds
            const int r = i / kCols, j = i - r * kCols, px = j / C, c = j - px * C;
            const int gy = t.y0 + r, gx = t.x0 + px;
            float m1 = 0.0f, m2 = 0.0f, e11 = 0.0f, e22 = 0.0f, e12 = 0.0f;
#pragma unroll
            for (int k = 0; k < kTaps; ++k) {
                const float w = win.taps[k];
                const int at = (r + k) * kCols + j;
                m1 = fmaf(w, moments[0][at], m1);
                m2 = fmaf(w, moments[1][at], m2);
                e11 = fmaf(w, moments[2][at], e11);
                e22 = fmaf(w, moments[3][at], e22);
                e12 = fmaf(w, moments[4][at], e12);
            }
            if (gy < H && gx < W) {
                const int centre = (r + kHalo) * kStride + j + kHalo * C;
                // 1 - the window weight inside the image, per axis: the taps' own deficit plus the taps cut off
                float dy = deficit, dx = deficit;
#pragma unroll
                for (int k = 0; k < kTaps; ++k) {
                    const int yy = gy + k - kHalo, xx = gx + k - kHalo;
                    dy += yy < 0 || yy >= H ? win.taps[k] : 0.0f;
                    dx += xx < 0 || xx >= W ? win.taps[k] : 0.0f;
                }
                const float lack = dy + dx - dy * dx, weight = 1.0f - lack;
                // back from the pivoted moments (header comment): x = x' + p inside the image, 0 outside
                const float p = pivots[0][c], q = pivots[1][c], pw = p * weight, qw = q * weight;
                const float s1 = (e11 - m1 * m1) + lack * (2.0f * p * m1 + p * pw);
                const float s2 = (e22 - m2 * m2) + lack * (2.0f * q * m2 + q * qw);
                const float s12 = (e12 - m1 * m2) + lack * (q * m1 + p * m2 + p * qw);
                m1 += pw;
                m2 += qw;
                const float m11 = m1 * m1, m22 = m2 * m2, m12 = m1 * m2;
                const float A1 = 2.0f * m12 + kC1, A2 = 2.0f * s12 + kC2;
                const float B1 = m11 + m22 + kC1, B2 = s1 + s2 + kC2;
                const float inv = 1.0f / (B1 * B2);
                l1_sum += fabsf(sx[centre] - sy[centre]);
                ssim_sum += A1 * A2 * inv;
                if (maps) {
                    const float d_e11 = -A1 * A2 * inv / B2;
                    const float d_e12 = 2.0f * A1 * inv;
                    const float d_m1 =
                        2.0f * m2 * A2 * inv - 2.0f * m1 * A1 * A2 * inv / B1 - 2.0f * m1 * d_e11 - m2 * d_e12;
                    const int64_t at = (((int64_t)n * H + gy) * W + gx) * C + c;
                    maps[at] = d_e11;
                    maps[plane + at] = d_e12;
                    maps[2 * plane + at] = d_m1;
                }
            }
        }

        // fixed order: a shuffle tree inside each wave, then the waves in ascending order
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1) {
            l1_sum += __shfl_down(l1_sum, off, kWave);
            ssim_sum += __shfl_down(ssim_sum, off, kWave);
        }
        if (threadIdx.x % kWave == 0) {
            wave_sums[0][threadIdx.x / kWave] = l1_sum;
            wave_sums[1][threadIdx.x / kWave] = ssim_sum;
        }
        __syncthreads();  // also: the tile's LDS is free for the next image
        if (threadIdx.x < 2) {
            float s = 0.0f;
            for (int w = 0; w < kWaves; ++w) s += wave_sums[threadIdx.x][w];
            partial[((int64_t)n * gridDim.x + blockIdx.x) * 2 + threadIdx.x] = s;
        }
        __syncthreads();
    }
}

// grid (N), block 64: sums [2, N]
__global__ __launch_bounds__(kWave) void finalize_kernel(int N, int tiles, const float *__restrict__ partial,
                                                         float *__restrict__ sums) {
    const int n = blockIdx.x;
    const float *p = partial + (int64_t)n * tiles * 2;
    float l1_sum = 0.0f, ssim_sum = 0.0f;
    for (int s = threadIdx.x; s < tiles; s += kWave) {
        l1_sum += p[2 * s];
        ssim_sum += p[2 * s + 1];
    }
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {  // wave_sum's order (wave_ops.h); two calls cost two more VGPRs
        l1_sum += __shfl_xor(l1_sum, off, kWave);
        ssim_sum += __shfl_xor(ssim_sum, off, kWave);
    }
    if (threadIdx.x == 0) {
        sums[n] = l1_sum;
        sums[(int64_t)N + n] = ssim_sum;
    }
}

// grid (tiles of one image, min(N, 65535)); maps [3, N, H, W, C] in the forward's order; gx [N, H, W, C]
template <int C>
__global__ __launch_bounds__(kBlock) void backward_kernel(int N, int H, int W, amav_image_view x, amav_image_view y,
                                                          amav_image_loss_window win, int tiles_x,
                                                          const float *__restrict__ maps,
                                                          const float *__restrict__ g_l1,
                                                          const float *__restrict__ g_ssim,
                                                          float *__restrict__ gx_out) {
    constexpr int kCols = kTile * C, kSpanCols = kSpan * C, kStride = stage_stride(C);
    __shared__ float staged[3][kSpan * kStride];
    __shared__ float rows[3][kSpan * kCols];
    const Tile t = tile_origin(tiles_x);
    const int64_t plane = (int64_t)N * H * W * C;

    for (int n = blockIdx.y; n < N; n += gridDim.y) {
        for (int i = threadIdx.x; i < kSpan * kSpanCols; i += kBlock) {
            const int r = i / kSpanCols, j = i - r * kSpanCols, px = j / C, c = j - px * C;
            const int gy = t.y0 + r - kHalo, gx = t.x0 + px - kHalo;
            const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
            const int64_t at = in ? (((int64_t)n * H + gy) * W + gx) * C + c : 0;
#pragma unroll
            for (int m = 0; m < 3; ++m) staged[m][r * kStride + j] = in ? maps[m * plane + at] : 0.0f;
        }
        __syncthreads();

        for (int i = threadIdx.x; i < kSpan * kCols; i += kBlock) {
            const int r = i / kCols, j = i - r * kCols;
            float acc[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int k = 0; k < kTaps; ++k)
#pragma unroll
                for (int m = 0; m < 3; ++m) acc[m] = fmaf(win.taps[k], staged[m][r * kStride + j + k * C], acc[m]);
#pragma unroll
            for (int m = 0; m < 3; ++m) rows[m][i] = acc[m];
        }
        __syncthreads();

        const float gl = g_l1[n], gs = g_ssim[n];
#pragma unroll
        for (int i = threadIdx.x; i < kTile * kCols; i += kBlock) {  // C rounds
            const int r = i / kCols, j = i - r * kCols, px = j / C, c = j - px * C;
            const int gy = t.y0 + r, gx = t.x0 + px;
            float acc[3] = {0.0f, 0.0f, 0.0f};  // conv of d_e11, d_e12, d_m1
#pragma unroll
            for (int k = 0; k < kTaps; ++k)
#pragma unroll
                for (int m = 0; m < 3; ++m) acc[m] = fmaf(win.taps[k], rows[m][(r + k) * kCols + j], acc[m]);
            if (gy < H && gx < W) {
                const float a = x.ptr[view_offset(x, n, gy, gx, c)], b = y.ptr[view_offset(y, n, gy, gx, c)];
                const float d = a - b;
                const float sign = (float)(d > 0.0f) - (float)(d < 0.0f);
                gx_out[(((int64_t)n * H + gy) * W + gx) * C + c] =
                    gl * sign + gs * (acc[2] + 2.0f * a * acc[0] + b * acc[1]);
            }
        }
        __syncthreads();  // the tile's LDS is free for the next image
    }
}

// f(std::integral_constant<int, C>) for the C = 1..4 the kernels are instantiated for
template <typename F>
inline void for_channels(int C, F &&f) {
    switch (C) {
        case 1: f(std::integral_constant<int, 1>{}); break;
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 3: f(std::integral_constant<int, 3>{}); break;
        default: f(std::integral_constant<int, 4>{}); break;
    }
}

struct Shape {
    int tiles_x, tiles;
};

inline Shape shape_of(int H, int W) {
    const int tx = (W + kTile - 1) / kTile, ty = (H + kTile - 1) / kTile;
    return {tx, tx * ty};  // H * W <= 2^31 - 1: the product fits
}

inline size_t workspace_bytes(int N, int H, int W) { return (size_t)N * shape_of(H, W).tiles * 2 * sizeof(float); }

// the checks the three entry points share; `what` names the entry point
inline int check_sizes(const char *what, int N, int H, int W, int C) {
    AMAV_REQUIRE(N >= 0 && H >= 0 && W >= 0, "%s: negative count N=%d H=%d W=%d", what, N, H, W);
    AMAV_REQUIRE(C >= 1 && C <= 4, "%s: channels=%d outside 1..4", what, C);
    AMAV_REQUIRE((int64_t)H * W * C <= INT_MAX, "%s: H * W * C exceeds 2^31 - 1 per image (H=%d W=%d C=%d)", what, H, W,
                 C);
    return AMAV_OK;
}

}  // namespace image_loss
}  // namespace amav

using namespace amav;
using namespace amav::image_loss;

extern "C" size_t amav_image_loss_workspace_bytes(int num_images, int height, int width) {
    if (num_images <= 0 || height <= 0 || width <= 0 || (int64_t)height * width > INT_MAX) return 0;
    return workspace_bytes(num_images, height, width);
}

extern "C" int amav_image_loss_forward(int num_images, int height, int width, int channels, const amav_image_view *x,
                                       const amav_image_view *y, const amav_image_loss_window *window, float *sums_dev,
                                       float *maps_dev, void *workspace_dev, size_t workspace_bytes_, void *stream_) {
    const int N = num_images, H = height, W = width, C = channels;
    if (int rc = check_sizes("amav_image_loss_forward", N, H, W, C)) return rc;
    if (N == 0 || H == 0 || W == 0) return AMAV_OK;  // an empty problem
    AMAV_REQUIRE(x && y && window, "amav_image_loss_forward: NULL pointer (x / y / window)");
    AMAV_REQUIRE(x->ptr && y->ptr, "amav_image_loss_forward: NULL pointer (x->ptr / y->ptr)");
    AMAV_REQUIRE(sums_dev, "amav_image_loss_forward: NULL pointer (sums)");
    const size_t need = workspace_bytes(N, H, W);
    if (!workspace_dev || workspace_bytes_ < need)
        return fail(AMAV_ERR_WORKSPACE, "amav_image_loss_forward: workspace of %zu bytes, %zu needed",
                    workspace_dev ? workspace_bytes_ : (size_t)0, need);
    const Shape s = shape_of(H, W);
    const dim3 grid((unsigned)s.tiles, (unsigned)N < kGridMax ? (unsigned)N : kGridMax);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    float *partial = static_cast<float *>(workspace_dev);
    double sum = 0.0;
    for (int k = 0; k < kTaps; ++k) sum += window->taps[k];
    const float deficit = (float)(1.0 - sum);
    for_channels(C, [&](auto c) {
        forward_kernel<decltype(c)::value><<<grid, kBlock, 0, stream>>>(N, H, W, *x, *y, *window, deficit, s.tiles_x, partial,
                                                                       maps_dev);
    });
    if (int rc = check_launch("amav_image_loss_forward: forward_kernel")) return rc;
    finalize_kernel<<<(unsigned)N, kWave, 0, stream>>>(N, s.tiles, partial, sums_dev);
    return check_launch("amav_image_loss_forward: finalize_kernel");
}

extern "C" int amav_image_loss_backward(int num_images, int height, int width, int channels, const amav_image_view *x,
                                        const amav_image_view *y, const amav_image_loss_window *window,
                                        const float *maps_dev, const float *grad_l1_dev, const float *grad_ssim_dev,
                                        float *grad_x_dev, void *stream_) {
    const int N = num_images, H = height, W = width, C = channels;
    if (int rc = check_sizes("amav_image_loss_backward", N, H, W, C)) return rc;
    if (N == 0 || H == 0 || W == 0) return AMAV_OK;  // an empty grad_x
    AMAV_REQUIRE(x && y && window, "amav_image_loss_backward: NULL pointer (x / y / window)");
    AMAV_REQUIRE(x->ptr && y->ptr, "amav_image_loss_backward: NULL pointer (x->ptr / y->ptr)");
    AMAV_REQUIRE(maps_dev && grad_l1_dev && grad_ssim_dev && grad_x_dev,
                 "amav_image_loss_backward: NULL pointer (maps / grad_l1 / grad_ssim / grad_x)");
    const Shape s = shape_of(H, W);
    const dim3 grid((unsigned)s.tiles, (unsigned)N < kGridMax ? (unsigned)N : kGridMax);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    for_channels(C, [&](auto c) {
        backward_kernel<decltype(c)::value><<<grid, kBlock, 0, stream>>>(N, H, W, *x, *y, *window, s.tiles_x, maps_dev,
                                                                        grad_l1_dev, grad_ssim_dev, grad_x_dev);
    });
    return check_launch("amav_image_loss_backward: backward_kernel");
}
