// Window cutting for the windowed triplane upsampler (renderer.py, TriplaneUpsampler.forward_tokens_windowed), for
// gfx950: K square windows of size x size are cut out of x [F,C,h,w] (zeros where a window leaves the source), and the
// transpose adds a gradient per window back into grad_x.  Pure data movement next to the library convolutions between
// which it sits: one thread per element, lanes along x, no LDS, no float atomics.
//
//   cut_kernel        thread = one output element (k, c, wy, wx): reads x[f_k, c, oy_k + wy, ox_k + wx] or writes 0.
//   transpose_kernel  thread = one grad_x element (f, c, y, x).  Window corners lie on a lattice, oy = a * step + off_y
//                     and ox = b * step + off_x, and the int32 table [F, A, B] names the window at (a, b) or -1: the
//                     thread walks the <= ceil(size / step)^2 positions whose window covers it and adds them in
//                     ascending window index (repeated selection of the smallest index above the last one: the walk is
//                     a handful of cached table reads, and nothing is kept in an array).  An element no window covers
//                     gets +0.0; every element is written.
// (k, c) and (f, c) are walked with grid strides in y / z, so no count is bounded by a grid dimension; element offsets
// are 64-bit.
#include <climits>
#include <cstddef>

#include "amav_common.h"

namespace amav {
namespace windows {

constexpr int kBlock = 256;
constexpr unsigned kGridMax = 65535;

// grid (ceil(size^2 / 256), min(C, 65535), min(K, 65535))
__global__ __launch_bounds__(kBlock) void cut_kernel(int F, int C, int h, int w, const float *__restrict__ x, int K,
                                                     int size, const int *__restrict__ frame,
                                                     const int *__restrict__ oy, const int *__restrict__ ox,
                                                     float *__restrict__ out) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= size * size) return;
    const int wy = i / size, wx = i - wy * size;
    for (int k = blockIdx.z; k < K; k += gridDim.z) {
        const int f = frame[k];
        // 64-bit: a corner may be any int32
        const long long y = (long long)oy[k] + wy, xx = (long long)ox[k] + wx;
        const bool in = f >= 0 && f < F && y >= 0 && y < h && xx >= 0 && xx < w;
        for (int c = blockIdx.y; c < C; c += gridDim.y) {
            const float v = in ? x[(((size_t)f * C + c) * h + (size_t)y) * w + (size_t)xx] : 0.0f;
            out[((size_t)k * C + c) * size * size + i] = v;
        }
    }
}

__device__ __forceinline__ int floor_div(int a, int b) {  // b > 0
    const int q = a / b;
    return q * b > a ? q - 1 : q;
}

// grid (ceil(h * w / 256), min(C, 65535), min(F, 65535))
__global__ __launch_bounds__(kBlock) void transpose_kernel(int F, int C, int h, int w, int K, int size,
                                                           const float *__restrict__ gw, int step, int off_y, int off_x,
                                                           int A, int B, const int *__restrict__ table,
                                                           float *__restrict__ gx) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= h * w) return;
    const int y = i / w, x = i - y * w;
    // lattice rows a with a * step + off_y <= y < a * step + off_y + size (columns alike)
    const int a0 = max(floor_div(y - off_y - size + step, step), 0), a1 = min(floor_div(y - off_y, step), A - 1);
    const int b0 = max(floor_div(x - off_x - size + step, step), 0), b1 = min(floor_div(x - off_x, step), B - 1);
    for (int f = blockIdx.z; f < F; f += gridDim.z) {
        const int *tf = table + (size_t)f * A * B;
        for (int c = blockIdx.y; c < C; c += gridDim.y) {
            float acc = 0.0f;
            int last = -1;
            while (true) {
                int best = INT_MAX, ba = 0, bb = 0;
                for (int a = a0; a <= a1; ++a)
                    for (int b = b0; b <= b1; ++b) {
                        const int k = tf[(size_t)a * B + b];
                        if (k > last && k < best) best = k, ba = a, bb = b;
                    }
                if (best >= K) break;  // none left (or an index past the windows: never read)
                const int wy = y - (ba * step + off_y), wx = x - (bb * step + off_x);
                acc += gw[(((size_t)best * C + c) * size + wy) * size + wx];
                last = best;
            }
            gx[((size_t)f * C + c) * h * w + i] = acc;
        }
    }
}

inline unsigned grid_dim(int n) { return (unsigned)n < kGridMax ? (unsigned)n : kGridMax; }

}  // namespace windows
}  // namespace amav

using namespace amav;
using namespace amav::windows;

extern "C" int amav_windows_cut(int num_frames, int channels, int height, int width, const float *x_dev,
                                int num_windows, int size, const int32_t *frame_dev, const int32_t *oy_dev,
                                const int32_t *ox_dev, float *out_dev, void *stream_) {
    const int F = num_frames, C = channels, h = height, w = width, K = num_windows;
    AMAV_REQUIRE(F >= 0 && C >= 0 && h >= 0 && w >= 0 && K >= 0,
                 "amav_windows_cut: negative count F=%d C=%d h=%d w=%d K=%d", F, C, h, w, K);
    AMAV_REQUIRE(size > 0, "amav_windows_cut: size=%d must be positive", size);
    AMAV_REQUIRE((int64_t)h * w <= INT_MAX && (int64_t)size * size <= INT_MAX,
                 "amav_windows_cut: h * w or size^2 exceeds 2^31 - 1 (h=%d w=%d size=%d)", h, w, size);
    if (K == 0 || C == 0) return AMAV_OK;  // an empty output
    AMAV_REQUIRE(frame_dev && oy_dev && ox_dev && out_dev, "amav_windows_cut: NULL pointer (frame / oy / ox / out)");
    AMAV_REQUIRE(x_dev || F == 0 || h == 0 || w == 0, "amav_windows_cut: NULL pointer (x)");
    const dim3 grid((unsigned)(((int64_t)size * size + kBlock - 1) / kBlock), grid_dim(C), grid_dim(K));
    cut_kernel<<<grid, kBlock, 0, static_cast<hipStream_t>(stream_)>>>(F, C, h, w, x_dev, K, size, frame_dev, oy_dev,
                                                                       ox_dev, out_dev);
    return check_launch("amav_windows_cut: cut_kernel");
}

extern "C" int amav_windows_cut_backward(int num_frames, int channels, int height, int width, int num_windows, int size,
                                         const float *grad_windows_dev, int step, int off_y, int off_x,
                                         int lattice_rows, int lattice_cols, const int32_t *lattice_dev,
                                         float *grad_x_dev, void *stream_) {
    const int F = num_frames, C = channels, h = height, w = width, K = num_windows, A = lattice_rows, B = lattice_cols;
    AMAV_REQUIRE(F >= 0 && C >= 0 && h >= 0 && w >= 0 && K >= 0 && A >= 0 && B >= 0,
                 "amav_windows_cut_backward: negative count F=%d C=%d h=%d w=%d K=%d lattice %d x %d", F, C, h, w, K, A, B);
    AMAV_REQUIRE(size > 0, "amav_windows_cut_backward: size=%d must be positive", size);
    AMAV_REQUIRE(step > 0, "amav_windows_cut_backward: step=%d must be positive", step);
    AMAV_REQUIRE((int64_t)h * w <= INT_MAX && (int64_t)size * size <= INT_MAX,
                 "amav_windows_cut_backward: h * w or size^2 exceeds 2^31 - 1 (h=%d w=%d size=%d)", h, w, size);
    // every corner a * step + off and every y - off - size + step stays an int32
    const int64_t reach = (int64_t)(A > B ? A : B) * step + size + (h > w ? h : w);
    AMAV_REQUIRE(reach + (off_y < 0 ? -(int64_t)off_y : off_y) <= INT_MAX &&
                     reach + (off_x < 0 ? -(int64_t)off_x : off_x) <= INT_MAX,
                 "amav_windows_cut_backward: lattice %d x %d of step %d with offsets (%d, %d) leaves the int32 range", A, B,
                 step, off_y, off_x);
    if (F == 0 || C == 0 || h == 0 || w == 0) return AMAV_OK;  // an empty grad_x
    AMAV_REQUIRE(grad_x_dev, "amav_windows_cut_backward: NULL pointer (grad_x)");
    AMAV_REQUIRE(lattice_dev || A == 0 || B == 0, "amav_windows_cut_backward: NULL pointer (lattice)");
    AMAV_REQUIRE(grad_windows_dev || K == 0, "amav_windows_cut_backward: NULL pointer (grad_windows)");
    const dim3 grid((unsigned)(((int64_t)h * w + kBlock - 1) / kBlock), grid_dim(C), grid_dim(F));
    transpose_kernel<<<grid, kBlock, 0, static_cast<hipStream_t>(stream_)>>>(F, C, h, w, K, size, grad_windows_dev, step,
                                                                             off_y, off_x, A, B, lattice_dev, grad_x_dev);
    return check_launch("amav_windows_cut_backward: transpose_kernel");
}
