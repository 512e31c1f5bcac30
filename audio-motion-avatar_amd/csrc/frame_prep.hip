// Training-clip frame preparation (include/amav.h, amav_frames_prepare): what the reference's dataset does to every
// decoded frame on the CPU (src/datasets/dataset_speech_vid.py:170-252, pad_image :319-331), in at most three launches.
//
//   images   composite over white with the mask, padded with ones to Hp x Wp.  Flat over one [Hp,Wp] plane in groups of
//            four floats that are aligned in the whole tensor, so every full group is one 16-byte store whatever Wp is.
//            Its first block per frame also initialises the frame's row of the box table (when there is no images
//            output, a launch of that part alone does).
//   box      bounding box of mask != 0 per frame: per-thread integer min / max, block reduction through LDS, then one
//            atomicMin / atomicMax per bound and block on the table (integers: the result does not depend on the order).
//   cropped  one thread per four consecutive output x.  The block derives the frame's crop box from the table in scalar
//            registers (dataset_speech_vid.py:198-216 in integers), the first block of a frame records it in `boxes`,
//            and every tap of the align_corners=True bilinear resolves to the squaring pad, the pad_ratio border (both 1)
//            or a frame pixel composited on the fly, so `images` never has to exist for `cropped` to be right.
//
// All arithmetic on pixel values is fp32 with contraction off, one rounding per operator, so the NumPy model of the tests
// (tests/frame_prep_model.py) reproduces the composite bit for bit.
#include <climits>
#include <type_traits>

#include "amav_common.h"
#include "wave_ops.h"

#pragma clang fp contract(off)

namespace amav {
namespace {

struct PrepSrc {
    const void *frames;
    const void *masks;  // nullptr: all ones
    long long fs_f, ms_f;                // frame strides, elements
    unsigned fs_c, fs_y, fs_x, ms_y, ms_x;  // strides inside a frame: the host checks that a frame's view stays below 2^31
    int frames_f32, masks_f32;
    int H, W, Hp, Wp, oy, ox;
};

struct PrepNorm {
    float mean[3], std[3];
    int on;
};

// byte / 255.0f, the dataset's `float() / 255.0`: the IEEE division is done once per block and value, not per tap
__device__ inline void fill_unit_table(float *unit) {
    for (int i = threadIdx.x; i < 256; i += blockDim.x) unit[i] = static_cast<float>(i) / 255.0f;
    __syncthreads();
}

// one frame's pixels and mask; `at` = offset inside the frame in elements.  The element types are template parameters
// (IF32: fp32 frames; MK: 0 no mask, 1 uint8, 2 fp32): chosen at run time, every load would sit behind a branch and
// wait for the one before it.
template <bool IF32, int MK>
struct PrepFrame {
    const void *img, *mask;
    const float *unit;
    __device__ PrepFrame(const PrepSrc &s, int f, const float *unit_table) : unit(unit_table) {
        img = IF32 ? static_cast<const void *>(static_cast<const float *>(s.frames) + f * s.fs_f)
                   : static_cast<const void *>(static_cast<const uint8_t *>(s.frames) + f * s.fs_f);
        mask = MK == 2 ? static_cast<const void *>(static_cast<const float *>(s.masks) + f * s.ms_f)
                       : static_cast<const void *>(static_cast<const uint8_t *>(s.masks) + f * s.ms_f);
    }
    __device__ float pixel(unsigned at) const {
        if constexpr (IF32) return static_cast<const float *>(img)[at];
        else return unit[static_cast<const uint8_t *>(img)[at]];
    }
    __device__ float coverage(unsigned at) const {
        if constexpr (MK == 0) return 1.0f;
        else if constexpr (MK == 2) return static_cast<const float *>(mask)[at];
        else return unit[static_cast<const uint8_t *>(mask)[at]];
    }
};

// image * mask + (1 - mask), every operator rounded on its own (dataset_speech_vid.py:184)
__device__ inline float composite(float img, float m) { return img * m + (1.0f - m); }

__device__ inline void init_table_row(int32_t *table, int f, const PrepSrc &s, int lane) {
    if (lane < 4) {
        const bool lower = (lane & 1) == 0;  // y_min, y_max, x_min, x_max
        int v = lower ? INT_MAX : -1;
        if (!s.masks) v = lower ? 0 : (lane == 1 ? s.H - 1 : s.W - 1);  // all ones: the box is the frame
        table[f * 4 + lane] = v;
    }
}

__global__ void __launch_bounds__(64) prep_init_table_kernel(PrepSrc s, int32_t *table) {
    init_table_row(table, blockIdx.x, s, threadIdx.x);
}

// grid (groups of one plane / 256, 3 F).  `images` is 16-byte aligned; group g of plane p covers the tensor's elements
// [a0 + 4 g, a0 + 4 g + 4) with a0 = the plane's first element rounded down to a multiple of four.
template <bool IF32, int MK>
__global__ void __launch_bounds__(256) prep_images_kernel(PrepSrc s, float *__restrict__ images, int32_t *table) {
    const int plane = blockIdx.y, f = plane / 3, c = plane - 3 * f;
    if (table && c == 0 && blockIdx.x == 0) init_table_row(table, f, s, threadIdx.x);
    __shared__ float unit[256];
    fill_unit_table(unit);
    const PrepFrame<IF32, MK> frame(s, f, unit);
    const long long plane_elems = static_cast<long long>(s.Hp) * s.Wp;
    const long long base = plane * plane_elems, a0 = base & ~3LL;
    const long long first = a0 + 4LL * (static_cast<long long>(blockIdx.x) * 256 + threadIdx.x);
    if (first >= base + plane_elems) return;
    float v[4];
    long long local = first - base;  // may be -3..-1 for the plane's first group
    const unsigned within = local >= 0 ? static_cast<unsigned>(local) : 0u;  // Hp Wp < 2^32: a 32-bit division
    int y = static_cast<int>(within / static_cast<unsigned>(s.Wp));
    int x = local >= 0 ? static_cast<int>(within - static_cast<unsigned>(y) * s.Wp) : static_cast<int>(local);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int fy = y - s.oy, fx = x - s.ox;
        const bool inside = x >= 0 && y < s.Hp && fy >= 0 && fy < s.H && fx >= 0 && fx < s.W;
        // the loads are unconditional (clamped into the frame) so that the four of a thread are in flight together
        const unsigned cy = min(max(fy, 0), s.H - 1), cx = min(max(fx, 0), s.W - 1);
        const float lit = composite(frame.pixel(c * s.fs_c + cy * s.fs_y + cx * s.fs_x), frame.coverage(cy * s.ms_y + cx * s.ms_x));
        const float val = inside ? lit : 1.0f;
        v[k] = val;
        if (++x == s.Wp) { x = 0; ++y; }
    }
    if (local >= 0 && local + 4 <= plane_elems) {
        *reinterpret_cast<float4 *>(images + first) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (local + k >= 0 && local + k < plane_elems) images[first + k] = v[k];
    }
}

// Box reduction shape.  Default: blocks of 256 threads, kBoxItems groups of four x per thread, as many blocks per frame
// as that takes, joined by integer atomics on the table.  -DAMAV_PREP_BOX_ONE_BLOCK=1 builds the alternative it was
// measured against (tools/time_frame_prep.py): one block of 1024 threads per frame.
#ifndef AMAV_PREP_BOX_ONE_BLOCK
#define AMAV_PREP_BOX_ONE_BLOCK 0
#endif
constexpr int kBoxThreads = AMAV_PREP_BOX_ONE_BLOCK ? 1024 : 256;
constexpr int kBoxItems = 4;

// grid (blocks per frame, F); the blocks of a frame stride over its H x ceil(W/4) groups
__global__ void __launch_bounds__(kBoxThreads) prep_box_kernel(PrepSrc s, int32_t *table) {
    const int f = blockIdx.y;
    const unsigned gpr = (s.W + 3) >> 2, groups = s.H * gpr;  // H, W <= 65535: below 2^30, 32-bit divisions
    int y_min = INT_MAX, y_max = -1, x_min = INT_MAX, x_max = -1;
    for (unsigned g = blockIdx.x * kBoxThreads + threadIdx.x; g < groups; g += gridDim.x * kBoxThreads) {
        const int y = static_cast<int>(g / gpr), x0 = static_cast<int>(g - y * gpr) * 4;
        unsigned hit = 0;  // bit k: mask(y, x0 + k) != 0
        const long long o = f * s.ms_f + static_cast<long long>(y) * s.ms_y + static_cast<long long>(x0) * s.ms_x;
        if (s.masks_f32) {
            const float *p = static_cast<const float *>(s.masks) + o;
            if (s.ms_x == 1 && x0 + 3 < s.W && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
                const float4 m = *reinterpret_cast<const float4 *>(p);
                hit = (m.x != 0.0f) | (m.y != 0.0f) << 1 | (m.z != 0.0f) << 2 | (m.w != 0.0f) << 3;
            } else {
                for (int k = 0; k < 4 && x0 + k < s.W; ++k) hit |= (p[k * s.ms_x] != 0.0f) << k;
            }
        } else {
            const uint8_t *p = static_cast<const uint8_t *>(s.masks) + o;
            if (s.ms_x == 1 && x0 + 3 < s.W && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
                const uint32_t m = *reinterpret_cast<const uint32_t *>(p);
                hit = ((m & 0xffu) != 0) | ((m & 0xff00u) != 0) << 1 | ((m & 0xff0000u) != 0) << 2 | ((m >> 24) != 0) << 3;
            } else {
                for (int k = 0; k < 4 && x0 + k < s.W; ++k) hit |= (p[k * s.ms_x] != 0) << k;
            }
        }
        if (hit) {
            y_min = min(y_min, y);
            y_max = max(y_max, y);
            x_min = min(x_min, x0 + __ffs(hit) - 1);
            x_max = max(x_max, x0 + 31 - __clz(hit));
        }
    }
    y_min = wave_min(y_min), y_max = wave_max(y_max), x_min = wave_min(x_min), x_max = wave_max(x_max);
    constexpr int kWaves = kBoxThreads / kWave;
    __shared__ int part[kWaves][4];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        part[wave][0] = y_min; part[wave][1] = y_max; part[wave][2] = x_min; part[wave][3] = x_max;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        const int b = threadIdx.x;
        int v = part[0][b];
        int seen = part[0][1];
        for (int w = 1; w < kWaves; ++w) {
            v = (b & 1) ? max(v, part[w][b]) : min(v, part[w][b]);
            seen = max(seen, part[w][1]);
        }
        if (seen >= 0) {  // the block saw a set pixel
            if (b & 1) atomicMax(&table[f * 4 + b], v);
            else atomicMin(&table[f * 4 + b], v);
        }
    }
}

struct CropBox {
    int y0, y1, x0, x1, side, top, left;
};

// dataset_speech_vid.py:189-238 in integers; the clamps are against the unpadded frame, the box is applied to the
// padded image.  int(e * 0.2) == e / 5 for every extent below 131072.
__device__ inline CropBox crop_box(const int32_t *row, const PrepSrc &s) {
    int y0 = row[0], y1 = row[1], x0 = row[2], x1 = row[3];
    if (y1 < 0) {  // empty mask: the whole padded image
        y0 = 0; y1 = s.Hp - 1; x0 = 0; x1 = s.Wp - 1;
    } else {
        const int py = (y1 - y0) / 5, px = (x1 - x0) / 5;
        y0 = max(0, y0 - py); y1 = min(s.H - 1, y1 + py);
        x0 = max(0, x0 - px); x1 = min(s.W - 1, x1 + px);
        const int half = max(y1 - y0, x1 - x0) / 2, cy = (y0 + y1) / 2, cx = (x0 + x1) / 2;
        y0 = max(0, cy - half); y1 = min(s.H - 1, cy + half);
        x0 = max(0, cx - half); x1 = min(s.W - 1, cx + half);
    }
    const int h = y1 - y0 + 1, w = x1 - x0 + 1, side = max(h, w);
    return {y0, y1, x0, x1, side, (side - h) / 2, (side - w) / 2};
}

// coordinate in the virtual square -> frame coordinate, or -1 where the square or the pad_ratio border holds a one
__device__ inline int resolve(int v, int pad, int lo, int hi, int offset, int extent) {
    const int p = v - pad + lo;  // in the padded image
    const int q = p - offset;
    return (p < lo || p > hi || q < 0 || q >= extent) ? -1 : q;
}

// grid (ceil(S x (S / V) / 256), F); V = 4 needs S % 4 == 0.  cropped == nullptr: one block per frame records the box.
template <int V, bool IF32, int MK>
__global__ void __launch_bounds__(256) prep_cropped_kernel(PrepSrc s, PrepNorm norm, const int32_t *table, int S,
                                                           float *__restrict__ cropped, int32_t *__restrict__ boxes) {
    const int f = blockIdx.y;
    const CropBox b = crop_box(table + f * 4, s);
    if (boxes && blockIdx.x == 0 && threadIdx.x == 0) {
        int32_t *o = boxes + f * 5;
        o[0] = b.y0; o[1] = b.y1; o[2] = b.x0; o[3] = b.x1; o[4] = b.side;
    }
    if (!cropped) return;
    __shared__ float unit[256];
    fill_unit_table(unit);
    const PrepFrame<IF32, MK> frame(s, f, unit);
    const unsigned gpr = S / V, g = blockIdx.x * 256 + threadIdx.x;  // S <= 65535: S gpr < 2^32, and so is the grid
    if (g >= S * gpr) return;
    const int oy = static_cast<int>(g / gpr), ox = static_cast<int>(g - oy * gpr) * V;
    const float scale = S > 1 ? static_cast<float>(b.side - 1) / static_cast<float>(S - 1) : 0.0f;

    const float sy = scale * static_cast<float>(oy);
    const int iy0 = static_cast<int>(sy), iy1 = min(iy0 + 1, b.side - 1);
    const float hy1 = sy - static_cast<float>(iy0), hy0 = 1.0f - hy1;
    const int fy[2] = {resolve(iy0, b.top, b.y0, b.y1, s.oy, s.H), resolve(iy1, b.top, b.y0, b.y1, s.oy, s.H)};

    float wx0[V], wx1[V], p[3][2][V][2];
#pragma unroll
    for (int k = 0; k < V; ++k) {
        const float sx = scale * static_cast<float>(ox + k);
        const int ix0 = static_cast<int>(sx), ix1 = min(ix0 + 1, b.side - 1);
        wx1[k] = sx - static_cast<float>(ix0);
        wx0[k] = 1.0f - wx1[k];
        const int fx[2] = {resolve(ix0, b.left, b.x0, b.x1, s.ox, s.W), resolve(ix1, b.left, b.x0, b.x1, s.ox, s.W)};
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                // unconditional loads (a tap outside the frame reads pixel 0 of its row or column and is replaced by a
                // one), so that all 64 of a thread are in flight together instead of one round trip per tap
                const bool inside = fy[r] >= 0 && fx[t] >= 0;
                const unsigned cy = max(fy[r], 0), cx = max(fx[t], 0);
                const float m = frame.coverage(cy * s.ms_y + cx * s.ms_x);
                const unsigned at = cy * s.fs_y + cx * s.fs_x;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float lit = composite(frame.pixel(at + c * s.fs_c), m);  // loaded before the choice
                    p[c][r][k][t] = inside ? lit : 1.0f;
                }
            }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float v[V];
#pragma unroll
        for (int k = 0; k < V; ++k) {
            v[k] = hy0 * (wx0[k] * p[c][0][k][0] + wx1[k] * p[c][0][k][1]) +
                   hy1 * (wx0[k] * p[c][1][k][0] + wx1[k] * p[c][1][k][1]);
            if (norm.on) v[k] = (v[k] - norm.mean[c]) / norm.std[c];
        }
        float *o = cropped + ((static_cast<long long>(f) * 3 + c) * S + oy) * S + ox;
        if constexpr (V == 4) *reinterpret_cast<float4 *>(o) = make_float4(v[0], v[1], v[2], v[3]);
        else o[0] = v[0];
    }
}

// the kernel instance for the element types of this call
template <typename Launch>
void dispatch(int frames_f32, int mask_kind, Launch launch) {
    auto with_frames = [&](auto kind) {
        if (frames_f32) launch(std::true_type{}, kind);
        else launch(std::false_type{}, kind);
    };
    if (mask_kind == 0) with_frames(std::integral_constant<int, 0>{});
    else if (mask_kind == 1) with_frames(std::integral_constant<int, 1>{});
    else with_frames(std::integral_constant<int, 2>{});
}

constexpr int kMaxExtent = 65535;  // of H, W, Hp, Wp and S: every plane stays below 2^32 elements
constexpr int kMaxFrames = 16384;  // 3 F is a grid dimension

}  // namespace
}  // namespace amav

using namespace amav;

extern "C" size_t amav_frames_prepare_workspace_bytes(int num_frames) {
    if (num_frames < 1 || num_frames > kMaxFrames) return 0;
    return align_up(static_cast<size_t>(num_frames) * 4 * sizeof(int32_t), 256);
}

extern "C" int amav_frames_prepare(int num_frames, int height, int width, const void *frames_dev, int frames_are_f32,
                                   int64_t frame_stride_f, int64_t frame_stride_c, int64_t frame_stride_y,
                                   int64_t frame_stride_x, const void *masks_dev, int masks_are_f32, int64_t mask_stride_f,
                                   int64_t mask_stride_y, int64_t mask_stride_x, int padded_height, int padded_width,
                                   int offset_y, int offset_x, int crop_side, const float *mean_host3,
                                   const float *std_host3, float *images_dev, size_t images_bytes, float *cropped_dev,
                                   size_t cropped_bytes, int32_t *boxes_dev, size_t boxes_bytes, void *workspace_dev,
                                   size_t workspace_bytes, void *stream) {
    const int F = num_frames, H = height, W = width, Hp = padded_height, Wp = padded_width, S = crop_side;
    AMAV_REQUIRE(frames_dev, "amav_frames_prepare: NULL frames");
    AMAV_REQUIRE(F >= 1 && F <= kMaxFrames, "amav_frames_prepare: F=%d outside 1..%d", F, kMaxFrames);
    AMAV_REQUIRE(H >= 1 && H <= kMaxExtent && W >= 1 && W <= kMaxExtent, "amav_frames_prepare: H=%d W=%d outside 1..%d", H, W,
                 kMaxExtent);
    AMAV_REQUIRE(Hp >= H && Wp >= W && Hp <= kMaxExtent && Wp <= kMaxExtent,
                 "amav_frames_prepare: padded size %d x %d is not within frame size %d x %d .. %d", Hp, Wp, H, W, kMaxExtent);
    AMAV_REQUIRE(offset_y >= 0 && offset_y <= Hp - H && offset_x >= 0 && offset_x <= Wp - W,
                 "amav_frames_prepare: offsets (%d, %d) put the frame outside the padded image", offset_y, offset_x);
    AMAV_REQUIRE(S >= 1 && S <= kMaxExtent, "amav_frames_prepare: crop_side %d outside 1..%d", S, kMaxExtent);
    AMAV_REQUIRE((frames_are_f32 | 1) == 1 && (masks_are_f32 | 1) == 1, "amav_frames_prepare: the *_are_f32 flags are 0 or 1");
    {
        const int64_t strides[7] = {frame_stride_c, frame_stride_y, frame_stride_x, mask_stride_y, mask_stride_x, 0, 0};
        bool ok = true;
        for (int64_t v : strides) ok = ok && v >= 0 && v < (int64_t(1) << 31);
        ok = ok && 2 * frame_stride_c + (H - 1) * frame_stride_y + (W - 1) * frame_stride_x < (int64_t(1) << 31) &&
             (H - 1) * mask_stride_y + (W - 1) * mask_stride_x < (int64_t(1) << 31);
        AMAV_REQUIRE(ok, "amav_frames_prepare: a stride inside a frame is negative or a frame's view spans 2^31 elements or more");
    }
    AMAV_REQUIRE((mean_host3 == nullptr) == (std_host3 == nullptr), "amav_frames_prepare: mean and std come together");
    PrepNorm norm = {};
    if (std_host3) {
        for (int c = 0; c < 3; ++c) {
            AMAV_REQUIRE(std_host3[c] != 0.0f && std_host3[c] == std_host3[c] && mean_host3[c] == mean_host3[c],
                         "amav_frames_prepare: std[%d] is zero or a value is NaN", c);
            norm.mean[c] = mean_host3[c];
            norm.std[c] = std_host3[c];
        }
        norm.on = 1;
    }
    AMAV_REQUIRE(aligned16(images_dev, cropped_dev) && (reinterpret_cast<uintptr_t>(boxes_dev) & 3) == 0 &&
                     (reinterpret_cast<uintptr_t>(frames_dev) & (frames_are_f32 ? 3 : 0)) == 0 &&
                     (reinterpret_cast<uintptr_t>(masks_dev) & (masks_are_f32 ? 3 : 0)) == 0,
                 "amav_frames_prepare: misaligned buffer (images, cropped: 16 bytes; boxes, fp32 inputs: 4)");
    const size_t images_need = static_cast<size_t>(F) * 3 * Hp * Wp * sizeof(float);
    const size_t cropped_need = static_cast<size_t>(F) * 3 * S * S * sizeof(float);
    const size_t boxes_need = static_cast<size_t>(F) * 5 * sizeof(int32_t);
    if (images_dev && images_bytes < images_need)
        return fail(AMAV_ERR_WORKSPACE, "amav_frames_prepare: images buffer %zu < %zu bytes", images_bytes, images_need);
    if (cropped_dev && cropped_bytes < cropped_need)
        return fail(AMAV_ERR_WORKSPACE, "amav_frames_prepare: cropped buffer %zu < %zu bytes", cropped_bytes, cropped_need);
    if (boxes_dev && boxes_bytes < boxes_need)
        return fail(AMAV_ERR_WORKSPACE, "amav_frames_prepare: boxes buffer %zu < %zu bytes", boxes_bytes, boxes_need);
    const bool need_box = cropped_dev || boxes_dev;
    const size_t ws_need = amav_frames_prepare_workspace_bytes(F);
    if (need_box) {
        if (!workspace_dev || workspace_bytes < ws_need)
            return fail(AMAV_ERR_WORKSPACE, "amav_frames_prepare: workspace %zu < %zu bytes", workspace_dev ? workspace_bytes : 0, ws_need);
        if (reinterpret_cast<uintptr_t>(workspace_dev) & 15)
            return fail(AMAV_ERR_WORKSPACE, "amav_frames_prepare: workspace is not 16-byte aligned");
    }

    hipStream_t st = static_cast<hipStream_t>(stream);
    PrepSrc s;
    s.frames = frames_dev; s.masks = masks_dev;
    s.fs_f = frame_stride_f; s.ms_f = mask_stride_f;
    s.fs_c = static_cast<unsigned>(frame_stride_c); s.fs_y = static_cast<unsigned>(frame_stride_y);
    s.fs_x = static_cast<unsigned>(frame_stride_x);
    s.ms_y = static_cast<unsigned>(mask_stride_y); s.ms_x = static_cast<unsigned>(mask_stride_x);
    s.frames_f32 = frames_are_f32; s.masks_f32 = masks_are_f32;
    s.H = H; s.W = W; s.Hp = Hp; s.Wp = Wp; s.oy = offset_y; s.ox = offset_x;
    int32_t *table = need_box ? static_cast<int32_t *>(workspace_dev) : nullptr;
    const int mk = !masks_dev ? 0 : masks_are_f32 ? 2 : 1;

    if (images_dev) {
        const long long groups = (static_cast<long long>(Hp) * Wp + 3) / 4 + 1;  // + 1: a plane may start inside a group
        const dim3 grid(blocks_for(groups), 3 * F);
        dispatch(frames_are_f32, mk, [&](auto if32, auto kind) {
            prep_images_kernel<decltype(if32)::value, decltype(kind)::value><<<grid, 256, 0, st>>>(s, images_dev, table);
        });
        if (int rc = check_launch("amav_frames_prepare (images)")) return rc;
    } else if (need_box) {
        prep_init_table_kernel<<<F, 64, 0, st>>>(s, table);
        if (int rc = check_launch("amav_frames_prepare (table)")) return rc;
    }
    if (!need_box) return AMAV_OK;
    if (masks_dev) {
        const long long groups = static_cast<long long>(H) * ((W + 3) / 4);
        const long long per_block = static_cast<long long>(kBoxThreads) * kBoxItems;
        const unsigned blocks = AMAV_PREP_BOX_ONE_BLOCK ? 1u : static_cast<unsigned>((groups + per_block - 1) / per_block);
        prep_box_kernel<<<dim3(blocks, F), kBoxThreads, 0, st>>>(s, table);
        if (int rc = check_launch("amav_frames_prepare (box)")) return rc;
    }
    dispatch(frames_are_f32, mk, [&](auto if32, auto kind) {
        if (cropped_dev && S % 4 == 0) {
            const dim3 grid(blocks_for(static_cast<long long>(S) * (S / 4)), F);
            prep_cropped_kernel<4, decltype(if32)::value, decltype(kind)::value><<<grid, 256, 0, st>>>(s, norm, table, S, cropped_dev, boxes_dev);
        } else {
            const dim3 grid(cropped_dev ? blocks_for(static_cast<long long>(S) * S) : 1, F);
            prep_cropped_kernel<1, decltype(if32)::value, decltype(kind)::value><<<grid, 256, 0, st>>>(s, norm, table, S, cropped_dev, boxes_dev);
        }
    });
    return check_launch("amav_frames_prepare (cropped)");
}
