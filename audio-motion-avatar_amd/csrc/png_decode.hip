// PNG frames (8-bit and sub-byte, non-interlaced) and bare DEFLATE streams decoded on the device.  The host parses the
// chunks (png.parse_png) and joins each frame's IDAT payloads into one zlib stream; what happens here:
//
//   inflate   one wave per stream, one wave per workgroup (png_inflate_core.h): the 32 KiB history is a ring in LDS, the
//             code tables are built by the wave in LDS, symbols are decoded wave-uniformly from a 64-bit bit buffer that
//             refills from an LDS-staged input window, a match is an LDS-to-LDS copy by all lanes, and the ring goes out
//             in whole 16-byte stores.  A PNG frame inflates into H x (1 + rowbytes) bytes of workspace.
//   unfilter  one wave per frame walks the rows as a skewed wavefront: lane r owns row y0 + r of a 64-row band and runs
//             one pixel behind lane r - 1, so the byte above and the byte above-left arrive from the neighbouring lane
//             (a lane shuffle) exactly when Average and Paeth need them; the last row of a band waits in LDS for lane 0
//             of the next.  Sub-byte pixels are unpacked, colour converted and the output layout written in the same pass.
// No float atomics (the status words take integer atomicOr), no host synchronisation, no memset: a frame's pixels are
// written by its own wave only.
#include "png_common.h"
#include "png_inflate_core.h"

namespace amav {
namespace png {

// channels of a colour type the decoder takes at this depth, else 0
__device__ __forceinline__ int channels_of(int color_type, int depth) {
    if (depth != 8 && !((depth == 1 || depth == 2 || depth == 4) && (color_type == 0 || color_type == 3))) return 0;
    return color_type == 0 || color_type == 3 ? 1 : color_type == 2 ? 3 : color_type == 4 ? 2 : color_type == 6 ? 4 : 0;
}
__device__ __forceinline__ long long row_bytes(int W, int channels, int depth) { return ((long long)W * channels * depth + 7) / 8; }

// grid: one wave per stream.  frames == nullptr: amav_inflate's records; else PNG frames, stream f -> workspace frame f.
__global__ __launch_bounds__(64) void png_inflate_kernel(const uint8_t *__restrict__ stream, long long stream_bytes,
                                                        const amav_inflate_stream *__restrict__ records,
                                                        const amav_png_frame *__restrict__ frames, int H, int W,
                                                        long long frame_stride, uint8_t *__restrict__ out, long long out_bytes,
                                                        long long *__restrict__ produced, int *__restrict__ status) {
    __shared__ inflate::Lds lds;
    const int n = blockIdx.x;
    long long in_begin, in_end, out_begin, cap;
    int wrapper = 1;
    if (frames) {
        const amav_png_frame r = frames[n];
        const int ch = channels_of(r.color_type, r.bit_depth);
        if (r.absent) {
            if (threadIdx.x == 0) status[n] = 0;
            return;
        }
        if (!ch) {  // a record no parser makes: flagged, nothing decoded
            if (threadIdx.x == 0) status[n] = AMAV_PNG_STATUS_INFLATE | AMAV_PNG_STATUS_SIZE;
            return;
        }
        in_begin = r.zlib_begin, in_end = r.zlib_end;
        out_begin = (long long)n * frame_stride, cap = H * (1 + row_bytes(W, ch, r.bit_depth));
    } else {
        const amav_inflate_stream r = records[n];
        in_begin = r.in_begin, in_end = r.in_end, out_begin = r.out_begin, cap = r.out_capacity, wrapper = r.wrapper != 0;
    }
    // whatever the record says, reads stay inside the stream buffer and writes inside the output buffer
    in_begin = clampll(in_begin, 0, stream_bytes), in_end = clampll(in_end, in_begin, stream_bytes);
    out_begin = clampll(out_begin, 0, out_bytes), cap = clampll(cap, 0, out_bytes - out_begin);
    long long made = 0;
    int st = inflate::inflate_stream(stream, in_begin, in_end, wrapper, out + out_begin, cap, &lds, &made);
    if (frames && made != cap) st |= AMAV_PNG_STATUS_SIZE;  // a frame needs exactly H x (1 + rowbytes)
    if (threadIdx.x == 0) {
        status[n] = st;
        if (produced) produced[n] = made;
    }
}

// ------------------------------------------------------------------------------------------------------- unfilter
template <bool kChwF32>
__device__ __forceinline__ void store_pixel(void *out, int mode_l, size_t f, int y, int x, int H, int W, unsigned R, unsigned G,
                                            unsigned B, bool grey) {
    const size_t hw = (size_t)H * W, at = (size_t)y * W + x;
    if (mode_l) {
        const unsigned L = grey ? R : (19595u * R + 38470u * G + 7471u * B + 0x8000u) >> 16;
        if (kChwF32)
            static_cast<float *>(out)[f * hw + at] = (float)L / 255.0f;
        else
            static_cast<uint8_t *>(out)[f * hw + at] = (uint8_t)L;
    } else if (kChwF32) {
        float *o = static_cast<float *>(out) + f * 3 * hw + at;
        o[0] = (float)R / 255.0f, o[hw] = (float)G / 255.0f, o[2 * hw] = (float)B / 255.0f;
    } else {
        uint8_t *o = static_cast<uint8_t *>(out) + (f * hw + at) * 3;
        o[0] = (uint8_t)R, o[1] = (uint8_t)G, o[2] = (uint8_t)B;
    }
}

constexpr int kAhead = 16;  // filtered units a lane loads before it works through them

// grid: one wave per frame; dynamic LDS: 4 bytes per unit of the widest row (<= 4 W), the band's last row.
// A unit is one pixel's bytes (bpp = 1..4) or, below 8 bits, one byte of packed pixels; it travels as one 32-bit word.
template <bool kChwF32>
__global__ __launch_bounds__(64) void png_unfilter_kernel(int H, int W, const uint8_t *__restrict__ ws, long long frame_stride,
                                                         const amav_png_frame *__restrict__ frames,
                                                         const uint8_t *__restrict__ stream, long long stream_bytes, int mode_l,
                                                         void *__restrict__ out, int *__restrict__ status) {
    extern __shared__ __align__(16) unsigned carry[];
    const int f = blockIdx.x, lane = threadIdx.x;
    const amav_png_frame r = frames[f];
    if (r.absent) {  // the reference's answer to a missing mask file: all ones
        const size_t count = (size_t)H * W * (mode_l ? 1 : 3);
        for (size_t i = lane; i < count; i += 64) {
            if (kChwF32)
                static_cast<float *>(out)[f * count + i] = 1.0f;
            else
                static_cast<uint8_t *>(out)[f * count + i] = 255;
        }
        return;
    }
    const int ct = r.color_type, depth = r.bit_depth, ch = channels_of(ct, depth);
    if (status[f] != 0) {  // the inflate kernel flagged it: the workspace does not hold a frame; its pixels are 0
        const size_t count = (size_t)H * W * (mode_l ? 1 : 3);
        for (size_t i = lane; i < count; i += 64) {
            if (kChwF32)
                static_cast<float *>(out)[f * count + i] = 0.0f;
            else
                static_cast<uint8_t *>(out)[f * count + i] = 0;
        }
        return;
    }
    const int rowbytes = (int)row_bytes(W, ch, depth);
    const int bpp = ch * depth >= 8 ? ch * depth / 8 : 1;
    const int units = rowbytes / bpp;       // <= W
    const int ppu = depth < 8 ? 8 / depth : 1;  // pixels per unit
    const unsigned maxval = (1u << depth) - 1u, scale = 255u / maxval;
    const bool grey = ct == 0 || ct == 4;
    // the palette lies in the stream buffer: clamp what the record says to it
    int entries = r.palette_entries < 0 ? 0 : (r.palette_entries > 256 ? 256 : r.palette_entries);
    const long long pal_at = r.palette_at;
    if (ct != 3 || pal_at < 0 || pal_at + 3LL * entries > stream_bytes) entries = 0;
    const uint8_t *pal = stream + (entries ? pal_at : 0);
    const uint8_t *frame = ws + (size_t)f * frame_stride;

    for (int y0 = 0; y0 < H; y0 += 64) {
        const int y = y0 + lane;
        const bool active = y < H;
        const uint8_t *row = frame + (size_t)(active ? y : 0) * (1 + rowbytes);
        unsigned ft = active ? row[0] : 0u;
        if (ft > 4u) {
            atomicOr(status + f, AMAV_PNG_STATUS_FILTER);
            ft = 0u;
        }
        unsigned left = 0, upleft = 0, mine = 0;  // the unit to the left, above-left, and this lane's newest
        const int steps = units + 63;
        for (int tc = 0; tc < steps; tc += kAhead) {
            unsigned raw[kAhead];
#pragma unroll
            for (int u = 0; u < kAhead; ++u) {
                const int x = tc + u - lane;
                raw[u] = 0;
                if (active && x >= 0 && x < units)
                    for (int c = 0; c < bpp; ++c) raw[u] |= (unsigned)row[1 + (size_t)x * bpp + c] << (8 * c);
            }
#pragma unroll
            for (int u = 0; u < kAhead; ++u) {
                const int x = tc + u - lane;  // lane r runs one unit behind lane r - 1
                const bool valid = active && x >= 0 && x < units;
                unsigned above = __shfl_up(mine, 1);  // lane r - 1 made unit x of row y - 1 in the step before
                if (lane == 0) above = (y0 > 0 && valid) ? carry[x] : 0u;
                if (!valid) continue;
                unsigned cur = 0;
                for (int c = 0; c < bpp; ++c) {
                    const unsigned v = (raw[u] >> (8 * c)) & 255u, a = (left >> (8 * c)) & 255u, b = (above >> (8 * c)) & 255u,
                                   cc = (upleft >> (8 * c)) & 255u;
                    const unsigned p = ft == 1 ? a : ft == 2 ? b : ft == 3 ? (a + b) >> 1 : ft == 4 ? (unsigned)paeth((int)a, (int)b, (int)cc) : 0u;
                    cur |= ((v + p) & 255u) << (8 * c);
                }
                left = cur, upleft = above, mine = cur;
                if (lane == 63) carry[x] = cur;  // stays for lane 0 of the next band
                if (depth == 8) {
                    unsigned R = cur & 255u, G = R, B = R;
                    if (ct == 2 || ct == 6) G = (cur >> 8) & 255u, B = (cur >> 16) & 255u;
                    if (ct == 3) {
                        const bool in = (int)R < entries;
                        const unsigned i = R;
                        R = in ? pal[3 * i] : 0u, G = in ? pal[3 * i + 1] : 0u, B = in ? pal[3 * i + 2] : 0u;
                    }
                    store_pixel<kChwF32>(out, mode_l, (size_t)f, y, x, H, W, R, G, B, grey);
                } else {
                    for (int k = 0; k < ppu; ++k) {  // MSB first
                        const int px = x * ppu + k;
                        if (px >= W) break;
                        const unsigned v = (cur >> (8 - depth * (k + 1))) & maxval;
                        unsigned R = v * scale, G = R, B = R;
                        if (ct == 3) {
                            const bool in = (int)v < entries;
                            R = in ? pal[3 * v] : 0u, G = in ? pal[3 * v + 1] : 0u, B = in ? pal[3 * v + 2] : 0u;
                        }
                        store_pixel<kChwF32>(out, mode_l, (size_t)f, y, px, H, W, R, G, B, grey);
                    }
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // the carried row is in LDS before the next band reads it
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

// ----------------------------------------------------------------------------------------------------------- host
// one frame's inflated bytes at 4 bytes per pixel, a multiple of 16 so that every frame starts 16-byte aligned
static long long frame_stride_of(int H, int W) { return (long long)align_up((size_t)H * (1 + 4 * (size_t)W), 16); }

}  // namespace png
}  // namespace amav

using namespace amav;
using namespace amav::png;

static_assert(inflate::kStatusInflate == AMAV_PNG_STATUS_INFLATE && inflate::kStatusSize == AMAV_PNG_STATUS_SIZE, "status bits");

extern "C" size_t amav_inflate_workspace_bytes(int num_streams) {
    return num_streams >= 1 && num_streams <= kMaxFrames ? 256 : 0;  // the kernel keeps its state in LDS; one granule, unused
}

extern "C" int amav_inflate(int N, const uint8_t *bytes, int64_t stream_bytes, const void *records, uint8_t *out, int64_t out_bytes,
                            int64_t *produced, int32_t *status, void *workspace, size_t workspace_bytes, void *stream_) {
    const char *who = "amav_inflate";
    AMAV_REQUIRE(N >= 1 && N <= kMaxFrames, "%s: num_streams %d outside 1..65535", who, N);
    AMAV_REQUIRE(bytes && records && out && produced && status, "%s: NULL stream, records, out, produced or status", who);
    AMAV_REQUIRE(stream_bytes >= 0 && out_bytes >= 0, "%s: negative stream_bytes or out_bytes", who);
    AMAV_REQUIRE((reinterpret_cast<uintptr_t>(records) & 7) == 0 && (reinterpret_cast<uintptr_t>(produced) & 7) == 0 &&
                     (reinterpret_cast<uintptr_t>(status) & 3) == 0,
                 "%s: misaligned records, produced or status", who);
    if (int rc = check_workspace(who, amav_inflate_workspace_bytes(N), workspace, workspace_bytes)) return rc;
    png_inflate_kernel<<<N, 64, 0, static_cast<hipStream_t>(stream_)>>>(bytes, stream_bytes, static_cast<const amav_inflate_stream *>(records),
                                                                       nullptr, 0, 0, 0, out, out_bytes,
                                                                       reinterpret_cast<long long *>(produced), status);
    return check_launch(who);
}

extern "C" size_t amav_png_decode_workspace_bytes(int F, int H, int W) {
    if (!sizes_ok(F, H, W)) return 0;
    return align_up((size_t)F * (size_t)frame_stride_of(H, W), 256);
}

extern "C" int amav_png_decode(int F, int H, int W, const uint8_t *bytes, int64_t stream_bytes, const void *records, int mode,
                               int layout, void *out, size_t out_bytes, int32_t *status, void *workspace, size_t workspace_bytes,
                               void *stream_) {
    const char *who = "amav_png_decode";
    AMAV_REQUIRE(F >= 1 && F <= kMaxFrames, "%s: num_frames %d outside 1..65535", who, F);
    AMAV_REQUIRE(H >= 1 && H <= kMaxSide && W >= 1 && W <= kMaxSide, "%s: height or width outside 1..16384 (H=%d W=%d)", who, H, W);
    AMAV_REQUIRE(mode == AMAV_PNG_RGB || mode == AMAV_PNG_L, "%s: unknown mode %d", who, mode);
    AMAV_REQUIRE(layout == AMAV_JPEG_HWC_U8 || layout == AMAV_JPEG_CHW_F32, "%s: unknown layout %d", who, layout);
    if (int rc = check_stream_args(who, bytes, stream_bytes, records, status)) return rc;
    AMAV_REQUIRE(out, "%s: NULL out", who);
    AMAV_REQUIRE(layout == AMAV_JPEG_HWC_U8 || (reinterpret_cast<uintptr_t>(out) & 3) == 0, "%s: misaligned out", who);
    const size_t need = (size_t)F * H * W * (mode == AMAV_PNG_L ? 1 : 3) * (layout == AMAV_JPEG_CHW_F32 ? sizeof(float) : 1);
    if (out_bytes < need) return fail(AMAV_ERR_WORKSPACE, "%s: output buffer %zu < %zu", who, out_bytes, need);
    const size_t ws_bytes = amav_png_decode_workspace_bytes(F, H, W);
    if (int rc = check_workspace(who, ws_bytes, workspace, workspace_bytes)) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const amav_png_frame *frames = static_cast<const amav_png_frame *>(records);
    uint8_t *ws = static_cast<uint8_t *>(workspace);
    const long long stride = frame_stride_of(H, W);
    png_inflate_kernel<<<F, 64, 0, stream>>>(bytes, stream_bytes, nullptr, frames, H, W, stride, ws, (long long)F * stride, nullptr,
                                             status);
    const size_t lds = (size_t)4 * W;  // <= 64 KiB
    if (layout == AMAV_JPEG_CHW_F32)
        png_unfilter_kernel<true><<<F, 64, lds, stream>>>(H, W, ws, stride, frames, bytes, stream_bytes, mode == AMAV_PNG_L, out, status);
    else
        png_unfilter_kernel<false><<<F, 64, lds, stream>>>(H, W, ws, stride, frames, bytes, stream_bytes, mode == AMAV_PNG_L, out, status);
    return check_launch(who);
}
