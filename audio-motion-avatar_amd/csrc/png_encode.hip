// PNG frames and bare DEFLATE streams encoded on the device: the counterpart of png_decode.hip.
//
//   filter    one wave per scanline: fp32 -> level conversion on the fly, the five PNG filters evaluated per row (or the
//             one the caller fixed), the filtered scanline (filter byte + row) into the workspace.  The previous row is
//             read from the image, so nothing depends on another wave.
//   deflate   png_deflate_core.h, one wave per piece of AMAV_DEFLATE_PIECE input bytes, run twice as the JPEG encoder
//             runs its entropy stage: once to size every piece, then, after one thread per stream (frame) has laid the
//             pieces back to back and joined their Adler-32 sums, once more to write them.  In a PNG every piece is one
//             IDAT chunk whose CRC-32 the wave computes over its staged bytes.
//   container signature, IHDR and IEND, one wave per frame.
// No allocation, no memset, no float atomics (LDS integer max / add / or only, order-independent), no host
// synchronisation; nothing is written at or past the capacity; the same bytes on every run.
#include "png_common.h"

// Diagnostic build (-DAMAV_PNG_STAMPS, tools/bench_png_encode.py): lane 0 of every deflate wave adds the wall-clock ticks
// (100 MHz) of each phase of encode_piece, over both runs of the pieces, to amav_png_stamp_totals: [0] loading the piece,
// matches and the parse, [1] histograms, [2] code construction and the choice, [3] emission, CRC-32 and the copy out.
#ifdef AMAV_PNG_STAMPS
__device__ unsigned long long amav_png_stamp_totals[4];
#define AMAV_STAMP_BEGIN long long stamp_prev_ = (long long)wall_clock64();
#define AMAV_STAMP(k)                                                                                            \
    {                                                                                                            \
        const long long now_ = (long long)wall_clock64();                                                        \
        if (threadIdx.x == 0) atomicAdd(&amav_png_stamp_totals[k], (unsigned long long)(now_ - stamp_prev_));    \
        stamp_prev_ = now_;                                                                                      \
    }
#endif
#include "png_deflate_core.h"
#include "wave_ops.h"

namespace amav {
namespace png_enc {

using png::kMaxFrames;
using png::kMaxSide;
using png::paeth;
using png::sizes_ok;

// what the three deflate kernels share
struct Job {
    const uint8_t *in;  // deflate: the caller's bytes; PNG: the filtered scanlines
    long long in_bytes;
    const amav_deflate_stream *records;  // nullptr: PNG frames
    int streams;            // N or F
    long long table;        // pieces the tables hold
    // PNG
    long long frame_stride, frame_bytes, pieces_per_frame;
    long long *frame_offsets;  // [F + 1], absolute
    long long capacity;
    // tables (workspace)
    long long *piece_start;  // deflate: [N + 1]
    int32_t *piece_bytes;
    uint32_t *s1, *s2, *adler;
    long long *offset;  // deflate: absolute byte of out; PNG: from the frame's start
    long long *frame_size;
    uint8_t *out;
    long long out_bytes;
    long long *produced;
    int32_t *status;
};

struct Range {
    long long in_begin, in_len, out_begin, cap;
    int wrapper;
};
// whatever the record says, reads stay inside the input buffer and writes inside the output buffer
__device__ __forceinline__ Range range_of(const Job &j, int n) {
    const amav_deflate_stream r = j.records[n];
    Range g;
    g.in_begin = clampll(r.in_begin, 0, j.in_bytes);
    g.in_len = clampll(r.in_end, g.in_begin, j.in_bytes) - g.in_begin;
    g.out_begin = clampll(r.out_begin, 0, j.out_bytes);
    g.cap = clampll(r.out_capacity, 0, j.out_bytes - g.out_begin);
    g.wrapper = r.wrapper != 0;
    return g;
}

// deflate: piece_start[n] = pieces before stream n.  A stream whose pieces would pass the table gets none (and is
// flagged by the layout).  One thread: the counts are a running sum.
__global__ void deflate_count_kernel(Job j) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    long long at = 0;
    for (int n = 0; n < j.streams; ++n) {
        j.piece_start[n] = at;
        const long long pieces = deflate::pieces_of(range_of(j, n).in_len);
        if (at + pieces <= j.table) at += pieces;
    }
    j.piece_start[j.streams] = at;
}

// grid-stride over the pieces, one wave each.  kWrite = false: sizes and Adler sums; true: the bytes.
template <bool kWrite>
__global__ __launch_bounds__(64) void deflate_pieces_kernel(Job j) {
    __shared__ deflate::Lds lds;
    const long long total = j.records ? j.piece_start[j.streams] : (long long)j.streams * j.pieces_per_frame;
    for (long long pid = blockIdx.x; pid < total; pid += gridDim.x) {
        const uint8_t *in;
        long long bytes, k, pieces, out_at = 0, out_end = 0;
        int n;
        bool wrapper = true;
        if (j.records) {
            int lo = 0, hi = j.streams;  // the last stream whose first piece is at or before pid and that has pieces
            while (hi - lo > 1) {
                const int mid = (lo + hi) / 2;
                if (j.piece_start[mid] <= pid) lo = mid; else hi = mid;
            }
            n = lo;
            const Range g = range_of(j, n);
            in = j.in + g.in_begin, bytes = g.in_len, k = pid - j.piece_start[n], wrapper = g.wrapper != 0;
            if (kWrite) out_at = j.offset[pid], out_end = g.out_begin + g.cap;
        } else {
            n = (int)(pid / j.pieces_per_frame), k = pid % j.pieces_per_frame;
            in = j.in + (long long)n * j.frame_stride, bytes = j.frame_bytes;
            if (kWrite) out_at = j.frame_offsets[n] + j.offset[pid], out_end = j.capacity;
        }
        pieces = deflate::pieces_of(bytes);
        const int len = deflate::piece_len(bytes, k), flags = deflate::piece_flags(pieces, k, wrapper, j.records == nullptr);
        uint32_t s1 = 0, s2 = 0;
        if (kWrite) {
            const long long room = out_end - out_at > 0 ? out_end - out_at : 0;  // bounds: encode_piece stores below `room` only
            deflate::encode_piece(in + k * deflate::kPiece, len, flags, deflate::kModeAny, j.adler[n], &lds, j.out + (room > 0 ? out_at : 0),
                                  room, &s1, &s2);
        } else {
            const int made = deflate::encode_piece(in + k * deflate::kPiece, len, flags, deflate::kModeAny, 0u, &lds, nullptr, 0, &s1, &s2);
            if (threadIdx.x == 0) j.piece_bytes[pid] = made, j.s1[pid] = s1, j.s2[pid] = s2;
        }
    }
}

// one thread per stream (frame): the pieces back to back, the Adler-32, and for a bare stream its size and status
__global__ void deflate_layout_kernel(Job j) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= j.streams) return;
    if (j.records) {
        const Range g = range_of(j, n);
        const long long first = j.piece_start[n], pieces = j.piece_start[n + 1] - first;
        if (pieces == 0) {  // the piece table is full (input ranges that overlap beyond what the workspace was sized for)
            j.produced[n] = 0, j.status[n] = AMAV_PNG_STATUS_TABLE, j.adler[n] = 0;
            return;
        }
        const long long end = deflate::layout_stream(g.in_len, pieces, j.piece_bytes + first, j.s1 + first, j.s2 + first, g.out_begin,
                                                     j.offset + first, j.adler + n);
        j.produced[n] = end - g.out_begin;
        j.status[n] = end - g.out_begin > g.cap ? AMAV_PNG_STATUS_SIZE : 0;
    } else {
        const long long first = (long long)n * j.pieces_per_frame;
        const long long end = deflate::layout_stream(j.frame_bytes, j.pieces_per_frame, j.piece_bytes + first, j.s1 + first, j.s2 + first,
                                                     33, j.offset + first, j.adler + n);
        j.frame_size[n] = end + 12;
    }
}

// PNG: the frames back to back.  One thread: a running sum over at most 65535 frames.
__global__ void png_offsets_kernel(Job j) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    long long at = 0;
    for (int f = 0; f < j.streams; ++f) {
        j.frame_offsets[f] = at;
        at += j.frame_size[f];
        j.status[f] = at > j.capacity ? AMAV_PNG_STATUS_SIZE : 0;
    }
    j.frame_offsets[j.streams] = at;
}

struct ContainerLds {  // the 45 bytes around a frame's IDAT chunks, and what crc_wave needs
    uint32_t stage[12];
    uint32_t lane_a[64];
    uint32_t sc[16];
};

// PNG: signature + IHDR in front of a frame's IDAT chunks, IEND behind them.  One wave per frame.
__global__ __launch_bounds__(64) void png_container_kernel(Job j, int H, int W, int color_type) {
    __shared__ ContainerLds lds;
    const int f = blockIdx.x, lane = threadIdx.x;
    uint8_t *stage = reinterpret_cast<uint8_t *>(lds.stage);
    if (lane == 0) {
        const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
        for (int i = 0; i < 8; ++i) stage[i] = sig[i];
        deflate::put_be32(stage + 8, 13);
        stage[12] = 'I', stage[13] = 'H', stage[14] = 'D', stage[15] = 'R';
        deflate::put_be32(stage + 16, (uint32_t)W), deflate::put_be32(stage + 20, (uint32_t)H);
        stage[24] = 8, stage[25] = (uint8_t)color_type, stage[26] = 0, stage[27] = 0, stage[28] = 0;
        deflate::put_be32(stage + 33, 0);
        stage[37] = 'I', stage[38] = 'E', stage[39] = 'N', stage[40] = 'D';
    }
    deflate::crc_wave(&lds, stage + 12, 17);
    if (lane == 0) deflate::put_be32(stage + 29, lds.sc[deflate::kScCrc]);
    deflate::crc_wave(&lds, stage + 37, 4);
    if (lane == 0) deflate::put_be32(stage + 41, lds.sc[deflate::kScCrc]);
    AMAV_WAVE_SYNC();
    const long long head = j.frame_offsets[f], tail = j.frame_offsets[f + 1] - 12;
    if (lane < 33 && head + lane < j.capacity) j.out[head + lane] = stage[lane];                // bounds: below the capacity
    if (lane < 12 && tail + lane < j.capacity) j.out[tail + lane] = stage[33 + lane];           // bounds: below the capacity
}

// ----------------------------------------------------------------------------------------------------------- filter
__device__ __forceinline__ unsigned to_level(float v, int rounding) {
    if (rounding == AMAV_PNG_ROUND_NEAREST)  // x 255, + 0.5, clamp, truncate: two roundings, never one fused operation
        return (unsigned)(int)fminf(fmaxf(__fadd_rn(__fmul_rn(v, 255.0f), 0.5f), 0.0f), 255.0f);  // fmaxf(NaN, 0) = 0
    return quant8(v);
}

// byte i (= pixel x channel) of row y of frame f, as the PNG stores it
template <int kLayout>
__device__ __forceinline__ unsigned sample(const void *frames, int rounding, size_t f, int y, int i, int H, int W) {
    const size_t hw = (size_t)H * W;
    if (kLayout == AMAV_PNG_IN_RGBA_F32) {
        const int x = i / 3, c = i - 3 * x;
        return to_level(static_cast<const float *>(frames)[(f * hw + (size_t)y * W + x) * 4 + c], rounding);
    } else if (kLayout == AMAV_PNG_IN_CHW_F32) {
        const int x = i / 3, c = i - 3 * x;
        return to_level(static_cast<const float *>(frames)[(f * 3 + c) * hw + (size_t)y * W + x], rounding);
    } else if (kLayout == AMAV_PNG_IN_RGB_U8) {
        return static_cast<const uint8_t *>(frames)[(f * hw + (size_t)y * W) * 3 + i];
    } else if (kLayout == AMAV_PNG_IN_GREY_U8) {
        return static_cast<const uint8_t *>(frames)[f * hw + (size_t)y * W + i];
    } else {
        return to_level(static_cast<const float *>(frames)[f * hw + (size_t)y * W + i], rounding);
    }
}

// grid-stride over the F x H scanlines, one wave each (the launch takes at most 2^20 workgroups, so any accepted F and H
// stay within the launch limits).  The filtered scanline of row y of frame f goes to ws + f frame_stride + y (1 + rowbytes).
template <int kLayout>
__global__ __launch_bounds__(64) void png_filter_kernel(const void *__restrict__ frames, int H, int W, int filter, int rounding,
                                                       uint8_t *__restrict__ ws, long long frame_stride, long long rows) {
    constexpr int C = (kLayout == AMAV_PNG_IN_GREY_U8 || kLayout == AMAV_PNG_IN_GREY_F32) ? 1 : 3;
    const int lane = threadIdx.x, rb = W * C;
    for (long long at = blockIdx.x; at < rows; at += gridDim.x) {
        const size_t f = (size_t)(at / H);
        const int y = (int)(at % H);
        uint8_t *row = ws + f * frame_stride + (size_t)y * (1 + rb);
        auto residuals = [&](int i, int (&r)[5]) {
            const int cur = (int)sample<kLayout>(frames, rounding, f, y, i, H, W);
            const int a = i >= C ? (int)sample<kLayout>(frames, rounding, f, y, i - C, H, W) : 0;
            const int b = y > 0 ? (int)sample<kLayout>(frames, rounding, f, y - 1, i, H, W) : 0;
            const int c = (y > 0 && i >= C) ? (int)sample<kLayout>(frames, rounding, f, y - 1, i - C, H, W) : 0;
            r[0] = cur, r[1] = (cur - a) & 255, r[2] = (cur - b) & 255, r[3] = (cur - ((a + b) >> 1)) & 255, r[4] = (cur - paeth(a, b, c)) & 255;
        };
        int ft = filter;
        if (filter == AMAV_PNG_FILTER_ADAPTIVE) {  // the smallest sum of |signed residual|, the lowest filter number on ties
            int sum[5] = {0, 0, 0, 0, 0};
            for (int i = lane; i < rb; i += 64) {
                int r[5];
                residuals(i, r);
#pragma unroll
                for (int k = 0; k < 5; ++k) sum[k] += r[k] < 128 ? r[k] : 256 - r[k];
            }
            ft = 0;
            int best = wave_sum(sum[0]);
#pragma unroll
            for (int k = 1; k < 5; ++k) {
                const int s = wave_sum(sum[k]);
                if (s < best) best = s, ft = k;
            }
        }
        if (lane == 0) row[0] = (uint8_t)ft;
        for (int i = lane; i < rb; i += 64) {
            int r[5];
            residuals(i, r);
            row[1 + i] = (uint8_t)(ft == 0 ? r[0] : ft == 1 ? r[1] : ft == 2 ? r[2] : ft == 3 ? r[3] : r[4]);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------- host
static int channels_of(int layout) { return layout == AMAV_PNG_IN_GREY_U8 || layout == AMAV_PNG_IN_GREY_F32 ? 1 : 3; }
static bool layout_ok(int layout) { return layout >= AMAV_PNG_IN_RGBA_F32 && layout <= AMAV_PNG_IN_GREY_F32; }
static long long frame_bytes_of(int H, int W, int C) { return (long long)H * (1 + (long long)W * C); }

static void carve_tables(Carver &c, Job &j, long long streams, long long table, bool bare) {
    j.table = table;
    j.piece_start = bare ? c.take<long long>(streams + 1) : nullptr;
    j.frame_size = bare ? nullptr : c.take<long long>(streams);
    j.adler = c.take<uint32_t>(streams);
    j.piece_bytes = c.take<int32_t>(table);
    j.s1 = c.take<uint32_t>(table);
    j.s2 = c.take<uint32_t>(table);
    j.offset = c.take<long long>(table);
}

static unsigned piece_grid(long long pieces) { return (unsigned)(pieces < 65536 ? (pieces > 0 ? pieces : 1) : 65536); }

}  // namespace png_enc
}  // namespace amav

using namespace amav;
using namespace amav::png_enc;

static_assert(deflate::kPiece == AMAV_DEFLATE_PIECE && AMAV_DEFLATE_PIECE <= 32768, "the piece size named in amav.h");
static_assert(sizeof(deflate::Lds) <= 160 * 1024 / 3 - 512, "three pieces' state fits a compute unit's LDS");

extern "C" size_t amav_deflate_workspace_bytes(int N, int64_t in_bytes) {
    if (N < 1 || N > kMaxFrames || in_bytes < 0) return 0;
    Carver c(nullptr);
    Job j{};
    carve_tables(c, j, N, in_bytes / AMAV_DEFLATE_PIECE + N, true);
    return c.total();
}

extern "C" int amav_deflate(int N, const uint8_t *bytes, int64_t in_bytes, const void *records, uint8_t *out, int64_t out_bytes,
                            int64_t *produced, int32_t *status, void *workspace, size_t workspace_bytes, void *stream_) {
    const char *who = "amav_deflate";
    AMAV_REQUIRE(N >= 1 && N <= kMaxFrames, "%s: num_streams %d outside 1..65535", who, N);
    AMAV_REQUIRE(bytes && records && out && produced && status, "%s: NULL input, records, out, produced or status", who);
    AMAV_REQUIRE(in_bytes >= 0 && out_bytes >= 0, "%s: negative in_bytes or out_bytes", who);
    AMAV_REQUIRE((reinterpret_cast<uintptr_t>(records) & 7) == 0 && (reinterpret_cast<uintptr_t>(produced) & 7) == 0 &&
                     (reinterpret_cast<uintptr_t>(status) & 3) == 0,
                 "%s: misaligned records, produced or status", who);
    if (int rc = check_workspace(who, amav_deflate_workspace_bytes(N, in_bytes), workspace, workspace_bytes)) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    Job j{};
    Carver c(workspace);
    carve_tables(c, j, N, in_bytes / AMAV_DEFLATE_PIECE + N, true);
    j.in = bytes, j.in_bytes = in_bytes, j.records = static_cast<const amav_deflate_stream *>(records), j.streams = N;
    j.out = out, j.out_bytes = out_bytes, j.produced = reinterpret_cast<long long *>(produced), j.status = status;
    const unsigned grid = piece_grid(j.table);
    deflate_count_kernel<<<1, 64, 0, stream>>>(j);
    deflate_pieces_kernel<false><<<grid, 64, 0, stream>>>(j);
    deflate_layout_kernel<<<(N + 63) / 64, 64, 0, stream>>>(j);
    deflate_pieces_kernel<true><<<grid, 64, 0, stream>>>(j);
    return check_launch(who);
}

extern "C" int64_t amav_png_stream_bound(int F, int H, int W, int layout) {
    if (!sizes_ok(F, H, W) || !layout_ok(layout)) return 0;
    const long long bytes = frame_bytes_of(H, W, channels_of(layout)), pieces = deflate::pieces_of(bytes);
    return (int64_t)F * (33 + 12 + 6 + bytes + pieces * (5 + 12));  // signature + IHDR, IEND, zlib wrapper, stored pieces as IDATs
}

extern "C" size_t amav_png_encode_workspace_bytes(int F, int H, int W, int layout) {
    if (!sizes_ok(F, H, W) || !layout_ok(layout)) return 0;
    const long long bytes = frame_bytes_of(H, W, channels_of(layout));
    Carver c(nullptr);
    Job j{};
    c.take<uint8_t>((size_t)F * align_up((size_t)bytes, 16));
    carve_tables(c, j, F, (long long)F * deflate::pieces_of(bytes), false);
    return c.total();
}

extern "C" int amav_png_encode(int F, int H, int W, const void *frames, int layout, int filter, int rounding, uint8_t *stream_out,
                               int64_t capacity, int64_t *frame_offsets, int32_t *status, void *workspace, size_t workspace_bytes,
                               void *stream_) {
    const char *who = "amav_png_encode";
    AMAV_REQUIRE(F >= 1 && F <= kMaxFrames, "%s: num_frames %d outside 1..65535", who, F);
    AMAV_REQUIRE(H >= 1 && H <= kMaxSide && W >= 1 && W <= kMaxSide, "%s: height or width outside 1..16384 (H=%d W=%d)", who, H, W);
    AMAV_REQUIRE(layout_ok(layout), "%s: unknown layout %d", who, layout);
    AMAV_REQUIRE(filter >= 0 && filter <= AMAV_PNG_FILTER_ADAPTIVE, "%s: unknown filter %d", who, filter);
    AMAV_REQUIRE(rounding == AMAV_PNG_ROUND_NEAREST || rounding == AMAV_PNG_ROUND_TRUNCATE, "%s: unknown rounding %d", who, rounding);
    AMAV_REQUIRE(frames && stream_out && frame_offsets && status, "%s: NULL frames, stream, frame_offsets or status", who);
    AMAV_REQUIRE(capacity >= 0, "%s: negative capacity", who);
    const bool f32 = layout == AMAV_PNG_IN_RGBA_F32 || layout == AMAV_PNG_IN_CHW_F32 || layout == AMAV_PNG_IN_GREY_F32;
    AMAV_REQUIRE((reinterpret_cast<uintptr_t>(frame_offsets) & 7) == 0 && (reinterpret_cast<uintptr_t>(status) & 3) == 0 &&
                     (!f32 || (reinterpret_cast<uintptr_t>(frames) & 3) == 0),
                 "%s: misaligned frames, frame_offsets or status", who);
    if (int rc = check_workspace(who, amav_png_encode_workspace_bytes(F, H, W, layout), workspace, workspace_bytes)) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int C = channels_of(layout);
    const long long bytes = frame_bytes_of(H, W, C), stride = (long long)align_up((size_t)bytes, 16);
    Job j{};
    Carver c(workspace);
    uint8_t *filtered = c.take<uint8_t>((size_t)F * stride);
    carve_tables(c, j, F, (long long)F * deflate::pieces_of(bytes), false);
    j.in = filtered, j.in_bytes = (long long)F * stride, j.streams = F;
    j.frame_stride = stride, j.frame_bytes = bytes, j.pieces_per_frame = deflate::pieces_of(bytes);
    j.frame_offsets = reinterpret_cast<long long *>(frame_offsets), j.capacity = capacity;
    j.out = stream_out, j.out_bytes = capacity, j.status = status;
    const long long all_rows = (long long)F * H;
    const unsigned rows = (unsigned)(all_rows < (1 << 20) ? all_rows : (1 << 20));
    switch (layout) {
        case AMAV_PNG_IN_RGBA_F32: png_filter_kernel<AMAV_PNG_IN_RGBA_F32><<<rows, 64, 0, stream>>>(frames, H, W, filter, rounding, filtered, stride, all_rows); break;
        case AMAV_PNG_IN_CHW_F32: png_filter_kernel<AMAV_PNG_IN_CHW_F32><<<rows, 64, 0, stream>>>(frames, H, W, filter, rounding, filtered, stride, all_rows); break;
        case AMAV_PNG_IN_RGB_U8: png_filter_kernel<AMAV_PNG_IN_RGB_U8><<<rows, 64, 0, stream>>>(frames, H, W, filter, rounding, filtered, stride, all_rows); break;
        case AMAV_PNG_IN_GREY_U8: png_filter_kernel<AMAV_PNG_IN_GREY_U8><<<rows, 64, 0, stream>>>(frames, H, W, filter, rounding, filtered, stride, all_rows); break;
        default: png_filter_kernel<AMAV_PNG_IN_GREY_F32><<<rows, 64, 0, stream>>>(frames, H, W, filter, rounding, filtered, stride, all_rows); break;
    }
    const unsigned grid = piece_grid(j.table);
    deflate_pieces_kernel<false><<<grid, 64, 0, stream>>>(j);
    deflate_layout_kernel<<<(F + 63) / 64, 64, 0, stream>>>(j);
    png_offsets_kernel<<<1, 64, 0, stream>>>(j);
    png_container_kernel<<<F, 64, 0, stream>>>(j, H, W, C == 1 ? 0 : 2);
    deflate_pieces_kernel<true><<<grid, 64, 0, stream>>>(j);
    return check_launch(who);
}

#ifdef AMAV_PNG_STAMPS
// diagnostic builds only (not declared in include/amav.h): reads and clears the phase totals
extern "C" int amav_debug_png_stamps(unsigned long long out[4]) {
    unsigned long long zero[4] = {0, 0, 0, 0};
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(amav_png_stamp_totals), sizeof(zero)) != hipSuccess) return -1;
    return hipMemcpyToSymbol(HIP_SYMBOL(amav_png_stamp_totals), zero, sizeof(zero)) == hipSuccess ? 0 : -1;
}
#endif
