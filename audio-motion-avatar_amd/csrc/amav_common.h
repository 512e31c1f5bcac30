// Shared host-side helpers of libamav_hip.so (error reporting, launch checks, workspace carving).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "../../include/amav.h"

namespace amav {

constexpr int kWave = 64;  // gfx950 wavefront width

char *error_buffer();  // thread-local, 512 bytes (api.hip)

inline int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(error_buffer(), 512, fmt, ap);
    va_end(ap);
    return code;
}

#define AMAV_REQUIRE(cond, ...)                                         \
    do {                                                                \
        if (!(cond)) return ::amav::fail(AMAV_ERR_INVALID_ARG, __VA_ARGS__); \
    } while (0)

// Check the launch that was just enqueued (no device sync: only launch-time errors).
inline int check_launch(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(AMAV_ERR_LAUNCH, "%s: %s", what, hipGetErrorString(e));
    return AMAV_OK;
}

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

__device__ __forceinline__ long long clampll(long long v, long long lo, long long hi) { return v < lo ? lo : (v > hi ? hi : v); }

inline unsigned blocks_for(long long threads) { return (unsigned)((threads + 255) / 256); }  // of 256 threads

template <typename... P>
inline bool aligned16(const P *...p) {
    return ((... | reinterpret_cast<uintptr_t>(p)) & 15) == 0;
}

// The caller's workspace holds `need` bytes and is 16-byte aligned (the codecs' common check and message).
inline int check_workspace(const char *who, size_t need, const void *workspace, size_t workspace_bytes) {
    if (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 15))
        return fail(AMAV_ERR_WORKSPACE, "%s: workspace %zu < %zu (or NULL / not 16-byte aligned)", who,
                    workspace ? workspace_bytes : (size_t)0, need);
    return AMAV_OK;
}

// What the decoders take next to their frames: a byte stream, 8-byte aligned records and 4-byte aligned status words.
inline int check_stream_args(const char *who, const void *stream, int64_t stream_bytes, const void *records, const void *status) {
    AMAV_REQUIRE(stream && records && status, "%s: NULL stream, records or status", who);
    AMAV_REQUIRE(stream_bytes >= 0, "%s: negative stream_bytes", who);
    AMAV_REQUIRE((reinterpret_cast<uintptr_t>(records) & 7) == 0 && (reinterpret_cast<uintptr_t>(status) & 3) == 0,
                 "%s: misaligned records or status", who);
    return AMAV_OK;
}

// The 8-bit level of a colour sample: clamp to [0, 1], x 255, truncate (the reference's `(frame * 255).astype(np.uint8)`).
// Raw rgb24 frames, the tile wire format (packed here or emitted by the rasterizer), the JPEG encoder's input and PNG
// rounding="truncate" all call this one function, which is why they agree bit for bit.
__host__ __device__ __forceinline__ unsigned char quant8(float v) { return (unsigned char)(fminf(fmaxf(v, 0.f), 1.f) * 255.0f); }

typedef float f32x16 __attribute__((ext_vector_type(16)));  // a 32x32 MFMA accumulator

// Tile-sparse wire format of the frame exchange (frames.hip has the description): shared with the rasterizer, which can
// emit it directly (amav_raster_args.wire)
constexpr int kWireHeaderInts = 16;
constexpr int kWireMagic = 0x414d4156;  // "AMAV"
constexpr int kWireTileBytes = 16 * 16 * 3;
inline size_t wire_payload_at(int F, int tiles) { return ((size_t)(kWireHeaderInts + F + tiles) * 4 + 15) / 16 * 16; }

// amav_set_option overrides (api.hip): -1 = follow the environment variable
int option_attn();  // 0: fp32 MFMA, 1: bf16 x 3, 2: fp16 x 2
int option_lbs();   // 0: fp32 MFMA, 1: split

// Zero `bytes` on `stream` with an ordinary kernel launch (api.hip).  Used instead of hipMemsetAsync so that a captured
// step holds kernel nodes only (HIP-graph note).
hipError_t zero_async(void *ptr, size_t bytes, hipStream_t stream);

// Bump allocator over the caller's workspace; with base == nullptr it only measures.
struct Carver {
    char *base;
    size_t off = 0;
    explicit Carver(void *b) : base(static_cast<char *>(b)) {}
    template <typename T>
    T *take(size_t count) {
        off = align_up(off, 256);
        T *p = base ? reinterpret_cast<T *>(base + off) : nullptr;
        off += count * sizeof(T);
        return p;
    }
    size_t total() const { return align_up(off, 256); }
};

}  // namespace amav
