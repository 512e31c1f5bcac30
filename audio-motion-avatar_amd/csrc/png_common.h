// What the PNG decoder (png_decode.hip) and encoder (png_encode.hip) share: the size limits, the Paeth predictor and
// the layout of the 40-byte records the host packs.
#pragma once
#include "amav_common.h"

namespace amav {
namespace png {

constexpr int kMaxFrames = 65535;  // frames of one call, and streams of amav_inflate / amav_deflate
constexpr int kMaxSide = 16384;    // height and width

inline bool sizes_ok(int F, int H, int W) { return F >= 1 && F <= kMaxFrames && H >= 1 && H <= kMaxSide && W >= 1 && W <= kMaxSide; }

// the PNG specification's predictor of filter type 4: a left, b above, c above-left
__device__ __forceinline__ int paeth(int a, int b, int c) {
    const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

static_assert(sizeof(amav_inflate_stream) == 40, "amav_inflate_stream is packed by the host as 40 bytes");
static_assert(sizeof(amav_deflate_stream) == 40, "amav_deflate_stream is packed by the host as 40 bytes");
static_assert(sizeof(amav_png_frame) == 40, "amav_png_frame is packed by the host as 40 bytes");

}  // namespace png
}  // namespace amav
