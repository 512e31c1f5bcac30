// Row kernels of the transformer step, the forward counterpart of attention_rows_backward.hip:
// the split operands of the fp32-equivalent GEMMs (amav_split_operand, amav_split_operand_transposed), the GEGLU gate
// (amav_geglu) and the residual adds + LayerNorm (amav_add_layernorm).  One pass over [rows, width] fp32 rows each.
#include <cmath>

#include "amav_common.h"
#include "gelu.h"
#include "split_bf16.h"
#include "split_f16.h"
#include "wave_ops.h"

using namespace amav;

// ---------------------------------------------------------------------------------------------------------------
// Split operands of an fp32-equivalent GEMM on the bf16 matrix pipe (the three-way split of split_bf16.h, as in
// selfattn_split_kernel): x = x1 + x2 + x3 with every part a bf16, and x W^T is the sum of the six partial products x_i W_j^T
// with i + j <= 4 (the dropped ones are below 2^-24 of the result).  The six products are ONE bf16 GEMM with fp32
// accumulation over operands concatenated along K, small terms first:
//     activations  A' = [x3 | x2 | x1 | x2 | x1 | x1]      weights  B' = [w1 | w2 | w3 | w1 | w2 | w1]      (K' = 6 K)
// which the matrix pipe runs at 16x the fp32 MFMA rate, i.e. 2.7x faster than the fp32 GEMM for the same result
// (measured 1.9e-6 max abs against fp64 on the 512 -> 4096 projection, 6.0e-6 for the library's fp32 GEMM).
namespace amav {
namespace rows_fwd {
template <bool kWeights>
__global__ __launch_bounds__(256) void split_operand_kernel(long long octs, int k8, const float *__restrict__ x,
                                                            long long row_stride, __bf16 *__restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= octs) return;
    const long long row = i / k8;
    const int c = (int)(i - row * k8) * 8;
    const float *src = x + row * row_stride + c;
    const float4 lo = *reinterpret_cast<const float4 *>(src), hi = *reinterpret_cast<const float4 *>(src + 4);
    const float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    bf16x8 p1, p2, p3;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        __bf16 a, b, cc;
        split3(v[j], a, b, cc);
        p1[j] = a, p2[j] = b, p3[j] = cc;
    }
    const long long K = (long long)k8 * 8;
    __bf16 *dst = out + row * 6 * K + c;
    auto put = [&](int block, const bf16x8 &p) { *reinterpret_cast<bf16x8 *>(dst + block * K) = p; };
    if (kWeights) {
        put(0, p1), put(1, p2), put(2, p3), put(3, p1), put(4, p2), put(5, p1);
    } else {
        put(0, p3), put(1, p2), put(2, p1), put(3, p2), put(4, p1), put(5, p1);
    }
}

// fp16 x 2 format: (x * prescale) = h1 + h2; activations [h2 | h1 | h1], weights [g1 | g2 | g1] (K' = 3 K), so that
// A' B'^T = h2 g1 + h1 g2 + h1 g1 -- the product to 2^-22, at half the MFMA work of the bf16 x 3 format.
template <bool kWeights>
__global__ __launch_bounds__(256) void split_operand_f16_kernel(long long octs, int k8, const float *__restrict__ x,
                                                                long long row_stride, float prescale,
                                                                _Float16 *__restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= octs) return;
    const long long row = i / k8;
    const int c = (int)(i - row * k8) * 8;
    const float *src = x + row * row_stride + c;
    const float4 lo = *reinterpret_cast<const float4 *>(src), hi = *reinterpret_cast<const float4 *>(src + 4);
    const float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    f16x8 p1, p2;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        _Float16 a, b;
        split2(v[j] * prescale, a, b);
        p1[j] = a, p2[j] = b;
    }
    const long long K = (long long)k8 * 8;
    _Float16 *dst = out + row * 3 * K + c;
    auto put = [&](int block, const f16x8 &p) { *reinterpret_cast<f16x8 *>(dst + block * K) = p; };
    if (kWeights) {
        put(0, p1), put(1, p2), put(2, p1);
    } else {
        put(0, p2), put(1, p1), put(2, p1);
    }
}
// The bf16 x 3 operand of x^T (and, with out_rows, split_operand_kernel<false>'s operand of x from the same read): what
// the two backward products of a linear layer contract over is the ROW dimension of their fp32 tensors (dW = g^T x over the
// rows of both, dx = g W over the rows of W), and the library GEMM wants the contraction dimension innermost.
// grid (row tiles, column tiles), 256 threads, one 64 x 64 fp32 tile: thread (pair = tid / 8, oct = tid % 8) reads rows
// 2 pair, 2 pair + 1 x columns 8 oct .. 8 oct + 7 (four float4; rows past the end read as +0, whose parts are +0: the zero
// tail of out_t), splits them in registers, writes the row-major operand with 16-byte stores, and stages each part in LDS
// transposed: stage[part][column][dword d] = rows (2 d, 2 d + 1) of the tile.  A column's 32 dwords are eight 16-byte
// slots, stored at slot ^ (column / 8):
//   * writes (4 bytes; bank = dword % 32 over half a wave = 8 octs x 4 pairs of one slot): slot ^ oct takes 8 values, the
//     pair's low bits the 4 dwords of a slot -- 32 banks, each once (unswizzled, all 8 octs would share 4 banks);
//   * reads (16 bytes; bank = dword % 64 over the read's 16-lane groups): a wave reads the 8 columns of one column / 8, so
//     the XOR permutes the slots of every column alike and keeps a 4-lane block on one half of a column; the groups' four
//     blocks then sit on (even column, low half), (odd, high), (even, high), (odd, low) or the mirror image: 64 banks, each
//     once.  A pad cannot serve both sides: 16-byte reads need a column stride that is a multiple of 4 dwords, and with any
//     such stride the 8 octs of a write land on 4 banks.
// out_t is written with 16-byte stores of 8 consecutive source rows, 8 lanes per column (128 contiguous bytes).
template <bool kWeights>
__global__ __launch_bounds__(256) void split_operand_transposed_kernel(long long rows, long long rows_padded, int k,
                                                                       const float *__restrict__ x, long long row_stride,
                                                                       __bf16 *__restrict__ out_rows,
                                                                       __bf16 *__restrict__ out_t) {
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    __shared__ uint4 stage[3][64][8];
    const int tid = threadIdx.x;
    const long long row0 = (long long)blockIdx.x * 64;
    const int col0 = blockIdx.y * 64;
    {
        const int pair = tid >> 3, oct = tid & 7;
        const int col = col0 + 8 * oct;
        float v[2][8];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const long long row = row0 + 2 * pair + h;
            if (row < rows && col < k) {
                const float *src = x + row * row_stride + col;
                const float4 lo = *reinterpret_cast<const float4 *>(src), hi = *reinterpret_cast<const float4 *>(src + 4);
                v[h][0] = lo.x, v[h][1] = lo.y, v[h][2] = lo.z, v[h][3] = lo.w;
                v[h][4] = hi.x, v[h][5] = hi.y, v[h][6] = hi.z, v[h][7] = hi.w;
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) v[h][j] = 0.0f;
            }
        }
        bf16x8 p[2][3];
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                __bf16 a, b, cc;
                split3(v[h][j], a, b, cc);
                p[h][0][j] = a, p[h][1][j] = b, p[h][2][j] = cc;
            }
        if (out_rows && col < k) {  // activation order, as split_operand_kernel<false>
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const long long row = row0 + 2 * pair + h;
                if (row >= rows) continue;
                __bf16 *dst = out_rows + row * 6 * k + col;
                auto put = [&](int block, const bf16x8 &q) { *reinterpret_cast<bf16x8 *>(dst + (long long)block * k) = q; };
                put(0, p[h][2]), put(1, p[h][1]), put(2, p[h][0]), put(3, p[h][1]), put(4, p[h][0]), put(5, p[h][0]);
            }
        }
        unsigned *words = reinterpret_cast<unsigned *>(&stage[0][0][0]);
        const int dword = (((pair >> 2) ^ oct) << 2) | (pair & 3);
#pragma unroll
        for (int part = 0; part < 3; ++part)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                bf16x2 two;
                two[0] = p[0][part][j], two[1] = p[1][part][j];
                words[(part * 64 + 8 * oct + j) * 32 + dword] = __builtin_bit_cast(unsigned, two);
            }
    }
    __syncthreads();
    const int slot = tid & 7;
    const long long row = row0 + 8 * slot;  // the first of this lane's 8 source rows
    if (row >= rows_padded) return;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int c = 32 * half + (tid >> 3);
        if (col0 + c >= k) continue;
        const uint4 p1 = stage[0][c][slot ^ (c >> 3)], p2 = stage[1][c][slot ^ (c >> 3)], p3 = stage[2][c][slot ^ (c >> 3)];
        __bf16 *dst = out_t + (long long)(col0 + c) * 6 * rows_padded + row;
        auto put = [&](int block, const uint4 &q) { *reinterpret_cast<uint4 *>(dst + block * rows_padded) = q; };
        if (kWeights) {
            put(0, p1), put(1, p2), put(2, p3), put(3, p1), put(4, p2), put(5, p1);
        } else {
            put(0, p3), put(1, p2), put(2, p1), put(3, p2), put(4, p1), put(5, p1);
        }
    }
}
}  // namespace rows_fwd
}  // namespace amav

static bool split_format_ok(int format, int scale_exp) {
    return format == AMAV_SPLIT_BF16X3 || (format == AMAV_SPLIT_FP16X2 && scale_exp >= -126 && scale_exp <= 126);
}

extern "C" int amav_split_operand(int64_t rows, int k, const float *x, int64_t x_row_stride, int weights, int format,
                                  int scale_exp, void *out, void *stream_) {
    AMAV_REQUIRE(rows > 0 && k > 0 && k % 8 == 0, "amav_split_operand: rows=%lld k=%d (k must be a multiple of 8)",
                 (long long)rows, k);
    AMAV_REQUIRE(x && out, "amav_split_operand: NULL pointer");
    AMAV_REQUIRE(x_row_stride >= k && x_row_stride % 4 == 0, "amav_split_operand: bad row stride");
    AMAV_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & 15) == 0,
                 "amav_split_operand: buffers must be 16-byte aligned");
    AMAV_REQUIRE(split_format_ok(format, scale_exp), "amav_split_operand: format %d / scale exponent %d", format, scale_exp);
    const long long octs = rows * (k / 8);
    const unsigned grid = (unsigned)((octs + 255) / 256);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (format == AMAV_SPLIT_FP16X2) {
        const float prescale = ldexpf(1.0f, scale_exp);
        _Float16 *o = static_cast<_Float16 *>(out);
        if (weights)
            amav::rows_fwd::split_operand_f16_kernel<true><<<grid, 256, 0, stream>>>(octs, k / 8, x, x_row_stride, prescale, o);
        else
            amav::rows_fwd::split_operand_f16_kernel<false><<<grid, 256, 0, stream>>>(octs, k / 8, x, x_row_stride, prescale, o);
    } else if (weights) {
        amav::rows_fwd::split_operand_kernel<true><<<grid, 256, 0, stream>>>(octs, k / 8, x, x_row_stride,
                                                                       static_cast<__bf16 *>(out));
    } else {
        amav::rows_fwd::split_operand_kernel<false><<<grid, 256, 0, stream>>>(octs, k / 8, x, x_row_stride,
                                                                        static_cast<__bf16 *>(out));
    }
    return check_launch("amav_split_operand");
}

extern "C" int64_t amav_split_transposed_rows(int64_t rows) { return rows > 0 ? (rows + 7) / 8 * 8 : 0; }

extern "C" int amav_split_operand_transposed(int64_t rows, int k, const float *x, int64_t x_row_stride, int weights,
                                             void *out_rows, void *out_t, void *stream_) {
    AMAV_REQUIRE(rows > 0 && k > 0 && k % 8 == 0,
                 "amav_split_operand_transposed: rows=%lld k=%d (k must be a multiple of 8)", (long long)rows, k);
    AMAV_REQUIRE(x && out_t, "amav_split_operand_transposed: NULL pointer");
    AMAV_REQUIRE(x_row_stride >= k && x_row_stride % 4 == 0, "amav_split_operand_transposed: bad row stride");
    AMAV_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out_rows) |
                   reinterpret_cast<uintptr_t>(out_t)) & 15) == 0,
                 "amav_split_operand_transposed: buffers must be 16-byte aligned");
    const long long row_tiles = (rows + 63) / 64, col_tiles = (k + 63) / 64;
    AMAV_REQUIRE(row_tiles <= 0x7fffffffLL && col_tiles <= 65535,
                 "amav_split_operand_transposed: rows=%lld k=%d exceed the launch grid", (long long)rows, k);
    const dim3 grid((unsigned)row_tiles, (unsigned)col_tiles);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const long long rows_padded = amav_split_transposed_rows(rows);
    __bf16 *o_rows = static_cast<__bf16 *>(out_rows), *o_t = static_cast<__bf16 *>(out_t);
    if (weights)
        amav::rows_fwd::split_operand_transposed_kernel<true><<<grid, 256, 0, stream>>>(rows, rows_padded, k, x, x_row_stride,
                                                                                  o_rows, o_t);
    else
        amav::rows_fwd::split_operand_transposed_kernel<false><<<grid, 256, 0, stream>>>(rows, rows_padded, k, x, x_row_stride,
                                                                                   o_rows, o_t);
    return check_launch("amav_split_operand_transposed");
}


// ---------------------------------------------------------------------------------------------------------------
// GEGLU gate of the feed-forward (src/models/transformers.py:484-508: hidden, gate = proj(x).chunk(2); hidden *
// gelu(gate), exact-erf GELU): one pass over the projection's [rows, 2 * inner] output instead of torch's two
// elementwise kernels (gelu, then mul), i.e. 1.5 instead of 2.5 tensor sweeps.
namespace amav {
namespace rows_fwd {
__global__ __launch_bounds__(256) void geglu_kernel(long long quads, int inner4, const float4 *__restrict__ in,
                                                    long long in_row4, const float4 *__restrict__ bias,
                                                    float4 *__restrict__ out, _Float16 *__restrict__ out_split,
                                                    float prescale) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= quads) return;
    const long long row = i / inner4;
    const int col = (int)(i - row * inner4);
    float4 h = in[row * in_row4 + col], g = in[row * in_row4 + inner4 + col];
    if (bias) {  // the projection's bias, when its GEMM ran without one
        const float4 bh = bias[col], bg = bias[inner4 + col];
        h = make_float4(h.x + bh.x, h.y + bh.y, h.z + bh.z, h.w + bh.w);
        g = make_float4(g.x + bg.x, g.y + bg.y, g.z + bg.z, g.w + bg.w);
    }
    const float4 y = make_float4(h.x * gelu(g.x), h.y * gelu(g.y), h.z * gelu(g.z), h.w * gelu(g.w));
    if (out_split) {  // the fp16 x 2 activation operand of the output projection (split_operand_f16_kernel's layout)
        const float yv[4] = {y.x, y.y, y.z, y.w};
        f16x4 p1, p2;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            // split2 with + 0 on the fp32 residual: an exactly-zero residual is +0, as x - x is (one that only underflows
            // fp16 keeps its sign).  Where y = -0 (a saturated gate) the compiler re-forms `a` for the subtraction as
            // fma(y, prescale, +0) = +0 and the residual came out as -0 - 0 = -0, unlike split_operand_f16_kernel's.
            const float ys = yv[j] * prescale;
            const _Float16 a = (_Float16)ys;
            p1[j] = a, p2[j] = (_Float16)(__builtin_fmaf((float)a, -1.0f, ys) + 0.0f);
        }
        const long long K = 4LL * inner4;
        _Float16 *dst = out_split + row * 3 * K + 4 * col;
        *reinterpret_cast<f16x4 *>(dst) = p2;
        *reinterpret_cast<f16x4 *>(dst + K) = p1;
        *reinterpret_cast<f16x4 *>(dst + 2 * K) = p1;
    } else {
        out[i] = y;
    }
}
}  // namespace rows_fwd
}  // namespace amav

extern "C" int amav_geglu(int64_t rows, int inner, const float *proj, int64_t proj_row_stride, const float *bias,
                          float *out, void *out_split, int split_scale_exp, void *stream) {
    AMAV_REQUIRE(rows > 0 && inner > 0 && inner % 4 == 0, "amav_geglu: bad sizes rows=%lld inner=%d", (long long)rows, inner);
    AMAV_REQUIRE(proj && ((out != nullptr) != (out_split != nullptr)),
                 "amav_geglu: NULL projection, or not exactly one of out (fp32) and out_split (fp16 x 2 operand)");
    AMAV_REQUIRE(split_scale_exp >= -126 && split_scale_exp <= 126, "amav_geglu: scale exponent %d", split_scale_exp);
    AMAV_REQUIRE(proj_row_stride >= 2LL * inner && proj_row_stride % 4 == 0, "amav_geglu: bad row stride");
    AMAV_REQUIRE(((reinterpret_cast<uintptr_t>(proj) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(bias) |
                   reinterpret_cast<uintptr_t>(out_split)) & 15) == 0,
                 "amav_geglu: buffers must be 16-byte aligned");
    const long long quads = rows * (inner / 4);
    amav::rows_fwd::geglu_kernel<<<(unsigned)((quads + 255) / 256), 256, 0, static_cast<hipStream_t>(stream)>>>(
        quads, inner / 4, reinterpret_cast<const float4 *>(proj), proj_row_stride / 4,
        reinterpret_cast<const float4 *>(bias), reinterpret_cast<float4 *>(out), static_cast<_Float16 *>(out_split),
        ldexpf(1.0f, split_scale_exp));
    return check_launch("amav_geglu");
}


// ---------------------------------------------------------------------------------------------------------------
// Residual adds + LayerNorm of BasicTransformerBlock (src/models/transformers.py:292-399) in one pass:
//   h = ((a + a_bias) + h);  h = (row_b + h);  n = LayerNorm(h) * w + b
// i.e. `attn1(...) + h`, then `attn2(...) + h` whose value is ONE row per batch item (single audio key), then norm3.
// torch runs two adds and two LayerNorms for this (norm2's result is never used on this path: the cross-attention
// output does not depend on its queries).  One wave per row, row in registers, two-pass mean / variance.
// a_bias is the bias of the projection that produced `a` when its GEMM ran without one; with kSplit the normalised row
// is written as the activation operand of the next projection's split GEMM (split_operand_kernel's layout) instead of
// fp32 -- the row never makes the round trip through HBM in between.
namespace amav {
namespace rows_fwd {
template <int kVec, int kSplit>  // float4 per lane: dim = 256 * kVec; kSplit 0: fp32 rows, 1: bf16 x 3, 2: fp16 x 2
__global__ __launch_bounds__(256) void add_layernorm_kernel(long long rows, long long rows_per_batch,
                                                            const float4 *__restrict__ a, const float4 *__restrict__ a_bias,
                                                            const float4 *__restrict__ brow,
                                                            const float4 *__restrict__ h, float4 *__restrict__ h_out,
                                                            const float4 *__restrict__ w,
                                                            const float4 *__restrict__ b, float eps,
                                                            float4 *__restrict__ out, void *__restrict__ out_split,
                                                            float prescale) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    constexpr int kRow4 = 64 * kVec;
    const float4 *br = brow ? brow + (row / rows_per_batch) * kRow4 : nullptr;
    float4 x[kVec];
    float sum = 0.f;
#pragma unroll
    for (int v = 0; v < kVec; ++v) {
        const int c = lane + 64 * v;
        float4 t = h[row * kRow4 + c];
        if (a) {
            float4 av = a[row * kRow4 + c];
            if (a_bias) {
                const float4 ab = a_bias[c];
                av = make_float4(av.x + ab.x, av.y + ab.y, av.z + ab.z, av.w + ab.w);
            }
            t = make_float4(av.x + t.x, av.y + t.y, av.z + t.z, av.w + t.w);
        }
        if (br) {
            const float4 rv = br[c];
            t = make_float4(rv.x + t.x, rv.y + t.y, rv.z + t.z, rv.w + t.w);
        }
        x[v] = t;
        h_out[row * kRow4 + c] = t;
        sum += (t.x + t.y) + (t.z + t.w);
    }
    const float mean = wave_sum(sum) * (1.0f / (256.0f * kVec));
    float var = 0.f;
#pragma unroll
    for (int v = 0; v < kVec; ++v) {
        const float dx = x[v].x - mean, dy = x[v].y - mean, dz = x[v].z - mean, dw = x[v].w - mean;
        var += (dx * dx + dy * dy) + (dz * dz + dw * dw);
    }
    const float rstd = 1.0f / sqrtf(wave_sum(var) * (1.0f / (256.0f * kVec)) + eps);
#pragma unroll
    for (int v = 0; v < kVec; ++v) {
        const int c = lane + 64 * v;
        const float4 wv = w[c], bv = b[c];
        const float4 n = make_float4((x[v].x - mean) * rstd * wv.x + bv.x, (x[v].y - mean) * rstd * wv.y + bv.y,
                                     (x[v].z - mean) * rstd * wv.z + bv.z, (x[v].w - mean) * rstd * wv.w + bv.w);
        if (kSplit == 2) {
            constexpr int K = 256 * kVec;
            const float nv[4] = {n.x, n.y, n.z, n.w};
            f16x4 p1, p2;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                _Float16 s1, s2;
                split2(nv[j] * prescale, s1, s2);
                p1[j] = s1, p2[j] = s2;
            }
            _Float16 *dst = static_cast<_Float16 *>(out_split) + row * 3 * K + 4 * c;
            *reinterpret_cast<f16x4 *>(dst) = p2;
            *reinterpret_cast<f16x4 *>(dst + K) = p1;
            *reinterpret_cast<f16x4 *>(dst + 2 * K) = p1;
        } else if (kSplit == 1) {
            constexpr int K = 256 * kVec;
            const float nv[4] = {n.x, n.y, n.z, n.w};
            bf16x4 p1, p2, p3;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                __bf16 s1, s2, s3;
                split3(nv[j], s1, s2, s3);
                p1[j] = s1, p2[j] = s2, p3[j] = s3;
            }
            __bf16 *dst = static_cast<__bf16 *>(out_split) + row * 6 * K + 4 * c;
            auto put = [&](int block, const bf16x4 &p) { *reinterpret_cast<bf16x4 *>(dst + block * K) = p; };
            put(0, p3), put(1, p2), put(2, p1), put(3, p2), put(4, p1), put(5, p1);
        } else {
            out[row * kRow4 + c] = n;
        }
    }
}
}  // namespace rows_fwd
}  // namespace amav

extern "C" int amav_add_layernorm(int64_t rows, int dim, int64_t rows_per_batch, const float *add, const float *add_bias,
                                  const float *batch_row, const float *hidden, float *hidden_out, const float *weight,
                                  const float *bias, float eps, float *out_norm, void *out_norm_split, int split_format,
                                  int split_scale_exp, void *stream_) {
    AMAV_REQUIRE(rows > 0 && rows_per_batch > 0 && (dim == 256 || dim == 512 || dim == 768 || dim == 1024),
                 "amav_add_layernorm: rows=%lld dim=%d (dim must be 256, 512, 768 or 1024)", (long long)rows, dim);
    AMAV_REQUIRE(hidden && hidden_out && weight && bias, "amav_add_layernorm: NULL pointer");
    AMAV_REQUIRE((out_norm != nullptr) != (out_norm_split != nullptr),
                 "amav_add_layernorm: give exactly one of out_norm (fp32) and out_norm_split (bf16 split operand)");
    AMAV_REQUIRE(add || !add_bias, "amav_add_layernorm: add_bias without add");
    AMAV_REQUIRE(!out_norm_split || split_format_ok(split_format, split_scale_exp),
                 "amav_add_layernorm: split format %d / scale exponent %d", split_format, split_scale_exp);
    AMAV_REQUIRE(((reinterpret_cast<uintptr_t>(hidden) | reinterpret_cast<uintptr_t>(hidden_out) |
                   reinterpret_cast<uintptr_t>(out_norm) | reinterpret_cast<uintptr_t>(out_norm_split) |
                   reinterpret_cast<uintptr_t>(add) | reinterpret_cast<uintptr_t>(add_bias) |
                   reinterpret_cast<uintptr_t>(batch_row) |
                   reinterpret_cast<uintptr_t>(weight) | reinterpret_cast<uintptr_t>(bias)) & 15) == 0,
                 "amav_add_layernorm: buffers must be 16-byte aligned");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const unsigned grid = (unsigned)((rows + 3) / 4);
    auto p4 = [](const float *p) { return reinterpret_cast<const float4 *>(p); };
    float4 *h4 = reinterpret_cast<float4 *>(hidden_out), *o4 = reinterpret_cast<float4 *>(out_norm);
    const float prescale = ldexpf(1.0f, out_norm_split && split_format == AMAV_SPLIT_FP16X2 ? split_scale_exp : 0);
#define AMAV_LN_ARGS rows, rows_per_batch, p4(add), p4(add_bias), p4(batch_row), p4(hidden), h4, p4(weight), p4(bias), eps, \
                     o4, out_norm_split, prescale
#define AMAV_LN_LAUNCH(V)                                                                                   \
    do {                                                                                                    \
        if (!out_norm_split)                                                                                \
            amav::rows_fwd::add_layernorm_kernel<V, 0><<<grid, 256, 0, stream>>>(AMAV_LN_ARGS);                 \
        else if (split_format == AMAV_SPLIT_FP16X2)                                                         \
            amav::rows_fwd::add_layernorm_kernel<V, 2><<<grid, 256, 0, stream>>>(AMAV_LN_ARGS);                 \
        else                                                                                                \
            amav::rows_fwd::add_layernorm_kernel<V, 1><<<grid, 256, 0, stream>>>(AMAV_LN_ARGS);                 \
    } while (0)
    if (dim == 256) AMAV_LN_LAUNCH(1);
    else if (dim == 512) AMAV_LN_LAUNCH(2);
    else if (dim == 768) AMAV_LN_LAUNCH(3);
    else AMAV_LN_LAUNCH(4);
#undef AMAV_LN_LAUNCH
#undef AMAV_LN_ARGS
    return check_launch("amav_add_layernorm");
}
