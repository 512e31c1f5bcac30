// 3x3 convolution over a batch of independent square cells, the hot path of the windowed triplane upsampler
// (TriplaneUpsampler._tile_block_hip).  Replaces the mosaic image that the library's Winograd
// kernel ran (reference: src/models/renderer.py:364-417, three nn.Conv2d per UpsampleBlock).
//
//   amav_conv3x3_prepare_weights_split   torch's [Cout,Cin,3,3] (x an optional per-output-channel scale) -> two fp16 parts
//                                        in MFMA fragment order, tap-major: the layout of subm_weights_split_kernel
//   amav_conv3x3_cells                   out [K,H,W,Cout] = epilogue(conv3x3(zero(prologue(x)))), channels-last
//
// Arithmetic: pair_gemm_f16_kernel's (cloud.hip): fp16 x 2 split operands, three v_mfma_f32_32x32x16_f16 per fp32 product,
// small terms first, fp32 accumulation, unscaled in the epilogue.
//
// Tiling: one workgroup (256 threads, 4 waves) owns 8 x 16 output texels of ONE cell and NT output channels; wave w owns
// tile rows 2w and 2w + 1, i.e. 32 GEMM rows x NT columns = NT / 32 accumulators of 16 VGPRs.  For every 32-channel chunk
// of Cin the 10 x 18 input patch (tile + halo) is read ONCE: prologue, zeroing, scaling and the split happen while it is
// staged, and the nine taps then read it at nine shifted LDS addresses, so the gather and the split cost a ninth of
// what nine separate K-segments would.  The contraction is walked chunk-outer / tap-inner for that reason; the
// prepared weights stay tap-major.  Weights of one (tap, chunk) are 4 KB per 32 columns, double-buffered in LDS, their
// global reads one tap ahead in registers; the next chunk's patch is read into registers while the nine taps of the
// current one run.
//   LDS: A 2 parts x 180 texels x 80 B (32 halfs + 8 pad: conflict-free 16-byte fragment reads) = 28 800 B,
//        B 2 buffers x NT / 32 x 4 KB = 32 KB at NT = 128; 61.6 KB per workgroup, two workgroups per CU.
#include <algorithm>
#include <climits>

#include "amav_common.h"
#include "split_f16.h"

namespace amav {
namespace upconv {

constexpr int kTileH = 8, kTileW = 16;
constexpr int kPatchW = kTileW + 2, kPatch = (kTileH + 2) * kPatchW;  // 180 texels
constexpr int kKC = 32, kLDA = kKC + 8;
constexpr int kAItems = (kPatch * (kKC / 4) + 255) / 256;  // float4 reads per thread and chunk: 6
constexpr size_t kWorkspaceBytes = 256;

struct Params {
    const float *x;
    const void *wsplit;
    const unsigned *amax;
    const float *in_scale, *in_shift, *bias, *residual;
    const int *origin;
    float *out;
    int H, W, Cin, Cout, extent, upsample, relu_out, tiles_x, tiles_per_cell;
};

__device__ __forceinline__ float prologue(float x, float s, float b) { return fmaxf(__builtin_fmaf(s, x, b), 0.f); }

// largest |operand| over x [n4 float4], after the prologue when there is one -> out[0] (bits of a non-negative float:
// an integer maximum, order-independent)
__global__ __launch_bounds__(256) void operand_absmax_kernel(const float4 *__restrict__ x4, long long n4, int cin4,
                                                             const float4 *__restrict__ scale4,
                                                             const float4 *__restrict__ shift4, unsigned *__restrict__ out) {
    float m = 0.f;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        float4 v = x4[i];
        if (scale4) {
            const int c = (int)(i % cin4);
            const float4 s = scale4[c], b = shift4[c];
            v = make_float4(prologue(v.x, s.x, b.x), prologue(v.y, s.y, b.y), prologue(v.z, s.z, b.z), prologue(v.w, s.w, b.w));
        }
        m = fmaxf(m, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    __shared__ float wm[4];
    if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(out, __float_as_uint(fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3]))));
}

// largest |w[co][ci][tap] * scale[co]| -> hdr[0]
__global__ __launch_bounds__(256) void weights_absmax_kernel(const float *__restrict__ w, long long n, int per_cout,
                                                             const float *__restrict__ scale, unsigned *__restrict__ hdr) {
    float m = 0.f;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        m = fmaxf(m, fabsf(scale ? w[i] * scale[i / per_cout] : w[i]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    __shared__ float wm[4];
    if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(hdr, __float_as_uint(fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3]))));
}

// w [cout][cin][3][3] (x scale[cout]) -> [tap][cout / 32][cin / 16][part][lane half hh][column c][8 k] fp16, as
// subm_weights_split_kernel (cloud.hip).  One thread per (tap, column block, k-step, hh, c).
__global__ __launch_bounds__(256) void weights_split_kernel(const float *__restrict__ w, const float *__restrict__ scale,
                                                            int cin, int cout, long long items, unsigned *__restrict__ hdr,
                                                            _Float16 *__restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int e = f16_scale_exp(__uint_as_float(hdr[0]));
    if (i == 0) reinterpret_cast<int *>(hdr)[1] = e;
    if (i >= items) return;
    const int c = (int)(i & 31), hh = (int)((i >> 5) & 1);
    const long long rest = i >> 6;  // (tap * nblk + nb) * ksteps + ks
    const int ksteps = cin / 16, nblk = cout / 32;
    const int ks = (int)(rest % ksteps), nb = (int)((rest / ksteps) % nblk);
    const int tap = (int)(rest / ksteps / nblk);
    const int co = nb * 32 + c;
    const float pow2 = ldexpf(1.0f, e), s = scale ? scale[co] : 1.0f;
    f16x8 p1, p2;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int k = 16 * ks + 8 * hh + j;
        const float v = w[((size_t)co * cin + k) * 9 + tap];
        _Float16 a, b;
        split2((scale ? v * s : v) * pow2, a, b);
        p1[j] = a, p2[j] = b;
    }
    _Float16 *dst = out + (rest * 2) * 512 + hh * 256 + c * 8;
    *reinterpret_cast<f16x8 *>(dst) = p1;
    *reinterpret_cast<f16x8 *>(dst + 512) = p2;
}

// grid (K * tiles per cell, Cout / NT), 256 threads
template <int NT>
__global__ __launch_bounds__(256, 2) void conv3x3_cells_kernel(const Params p) {
    constexpr int NACC = NT / 32;
    __shared__ _Float16 As[2][kPatch * kLDA];  // [part][patch texel][k]
    __shared__ float4 Bs[2][NACC * 256];       // [buffer][column block][k-step][part][hh][c][8 k]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 31, hh = lane >> 5;
    const long long cell = blockIdx.x / p.tiles_per_cell;
    const int tile = (int)(blockIdx.x - cell * p.tiles_per_cell);
    const int ty0 = (tile / p.tiles_x) * kTileH, tx0 = (tile % p.tiles_x) * kTileW;
    const int n0 = blockIdx.y * NT;
    const int H = p.H, W = p.W, Cin = p.Cin, Cout = p.Cout;
    const int ea = f16_scale_exp(__uint_as_float(p.amax[0]));
    const int ew = reinterpret_cast<const int *>(p.wsplit)[1];
    const float a_scale = ldexpf(1.0f, ea);
    const int ksteps = Cin / 16, nblk = Cout / 32, nchunks = Cin / kKC;
    // prepared weights of (tap, column block nb, k-step ks) at ((tap * nblk + nb) * ksteps + ks) * 128 float4
    const float4 *wbase = reinterpret_cast<const float4 *>(static_cast<const char *>(p.wsplit) + kSplitHeader) +
                          (size_t)(n0 / 32) * ksteps * 128 + tid;
    const size_t tap_stride = (size_t)nblk * ksteps * 128, blk_stride = (size_t)ksteps * 128;

    // the patch texels this thread stages: item i = tid + 256 j is (texel i / 8, channels 4 (i % 8) .. + 3) of the chunk
    const int ak = (tid & 7) * 4;
    const int h_in = p.upsample ? H >> 1 : H, w_in = p.upsample ? W >> 1 : W;
    int oy = 0, ox = 0;
    if (p.origin) oy = p.origin[2 * cell], ox = p.origin[2 * cell + 1];
    long long aoff[kAItems];  // float offset of the source texel's channel ak, or -1: a zero of the operand
#pragma unroll
    for (int j = 0; j < kAItems; ++j) {
        const int texel = (tid >> 3) + 32 * j;
        const int y = ty0 + texel / kPatchW - 1, x = tx0 + texel % kPatchW - 1;
        bool ok = texel < kPatch && y >= 0 && y < H && x >= 0 && x < W;  // zero padding at the output's resolution
        if (p.origin) ok = ok && oy + y >= 0 && oy + y < p.extent && ox + x >= 0 && ox + x < p.extent;
        const int sy = p.upsample ? y >> 1 : y, sx = p.upsample ? x >> 1 : x;
        aoff[j] = ok ? ((cell * h_in + sy) * w_in + sx) * (long long)Cin + ak : -1;
    }
    float4 av[kAItems], sc, sh, b0, b1, b2, b3;
    sc = sh = b1 = b2 = b3 = make_float4(0.f, 0.f, 0.f, 0.f);
#define AMAV_UC_LOAD_A(k0_)                                                                                   \
    {                                                                                                         \
        _Pragma("unroll") for (int j = 0; j < kAItems; ++j) av[j] =                                           \
            aoff[j] >= 0 ? *reinterpret_cast<const float4 *>(p.x + aoff[j] + (k0_)) : make_float4(0.f, 0.f, 0.f, 0.f); \
        if (p.in_scale) {                                                                                     \
            sc = *reinterpret_cast<const float4 *>(p.in_scale + (k0_) + ak);                                  \
            sh = *reinterpret_cast<const float4 *>(p.in_shift + (k0_) + ak);                                  \
        }                                                                                                     \
    }
#define AMAV_UC_LOAD_B(tap_, chunk_)                                                      \
    {                                                                                     \
        const float4 *src_ = wbase + (size_t)(tap_) * tap_stride + (size_t)(chunk_) * 256; \
        b0 = src_[0];                                                                     \
        if (NACC > 1) b1 = src_[blk_stride];                                              \
        if (NACC > 2) b2 = src_[2 * blk_stride], b3 = src_[3 * blk_stride];               \
    }
    f32x16 acc[NACC];
#pragma unroll
    for (int a = 0; a < NACC; ++a)
#pragma unroll
        for (int t = 0; t < 16; ++t) acc[a][t] = 0.f;

    // this lane's A row: GEMM row wave * 32 + c = tile texel (2 wave + (c >> 4), c & 15); tap (dy, dx) reads the patch
    // texel (row + dy, column + dx)
    const int arow = (2 * wave + (c >> 4)) * kPatchW + (c & 15);

    AMAV_UC_LOAD_A(0)
    AMAV_UC_LOAD_B(0, 0)
    int buf = 0;
    for (int chunk = 0; chunk < nchunks; ++chunk) {
        __syncthreads();  // the previous chunk's taps have read the patch
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
                *reinterpret_cast<f16x4 *>(&As[0][texel * kLDA + ak]) = h1;
                *reinterpret_cast<f16x4 *>(&As[1][texel * kLDA + ak]) = h2;
            }
        }
        if (chunk + 1 < nchunks) AMAV_UC_LOAD_A((chunk + 1) * kKC)
        for (int tap = 0; tap < 9; ++tap, buf ^= 1) {
            Bs[buf][tid] = b0;
            if (NACC > 1) Bs[buf][256 + tid] = b1;
            if (NACC > 2) Bs[buf][512 + tid] = b2, Bs[buf][768 + tid] = b3;
            __syncthreads();  // one barrier per tap: the other buffer was last read before the previous one
            if (tap < 8) AMAV_UC_LOAD_B(tap + 1, chunk)
            else if (chunk + 1 < nchunks) AMAV_UC_LOAD_B(0, chunk + 1)
            const int dy = tap / 3, dx = tap - 3 * dy;
            const _Float16 *al = &As[0][(arow + dy * kPatchW + dx) * kLDA + 8 * hh];
            const _Float16 *bl = reinterpret_cast<const _Float16 *>(Bs[buf]) + hh * 256 + c * 8;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const f16x8 h1 = *reinterpret_cast<const f16x8 *>(al + 16 * s);
                const f16x8 h2 = *reinterpret_cast<const f16x8 *>(al + kPatch * kLDA + 16 * s);
#pragma unroll
                for (int a = 0; a < NACC; ++a) {
                    const f16x8 g1 = *reinterpret_cast<const f16x8 *>(bl + (a * 4 + s * 2 + 0) * 512);
                    const f16x8 g2 = *reinterpret_cast<const f16x8 *>(bl + (a * 4 + s * 2 + 1) * 512);
                    acc[a] = __builtin_amdgcn_mfma_f32_32x32x16_f16(h2, g1, acc[a], 0, 0, 0);  // small terms first
                    acc[a] = __builtin_amdgcn_mfma_f32_32x32x16_f16(h1, g2, acc[a], 0, 0, 0);
                    acc[a] = __builtin_amdgcn_mfma_f32_32x32x16_f16(h1, g1, acc[a], 0, 0, 0);
                }
            }
        }
    }
#undef AMAV_UC_LOAD_A
#undef AMAV_UC_LOAD_B
    const float unscale = ldexpf(1.0f, -(ea + ew));
    float bias[NACC];
#pragma unroll
    for (int a = 0; a < NACC; ++a) bias[a] = p.bias ? p.bias[n0 + 32 * a + c] : 0.f;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const int r = wave * 32 + (t & 3) + 8 * (t >> 2) + 4 * hh;
        const int y = ty0 + (r >> 4), x = tx0 + (r & 15);
        if (y < H && x < W) {
            const size_t o = (((size_t)cell * H + y) * W + x) * Cout + n0 + c;
#pragma unroll
            for (int a = 0; a < NACC; ++a) {
                float v = acc[a][t] * unscale + bias[a];
                if (p.relu_out) v = fmaxf(v, 0.f);
                if (p.residual) v += p.residual[o + 32 * a];
                p.out[o + 32 * a] = v;
            }
        }
    }
}

}  // namespace upconv
}  // namespace amav

using namespace amav;

static bool conv3x3_sizes_ok(int cin, int cout) { return cin > 0 && cin % 32 == 0 && cout > 0 && cout % 32 == 0; }

static size_t conv3x3_split_bytes(int cin, int cout) { return kSplitHeader + (size_t)9 * cin * cout * 2 * sizeof(_Float16); }

extern "C" size_t amav_conv3x3_weights_split_bytes(int cin, int cout) {
    return conv3x3_sizes_ok(cin, cout) ? conv3x3_split_bytes(cin, cout) : 0;
}

extern "C" size_t amav_conv3x3_workspace_bytes(void) { return upconv::kWorkspaceBytes; }

extern "C" int amav_conv3x3_prepare_weights_split(int cin, int cout, const float *weights, const float *out_scale, void *out,
                                                  size_t out_bytes, void *stream_) {
    AMAV_REQUIRE(conv3x3_sizes_ok(cin, cout),
                 "amav_conv3x3_prepare_weights_split: channels must be multiples of 32 (C_in %d, C_out %d)", cin, cout);
    AMAV_REQUIRE(weights && out && (reinterpret_cast<uintptr_t>(out) & 255) == 0,
                 "amav_conv3x3_prepare_weights_split: NULL / misaligned pointer (out: 256 bytes)");
    if (out_bytes < conv3x3_split_bytes(cin, cout))
        return fail(AMAV_ERR_WORKSPACE, "amav_conv3x3_prepare_weights_split: buffer %zu < required %zu", out_bytes,
                    conv3x3_split_bytes(cin, cout));
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    unsigned *hdr = static_cast<unsigned *>(out);
    AMAV_REQUIRE(zero_async(hdr, kSplitHeader, stream) == hipSuccess, "amav_conv3x3_prepare_weights_split: header clear failed");
    const long long n = (long long)9 * cin * cout;
    upconv::weights_absmax_kernel<<<(unsigned)std::min<long long>((n + 255) / 256, 256), 256, 0, stream>>>(weights, n, 9 * cin,
                                                                                                            out_scale, hdr);
    const long long items = (long long)9 * (cout / 32) * (cin / 16) * 64;
    upconv::weights_split_kernel<<<blocks_for(items), 256, 0, stream>>>(
        weights, out_scale, cin, cout, items, hdr, reinterpret_cast<_Float16 *>(static_cast<char *>(out) + kSplitHeader));
    return check_launch("amav_conv3x3_prepare_weights_split");
}

extern "C" int amav_conv3x3_cells(const amav_conv3x3_args *a, void *stream_) {
    AMAV_REQUIRE(a != nullptr, "amav_conv3x3_cells: args is NULL");
    const int H = a->height, W = a->width, cin = a->cin, cout = a->cout;
    AMAV_REQUIRE(a->cells > 0 && H > 0 && W > 0, "amav_conv3x3_cells: bad sizes cells=%lld H=%d W=%d", (long long)a->cells, H, W);
    AMAV_REQUIRE(conv3x3_sizes_ok(cin, cout), "amav_conv3x3_cells: channels must be multiples of 32 (C_in %d, C_out %d)", cin,
                 cout);
    AMAV_REQUIRE(!a->upsample_input || (H % 2 == 0 && W % 2 == 0),
                 "amav_conv3x3_cells: upsample_input needs even H and W (H=%d W=%d)", H, W);
    AMAV_REQUIRE(a->x_dev && a->weights_split_dev && a->out_dev, "amav_conv3x3_cells: NULL pointer (x, weights_split, out)");
    AMAV_REQUIRE(!a->in_scale_dev == !a->in_shift_dev, "amav_conv3x3_cells: in_scale and in_shift come together");
    AMAV_REQUIRE(!a->origin_dev || a->extent > 0, "amav_conv3x3_cells: origin needs a positive extent, got %d", a->extent);
    AMAV_REQUIRE(aligned16(a->x_dev, a->in_scale_dev, a->in_shift_dev) && aligned16(a->weights_split_dev),
                 "amav_conv3x3_cells: x, in_scale, in_shift and weights_split must be 16-byte aligned");
    if (a->weights_split_bytes < conv3x3_split_bytes(cin, cout))
        return fail(AMAV_ERR_WORKSPACE, "amav_conv3x3_cells: weights_split %zu < required %zu", a->weights_split_bytes,
                    conv3x3_split_bytes(cin, cout));
    if (!a->workspace_dev || a->workspace_bytes < upconv::kWorkspaceBytes || (reinterpret_cast<uintptr_t>(a->workspace_dev) & 15))
        return fail(AMAV_ERR_WORKSPACE, "amav_conv3x3_cells: workspace %zu < required %zu (or NULL / misaligned)",
                    a->workspace_bytes, upconv::kWorkspaceBytes);
    const int tiles_x = (W + upconv::kTileW - 1) / upconv::kTileW, tiles_y = (H + upconv::kTileH - 1) / upconv::kTileH;
    const long long blocks = a->cells * tiles_x * tiles_y;
    AMAV_REQUIRE(blocks <= INT_MAX, "amav_conv3x3_cells: %lld tiles exceed the grid", blocks);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    unsigned *amax = static_cast<unsigned *>(a->workspace_dev);
    AMAV_REQUIRE(zero_async(amax, 16, stream) == hipSuccess, "amav_conv3x3_cells: workspace clear failed");
    const int h_in = a->upsample_input ? H / 2 : H, w_in = a->upsample_input ? W / 2 : W;
    const long long n4 = a->cells * h_in * w_in * (cin / 4);
    upconv::operand_absmax_kernel<<<(unsigned)std::min<long long>((n4 + 255) / 256, 1024), 256, 0, stream>>>(
        reinterpret_cast<const float4 *>(a->x_dev), n4, cin / 4, reinterpret_cast<const float4 *>(a->in_scale_dev),
        reinterpret_cast<const float4 *>(a->in_shift_dev), amax);
    upconv::Params p;
    p.x = a->x_dev, p.wsplit = a->weights_split_dev, p.amax = amax;
    p.in_scale = a->in_scale_dev, p.in_shift = a->in_shift_dev, p.bias = a->bias_dev, p.residual = a->residual_dev;
    p.origin = a->origin_dev, p.out = a->out_dev;
    p.H = H, p.W = W, p.Cin = cin, p.Cout = cout, p.extent = a->extent, p.upsample = a->upsample_input != 0;
    p.relu_out = a->relu_out != 0, p.tiles_x = tiles_x, p.tiles_per_cell = tiles_x * tiles_y;
    const int nt = cout % 128 == 0 ? 128 : (cout % 64 == 0 ? 64 : 32);
    const dim3 grid((unsigned)blocks, (unsigned)(cout / nt));
    if (nt == 128)
        upconv::conv3x3_cells_kernel<128><<<grid, 256, 0, stream>>>(p);
    else if (nt == 64)
        upconv::conv3x3_cells_kernel<64><<<grid, 256, 0, stream>>>(p);
    else
        upconv::conv3x3_cells_kernel<32><<<grid, 256, 0, stream>>>(p);
    return check_launch("amav_conv3x3_cells");
}
