// 3x3 convolution over a batch of independent square cells, the hot path of the windowed triplane upsampler
// (TriplaneUpsampler._tile_block_hip).  Replaces the mosaic image that the library's Winograd
// kernel ran (reference: src/models/renderer.py:364-417, three nn.Conv2d per UpsampleBlock).
//
//   amav_conv3x3_prepare_weights_split   torch's [Cout,Cin,3,3] (x an optional per-output-channel scale) -> two fp16 parts
//                                        in MFMA fragment order, tap-major: the layout of subm_weights_split_kernel
//   amav_conv3x3_cells                   out [K,H,W,Cout] = epilogue(conv3x3(zero(prologue(x)))), channels-last
//   amav_conv3x3_cells_backward          its gradients: the data gradient on conv3x3_cells_kernel
//                                        itself (gated operand, weights from ..._prepare_weights_split_transposed), a row
//                                        kernel for the operand's backward, conv3x3_wgrad_kernel for the weights, two-stage
//                                        column sums; fixed summation orders, no float atomics
//
// Arithmetic: pair_gemm_f16_kernel's (cloud.hip): fp16 x 2 split operands, three v_mfma_f32_32x32x16_f16 per fp32 product,
// small terms first, fp32 accumulation, unscaled in the epilogue.
//
// The operand staging (PatchStage) is in upsample_conv_stage.h, shared with the weight-gradient kernel.
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
#include "upsample_conv_stage.h"
#include "wave_ops.h"

namespace amav {
namespace upconv {

constexpr size_t kWorkspaceBytes = 256;

// largest |operand| over x [n4 float4], after the prologue when there is one, after the gate (x where gate4 > 0) when
// there is one -> out[0] (bits of a non-negative float: an integer maximum, order-independent)
__global__ __launch_bounds__(256) void operand_absmax_kernel(const float4 *__restrict__ x4, long long n4, int cin4,
                                                             const float4 *__restrict__ scale4,
                                                             const float4 *__restrict__ shift4,
                                                             const float4 *__restrict__ gate4, unsigned *__restrict__ out) {
    float m = 0.f;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        float4 v = x4[i];
        if (gate4) v = gated(v, gate4[i]);
        if (scale4) {
            const int c = (int)(i % cin4);
            const float4 s = scale4[c], b = shift4[c];
            v = make_float4(prologue(v.x, s.x, b.x), prologue(v.y, s.y, b.y), prologue(v.z, s.z, b.z), prologue(v.w, s.w, b.w));
        }
        m = absmax4(m, v);
    }
    block_absmax_publish(m, out);
}

// largest |w[co][ci][tap] * scale[co]| -> hdr[0]
__global__ __launch_bounds__(256) void weights_absmax_kernel(const float *__restrict__ w, long long n, int per_cout,
                                                             const float *__restrict__ scale, unsigned *__restrict__ hdr) {
    float m = 0.f;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        m = fmaxf(m, fabsf(scale ? w[i] * scale[i / per_cout] : w[i]));
    block_absmax_publish(m, hdr);
}

// w [cout][cin][3][3] (x scale[cout]) -> [tap][cout / 32][cin / 16][part][lane half hh][column c][8 k] fp16, as
// subm_weights_split_kernel (cloud.hip).  One thread per (tap, column block, k-step, hh, c).  transposed: `w` is
// [cin][cout][3][3] and the prepared weights are those of the data gradient, W'[co][k][tap] = w[k][co][8 - tap] (the
// roles of the channel counts swapped by the caller, the taps flipped); no scale.
__global__ __launch_bounds__(256) void weights_split_kernel(const float *__restrict__ w, const float *__restrict__ scale,
                                                            int cin, int cout, int transposed, long long items,
                                                            unsigned *__restrict__ hdr, _Float16 *__restrict__ out) {
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
        const float v = transposed ? w[((size_t)k * cout + co) * 9 + (8 - tap)] : w[((size_t)co * cin + k) * 9 + tap];
        _Float16 a, b;
        split2((scale ? v * s : v) * pow2, a, b);
        p1[j] = a, p2[j] = b;
    }
    _Float16 *dst = out + (rest * 2) * 512 + hh * 256 + c * 8;
    *reinterpret_cast<f16x8 *>(dst) = p1;
    *reinterpret_cast<f16x8 *>(dst + 512) = p2;
}

// grid (K * tiles per cell, Cout / NT), 256 threads.  GATE: the operand is p.x where p.gate > 0 (the data gradient runs
// this kernel on the gated output gradient and the transposed, flipped weights).
template <int NT, bool GATE>
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

    PatchStage st;
    st.locate(p, cell, ty0, tx0, tid);
    float4 b0, b1, b2, b3;
    b1 = b2 = b3 = make_float4(0.f, 0.f, 0.f, 0.f);
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

    st.template load<GATE>(p, 0);
    AMAV_UC_LOAD_B(0, 0)
    int buf = 0;
    for (int chunk = 0; chunk < nchunks; ++chunk) {
        __syncthreads();  // the previous chunk's taps have read the patch
        st.stage(p, a_scale, tid, [&](int texel, int ak, f16x4 h1, f16x4 h2) {
            *reinterpret_cast<f16x4 *>(&As[0][texel * kLDA + ak]) = h1;
            *reinterpret_cast<f16x4 *>(&As[1][texel * kLDA + ak]) = h2;
        });
        if (chunk + 1 < nchunks) st.template load<GATE>(p, (chunk + 1) * kKC);
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


// ---- backward ------------------------------------------------------------------------------------------------------

constexpr int kColBlocks = 256;  // first-stage blocks of every column sum: each owns a contiguous range of rows

// first stage of grad_bias: partial[b][c] = sum over the rows of block b of ga[row][c], ga = g (where gate > 0).  Thread
// (row lane tid / 8 of 32, channels 4 (tid % 8) .. + 3 of the 32-channel block) adds its rows in ascending order, the 32
// row lanes are added in ascending order: a fixed order, no atomics.
__global__ __launch_bounds__(256) void bias_partial_kernel(const float *__restrict__ g, const float *__restrict__ gate,
                                                           long long rows, int C, float *__restrict__ partial) {
    __shared__ float4 red[256];
    const int tid = threadIdx.x, q = tid & 7, rl = tid >> 3;
    const long long r0 = rows * blockIdx.x / gridDim.x, r1 = rows * (blockIdx.x + 1) / gridDim.x;
    for (int c0 = 0; c0 < C; c0 += 32) {
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        for (long long r = r0 + rl; r < r1; r += 32) {
            const size_t o = (size_t)r * C + c0 + 4 * q;
            float4 v = *reinterpret_cast<const float4 *>(g + o);
            if (gate) v = gated(v, *reinterpret_cast<const float4 *>(gate + o));
            s.x += v.x, s.y += v.y, s.z += v.z, s.w += v.w;
        }
        red[tid] = s;
        __syncthreads();
        if (rl == 0) {
            for (int i = 1; i < 32; ++i) {
                const float4 v = red[8 * i + q];
                s.x += v.x, s.y += v.y, s.z += v.z, s.w += v.w;
            }
            *reinterpret_cast<float4 *>(partial + (size_t)blockIdx.x * C + c0 + 4 * q) = s;
        }
        __syncthreads();
    }
}

// second stage of every column sum: out[c] = partial[0][c] + partial[1][c] + ... in ascending order (rows `stride` apart)
__global__ __launch_bounds__(256) void column_finish_kernel(const float *__restrict__ partial, int blocks, int stride, int C,
                                                            float *__restrict__ out) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    float s = 0.f;
    for (int b = 0; b < blocks; ++b) s += partial[(size_t)b * stride + c];
    out[c] = s;
}

// The operand's backward, one row kernel behind the data gradient gz [K,H,W,Cin] = dL/dZ: with
// m = inside (the plane rule; the cell's own padding holds no texel of gz) x [in_scale x + in_shift > 0],
//   grad_x [K,h,w,Cin] = in_scale * (sum over the 1 or 2 x 2 fine texels of gz m), the fine texels in row-major order;
//   partial[b][0][c] = sum over the rows of block b of gz m up(x)   (grad_in_scale's first stage)
//   partial[b][1][c] = sum over the rows of block b of gz m         (grad_in_shift's)
// rows are the texels of x (coarse with upsample), threads and order as bias_partial_kernel.
__global__ __launch_bounds__(256) void operand_backward_kernel(const Params p, const float *__restrict__ gz, long long rows,
                                                               float *__restrict__ grad_x, float *__restrict__ partial) {
    __shared__ float4 red[2][256];
    const int tid = threadIdx.x, q = tid & 7, rl = tid >> 3;
    const int H = p.H, W = p.W, C = p.Cin, f = p.upsample ? 2 : 1;
    const int h_in = H / f, w_in = W / f;
    const long long r0 = rows * blockIdx.x / gridDim.x, r1 = rows * (blockIdx.x + 1) / gridDim.x;
    for (int c0 = 0; c0 < C; c0 += 32) {
        const int ch = c0 + 4 * q;
        float4 sc = make_float4(1.f, 1.f, 1.f, 1.f), sh = make_float4(0.f, 0.f, 0.f, 0.f);
        if (p.in_scale) sc = *reinterpret_cast<const float4 *>(p.in_scale + ch), sh = *reinterpret_cast<const float4 *>(p.in_shift + ch);
        float4 ss = make_float4(0.f, 0.f, 0.f, 0.f), st = ss;
        for (long long r = r0 + rl; r < r1; r += 32) {
            const long long cell = r / ((long long)h_in * w_in);
            const int rem = (int)(r - cell * h_in * w_in), sy = rem / w_in, sx = rem - sy * w_in;
            int oy = 0, ox = 0;
            if (p.origin) oy = p.origin[2 * cell], ox = p.origin[2 * cell + 1];
            float4 xv = make_float4(0.f, 0.f, 0.f, 0.f);
            bool mx = true, my = true, mz = true, mw = true;
            if (p.in_scale) {
                xv = *reinterpret_cast<const float4 *>(p.x + (size_t)r * C + ch);
                mx = __builtin_fmaf(sc.x, xv.x, sh.x) > 0.f, my = __builtin_fmaf(sc.y, xv.y, sh.y) > 0.f;
                mz = __builtin_fmaf(sc.z, xv.z, sh.z) > 0.f, mw = __builtin_fmaf(sc.w, xv.w, sh.w) > 0.f;
            }
            float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int i = 0; i < f * f; ++i) {
                const int y = sy * f + i / f, x = sx * f + i % f;
                if (p.origin && !(oy + y >= 0 && oy + y < p.extent && ox + x >= 0 && ox + x < p.extent)) continue;
                const float4 v = *reinterpret_cast<const float4 *>(gz + (((size_t)cell * H + y) * W + x) * C + ch);
                s.x += v.x, s.y += v.y, s.z += v.z, s.w += v.w;
            }
            s = make_float4(mx ? s.x : 0.f, my ? s.y : 0.f, mz ? s.z : 0.f, mw ? s.w : 0.f);
            if (grad_x)
                *reinterpret_cast<float4 *>(grad_x + (size_t)r * C + ch) = make_float4(s.x * sc.x, s.y * sc.y, s.z * sc.z, s.w * sc.w);
            ss.x += s.x * xv.x, ss.y += s.y * xv.y, ss.z += s.z * xv.z, ss.w += s.w * xv.w;
            st.x += s.x, st.y += s.y, st.z += s.z, st.w += s.w;
        }
        if (partial) {  // uniform over the grid
            red[0][tid] = ss, red[1][tid] = st;
            __syncthreads();
            if (rl == 0) {
                for (int i = 1; i < 32; ++i) {
                    const float4 a = red[0][8 * i + q], b = red[1][8 * i + q];
                    ss.x += a.x, ss.y += a.y, ss.z += a.z, ss.w += a.w;
                    st.x += b.x, st.y += b.y, st.z += b.z, st.w += b.w;
                }
                *reinterpret_cast<float4 *>(partial + ((size_t)blockIdx.x * 2 + 0) * C + ch) = ss;
                *reinterpret_cast<float4 *>(partial + ((size_t)blockIdx.x * 2 + 1) * C + ch) = st;
            }
            __syncthreads();
        }
    }
}

// Weight gradient: gw[tap][ci][co] = sum over the texels of ga[texel][co] Z[texel + tap][ci], a GEMM whose contraction
// runs over all K H W texels, in the forward's arithmetic (fp16 x 2 parts of Z and of ga, three MFMAs per product, small
// terms first; exponents from the forward's sweep of the operand and the data gradient's sweep of ga).
//
// grid (slices, ceil(Cout / 64), ceil(Cin / 64)), 256 threads.  A workgroup owns 64 output x 64 input channels and the
// contiguous range of (cell, tile) pairs of its slice; wave w owns the 32 x 32 block (ci block w / 2, co block w % 2) and
// keeps all nine taps' accumulators (9 x 16 VGPRs).  Per pair, Z's 10 x 18 patch is rebuilt by PatchStage for the two
// 32-channel chunks and ga's 8 x 16 tile is read with its gate; both go to LDS TRANSPOSED relative to the forward --
// [channel][texel], the texels of a row contiguous -- because the contraction index, the texel, is the MFMA's k: k-step ks
// is tile row ks, lane half hh holds its texels 8 hh .. 8 hh + 7, for Z shifted by the tap.
//   Zt [part][64 ci][10 rows x 24 halfs, 248 per channel]: a tap row starts 16-byte aligned; the lane reads the aligned
//      16 halfs from 8 hh on and shifts them by dx = 0, 1, 2 halfs in registers (one read serves three taps).
//   Gt [part][64 co][128 texels, 136 per channel].
//   248 = 8 x 31 and 136 = 8 x 17: odd multiples of 16 bytes per lane, conflict-free 16-byte reads.  The stores are
//   two-byte and transposed: a wave holds 8 texels x 8 groups of 4 channels, so the channels of a chunk are permuted
//   over its 32 rows (chunk_channel) -- the 8 lanes that store one channel each then hit rows q + 8 e, 8 banks a multiple
//   of 4 apart, and the 8 texels fill the 4 dwords between them, instead of 8 lanes on 2 banks.  MFMA row / column r is
//   the channel of LDS row r; the epilogue undoes the permutation.  96 KB, one workgroup per CU; the next pair's global
//   reads are in flight while the current pair's MFMAs run.
// Every workgroup writes its slot [slice][tap][ci][co] (zeros for an empty range): nothing is memset, nothing atomic.
constexpr int kZRow = 24, kZStride = 248, kGStride = 136, kWgC = 64;
constexpr int kGItems = kTileH * kTileW * (kKC / 4) / 256;  // float4 reads of ga per thread and 32-channel chunk: 4
constexpr size_t kWgradLds = (size_t)(2 * kWgC * kZStride + 2 * kWgC * kGStride) * sizeof(_Float16);

struct WgradParams {
    Params z;  // the forward's operand: x, prologue, origin / extent, upsample, H, W, Cin, the tiling; amax: the operand's
    const float *g, *gate;
    const unsigned *amax_g;
    float *slots;
    long long pairs;
    int Cout;
};

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// LDS row r of a 32-channel chunk holds channel 4 (r % 8) + r / 8, i.e. channel 4 q + e sits in row q + 8 e
__device__ __forceinline__ int chunk_channel(int r) { return 4 * (r & 7) + (r >> 3); }

// halfs dx .. dx + 7 of the 16 halfs (lo, hi)
__device__ __forceinline__ f16x8 shifted_halfs(u32x4 lo, u32x4 hi, int dx) {
    u32x4 r = lo;
    if (dx == 1) {
        r.x = (lo.x >> 16) | (lo.y << 16), r.y = (lo.y >> 16) | (lo.z << 16);
        r.z = (lo.z >> 16) | (lo.w << 16), r.w = (lo.w >> 16) | (hi.x << 16);
    } else if (dx == 2) {
        r.x = lo.y, r.y = lo.z, r.z = lo.w, r.w = hi.x;
    }
    return __builtin_bit_cast(f16x8, r);
}

__global__ __launch_bounds__(256, 1) void conv3x3_wgrad_kernel(const WgradParams q) {
    extern __shared__ __align__(16) _Float16 wg_lds[];
    _Float16 *Zt = wg_lds, *Gt = wg_lds + 2 * kWgC * kZStride;
    const Params &p = q.z;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 31, hh = lane >> 5;
    const int cb = wave & 1, ib = wave >> 1;
    const int H = p.H, W = p.W, Cin = p.Cin, Cout = q.Cout;
    const int co0 = blockIdx.y * kWgC, ci0 = blockIdx.z * kWgC;
    const int zchunks = min(2, (Cin - ci0) / kKC), gchunks = min(2, (Cout - co0) / kKC);
    const bool active = ib < zchunks && cb < gchunks;
    const int ea = f16_scale_exp(__uint_as_float(p.amax[0])), eg = f16_scale_exp(__uint_as_float(q.amax_g[0]));
    const float a_scale = ldexpf(1.0f, ea), g_scale = ldexpf(1.0f, eg);
    const long long p0 = q.pairs * blockIdx.x / gridDim.x, p1 = q.pairs * (blockIdx.x + 1) / gridDim.x;

    f32x16 acc[9];
#pragma unroll
    for (int t9 = 0; t9 < 9; ++t9)
#pragma unroll
        for (int t = 0; t < 16; ++t) acc[t9][t] = 0.f;

    PatchStage st[2];
    float4 gv[2][kGItems];
    const int gk = (tid & 7) * 4;
    auto load_pair = [&](long long pair) {
        const long long cell = pair / p.tiles_per_cell;
        const int tile = (int)(pair - cell * p.tiles_per_cell);
        const int ty0 = (tile / p.tiles_x) * kTileH, tx0 = (tile % p.tiles_x) * kTileW;
        st[0].locate(p, cell, ty0, tx0, tid);
        st[0].template load<false>(p, ci0);
        if (zchunks > 1) {
            st[1] = st[0];
            st[1].template load<false>(p, ci0 + kKC);
        }
#pragma unroll
        for (int j = 0; j < kGItems; ++j) {
            const int texel = (tid >> 3) + 32 * j;
            const int y = ty0 + texel / kTileW, x = tx0 + texel % kTileW;
            const bool ok = y < H && x < W;
            const size_t o = (((size_t)cell * H + y) * W + x) * Cout + co0 + gk;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (ok && h < gchunks) {
                    v = *reinterpret_cast<const float4 *>(q.g + o + h * kKC);
                    if (q.gate) v = gated(v, *reinterpret_cast<const float4 *>(q.gate + o + h * kKC));
                }
                gv[h][j] = v;
            }
        }
    };

    if (p0 < p1) load_pair(p0);
    for (long long pair = p0; pair < p1; ++pair) {
        __syncthreads();  // the previous pair's MFMAs have read LDS
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (h < zchunks)
                st[h].stage(p, a_scale, tid, [&](int texel, int ak, f16x4 h1, f16x4 h2) {
                    _Float16 *d = Zt + (h * kKC + (ak >> 2)) * kZStride + (texel / kPatchW) * kZRow + texel % kPatchW;
#pragma unroll
                    for (int e = 0; e < 4; ++e) d[8 * e * kZStride] = h1[e], d[(kWgC + 8 * e) * kZStride] = h2[e];
                });
            if (h < gchunks) {
#pragma unroll
                for (int j = 0; j < kGItems; ++j) {
                    const float v_[4] = {gv[h][j].x, gv[h][j].y, gv[h][j].z, gv[h][j].w};
                    _Float16 *d = Gt + (h * kKC + (gk >> 2)) * kGStride + (tid >> 3) + 32 * j;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        _Float16 u, l;
                        split2(v_[e] * g_scale, u, l);
                        d[8 * e * kGStride] = u, d[(kWgC + 8 * e) * kGStride] = l;
                    }
                }
            }
        }
        __syncthreads();
        if (pair + 1 < p1) load_pair(pair + 1);
        if (active) {
            const _Float16 *zt = Zt + (ib * kKC + c) * kZStride + 8 * hh;
            const _Float16 *gt = Gt + (cb * kKC + c) * kGStride + 8 * hh;
#pragma unroll 1
            for (int ks = 0; ks < kTileH; ++ks) {
                const f16x8 g1 = *reinterpret_cast<const f16x8 *>(gt + ks * kTileW);
                const f16x8 g2 = *reinterpret_cast<const f16x8 *>(gt + kWgC * kGStride + ks * kTileW);
#pragma unroll
                for (int dy = 0; dy < 3; ++dy) {
                    const _Float16 *zr = zt + (ks + dy) * kZRow;
                    const u32x4 lo1 = *reinterpret_cast<const u32x4 *>(zr), hi1 = *reinterpret_cast<const u32x4 *>(zr + 8);
                    const u32x4 lo2 = *reinterpret_cast<const u32x4 *>(zr + kWgC * kZStride);
                    const u32x4 hi2 = *reinterpret_cast<const u32x4 *>(zr + kWgC * kZStride + 8);
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) {
                        const f16x8 h1 = shifted_halfs(lo1, hi1, dx), h2 = shifted_halfs(lo2, hi2, dx);
                        f32x16 a = acc[dy * 3 + dx];
                        a = __builtin_amdgcn_mfma_f32_32x32x16_f16(h2, g1, a, 0, 0, 0);  // small terms first
                        a = __builtin_amdgcn_mfma_f32_32x32x16_f16(h1, g2, a, 0, 0, 0);
                        a = __builtin_amdgcn_mfma_f32_32x32x16_f16(h1, g1, a, 0, 0, 0);
                        acc[dy * 3 + dx] = a;
                    }
                }
            }
        }
    }
    if (!active) return;
    const float unscale = ldexpf(1.0f, -(ea + eg));
    float *slot = q.slots + (size_t)blockIdx.x * 9 * Cin * Cout;
#pragma unroll
    for (int t9 = 0; t9 < 9; ++t9)
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const int r = (t & 3) + 8 * (t >> 2) + 4 * hh;
            slot[((size_t)t9 * Cin + ci0 + ib * kKC + chunk_channel(r)) * Cout + co0 + cb * kKC + chunk_channel(c)] =
                acc[t9][t] * unscale;
        }
}

// slots [slices][9][Cin][Cout] -> gw [Cout][Cin][3][3], the slices added in ascending order
__global__ __launch_bounds__(256) void wgrad_finish_kernel(const float *__restrict__ slots, int slices, int cin, int cout,
                                                           float *__restrict__ gw) {
    const long long n = (long long)9 * cin * cout, i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float s = 0.f;
    for (int k = 0; k < slices; ++k) s += slots[(size_t)k * n + i];
    const int co = (int)(i % cout), ci = (int)(i / cout % cin), tap = (int)(i / cout / cin);
    gw[((size_t)co * cin + ci) * 9 + tap] = s;
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
        weights, out_scale, cin, cout, 0, items, hdr, reinterpret_cast<_Float16 *>(static_cast<char *>(out) + kSplitHeader));
    return check_launch("amav_conv3x3_prepare_weights_split");
}

// conv3x3_cells_kernel by the width of Cout; p.gate selects the gated operand
template <bool GATE>
static void launch_conv_nt(const upconv::Params &p, long long blocks, hipStream_t stream) {
    const int nt = p.Cout % 128 == 0 ? 128 : (p.Cout % 64 == 0 ? 64 : 32);
    const dim3 grid((unsigned)blocks, (unsigned)(p.Cout / nt));
    if (nt == 128)
        upconv::conv3x3_cells_kernel<128, GATE><<<grid, 256, 0, stream>>>(p);
    else if (nt == 64)
        upconv::conv3x3_cells_kernel<64, GATE><<<grid, 256, 0, stream>>>(p);
    else
        upconv::conv3x3_cells_kernel<32, GATE><<<grid, 256, 0, stream>>>(p);
}

static void launch_conv(const upconv::Params &p, long long blocks, hipStream_t stream) {
    if (p.gate)
        launch_conv_nt<true>(p, blocks, stream);
    else
        launch_conv_nt<false>(p, blocks, stream);
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
        reinterpret_cast<const float4 *>(a->in_shift_dev), nullptr, amax);
    upconv::Params p;
    p.x = a->x_dev, p.wsplit = a->weights_split_dev, p.amax = amax;
    p.in_scale = a->in_scale_dev, p.in_shift = a->in_shift_dev, p.bias = a->bias_dev, p.residual = a->residual_dev;
    p.gate = nullptr;
    p.origin = a->origin_dev, p.out = a->out_dev;
    p.H = H, p.W = W, p.Cin = cin, p.Cout = cout, p.extent = a->extent, p.upsample = a->upsample_input != 0;
    p.relu_out = a->relu_out != 0, p.tiles_x = tiles_x, p.tiles_per_cell = tiles_x * tiles_y;
    launch_conv(p, blocks, stream);
    return check_launch("amav_conv3x3_cells");
}

extern "C" int amav_conv3x3_prepare_weights_split_transposed(int cin, int cout, const float *weights, void *out, size_t out_bytes,
                                                             void *stream_) {
    AMAV_REQUIRE(conv3x3_sizes_ok(cin, cout),
                 "amav_conv3x3_prepare_weights_split_transposed: channels must be multiples of 32 (C_in %d, C_out %d)", cin, cout);
    AMAV_REQUIRE(weights && out && (reinterpret_cast<uintptr_t>(out) & 255) == 0,
                 "amav_conv3x3_prepare_weights_split_transposed: NULL / misaligned pointer (out: 256 bytes)");
    if (out_bytes < conv3x3_split_bytes(cout, cin))
        return fail(AMAV_ERR_WORKSPACE, "amav_conv3x3_prepare_weights_split_transposed: buffer %zu < required %zu", out_bytes,
                    conv3x3_split_bytes(cout, cin));
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    unsigned *hdr = static_cast<unsigned *>(out);
    AMAV_REQUIRE(zero_async(hdr, kSplitHeader, stream) == hipSuccess,
                 "amav_conv3x3_prepare_weights_split_transposed: header clear failed");
    const long long n = (long long)9 * cin * cout;
    upconv::weights_absmax_kernel<<<(unsigned)std::min<long long>((n + 255) / 256, 256), 256, 0, stream>>>(weights, n, 9 * cin,
                                                                                                            nullptr, hdr);
    // the data gradient contracts over the forward's output channels and produces its input channels
    const long long items = (long long)9 * (cin / 32) * (cout / 16) * 64;
    upconv::weights_split_kernel<<<blocks_for(items), 256, 0, stream>>>(
        weights, nullptr, cout, cin, 1, items, hdr, reinterpret_cast<_Float16 *>(static_cast<char *>(out) + kSplitHeader));
    return check_launch("amav_conv3x3_prepare_weights_split_transposed");
}

namespace {

constexpr int kMaxSlices = 4096;
constexpr size_t kSlotBudget = (size_t)64 << 20;

struct BackwardPlan {
    int tiles_x, tiles_y, slices, col_blocks_out, col_blocks_in;
    long long pairs, rows_out, rows_in;
    bool need_gz, gz_is_grad_x, need_data;
    unsigned *amax;
    float *gz, *bias_partial, *operand_partial, *slots;
    size_t bytes;
};

// Validates everything but the workspace and lays the workspace out; `base` NULL only measures.
int plan_backward(const amav_conv3x3_backward_args *a, int slices, void *base, BackwardPlan &pl) {
    const char *who = "amav_conv3x3_cells_backward";
    AMAV_REQUIRE(a != nullptr, "%s: args is NULL", who);
    const int H = a->height, W = a->width, cin = a->cin, cout = a->cout;
    AMAV_REQUIRE(a->cells > 0 && H > 0 && W > 0, "%s: bad sizes cells=%lld H=%d W=%d", who, (long long)a->cells, H, W);
    AMAV_REQUIRE(conv3x3_sizes_ok(cin, cout), "%s: channels must be multiples of 32 (C_in %d, C_out %d)", who, cin, cout);
    AMAV_REQUIRE(!a->upsample_input || (H % 2 == 0 && W % 2 == 0), "%s: upsample_input needs even H and W (H=%d W=%d)", who, H, W);
    AMAV_REQUIRE(a->x_dev && a->grad_out_dev, "%s: NULL pointer (x, grad_out)", who);
    AMAV_REQUIRE(!a->relu_out || a->out_dev, "%s: relu_out needs the forward's out", who);
    AMAV_REQUIRE(!a->in_scale_dev == !a->in_shift_dev, "%s: in_scale and in_shift come together", who);
    AMAV_REQUIRE(!a->grad_in_scale_dev == !a->grad_in_shift_dev, "%s: grad_in_scale and grad_in_shift come together", who);
    AMAV_REQUIRE(!a->grad_in_scale_dev || a->in_scale_dev, "%s: grad_in_scale without a prologue", who);
    AMAV_REQUIRE(!a->origin_dev || a->extent > 0, "%s: origin needs a positive extent, got %d", who, a->extent);
    AMAV_REQUIRE(a->grad_x_dev || a->grad_weight_dev || a->grad_bias_dev || a->grad_in_scale_dev, "%s: no gradient asked for", who);
    AMAV_REQUIRE(aligned16(a->x_dev, a->in_scale_dev, a->in_shift_dev, a->out_dev, a->grad_out_dev) &&
                     aligned16(a->grad_x_dev, a->grad_bias_dev, a->grad_in_scale_dev, a->grad_in_shift_dev, a->grad_weight_dev),
                 "%s: x, in_scale, in_shift, out, grad_out and the gradients must be 16-byte aligned", who);
    AMAV_REQUIRE(slices >= 0 && slices <= kMaxSlices, "%s: wgrad_slices %d outside [0, %d]", who, slices, kMaxSlices);
    pl.tiles_x = (W + upconv::kTileW - 1) / upconv::kTileW, pl.tiles_y = (H + upconv::kTileH - 1) / upconv::kTileH;
    pl.pairs = a->cells * pl.tiles_x * pl.tiles_y;
    AMAV_REQUIRE(pl.pairs <= INT_MAX, "%s: %lld tiles exceed the grid", who, pl.pairs);
    pl.need_data = a->grad_x_dev || a->grad_in_scale_dev;
    if (pl.need_data) {
        AMAV_REQUIRE(a->weights_split_t_dev && aligned16(a->weights_split_t_dev), "%s: NULL / misaligned weights_split_t", who);
        if (a->weights_split_t_bytes < conv3x3_split_bytes(cout, cin))
            return fail(AMAV_ERR_WORKSPACE, "%s: weights_split_t %zu < required %zu", who, a->weights_split_t_bytes,
                        conv3x3_split_bytes(cout, cin));
    }
    const int f = a->upsample_input ? 2 : 1;
    pl.rows_out = a->cells * H * W, pl.rows_in = a->cells * (H / f) * (W / f);
    // the data gradient IS grad_x when the operand is x itself
    pl.gz_is_grad_x = pl.need_data && !a->in_scale_dev && !a->origin_dev && !a->upsample_input;
    pl.need_gz = pl.need_data && !pl.gz_is_grad_x;
    if (slices == 0) {  // fill the CUs (one workgroup each), within the slot budget
        const int per_slice = ((cout + 63) / 64) * ((cin + 63) / 64);
        slices = std::max(1, 256 / per_slice);
        slices = (int)std::min<size_t>((size_t)slices, std::max<size_t>(1, kSlotBudget / ((size_t)9 * cin * cout * sizeof(float))));
        slices = (int)std::min<long long>(slices, pl.pairs);
    }
    pl.slices = slices;
    pl.col_blocks_out = (int)std::min<long long>(upconv::kColBlocks, (pl.rows_out + 31) / 32);
    pl.col_blocks_in = (int)std::min<long long>(upconv::kColBlocks, (pl.rows_in + 31) / 32);
    Carver carve(base);
    pl.amax = carve.take<unsigned>(64);
    pl.gz = pl.need_gz ? carve.take<float>((size_t)pl.rows_out * cin) : nullptr;
    pl.bias_partial = a->grad_bias_dev ? carve.take<float>((size_t)pl.col_blocks_out * cout) : nullptr;
    pl.operand_partial = a->grad_in_scale_dev ? carve.take<float>((size_t)pl.col_blocks_in * 2 * cin) : nullptr;
    pl.slots = a->grad_weight_dev ? carve.take<float>((size_t)slices * 9 * cin * cout) : nullptr;
    pl.bytes = carve.total();
    return AMAV_OK;
}

}  // namespace

extern "C" size_t amav_conv3x3_backward_workspace_bytes(const amav_conv3x3_backward_args *a, int wgrad_slices) {
    BackwardPlan pl;
    return plan_backward(a, wgrad_slices, nullptr, pl) == AMAV_OK ? pl.bytes : 0;
}

extern "C" int amav_conv3x3_cells_backward(const amav_conv3x3_backward_args *a, void *stream_) {
    BackwardPlan pl;
    if (int rc = plan_backward(a, a ? a->wgrad_slices : 0, a ? a->workspace_dev : nullptr, pl)) return rc;
    if (!a->workspace_dev || a->workspace_bytes < pl.bytes || (reinterpret_cast<uintptr_t>(a->workspace_dev) & 255))
        return fail(AMAV_ERR_WORKSPACE, "amav_conv3x3_cells_backward: workspace %zu < required %zu (or NULL / not 256-byte aligned)",
                    a->workspace_bytes, pl.bytes);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int H = a->height, W = a->width, cin = a->cin, cout = a->cout;
    const float *gate = a->relu_out ? a->out_dev : nullptr;
    unsigned *amax_x = pl.amax, *amax_g = pl.amax + 4;
    AMAV_REQUIRE(zero_async(pl.amax, 32, stream) == hipSuccess, "amav_conv3x3_cells_backward: workspace clear failed");

    if (a->grad_bias_dev) {
        upconv::bias_partial_kernel<<<pl.col_blocks_out, 256, 0, stream>>>(a->grad_out_dev, gate, pl.rows_out, cout, pl.bias_partial);
        upconv::column_finish_kernel<<<(cout + 255) / 256, 256, 0, stream>>>(pl.bias_partial, pl.col_blocks_out, cout, cout, a->grad_bias_dev);
    }
    if (pl.need_data || a->grad_weight_dev) {  // the gated gradient's exponent, for both GEMMs
        const long long n4 = pl.rows_out * (cout / 4);
        upconv::operand_absmax_kernel<<<(unsigned)std::min<long long>((n4 + 255) / 256, 1024), 256, 0, stream>>>(
            reinterpret_cast<const float4 *>(a->grad_out_dev), n4, cout / 4, nullptr, nullptr,
            reinterpret_cast<const float4 *>(gate), amax_g);
    }
    upconv::Params z;  // the forward's operand
    z.x = a->x_dev, z.wsplit = nullptr, z.amax = amax_x;
    z.in_scale = a->in_scale_dev, z.in_shift = a->in_shift_dev, z.bias = nullptr, z.residual = nullptr, z.gate = nullptr;
    z.origin = a->origin_dev, z.out = nullptr;
    z.H = H, z.W = W, z.Cin = cin, z.Cout = cout, z.extent = a->extent, z.upsample = a->upsample_input != 0;
    z.relu_out = 0, z.tiles_x = pl.tiles_x, z.tiles_per_cell = pl.tiles_x * pl.tiles_y;
    if (pl.need_data) {
        upconv::Params p = z;  // the same kernel on ga: channel counts swapped, the cell's own padding only
        p.x = a->grad_out_dev, p.gate = gate, p.wsplit = a->weights_split_t_dev, p.amax = amax_g;
        p.in_scale = p.in_shift = nullptr, p.origin = nullptr, p.upsample = 0;
        p.Cin = cout, p.Cout = cin, p.out = pl.gz_is_grad_x ? a->grad_x_dev : pl.gz;
        launch_conv(p, pl.pairs, stream);
        if (pl.need_gz)
            upconv::operand_backward_kernel<<<pl.col_blocks_in, 256, 0, stream>>>(z, pl.gz, pl.rows_in, a->grad_x_dev,
                                                                                  pl.operand_partial);
        if (a->grad_in_scale_dev) {
            upconv::column_finish_kernel<<<(cin + 255) / 256, 256, 0, stream>>>(pl.operand_partial, pl.col_blocks_in, 2 * cin, cin,
                                                                               a->grad_in_scale_dev);
            upconv::column_finish_kernel<<<(cin + 255) / 256, 256, 0, stream>>>(pl.operand_partial + cin, pl.col_blocks_in, 2 * cin,
                                                                               cin, a->grad_in_shift_dev);
        }
    }
    if (a->grad_weight_dev) {
        const long long n4 = pl.rows_in * (cin / 4);  // the forward's own sweep of its operand
        upconv::operand_absmax_kernel<<<(unsigned)std::min<long long>((n4 + 255) / 256, 1024), 256, 0, stream>>>(
            reinterpret_cast<const float4 *>(a->x_dev), n4, cin / 4, reinterpret_cast<const float4 *>(a->in_scale_dev),
            reinterpret_cast<const float4 *>(a->in_shift_dev), nullptr, amax_x);
        static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void *>(&upconv::conv3x3_wgrad_kernel),
                                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)upconv::kWgradLds);
        if (attr != hipSuccess) return fail(AMAV_ERR_LAUNCH, "amav_conv3x3_cells_backward: cannot raise the dynamic LDS limit");
        upconv::WgradParams q;
        q.z = z, q.g = a->grad_out_dev, q.gate = gate, q.amax_g = amax_g, q.slots = pl.slots, q.pairs = pl.pairs, q.Cout = cout;
        const dim3 grid((unsigned)pl.slices, (unsigned)((cout + 63) / 64), (unsigned)((cin + 63) / 64));
        upconv::conv3x3_wgrad_kernel<<<grid, 256, upconv::kWgradLds, stream>>>(q);
        const long long n = (long long)9 * cin * cout;
        upconv::wgrad_finish_kernel<<<blocks_for(n), 256, 0, stream>>>(pl.slots, pl.slices, cin, cout, a->grad_weight_dev);
    }
    return check_launch("amav_conv3x3_cells_backward");
}
