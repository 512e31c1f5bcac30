// Triplane feature sampling, backward, for gfx950: gradients of amav_triplane_sample_features (triplane.hip,
// Renderer.sample_from_triplane = three bilinear grid_samples, align_corners=False, zero padding, of clamp(p / radius))
// with respect to the planes and the points, given grad_out [F,N,3C].  One pair of kernels serves every C (the
// forward's two kernels compute the same bits, so there is one function to differentiate).  No float atomics, no host
// synchronisation, one workspace.
//
//   grad_planes   The transpose of the sampling is a scatter of N rows of C floats onto <= 4 texels each.  It is
//                 turned into a gather by ORDERING the frame's points by the texel of their first tap:
//     bin_kernel      one workgroup per (frame, plane): a stable counting sort of the points by base cell (ix0, iy0)
//                     in [-1, R-1]^2 -- per-wave histograms of contiguous point segments (integer atomics: counts do
//                     not depend on their order), one exclusive scan over (cell, wave), then every wave places its
//                     segment in point order (rank among the equal keys of the lower lanes).  Output: per (frame,
//                     plane) the point ids and their four tap weights in cell-then-point order, and the cells' starts.
//     texel_kernel    one wave per (frame, plane, 4 x 4 texel tile, 64 channels), lanes along the channels: walks
//                     the 5 x 5 base cells whose taps reach the tile, row by row, and each cell's points in order; a
//                     cell's four texels are the same for all its points, so their sums stay in registers over the
//                     cell (taps outside the tile go to a spare row).  Every point's 256-byte row of grad_out is read
//                     by the tiles its taps touch (1.56 x on average).  The [texel][channel] tile is written with
//                     lanes along x; every texel of the plane is written, exact zeros where no tap lands.
//                 A texel's sum therefore runs over its four cells (rows, then columns), points ascending inside a
//                 cell: a function of that frame's points alone.
//   grad_points   point_kernel: a block is 64 points, lanes along the POINTS.  Per plane and per 64 channels the
//                 block's [64 points][64 channels] piece of grad_out is read with lanes along the channels and
//                 transposed through LDS; then wave w takes channels w, w + 4, ... one channel image at a time (the
//                 forward-tiled kernel's read pattern) and adds g * texel value per tap, channels ascending.  The four
//                 waves' partials are summed in wave order.  Bilinear-weight derivative as torch's
//                 grid_sampler_2d_backward (out-of-plane taps count with value 0), * R / 2, through the clamp (gradient
//                 where -1 <= p / radius <= 1), / radius; each coordinate collects from its two planes.
#include <cstddef>

#include "amav_common.h"
#include "sample_taps.h"
#include "wave_ops.h"

namespace amav {
namespace sample_bwd {

using triplane::make_taps;
using triplane::sample_unit;
using triplane::Taps;

constexpr int kBinWaves = 8;               // waves of a bin_kernel workgroup (one point segment each)
constexpr int kBinLdsBytes = 64 * 1024;    // histograms in LDS when (kBinWaves + 1) * cells ints fit, else in the workspace
constexpr int kTile = 4;                   // texel_kernel: tile edge in texels
constexpr int kTileRow = 65;               // LDS row of one texel: 64 channels + pad
constexpr int kSpare = kTile * kTile;      // LDS row that takes the taps outside the tile

__device__ __forceinline__ int cells_of(int R) { return (R + 1) * (R + 1); }

// The taps of point n of frame f on `plane`: base cell, and the four weights (dy, dx) as the forward forms them.
__device__ __forceinline__ int point_cell(const float *__restrict__ pp, int plane, float radius, int R, float4 &w) {
    const float u0 = sample_unit(pp[0], radius), u1 = sample_unit(pp[1], radius), u2 = sample_unit(pp[2], radius);
    const Taps t = make_taps(plane == 2 ? u1 : u0, plane == 0 ? u1 : u2, R);
    w = make_float4(t.wx0 * t.wy0, t.wx1 * t.wy0, t.wx0 * t.wy1, t.wx1 * t.wy1);
    const int bx = min(max(t.ix0, -1), R - 1), by = min(max(t.iy0, -1), R - 1);  // always inside: |u| <= 1
    return (by + 1) * (R + 1) + bx + 1;
}

// grid (3, F), kBinWaves * 64 threads.  hist_global: NULL = the histograms live in dynamic LDS.
__global__ __launch_bounds__(kBinWaves * 64) void bin_kernel(int N, int R, const float *__restrict__ points, float radius,
                                                            int *__restrict__ ids, float4 *__restrict__ wts,
                                                            int *__restrict__ cell_start, int *__restrict__ hist_global) {
    extern __shared__ __align__(16) int bin_lds[];
    const int plane = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63, cells = cells_of(R);
    const size_t fp = (size_t)f * 3 + plane;
    int *hist = hist_global ? hist_global + fp * (kBinWaves + 1) * cells : bin_lds;  // [wave][cell]
    int *tot = hist + kBinWaves * cells;                                             // [cell]
    for (int i = tid; i < kBinWaves * cells; i += blockDim.x) hist[i] = 0;
    __syncthreads();
    const int seg = (((N + kBinWaves - 1) / kBinWaves) + 63) & ~63;
    const int n_begin = min(wave * seg, N), n_end = min(n_begin + seg, N);
    const float *fpts = points + (size_t)f * N * 3;
    int *my_hist = hist + wave * cells;
    for (int n0 = n_begin; n0 < n_end; n0 += 64) {
        const int n = n0 + lane;
        if (n < n_end) {
            float4 w;
            atomicAdd(&my_hist[point_cell(fpts + (size_t)n * 3, plane, radius, R, w)], 1);
        }
    }
    __syncthreads();
    for (int c = tid; c < cells; c += blockDim.x) {
        int s = 0;
        for (int w = 0; w < kBinWaves; ++w) s += hist[w * cells + c];
        tot[c] = s;
    }
    __syncthreads();
    if (wave == 0) {  // exclusive scan of the cell totals, 64 cells at a time
        int run = 0;
        for (int c0 = 0; c0 < cells; c0 += 64) {
            const int c = c0 + lane, v = c < cells ? tot[c] : 0;
            const int incl = wave_inclusive_sum(v, lane);
            if (c < cells) tot[c] = run + incl - v;
            run += __shfl(incl, 63, 64);
        }
    }
    __syncthreads();
    int *cs = cell_start + fp * (cells + 1);
    for (int c = tid; c < cells; c += blockDim.x) {
        int run = tot[c];
        cs[c] = run;
        for (int w = 0; w < kBinWaves; ++w) {  // -> where wave w's first point of cell c goes
            const int t = hist[w * cells + c];
            hist[w * cells + c] = run;
            run += t;
        }
    }
    if (tid == 0) cs[cells] = N;
    __syncthreads();
    int *out_ids = ids + fp * N;
    float4 *out_w = wts + fp * N;
    for (int n0 = n_begin; n0 < n_end; n0 += 64) {
        const int n = n0 + lane;
        const bool valid = n < n_end;
        float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
        const int key = valid ? point_cell(fpts + (size_t)n * 3, plane, radius, R, w) : -1;
        int rank = 0, cnt = 0;  // equal keys in the lower lanes / in the wave
#pragma unroll
        for (int j = 0; j < 64; ++j) {
            const int kj = __builtin_amdgcn_readlane(key, j);
            rank += (kj == key && j < lane) ? 1 : 0;
            cnt += kj == key ? 1 : 0;
        }
        if (valid) {
            const int base = my_hist[key];  // every lane reads before the key's last lane moves the cursor on
            out_ids[base + rank] = n;
            out_w[base + rank] = w;
            if (rank == cnt - 1) my_hist[key] = base + cnt;
        }
    }
}

// grid (tiles, 3 * ceil(C / 64), F), one wave.  The output strides address element (f, plane, c, y, x) at
// f * fs + plane * ps + c * cs + y * R + x.
__global__ __launch_bounds__(64) void texel_kernel(int N, int C, int R, const int *__restrict__ ids,
                                                   const float4 *__restrict__ wts, const int *__restrict__ cell_start,
                                                   const float *__restrict__ gout, float *__restrict__ gplanes,
                                                   long long fs, long long ps, long long cs) {
    __shared__ float tile[(kTile * kTile + 1) * kTileRow];  // [texel | spare][channel]
    const int lane = threadIdx.x, f = blockIdx.z;
    const int chunks = (C + 63) >> 6, plane = blockIdx.y / chunks, c0 = (blockIdx.y - plane * chunks) * 64;
    const int tiles_x = (R + kTile - 1) / kTile;
    const int tx0 = (blockIdx.x % tiles_x) * kTile, ty0 = (blockIdx.x / tiles_x) * kTile;
    const int cw = R + 1, cells = cw * cw;
    const size_t fp = (size_t)f * 3 + plane;
    const int *cst = cell_start + fp * (cells + 1);
    const int *pid = ids + fp * N;
    const float4 *pw = wts + fp * N;
    const size_t row = (size_t)3 * C;
    // lanes past C read the chunk's first channel and are not written
    const float *g0 = gout + (size_t)f * N * row + (size_t)plane * C + (c0 + lane < C ? c0 + lane : c0);
    for (int i = lane; i < (kTile * kTile + 1) * kTileRow; i += 64) tile[i] = 0.0f;
    __syncthreads();
    // base cell (bx, by) has taps on texels (bx + dx, by + dy); the tile is reached from bx in [tx0 - 1, tx0 + kTile - 1]
    for (int cy = 0; cy <= kTile; ++cy) {
        const int by = ty0 - 1 + cy;
        if (by > R - 1) break;
        for (int cx = 0; cx <= kTile; ++cx) {
            const int bx = tx0 - 1 + cx;
            if (bx > R - 1) break;
            const int cell = (by + 1) * cw + bx + 1;
            const int s0 = cst[cell], s1 = cst[cell + 1];
            if (s0 == s1) continue;
            int slot[4];  // LDS row of tap (dy, dx)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int lx = cx - 1 + (k & 1), ly = cy - 1 + (k >> 1);
                slot[k] = (lx >= 0 && lx < kTile && ly >= 0 && ly < kTile ? ly * kTile + lx : kSpare) * kTileRow + lane;
            }
            float a0 = tile[slot[0]], a1 = tile[slot[1]], a2 = tile[slot[2]], a3 = tile[slot[3]];
#pragma unroll 4
            for (int s = s0; s < s1; ++s) {
                const float4 w = pw[s];
                const float g = g0[(size_t)pid[s] * row];
                a0 = fmaf(w.x, g, a0), a1 = fmaf(w.y, g, a1), a2 = fmaf(w.z, g, a2), a3 = fmaf(w.w, g, a3);
            }
            // the spare row may be named by several taps: whatever lands there is never read back as a texel
            tile[slot[0]] = a0, tile[slot[1]] = a1, tile[slot[2]] = a2, tile[slot[3]] = a3;
        }
    }
    __syncthreads();
    // lanes along x: lane = (channel % 4, y, x); 16 trips cover the 64 channels
    const int lx = lane & (kTile - 1), ly = (lane >> 2) & (kTile - 1), x = tx0 + lx, y = ty0 + ly;
    if (x < R && y < R) {
        float *dst = gplanes + (size_t)f * fs + (size_t)plane * ps + (size_t)y * R + x;
        for (int cc = lane >> 4; cc < 64 && c0 + cc < C; cc += 4)
            dst[(size_t)(c0 + cc) * cs] = tile[(ly * kTile + lx) * kTileRow + cc];
    }
}

// grid (ceil(N / 64), F), 256 threads.
__global__ __launch_bounds__(256) void point_kernel(int N, int C, int R, const float *__restrict__ planes, long long fs,
                                                    long long ps, long long cs, const float *__restrict__ points,
                                                    float radius, const float *__restrict__ gout,
                                                    float *__restrict__ gpoints) {
    __shared__ float tile[64 * 65];      // [channel][point]
    __shared__ float part[4][6][64];     // [wave][plane: d/dx, d/dy][point]
    const int f = blockIdx.y, n0 = blockIdx.x * 64;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n = min(n0 + lane, N - 1);
    const float *pp = points + ((size_t)f * N + n) * 3;
    const float p[3] = {pp[0], pp[1], pp[2]};
    const float u0 = sample_unit(p[0], radius), u1 = sample_unit(p[1], radius), u2 = sample_unit(p[2], radius);
    const size_t row = (size_t)3 * C;
    const float *gf = gout + (size_t)f * N * row;
#pragma unroll 1
    for (int plane = 0; plane < 3; ++plane) {
        const Taps t = make_taps(plane == 2 ? u1 : u0, plane == 0 ? u1 : u2, R);
        int off[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int ix = t.ix0 + (k & 1), iy = t.iy0 + (k >> 1);
            off[k] = ix >= 0 && ix < R && iy >= 0 && iy < R ? iy * R + ix : -1;
        }
        float vt[4] = {0.f, 0.f, 0.f, 0.f};  // sum over channels of g * texel value, per tap
        const float *pl = planes + (size_t)f * fs + (size_t)plane * ps;
        for (int c0 = 0; c0 < C; c0 += 64) {
            __syncthreads();
            const bool chan = c0 + lane < C;
#pragma unroll 4
            for (int q = wave; q < 64; q += 4)
                tile[lane * 65 + q] = chan && n0 + q < N ? gf[(size_t)(n0 + q) * row + (size_t)plane * C + c0 + lane] : 0.0f;
            __syncthreads();
            const int kend = min(64, C - c0);
#pragma unroll 4
            for (int k = wave; k < kend; k += 4) {
                const float *img = pl + (size_t)(c0 + k) * cs;
                const float g = tile[k * 65 + lane];
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (off[q] >= 0) vt[q] = fmaf(img[off[q]], g, vt[q]);
            }
        }
        // d/d(pixel x) = sum over taps of +-(value * other axis' weight); out-of-plane taps hold vt = 0
        const float sx = ((vt[1] * t.wy0 - vt[0] * t.wy0) + vt[3] * t.wy1) - vt[2] * t.wy1;
        const float sy = ((vt[2] * t.wx0 - vt[0] * t.wx0) + vt[3] * t.wx1) - vt[1] * t.wx1;
        part[wave][plane * 2][lane] = sx, part[wave][plane * 2 + 1][lane] = sy;
    }
    __syncthreads();
    if (wave == 0 && n0 + lane < N) {
        float s[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) s[i] = ((part[0][i][lane] + part[1][i][lane]) + part[2][i][lane]) + part[3][i][lane];
        const float half = 0.5f * (float)R;
        // plane 0 samples (u0, u1), plane 1 (u0, u2), plane 2 (u1, u2)
        const float du[3] = {s[0] * half + s[2] * half, s[1] * half + s[4] * half, s[3] * half + s[5] * half};
        float *o = gpoints + ((size_t)f * N + n) * 3;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const float q = p[i] / radius;
            o[i] = (q >= -1.0f && q <= 1.0f) ? du[i] / radius : 0.0f;
        }
    }
}

struct Scratch {
    int *ids, *cell_start, *hist;
    float4 *wts;
    size_t bytes;
};
inline bool hist_in_lds(int R) { return (size_t)(kBinWaves + 1) * (R + 1) * (R + 1) * sizeof(int) <= kBinLdsBytes; }
inline Scratch carve(void *base, int F, int N, int R) {
    Carver cv(base);
    Scratch s;
    const size_t cells = (size_t)(R + 1) * (R + 1);
    s.wts = cv.take<float4>((size_t)F * 3 * N);
    s.ids = cv.take<int>((size_t)F * 3 * N);
    s.cell_start = cv.take<int>((size_t)F * 3 * (cells + 1));
    s.hist = hist_in_lds(R) ? nullptr : cv.take<int>((size_t)F * 3 * (kBinWaves + 1) * cells);
    s.bytes = cv.total();
    return s;
}

}  // namespace sample_bwd
}  // namespace amav

using namespace amav;
using namespace amav::sample_bwd;

extern "C" size_t amav_triplane_sample_features_backward_bytes(int F, int N, int C, int R) {
    if (F <= 0 || N <= 0 || C <= 0 || R <= 0) return 0;
    return carve(nullptr, F, N, R).bytes;
}

extern "C" int amav_triplane_sample_features_backward(const amav_triplane_sample_backward_args *a, void *stream_) {
    AMAV_REQUIRE(a != nullptr, "amav_triplane_sample_features_backward: args is NULL");
    const int F = a->num_frames, N = a->num_points, C = a->channels, R = a->resolution;
    AMAV_REQUIRE(F > 0 && N > 0 && C > 0 && R > 0, "amav_triplane_sample_features_backward: bad sizes F=%d N=%d C=%d R=%d",
                 F, N, C, R);
    AMAV_REQUIRE(F <= 65535, "amav_triplane_sample_features_backward: F=%d exceeds grid.z", F);
    AMAV_REQUIRE(R <= 4096 && (size_t)3 * ((C + 63) / 64) <= 65535,
                 "amav_triplane_sample_features_backward: R=%d or C=%d too large for the grid", R, C);
    AMAV_REQUIRE(a->radius > 0.0f, "amav_triplane_sample_features_backward: radius must be positive");
    AMAV_REQUIRE(a->points && a->grad_out, "amav_triplane_sample_features_backward: NULL pointer (points / grad_out)");
    AMAV_REQUIRE(a->grad_planes || a->grad_points,
                 "amav_triplane_sample_features_backward: NULL pointer (neither grad_planes nor grad_points is wanted)");
    AMAV_REQUIRE(!a->grad_points || a->planes,
                 "amav_triplane_sample_features_backward: NULL pointer (grad_points needs the planes)");
    const int64_t RR = (int64_t)R * R;
    AMAV_REQUIRE(!a->grad_points || (a->planes_frame_stride >= 0 && a->planes_plane_stride >= 0 && a->planes_chan_stride >= 0),
                 "amav_triplane_sample_features_backward: negative planes stride");
    AMAV_REQUIRE(!a->grad_planes || (a->grad_plane_stride >= RR && a->grad_chan_stride >= RR &&
                                     a->grad_frame_stride >= 3 * (int64_t)C * RR),
                 "amav_triplane_sample_features_backward: grad_planes strides (%lld, %lld, %lld) overlap for C=%d R=%d",
                 (long long)a->grad_frame_stride, (long long)a->grad_plane_stride, (long long)a->grad_chan_stride, C, R);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (a->grad_planes) {
        AMAV_REQUIRE(a->scratch != nullptr, "amav_triplane_sample_features_backward: scratch is NULL");
        AMAV_REQUIRE((reinterpret_cast<uintptr_t>(a->scratch) & 15) == 0,
                     "amav_triplane_sample_features_backward: scratch not 16-B aligned");
        const Scratch s = carve(a->scratch, F, N, R);
        if (a->scratch_bytes < s.bytes)
            return fail(AMAV_ERR_WORKSPACE, "amav_triplane_sample_features_backward: scratch %zu < required %zu",
                        a->scratch_bytes, s.bytes);
        const size_t lds = s.hist ? 0 : (size_t)(kBinWaves + 1) * (R + 1) * (R + 1) * sizeof(int);
        bin_kernel<<<dim3(3, F), kBinWaves * 64, lds, stream>>>(N, R, a->points, a->radius, s.ids, s.wts, s.cell_start, s.hist);
        int rc = check_launch("amav_triplane_sample_features_backward: bin_kernel");
        if (rc) return rc;
        const int tiles_x = (R + kTile - 1) / kTile;
        texel_kernel<<<dim3((unsigned)(tiles_x * tiles_x), (unsigned)(3 * ((C + 63) / 64)), F), 64, 0, stream>>>(
            N, C, R, s.ids, s.wts, s.cell_start, a->grad_out, a->grad_planes, a->grad_frame_stride, a->grad_plane_stride,
            a->grad_chan_stride);
        if ((rc = check_launch("amav_triplane_sample_features_backward: texel_kernel"))) return rc;
    }
    if (a->grad_points) {
        point_kernel<<<dim3((unsigned)((N + 63) / 64), F), 256, 0, stream>>>(
            N, C, R, a->planes, a->planes_frame_stride, a->planes_plane_stride, a->planes_chan_stride, a->points, a->radius,
            a->grad_out, a->grad_points);
        return check_launch("amav_triplane_sample_features_backward: point_kernel");
    }
    return AMAV_OK;
}
