// Backwards of the stage-1 encoder's reductions (splat.hip), for training TriplaneGaussianAvatar (the reference's
// lightning_model_wrapper.py:82-170).  No float atomics: every output element is written by exactly one thread and
// every sum runs in a fixed order, so the gradients are reproducible bit for bit and independent of how frames are
// batched (every frame is its own grid slice).
//
//   amav_cell_max_backward   pool_local (scatter_max + gather + sum over planes):
//                            dfeat[n][c] = sum over planes p (in order 0, 1, 2) of [n == arg_p(cell_p(n), c)] * S_p,
//                            S_p(cell, c) = sum of dout[m][c] over the cell's points m in ascending point id, arg = the
//                            point that holds the maximum, the LOWEST point id among ties (a sequential scan with a
//                            strict >; torch_scatter's scatter_max backward routes the whole gradient to one point)
//   amav_cell_mean_backward  generate_plane_features (scatter_mean): dfeat[n][c] = dplane[c][cell(n)] / count(cell(n))
//   amav_points_project_backward  points_projection's index_put, w.r.t. the features: every pixel a point wins takes
//                            that point's output row, dfeat[c][y][x] = dout[winner(y, x)][c], 0 where no point won
//                            (the forward keeps only the last won pixel, but index_put's backward credits them all)
//   amav_points_project_grid_backward  the same credit carried on through the bilinear resize into the grid, without
//                            the image-sized gradient: dgrid[j][i][c] = sum over the won pixels that have node (j, i) as
//                            a corner of weight * dout[winner][3 + c], in ascending pixel index, corners 00 01 10 11
#include "amav_common.h"
#include "grid_bilinear.h"

namespace amav {
namespace splat_bwd {

using splat::grid_axis;
using splat::grid_axis_first_pixel;
using splat::GridAxis;

// pool_local, pass 1: one block per (cell, plane, b); thread = channel (strided).  Walks the cell's run of `order` once:
// arg = first point of the maximum (strict >), S = sum of dout over the run in ascending point id.  Tables [B,3,cells,C].
__global__ __launch_bounds__(256) void cell_max_route_kernel(int N, int C, int cells, const float *__restrict__ feat,
                                                             const int *__restrict__ order, const int *__restrict__ seg,
                                                             const float *__restrict__ dout, int *__restrict__ arg_tab,
                                                             float *__restrict__ sum_tab) {
    const int cell = blockIdx.x, plane = blockIdx.y, b = blockIdx.z;
    const size_t pb = (size_t)b * 3 + plane;
    const int *sg = seg + pb * (cells + 1);
    const int beg = sg[cell], end = sg[cell + 1];
    const int *ord = order + pb * N;
    const float *fb = feat + (size_t)b * N * C, *gb = dout + (size_t)b * N * C;
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        int arg = -1;
        float m = 0.0f, s = 0.0f;
        for (int k = beg; k < end; ++k) {
            const int n = ord[k];
            if ((unsigned)n >= (unsigned)N) continue;  // not a point id: order is not this forward's
            const float v = fb[(size_t)n * C + c];
            if (arg < 0 || v > m) m = v, arg = n;
            s += gb[(size_t)n * C + c];
        }
        arg_tab[(pb * cells + cell) * C + c] = arg;
        sum_tab[(pb * cells + cell) * C + c] = s;
    }
}

// pool_local, pass 2: one wave per (point, b): dfeat = (v0 + v1) + v2, v_p = S_p where the point holds plane p's maximum
__global__ __launch_bounds__(256) void cell_max_scatter_kernel(int N, int C, int cells, const int *__restrict__ cell_of,
                                                               const int *__restrict__ arg_tab,
                                                               const float *__restrict__ sum_tab,
                                                               float *__restrict__ dfeat) {
    const int b = blockIdx.y;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (n >= N) return;
    size_t row[3];
    bool ok[3];
    for (int p = 0; p < 3; ++p) {
        const int cell = cell_of[((size_t)b * 3 + p) * N + n];
        ok[p] = (unsigned)cell < (unsigned)cells;
        row[p] = (((size_t)b * 3 + p) * cells + (ok[p] ? cell : 0)) * C;
    }
    float *o = dfeat + ((size_t)b * N + n) * C;
    for (int c = lane; c < C; c += 64) {
        const float v0 = ok[0] && arg_tab[row[0] + c] == n ? sum_tab[row[0] + c] : 0.0f;
        const float v1 = ok[1] && arg_tab[row[1] + c] == n ? sum_tab[row[1] + c] : 0.0f;
        const float v2 = ok[2] && arg_tab[row[2] + c] == n ? sum_tab[row[2] + c] : 0.0f;
        o[c] = (v0 + v1) + v2;
    }
}

// generate_plane_features: one block per (cell, b); thread = channel.  One fp32 division per (cell, channel), then the
// quotient is copied to every point of the cell's run (each point lies in exactly one run: every row is written once).
__global__ __launch_bounds__(256) void cell_mean_backward_kernel(int N, int C, int cells, const int *__restrict__ order,
                                                                 const int *__restrict__ seg,
                                                                 const float *__restrict__ dplane,
                                                                 float *__restrict__ dfeat) {
    const int cell = blockIdx.x, b = blockIdx.y;
    const int *sg = seg + (size_t)b * (cells + 1);
    const int beg = sg[cell], end = sg[cell + 1];
    if (end <= beg) return;
    const int *ord = order + (size_t)b * N;
    float *fb = dfeat + (size_t)b * N * C;
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        const float g = dplane[((size_t)b * C + c) * cells + cell] / (float)(end - beg);
        for (int k = beg; k < end; ++k) {
            const int n = ord[k];
            if ((unsigned)n < (unsigned)N) fb[(size_t)n * C + c] = g;
        }
    }
}

// points_projection: one thread per (pixel, b): the pixel's winner is the low 32 bits of the forward's z-buffer key.
// dout rows are `row` floats apart, of which the first C are taken (row > C: the RGB columns of the grid form's rows).
__global__ __launch_bounds__(256) void project_backward_kernel(int N, int C, int row, int H, int W,
                                                               const unsigned long long *__restrict__ zbuf,
                                                               const float *__restrict__ dout, float *__restrict__ dfeat) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    const size_t HW = (size_t)H * W;
    if (i >= (int)HW) return;
    const unsigned long long key = zbuf[b * HW + i];
    const unsigned id = (unsigned)key;
    const bool won = key != ~0ull && id < (unsigned)N;
    const float *g = dout + ((size_t)b * N + (won ? id : 0)) * row;
    float *o = dfeat + (size_t)b * C * HW + i;
    for (int c = 0; c < C; ++c) o[c * HW] = won ? g[c] : 0.0f;
}

// amav_points_project_grid, w.r.t. the grid: a gather, one wave per (node, b), lanes along channels (two accumulators
// per lane: 128 channels per sweep).  The node (j, i) is a corner of the pixels whose i0 is j - 1 or j (rows) and i - 1
// or i (columns): a rectangle, found by bisection over grid_axis itself.  The wave walks the rectangle in row-major
// order (= ascending pixel index y * W + x) 64 pixels at a time: every lane reads one z-buffer key, a ballot finds the
// won pixels, and the set bits are taken in ascending order; within a pixel the corners 00, 01, 10, 11 that are this
// node each add one term w * g (in the clamped half-cells i0 == i1: two separate terms).
__global__ __launch_bounds__(256) void project_grid_backward_kernel(int N, int H, int W, int Gh, int Gw, int Cg,
                                                                    const unsigned long long *__restrict__ zbuf,
                                                                    const float *__restrict__ dout,
                                                                    float *__restrict__ dgrid) {
#pragma clang fp contract(off)  // w = wy * wx, then acc += w * g: three roundings per term, in that order
    const int b = blockIdx.y;
    const int node = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (node >= Gh * Gw) return;
    const int j = node / Gw, i = node - j * Gw;
    const int ylo = grid_axis_first_pixel(j - 1, H, Gh), yhi = grid_axis_first_pixel(j + 1, H, Gh);
    const int xlo = grid_axis_first_pixel(i - 1, W, Gw), xhi = grid_axis_first_pixel(i + 1, W, Gw);
    const int fw = xhi - xlo, count = fw * (yhi - ylo);  // at most H * W < 2^31
    const unsigned long long *zb = zbuf + (size_t)b * H * W;
    const int row = 3 + Cg;
    const float *gb = dout + (size_t)b * N * row + 3;
    float *o = dgrid + (((size_t)b * Gh + j) * Gw + i) * Cg;
    for (int c0 = 0; c0 < Cg; c0 += 128) {
        const int ca = c0 + lane, cb = c0 + 64 + lane;
        float acc_a = 0.0f, acc_b = 0.0f;
        for (int k0 = 0; k0 < count; k0 += 64) {
            const int k = k0 + lane;
            unsigned id = 0;
            bool won = false;
            if (k < count) {
                const int y = ylo + k / fw, x = xlo + k % fw;
                const unsigned long long key = zb[(size_t)y * W + x];
                id = (unsigned)key;
                won = key != ~0ull && id < (unsigned)N;
            }
            unsigned long long mask = __ballot(won);
            while (mask) {
                const int bit = __ffsll((long long)mask) - 1;
                mask &= mask - 1;
                const int kk = k0 + bit;
                const int y = ylo + kk / fw, x = xlo + kk % fw;
                const unsigned n = (unsigned)__shfl((int)id, bit);
                const GridAxis ay = grid_axis(y, H, Gh), ax = grid_axis(x, W, Gw);
                const float *g = gb + (size_t)n * row;
                const float ga = ca < Cg ? g[ca] : 0.0f, gc = cb < Cg ? g[cb] : 0.0f;
                for (int corner = 0; corner < 4; ++corner) {
                    const int cy = corner >> 1 ? ay.i1 : ay.i0, cx = corner & 1 ? ax.i1 : ax.i0;
                    if (cy != j || cx != i) continue;
                    const float w = (corner >> 1 ? ay.l : ay.h) * (corner & 1 ? ax.l : ax.h);
                    acc_a = acc_a + w * ga;
                    acc_b = acc_b + w * gc;
                }
            }
        }
        if (ca < Cg) o[ca] = acc_a;
        if (cb < Cg) o[cb] = acc_b;
    }
}

inline unsigned channel_threads(int C) { return (unsigned)min(256, (C + kWave - 1) / kWave * kWave); }

}  // namespace splat_bwd
}  // namespace amav

using namespace amav;
using namespace amav::splat_bwd;

extern "C" size_t amav_cell_max_backward_workspace_bytes(int B, int C, int cells) {
    if (B <= 0 || C <= 0 || cells <= 0) return 0;
    Carver c(nullptr);
    c.take<int>((size_t)B * 3 * cells * C);
    c.take<float>((size_t)B * 3 * cells * C);
    return c.total();
}

extern "C" int amav_cell_max_backward(int B, int N, int C, int cells, const float *feat, const int32_t *order,
                                      const int32_t *seg, const int32_t *cell_of, const float *grad_out,
                                      float *grad_feat, void *workspace, size_t workspace_bytes, void *stream_) {
    AMAV_REQUIRE(B > 0 && N > 0 && C > 0 && cells > 0 && B <= 65535, "amav_cell_max_backward: bad sizes");
    AMAV_REQUIRE(feat && order && seg && cell_of && grad_out && grad_feat, "amav_cell_max_backward: NULL pointer");
    const size_t need = amav_cell_max_backward_workspace_bytes(B, C, cells);
    if (!workspace || workspace_bytes < need)
        return fail(AMAV_ERR_WORKSPACE, "amav_cell_max_backward: workspace %zu < required %zu",
                    workspace ? workspace_bytes : 0, need);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    Carver w(workspace);
    int *arg_tab = w.take<int>((size_t)B * 3 * cells * C);
    float *sum_tab = w.take<float>((size_t)B * 3 * cells * C);
    cell_max_route_kernel<<<dim3((unsigned)cells, 3, (unsigned)B), channel_threads(C), 0, stream>>>(
        N, C, cells, feat, order, seg, grad_out, arg_tab, sum_tab);
    cell_max_scatter_kernel<<<dim3((unsigned)((N + 3) / 4), (unsigned)B), 256, 0, stream>>>(N, C, cells, cell_of,
                                                                                           arg_tab, sum_tab, grad_feat);
    return check_launch("amav_cell_max_backward");
}

extern "C" int amav_cell_mean_backward(int B, int N, int C, int cells, const int32_t *order, const int32_t *seg,
                                       const float *grad_planes, float *grad_feat, void *stream) {
    AMAV_REQUIRE(B > 0 && N > 0 && C > 0 && cells > 0 && B <= 65535, "amav_cell_mean_backward: bad sizes");
    AMAV_REQUIRE(order && seg && grad_planes && grad_feat, "amav_cell_mean_backward: NULL pointer");
    cell_mean_backward_kernel<<<dim3((unsigned)cells, (unsigned)B), channel_threads(C), 0,
                                static_cast<hipStream_t>(stream)>>>(N, C, cells, order, seg, grad_planes, grad_feat);
    return check_launch("amav_cell_mean_backward");
}

extern "C" int amav_points_project_backward(int B, int N, int C, int H, int W, const float *grad_out,
                                            const void *workspace, size_t workspace_bytes, float *grad_features,
                                            void *stream) {
    AMAV_REQUIRE(B > 0 && N > 0 && C > 0 && H > 0 && W > 0 && B <= 65535, "amav_points_project_backward: bad sizes");
    AMAV_REQUIRE((long long)H * W < (1ll << 31), "amav_points_project_backward: image too large");
    AMAV_REQUIRE(grad_out && grad_features, "amav_points_project_backward: NULL pointer");
    const size_t need = amav_points_project_workspace_bytes(B, N, H, W);
    if (!workspace || workspace_bytes < need)
        return fail(AMAV_ERR_WORKSPACE, "amav_points_project_backward: workspace %zu < required %zu",
                    workspace ? workspace_bytes : 0, need);
    // the z-buffer is the first carve of amav_points_project's workspace (splat.hip)
    const unsigned long long *zbuf = static_cast<const unsigned long long *>(workspace);
    project_backward_kernel<<<dim3((unsigned)(((size_t)H * W + 255) / 256), (unsigned)B), 256, 0,
                              static_cast<hipStream_t>(stream)>>>(N, C, C, H, W, zbuf, grad_out, grad_features);
    return check_launch("amav_points_project_backward");
}

extern "C" int amav_points_project_grid_backward(int B, int N, int H, int W, int Gh, int Gw, int Cg,
                                                 const float *grad_out, const void *workspace, size_t workspace_bytes,
                                                 float *grad_grid, float *grad_rgb, void *stream_) {
    AMAV_REQUIRE(B > 0 && N > 0 && H > 0 && W > 0 && Gh > 0 && Gw > 0 && Cg > 0 && B <= 65535,
                 "amav_points_project_grid_backward: bad sizes");
    AMAV_REQUIRE((long long)H * W < (1ll << 31), "amav_points_project_grid_backward: image too large");
    AMAV_REQUIRE((long long)Gh * Gw < (1ll << 31), "amav_points_project_grid_backward: grid too large");
    AMAV_REQUIRE(grad_out && grad_grid, "amav_points_project_grid_backward: NULL pointer");
    const size_t need = amav_points_project_workspace_bytes(B, N, H, W);
    if (!workspace || workspace_bytes < need)
        return fail(AMAV_ERR_WORKSPACE, "amav_points_project_grid_backward: workspace %zu < required %zu",
                    workspace ? workspace_bytes : 0, need);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const unsigned long long *zbuf = static_cast<const unsigned long long *>(workspace);  // the first carve (splat.hip)
    project_grid_backward_kernel<<<dim3((unsigned)(((size_t)Gh * Gw + 3) / 4), (unsigned)B), 256, 0, stream>>>(
        N, H, W, Gh, Gw, Cg, zbuf, grad_out, grad_grid);
    if (grad_rgb)  // the first three columns of every winner's row, as amav_points_project_backward routes them
        project_backward_kernel<<<dim3((unsigned)(((size_t)H * W + 255) / 256), (unsigned)B), 256, 0, stream>>>(
            N, 3, 3 + Cg, H, W, zbuf, grad_out, grad_rgb);
    return check_launch("amav_points_project_grid_backward");
}
