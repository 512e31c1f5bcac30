// Triplane decode, backward, for gfx950: gradients of the packed Gaussian records [F,N,16] that project_kernel +
// sample_decode_kernel (triplane.hip, decode_quad.h) produce, with respect to the token slab, the head weights, the
// points and transl.  The forward is "project, then sample"; the backward mirrors it, "scatter, then unproject", so
// the [N, 3C] feature tensor never exists here either.  Five launches, no float atomics, no host synchronisation:
//
//   point_kernel      one thread per (frame, point), blocks never straddle frames.  Recomputes the sixteen raw head
//                     outputs with the forward's own functions (decode_quad.h: the twelve taps, group_raw), takes
//                     the epilogue's backward (F.normalize with its eps branch, s (1 - s) of the sigmoid) -> gRaw
//                     [F,N,16] (scratch); dPoints = direct xyz term + W_xyz^T gRaw + the bilinear weights' derivative
//                     (torch grid_sampler's backward, zero padding, through clamp(p / radius)); fixed-order block
//                     partials of d head_w_point and of dtransl.
//   texel_kernel      G[f,p,t,:] = sum over the taps (n, k) of frame f that land on texel t of plane p of w * gRaw[f,n,:]
//                     -- the transpose of the sampling -- summed in POINT order, so a frame's G does not depend on how
//                     frames are grouped into calls.  One wave per workgroup owns a tile of <= 256 texels of one (frame,
//                     plane) in LDS and walks the frame's points in chunks of 64: the lanes test their point's four
//                     taps against the tile, a ballot picks the chunk's points that touch it, and those are added one
//                     point at a time with the lanes over (tap, channel) -- the four taps of a point are distinct
//                     texels, so one point is one conflict-free read-modify-write of LDS, in order.
//   dtokens_kernel    dTokens[f,c,p,t] = sum_k W_plane[p,c,k] G[f,p,t,k]: streams the [F,C,3R^2] gradient slab out once
//                     (4 texels per thread, the plane's weights broadcast from LDS, as project_kernel reads them).
//   dwplane_kernel    per (frame, plane, 64 channels): sum_t tokens[f,c,p,t] G[f,p,t,:] over the frame's rectangle, a
//                     GEMM of K = rectangle texels through LDS tiles -> partial slab [F,3,C,16].
//   finalize_kernel   fixed-order sums of the partial slabs: d head_w_plane (over frames), d head_w_point (over
//                     blocks), dtransl (over the frame's blocks).
//
// Region contract (amav_triplane_project_region): with boxes, only the frame's projected rectangle of each plane
// (triplane_region.h, x widened to whole texel quads as the projection walks them) is read from the slab or from G; the
// gradient slab is written everywhere, exact zeros outside.
#include <cstddef>

#include "amav_common.h"
#include "decode_quad.h"
#include "triplane_region.h"
#include "wave_ops.h"

namespace amav {
namespace triplane_bwd {

// the forward's tap and record arithmetic
using decode::clamp_unit;
using decode::group_raw;
using decode::normalize4;
using decode::plane_taps;
using decode::PlaneTaps;
using decode::sigmoid;

constexpr int kTileTexels = 256;  // texels of G one texel_kernel wave keeps in LDS (16 KB)
constexpr int kPointBlock = 256;  // points per point_kernel block
constexpr int kPointPart = 68;    // per block: d head_w_point [16][4], dtransl [3], pad
constexpr int kWChunk = 64;       // dwplane_kernel: channels per block and texels per LDS tile

// The frame's rectangle of plane `plane` the forward projected (texels [x0, x1] x [y0, y1]); the whole plane without
// boxes or when R % 4 != 0 (amav_triplane_project_region ignores boxes then).
__device__ __forceinline__ triplane::TexelRect backward_rect(const float *__restrict__ boxes, int f, int plane,
                                                             float radius, int R) {
    triplane::TexelRect r{0, R - 1, 0, R - 1};
    if (boxes && (R & 3) == 0) {
        r = triplane::region_of(boxes + (size_t)f * 6, plane, radius, R);
        r.x0 &= ~3, r.x1 |= 3;  // the projection walks whole quads of a row
    }
    return r;
}

// grid: F * ceil(N / 256) blocks of 256 threads, block b = frame b / bpf.
__global__ __launch_bounds__(256) void point_kernel(int N, int R, const float *__restrict__ proj,
                                                    const float *__restrict__ points, float radius,
                                                    const float *__restrict__ wpoint, const float *__restrict__ grec,
                                                    float *__restrict__ graw, float *__restrict__ dpoints,
                                                    float *__restrict__ part) {
#pragma clang fp contract(off)
    __shared__ float wave_part[4][kPointPart];
    const int bpf = (N + kPointBlock - 1) / kPointBlock;
    const int f = blockIdx.x / bpf, n = (blockIdx.x % bpf) * kPointBlock + threadIdx.x;
    const bool live = n < N;
    const size_t pt = (size_t)f * N + (live ? n : 0);
    const float p[3] = {points[pt * 3], points[pt * 3 + 1], points[pt * 3 + 2]};
    const float4 *g4 = reinterpret_cast<const float4 *>(grec) + pt * 4;
    const float u[3] = {clamp_unit(p[0], radius), clamp_unit(p[1], radius), clamp_unit(p[2], radius)};
    // the twelve taps (plane, dy, dx) as the forward forms them (decode_quad.h)
    PlaneTaps pt3[3];
    int off[12];
    float w[12];
    bool in[12];
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) {
        pt3[pl] = plane_taps(pl == 2 ? u[1] : u[0], pl == 0 ? u[1] : u[2], R);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            in[pl * 4 + k] = pt3[pl].in[k], w[pl * 4 + k] = pt3[pl].w[k];
            off[pl * 4 + k] = pl * R * R * 4 + pt3[pl].off[k];  // float4 units from the frame's plane 0
        }
    }
    const float4 *pl0 = reinterpret_cast<const float4 *>(proj + (size_t)f * 3 * R * R * 16);
    const float4 *wq = reinterpret_cast<const float4 *>(wpoint);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float vt[12];  // sum_k proj[tap][k] gRaw[k] per tap
#pragma unroll
    for (int k = 0; k < 12; ++k) vt[k] = 0.0f;
    float dpw[3] = {0.f, 0.f, 0.f};  // W_xyz^T gRaw
    // one group of four channels (one quad lane of the forward) at a time: twelve float4 taps live, not 48
#pragma unroll 1
    for (int q = 0; q < 4; ++q) {
        // raw channels 4q..4q+3 as quad_record forms them
        float4 tv[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) tv[k] = pl0[off[k] + q];
        const float4 wrow[4] = {wq[q * 4], wq[q * 4 + 1], wq[q * 4 + 2], wq[q * 4 + 3]};
        const float4 acc = group_raw(tv, w, wrow, p[0], p[1], p[2]);
        const float4 gq = g4[q];
        float d[4] = {gq.x, gq.y, gq.z, gq.w};
        if (q == 1) {
            // y = v / max(|v|, 1e-12): dv = (g - y (y . g)) / |v| above eps, g / eps below (torch's clamp_min branch)
            float nrm_raw, inv;
            const float4 y4 = normalize4(acc, nrm_raw, inv);
            const float y[4] = {y4.x, y4.y, y4.z, y4.w};
            const float dot = d[0] * y[0] + d[1] * y[1] + d[2] * y[2] + d[3] * y[3];
#pragma unroll
            for (int e = 0; e < 4; ++e) d[e] = nrm_raw >= 1e-12f ? (d[e] - y[e] * dot) * inv : d[e] * inv;
        } else if (q == 2) {
            d[3] = 0.0f;  // pad
        } else if (q == 3) {
            const float a[3] = {acc.x, acc.y, acc.z};
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                const float s = sigmoid(a[e]);
                d[e] = d[e] * (s * (1.0f - s));
            }
            d[3] = 0.0f;  // pad
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) d[e] = live ? d[e] : 0.0f;
        if (live) reinterpret_cast<float4 *>(graw)[pt * 4 + q] = make_float4(d[0], d[1], d[2], d[3]);
#pragma unroll
        for (int k = 0; k < 12; ++k)
            vt[k] = fmaf(tv[k].w, d[3], fmaf(tv[k].z, d[2], fmaf(tv[k].y, d[1], fmaf(tv[k].x, d[0], vt[k]))));
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            dpw[0] = fmaf(d[e], wrow[e].x, dpw[0]), dpw[1] = fmaf(d[e], wrow[e].y, dpw[1]);
            dpw[2] = fmaf(d[e], wrow[e].z, dpw[2]);
        }
        // this group's rows of the block partial of d head_w_point: butterfly inside the wave (fixed order)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float s0 = wave_sum(live ? d[e] * p[0] : 0.0f), s1 = wave_sum(live ? d[e] * p[1] : 0.0f);
            const float s2 = wave_sum(live ? d[e] * p[2] : 0.0f), s3 = wave_sum(d[e]);
            if (lane == 0) {
                float *wp = &wave_part[wave][(4 * q + e) * 4];
                wp[0] = s0, wp[1] = s1, wp[2] = s2, wp[3] = s3;
            }
        }
    }
    const float4 gx = g4[0];  // xyz = p + offset + transl: direct terms
    const float gxyz[3] = {live ? gx.x : 0.0f, live ? gx.y : 0.0f, live ? gx.z : 0.0f};
    if (dpoints && live) {
        // sampling term: d/d(pixel x, y) of the in-plane taps (torch grid_sampler_2d_backward), * R / 2, through the
        // clamp (gradient where -1 <= p / radius <= 1), / radius
        float du[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) {
            float sx = 0.f, sy = 0.f;
#pragma unroll
            for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                for (int dx = 0; dx < 2; ++dx) {
                    const int k = pl * 4 + dy * 2 + dx;
                    if (!in[k]) continue;
                    const float wy = dy ? pt3[pl].wy1 : pt3[pl].wy0, wx = dx ? pt3[pl].wx1 : pt3[pl].wx0;
                    sx += dx ? vt[k] * wy : -(vt[k] * wy);
                    sy += dy ? vt[k] * wx : -(vt[k] * wx);
                }
            const float half = 0.5f * (float)R;
            du[pl == 2 ? 1 : 0] += sx * half;
            du[pl == 0 ? 1 : 2] += sy * half;
        }
        float *o = dpoints + pt * 3;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const float s = p[i] / radius, v = gxyz[i] + dpw[i];
            o[i] = (s >= -1.0f && s <= 1.0f) ? v + du[i] / radius : v;
        }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float s = wave_sum(gxyz[i]);
        if (lane == 0) wave_part[wave][64 + i] = s;
    }
    __syncthreads();
    if (threadIdx.x < kPointPart) {
        const int j = threadIdx.x;
        part[(size_t)blockIdx.x * kPointPart + j] =
            j < 67 ? ((wave_part[0][j] + wave_part[1][j]) + wave_part[2][j]) + wave_part[3][j] : 0.0f;
    }
}

// grid: (tile slots, 3 planes, F), one wave per workgroup; a slot walks the tiles slot, slot + gridDim.x, ... of the
// frame's rectangle.  A tile is TR rows x TC columns of the rectangle, TC = min(width, 256), TR = 256 / TC.
__global__ __launch_bounds__(64) void texel_kernel(int N, int R, const float *__restrict__ points, float radius,
                                                   const float *__restrict__ graw, const float *__restrict__ boxes,
                                                   float *__restrict__ G) {
    __shared__ __align__(16) float tile_g[kTileTexels * 16];
    __shared__ __align__(16) float st_g[64 * 16];  // gRaw of the chunk's points
    __shared__ __align__(16) int st_tex[64 * 4];   // tile texel of each tap (-1: elsewhere)
    __shared__ __align__(16) float st_w[64 * 4];
    const int plane = blockIdx.y, f = blockIdx.z, lane = threadIdx.x;
    const triplane::TexelRect rc = backward_rect(boxes, f, plane, radius, R);
    const int rw = rc.x1 - rc.x0 + 1, rh = rc.y1 - rc.y0 + 1;
    const int TC = min(rw, kTileTexels), TR = kTileTexels / TC;
    const int tiles_x = (rw + TC - 1) / TC, tiles = tiles_x * ((rh + TR - 1) / TR);
    const float *fp = points + (size_t)f * N * 3;
    const float4 *fg = reinterpret_cast<const float4 *>(graw) + (size_t)f * N * 4;
    const int tap = lane >> 4, ch = lane & 15;
    for (int ti = blockIdx.x; ti < tiles; ti += gridDim.x) {
        const int tx0 = rc.x0 + (ti % tiles_x) * TC, ty0 = rc.y0 + (ti / tiles_x) * TR;
        const int tx1 = min(tx0 + TC, rc.x1 + 1), ty1 = min(ty0 + TR, rc.y1 + 1);  // exclusive
        for (int i = lane; i < kTileTexels * 16; i += 64) tile_g[i] = 0.0f;
        // Two-stage pipeline over the chunks of 64 points: while chunk c is added, the record gradients of chunk c + 1's
        // touching points and the coordinates of chunk c + 2 are in flight.
        struct Chunk {  // vector members, not arrays: the copy below stays in registers
            int4 tex;
            float4 wt, g0, g1, g2, g3;
            bool touch;
        };
        auto classify = [&](int n, float x, float y, float z, Chunk &ck) {
            ck.touch = false;
            ck.tex = make_int4(-1, -1, -1, -1), ck.wt = make_float4(0.f, 0.f, 0.f, 0.f);
            if (n >= N) return;
            const float u0 = clamp_unit(x, radius), u1 = clamp_unit(y, radius), u2 = clamp_unit(z, radius);
            const PlaneTaps t = plane_taps(plane == 2 ? u1 : u0, plane == 0 ? u1 : u2, R);
#pragma unroll
            for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                for (int dx = 0; dx < 2; ++dx) {
                    const int px = t.ix0 + dx, py = t.iy0 + dy;
                    if (px >= tx0 && px < tx1 && py >= ty0 && py < ty1) {  // inside the tile: inside the plane too
                        const int tt = (py - ty0) * TC + (px - tx0);
                        const float ww = (dx ? t.wx1 : t.wx0) * (dy ? t.wy1 : t.wy0);
                        if (dy == 0 && dx == 0) ck.tex.x = tt, ck.wt.x = ww;
                        if (dy == 0 && dx == 1) ck.tex.y = tt, ck.wt.y = ww;
                        if (dy == 1 && dx == 0) ck.tex.z = tt, ck.wt.z = ww;
                        if (dy == 1 && dx == 1) ck.tex.w = tt, ck.wt.w = ww;
                        ck.touch = true;
                    }
                }
            if (ck.touch) {
                const float4 *src = fg + (size_t)n * 4;
                ck.g0 = src[0], ck.g1 = src[1], ck.g2 = src[2], ck.g3 = src[3];
            }
        };
        auto load_point = [&](int n, float &x, float &y, float &z) {
            const int m = min(n, N - 1);
            x = fp[m * 3], y = fp[m * 3 + 1], z = fp[m * 3 + 2];
        };
        float nx, ny, nz;
        Chunk cur, next;
        load_point(lane, nx, ny, nz);
        classify(lane, nx, ny, nz, cur);
        load_point(64 + lane, nx, ny, nz);
        for (int c0 = 0; c0 < N; c0 += 64) {
            unsigned long long m = __ballot(cur.touch);
            if (c0 + 64 < N) {
                classify(c0 + 64 + lane, nx, ny, nz, next);
                load_point(c0 + 128 + lane, nx, ny, nz);
            }
            if (m) {
                if (cur.touch) {
                    float4 *dst = reinterpret_cast<float4 *>(st_g) + lane * 4;
                    dst[0] = cur.g0, dst[1] = cur.g1, dst[2] = cur.g2, dst[3] = cur.g3;
                    reinterpret_cast<int4 *>(st_tex)[lane] = cur.tex;
                    reinterpret_cast<float4 *>(st_w)[lane] = cur.wt;
                }
                __syncthreads();
                // points in order; one point's four taps are four different texels: lanes (tap, channel) never
                // collide.  The next point's staged values are read ahead of this point's read-modify-write.
                int j = __builtin_ctzll(m);
                int t = st_tex[j * 4 + tap];
                float wv = st_w[j * 4 + tap], gv = st_g[j * 16 + ch];
                while (true) {
                    m &= m - 1;
                    int tn = -1;
                    float wn = 0.0f, gn = 0.0f;
                    if (m) {
                        j = __builtin_ctzll(m);
                        tn = st_tex[j * 4 + tap], wn = st_w[j * 4 + tap], gn = st_g[j * 16 + ch];
                    }
                    if (t >= 0) tile_g[t * 16 + ch] = fmaf(wv, gv, tile_g[t * 16 + ch]);
                    if (!m) break;
                    t = tn, wv = wn, gv = gn;
                }
                __syncthreads();
            }
            cur = next;
        }
        // the tile's rows of G (every texel of the rectangle is written: zero where no tap landed)
        const int tw = tx1 - tx0, cnt = (ty1 - ty0) * tw * 4;
        float4 *g4 = reinterpret_cast<float4 *>(G + ((size_t)f * 3 + plane) * R * R * 16);
        const float4 *l4 = reinterpret_cast<const float4 *>(tile_g);
        for (int i = lane; i < cnt; i += 64) {
            const int texel = i >> 2, r = texel / tw, c = texel - r * tw;
            g4[((size_t)(ty0 + r) * R + tx0 + c) * 4 + (i & 3)] = l4[(r * TC + c) * 4 + (i & 3)];
        }
        __syncthreads();
    }
}

// grid: (ceil(R*R / kVec / 256), 3, F); thread = kVec consecutive texels of one plane (kVec = 4 needs R*R % 4 == 0; a
// quad is then wholly inside or outside the rectangle, whose x bounds are quad-aligned whenever there is a region).
template <int kVec>
__global__ __launch_bounds__(256) void dtokens_kernel(int C, int R, const float *__restrict__ wplane,
                                                      const float *__restrict__ G, const float *__restrict__ boxes,
                                                      float radius, float *__restrict__ dtok) {
#pragma clang fp contract(off)
    extern __shared__ __align__(16) float w_lds[];  // [C][16]
    const int plane = blockIdx.y, f = blockIdx.z, RR = R * R;
    {
        const float4 *src4 = reinterpret_cast<const float4 *>(wplane + (size_t)plane * C * 16);
        float4 *dst4 = reinterpret_cast<float4 *>(w_lds);
        for (int i = threadIdx.x; i < C * 4; i += blockDim.x) dst4[i] = src4[i];
    }
    __syncthreads();
    const int t0 = (blockIdx.x * blockDim.x + threadIdx.x) * kVec;
    if (t0 >= RR) return;
    const triplane::TexelRect rc = backward_rect(boxes, f, plane, radius, R);
    const int y = t0 / R, x = t0 - y * R;
    const bool inside = y >= rc.y0 && y <= rc.y1 && x >= rc.x0 && x <= rc.x1;
    float g[kVec][16];
    if (inside) {
        const float4 *g4 = reinterpret_cast<const float4 *>(G + (((size_t)f * 3 + plane) * RR + t0) * 16);
#pragma unroll
        for (int v = 0; v < kVec; ++v)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 a = g4[v * 4 + q];
                g[v][4 * q] = a.x, g[v][4 * q + 1] = a.y, g[v][4 * q + 2] = a.z, g[v][4 * q + 3] = a.w;
            }
    }
    float *dst = dtok + (size_t)f * C * 3 * RR + (size_t)plane * RR + t0;
    for (int c = 0; c < C; ++c) {
        float o[kVec];
        if (inside) {
            const float4 *wc = reinterpret_cast<const float4 *>(w_lds + c * 16);
            const float4 w4[4] = {wc[0], wc[1], wc[2], wc[3]};
            const float wv[16] = {w4[0].x, w4[0].y, w4[0].z, w4[0].w, w4[1].x, w4[1].y, w4[1].z, w4[1].w,
                                  w4[2].x, w4[2].y, w4[2].z, w4[2].w, w4[3].x, w4[3].y, w4[3].z, w4[3].w};
#pragma unroll
            for (int v = 0; v < kVec; ++v) {
                float a = wv[0] * g[v][0];
#pragma unroll
                for (int k = 1; k < 16; ++k) a = fmaf(wv[k], g[v][k], a);
                o[v] = a;
            }
        } else {
#pragma unroll
            for (int v = 0; v < kVec; ++v) o[v] = 0.0f;
        }
        float *d = dst + (size_t)c * 3 * RR;
        if constexpr (kVec == 4)
            *reinterpret_cast<float4 *>(d) = make_float4(o[0], o[1], o[2], o[3]);
        else
            d[0] = o[0];
    }
}

// grid: (ceil(C / 64), 3, F), 256 threads: thread (channel tid / 4, output quad tid % 4) of the block's 64 channels.
// part[f][plane][c][16] = sum over the rectangle's texels (row-major, 64 at a time) of tokens[f,c,plane,t] G[f,plane,t,:].
__global__ __launch_bounds__(256) void dwplane_kernel(int C, int R, const float *__restrict__ tokens,
                                                      long long frame_stride, const float *__restrict__ G,
                                                      const float *__restrict__ boxes, float radius,
                                                      float *__restrict__ part) {
#pragma clang fp contract(off)
    __shared__ float tok[kWChunk][kWChunk + 1];        // [channel][texel]
    __shared__ __align__(16) float gt[kWChunk][16];    // [texel][k]
    const int plane = blockIdx.y, f = blockIdx.z, c0 = blockIdx.x * kWChunk, RR = R * R;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const triplane::TexelRect rc = backward_rect(boxes, f, plane, radius, R);
    const int rw = rc.x1 - rc.x0 + 1, total = rw * (rc.y1 - rc.y0 + 1);
    const float *src = tokens + (size_t)f * frame_stride + (size_t)plane * RR;
    const float *gp = G + ((size_t)f * 3 + plane) * RR * 16;
    const int mc = tid >> 2, mq = tid & 3;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i0 = 0; i0 < total; i0 += kWChunk) {
        // texel of lane / of this thread's G row: the rectangle in row-major order
        const int i = i0 + lane, r = i / rw, t = (rc.y0 + r) * R + rc.x0 + (i - r * rw);
        const bool ok = i < total;
#pragma unroll 4
        for (int k = 0; k < 16; ++k) {
            const int c = c0 + wave * 16 + k;
            tok[wave * 16 + k][lane] = ok && c < C ? src[(size_t)c * 3 * RR + t] : 0.0f;
        }
        {
            const int gi = i0 + (tid >> 2), gr = gi / rw, gtex = (rc.y0 + gr) * R + rc.x0 + (gi - gr * rw);
            reinterpret_cast<float4 *>(gt[tid >> 2])[tid & 3] =
                gi < total ? reinterpret_cast<const float4 *>(gp + (size_t)gtex * 16)[tid & 3] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        __syncthreads();
#pragma unroll 8
        for (int j = 0; j < kWChunk; ++j) {
            const float a = tok[mc][j];
            const float4 b = reinterpret_cast<const float4 *>(gt[j])[mq];
            acc[0] = fmaf(a, b.x, acc[0]), acc[1] = fmaf(a, b.y, acc[1]);
            acc[2] = fmaf(a, b.z, acc[2]), acc[3] = fmaf(a, b.w, acc[3]);
        }
        __syncthreads();
    }
    const int c = c0 + mc;
    if (c < C)
        reinterpret_cast<float4 *>(part + (((size_t)f * 3 + plane) * C + c) * 16)[mq] =
            make_float4(acc[0], acc[1], acc[2], acc[3]);
}

// Blocks [0, nb_plane): d head_w_plane element per thread, summed over frames in order.  Next 64 blocks: one
// d head_w_point element each (256 strided partial sums, then a fixed tree).  Then dtransl: one (frame, axis) per thread.
__global__ __launch_bounds__(256) void finalize_kernel(int F, int C, int nblocks_point, int bpf, int nb_plane,
                                                       const float *__restrict__ part_plane,
                                                       const float *__restrict__ part_point, float *__restrict__ dwplane,
                                                       float *__restrict__ dwpoint, float *__restrict__ dtransl) {
    __shared__ float red[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (b < nb_plane) {
        const int e = b * 256 + tid, E = 3 * C * 16;
        if (e >= E) return;
        float s = 0.0f;
        for (int f = 0; f < F; ++f) s += part_plane[(size_t)f * E + e];
        dwplane[e] = s;
    } else if (b < nb_plane + 64) {
        const int e = b - nb_plane;
        float s = 0.0f;
        for (int i = tid; i < nblocks_point; i += 256) s += part_point[(size_t)i * kPointPart + e];
        red[tid] = s;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (tid < o) red[tid] += red[tid + o];
            __syncthreads();
        }
        if (tid == 0) dwpoint[e] = red[0];
    } else {
        const int e = (b - nb_plane - 64) * 256 + tid;
        if (!dtransl || e >= F * 3) return;
        const int f = e / 3, i = e - f * 3;
        float s = 0.0f;
        for (int j = 0; j < bpf; ++j) s += part_point[((size_t)f * bpf + j) * kPointPart + 64 + i];
        dtransl[e] = s;
    }
}

struct Scratch {
    float *graw, *G, *part_point, *part_plane;
    size_t bytes;
};
inline Scratch carve(void *base, int F, int N, int C, int R) {
    Carver cv(base);
    Scratch s;
    const int bpf = (N + kPointBlock - 1) / kPointBlock;
    s.graw = cv.take<float>((size_t)F * N * 16);
    s.G = cv.take<float>((size_t)F * 3 * R * R * 16);
    s.part_point = cv.take<float>((size_t)F * bpf * kPointPart);
    s.part_plane = cv.take<float>((size_t)F * 3 * C * 16);
    s.bytes = cv.total();
    return s;
}

}  // namespace triplane_bwd
}  // namespace amav

using namespace amav;
using namespace amav::triplane_bwd;

extern "C" size_t amav_triplane_decode_backward_bytes(int F, int N, int C, int R) {
    if (F <= 0 || N <= 0 || C <= 0 || R <= 0) return 0;
    return carve(nullptr, F, N, C, R).bytes;
}

extern "C" int amav_triplane_decode_backward(const amav_triplane_decode_backward_args *a, void *stream_) {
    AMAV_REQUIRE(a != nullptr, "amav_triplane_decode_backward: args is NULL");
    const int F = a->num_frames, N = a->num_points, C = a->channels, R = a->resolution;
    AMAV_REQUIRE(F > 0 && N > 0 && C > 0 && R > 0, "amav_triplane_decode_backward: bad sizes F=%d N=%d C=%d R=%d", F, N,
                 C, R);
    AMAV_REQUIRE(F <= 65535, "amav_triplane_decode_backward: F=%d exceeds grid.z", F);
    AMAV_REQUIRE((size_t)C * 64 <= 64 * 1024, "amav_triplane_decode_backward: C=%d needs more than 64 KiB of LDS for the weights", C);
    AMAV_REQUIRE((size_t)R * R <= (size_t)1 << 26, "amav_triplane_decode_backward: R=%d too large", R);
    AMAV_REQUIRE(a->radius > 0.0f, "amav_triplane_decode_backward: radius must be positive");
    AMAV_REQUIRE(a->tokens && a->head_w_plane && a->head_w_point && a->points && a->proj && a->grad_records &&
                     a->grad_tokens && a->grad_head_w_plane && a->grad_head_w_point,
                 "amav_triplane_decode_backward: NULL pointer");
    AMAV_REQUIRE(a->tokens_frame_stride >= (int64_t)C * 3 * R * R,
                 "amav_triplane_decode_backward: tokens_frame_stride %lld < C * 3 R^2", (long long)a->tokens_frame_stride);
    AMAV_REQUIRE(((reinterpret_cast<uintptr_t>(a->proj) | reinterpret_cast<uintptr_t>(a->grad_records) |
                   reinterpret_cast<uintptr_t>(a->head_w_plane) | reinterpret_cast<uintptr_t>(a->head_w_point) |
                   reinterpret_cast<uintptr_t>(a->grad_tokens) | reinterpret_cast<uintptr_t>(a->scratch)) & 15) == 0,
                 "amav_triplane_decode_backward: proj / grad_records / head weights / grad_tokens / scratch not 16-B aligned");
    AMAV_REQUIRE(a->scratch != nullptr, "amav_triplane_decode_backward: scratch is NULL");
    const Scratch s = carve(a->scratch, F, N, C, R);
    if (a->scratch_bytes < s.bytes)
        return fail(AMAV_ERR_WORKSPACE, "amav_triplane_decode_backward: scratch %zu < required %zu", a->scratch_bytes, s.bytes);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int bpf = (N + kPointBlock - 1) / kPointBlock, RR = R * R;

    point_kernel<<<(unsigned)F * bpf, kPointBlock, 0, stream>>>(N, R, a->proj, a->points, a->radius, a->head_w_point,
                                                                 a->grad_records, s.graw, a->grad_points, s.part_point);
    int rc = check_launch("amav_triplane_decode_backward: point_kernel");
    if (rc) return rc;
    texel_kernel<<<dim3((unsigned)((RR + kTileTexels - 1) / kTileTexels), 3, F), 64, 0, stream>>>(
        N, R, a->points, a->radius, s.graw, a->boxes, s.G);
    if ((rc = check_launch("amav_triplane_decode_backward: texel_kernel"))) return rc;
    const size_t lds = (size_t)C * 16 * sizeof(float);
    if (RR % 4 == 0)
        dtokens_kernel<4><<<dim3((unsigned)((RR / 4 + 255) / 256), 3, F), 256, lds, stream>>>(
            C, R, a->head_w_plane, s.G, a->boxes, a->radius, a->grad_tokens);
    else
        dtokens_kernel<1><<<dim3((unsigned)((RR + 255) / 256), 3, F), 256, lds, stream>>>(
            C, R, a->head_w_plane, s.G, a->boxes, a->radius, a->grad_tokens);
    if ((rc = check_launch("amav_triplane_decode_backward: dtokens_kernel"))) return rc;
    dwplane_kernel<<<dim3((unsigned)((C + kWChunk - 1) / kWChunk), 3, F), 256, 0, stream>>>(
        C, R, a->tokens, a->tokens_frame_stride, s.G, a->boxes, a->radius, s.part_plane);
    if ((rc = check_launch("amav_triplane_decode_backward: dwplane_kernel"))) return rc;
    const int nb_plane = (3 * C * 16 + 255) / 256, nb_transl = (F * 3 + 255) / 256;
    finalize_kernel<<<nb_plane + 64 + nb_transl, 256, 0, stream>>>(F, C, F * bpf, bpf, nb_plane, s.part_plane,
                                                                   s.part_point, a->grad_head_w_plane,
                                                                   a->grad_head_w_point, a->grad_transl);
    return check_launch("amav_triplane_decode_backward: finalize_kernel");
}
