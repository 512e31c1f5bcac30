// Gaussian tile rasterizer, backward (diff_gaussian_rasterization's backward) for gfx950.
//
// Reads what the LAST forward left in its workspace (raster_workspace.h): the per-Gaussian blend records (geom), the
// binned tile rectangles (rectd), the tile lists (tile_off, keys) and sort_big's order of the long lists (sorted).
// Three launches, no float atomics, no host synchronisation:
//
//   seg_kernel            one block per frame: exclusive scan of the binned rectangle areas -> every (frame, Gaussian)
//                         owns a contiguous segment of partial-sum slots, one per tile of its rectangle.  A frame's
//                         slots are exactly its instances (the areas sum to tile_off[T]).
//   tile_grad_kernel      one 256-thread block per tile, one pixel per thread.  The tile's list is put in blend order
//                         (lists <= 512 keys are only ever sorted inside the forward's wave: sorted again here; keys are
//                         unique, so any exact sort gives the forward's order; longer lists come from `sorted`), then
//                         walked twice:
//                           1. REPLAY of the forward front to back with its exact arithmetic (the per-tile k0, k1, the
//                              five FMAs, v_exp_f32, min(0.99), the 1/255 test, T' = fma(-a, T, T) < 1e-4, and the
//                              quadrant box test), giving every pixel's final transmittance and total colour;
//                           2. GRADIENT pass over the same list.  With the replay's totals, the colour behind Gaussian j
//                              is (C_total - C_through_j) + T_final bg, accumulated front to back with the replay's own
//                              FMAs, so nothing is recovered by dividing T by (1 - alpha) step after step.
//                         Per Gaussian, the block's pixel terms -- d/d(x, y) of the pixel-space mean, d/d(qa, qb, qc, L)
//                         of the Cholesky form the records store, d/d(r, g, b) -- are reduced in a fixed order (DPP
//                         inside the wave, then the four waves through LDS) and stored to the instance's slot.
//   gauss_grad_kernel     one thread per (frame, Gaussian): sums its slots in order and carries the result through
//                         Cholesky form -> conic -> 2D covariance -> J W Sigma W^T J^T -> scale / rotation, the
//                         projection -> means3D (and J's dependence on the view-space mean), and the activations.
#include <cmath>
#include <cstddef>

#include "amav_common.h"
#include "raster_project.h"
#include "raster_workspace.h"
#include "wave_ops.h"

namespace amav {
namespace raster_bwd {

using raster::at;
using raster::kLog2e;
using raster::kTile;

constexpr int kChunk = 64;       // Gaussians staged per round
constexpr int kLocalSort = 512;  // lists up to this length are sorted by the block (the forward's kSortCap)
constexpr int kComp = 9;         // per-instance partials: dx, dy, dqa, dqb, dqc, dL, dr, dg, db
constexpr float kLn2 = 0.6931471805599453f;

struct Params {
    int F, N, H, W, gx, gy, T;
    amav_attr means3d, rotations, scales, opacities, colors;
    const float *view, *proj, *tanfov;
    float bg[3];
    float scale_modifier;
    int apply_activations;
    float scale_bias, scale_max, opacity_bias;
    raster::WorkspaceView ws;
    const float *grad_rgba;
    float *g_means, *g_rot, *g_scale, *g_opac, *g_color;
    float *debug_alpha;
    long long slots_per_frame;  // S: slot rows per frame
    int *seg;                   // [F*N] first slot of each Gaussian inside its frame
    float *slots;               // [F][S][kComp]
};

__device__ __forceinline__ int rect_area(uint4 rd) {
    if (rd.w == 0u) return 0;
    const int cx0 = rd.x & 0xffff, cy0 = rd.x >> 16, cx1 = rd.y & 0xffff, cy1 = rd.y >> 16;
    return max(0, cx1 - cx0) * max(0, cy1 - cy0);
}

// a frame whose slots would not fit (never for a consistent caller: the areas sum to the frame's instance count, at
// most max_frame_instances) is left out entirely, so a bad argument cannot write out of bounds
__device__ __forceinline__ bool frame_ok(const Params &p, int f) {
    return (long long)p.ws.tile_off[(size_t)f * (p.T + 1) + p.T] <= p.slots_per_frame;
}

// ------------------------------------------------------------------------------------------------------- segments
__global__ __launch_bounds__(1024) void seg_kernel(Params p) {
    __shared__ int wave_tot[16];
    __shared__ int carry_s;
    if (*p.ws.overflow) return;
    const int f = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (int base = 0; base < p.N; base += 1024) {  // block-uniform trip count
        const int i = base + threadIdx.x;
        const int a = i < p.N ? rect_area(p.ws.rectd[(size_t)f * p.N + i]) : 0;
        const int incl = wave_inclusive_sum(a, lane);
        if (lane == 63) wave_tot[wave] = incl;
        __syncthreads();
        int before = carry_s;
        int tot = 0;
        for (int w = 0; w < 16; ++w) {
            if (w < wave) before += wave_tot[w];
            tot += wave_tot[w];
        }
        if (i < p.N) p.seg[(size_t)f * p.N + i] = before + incl - a;
        __syncthreads();
        if (threadIdx.x == 0) carry_s += tot;
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------------ tile pass
struct TileLds {
    union {
        unsigned long long keys[kLocalSort];  // the list while it is sorted
        float part[4][kComp][kChunk];         // per-wave sums of the current round (gradient pass)
    };
    unsigned order[kLocalSort];  // blend order (lists <= kLocalSort)
    float4 geo[kChunk];          // {k0, k1, qa, qb}
    float4 geo2[kChunk];         // {qc, L, x, y}
    float4 col[kChunk];          // {r, g, b, -}
    int qmask[kChunk];           // quadrants the alpha >= 1/255 box reaches (the forward's test)
    int slot[kChunk];            // slot row of the instance inside the frame
};

// One Gaussian of the blend at one pixel, the forward's arithmetic (rasterizer.hip AMAV_BLEND_GEO / AMAV_BLEND_REST):
// returns alpha (0 = skipped) and leaves u, v, the unclamped 2^e.
__device__ __forceinline__ float blend_alpha(const float4 &g, const float4 &g2, float lx, float ly, float &u, float &v,
                                             float &araw) {
#pragma clang fp contract(off)
    const float t = fmaf(-g.w, ly, g.x);
    v = fmaf(-g2.x, ly, g.y);
    u = fmaf(-g.z, lx, t);
    float e = fmaf(-u, u, g2.y);
    e = fmaf(-v, v, e);
    araw = __builtin_amdgcn_exp2f(e);
    const float a = fminf(0.99f, araw);
    return (a >= 0.003921568859368563f) ? a : 0.0f;  // 1/255 as the forward's constant 0x3b808081
}

__global__ __launch_bounds__(256) void tile_grad_kernel(Params p) {
#pragma clang fp contract(off)
    __shared__ TileLds L;
    if (*p.ws.overflow) return;
    const int t = blockIdx.x, f = blockIdx.y;
    const int *off = p.ws.tile_off + (size_t)f * (p.T + 1);
    const int beg = off[t], n = off[t + 1] - beg;
    if (n <= 0 || !frame_ok(p, f)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tx = t % p.gx, ty = t / p.gx;
    const int X0 = tx * kTile, Y0 = ty * kTile;
    const float X0f = (float)X0, Y0f = (float)Y0;
    // pixel of this thread: 16 columns x 16 rows, a wave = 4 rows
    const int lxi = tid & 15, lyi = tid >> 4;
    const int px = X0 + lxi, py = Y0 + lyi;
    const bool inimg = px < p.W && py < p.H;
    const float lx = (float)lxi, ly = (float)lyi;
    const int quad = (lxi >> 3) | ((lyi >> 3) << 1);
    const bool local = n <= kLocalSort;
    const unsigned long long *keys = p.ws.keys + (size_t)f * p.ws.cap_per_frame + beg;
    const unsigned *sorted = p.ws.sorted + (size_t)f * p.ws.cap_per_frame + beg;

    // ---- blend order of a short list: rank sort of the unique keys
    if (local) {
        for (int k = tid; k < n; k += 256) L.keys[k] = keys[k];
        __syncthreads();
        unsigned long long my[2] = {~0ull, ~0ull};
        int rank[2] = {0, 0};
#pragma unroll
        for (int m = 0; m < 2; ++m)
            if (tid + 256 * m < n) my[m] = L.keys[tid + 256 * m];
        for (int j = 0; j < n; ++j) {
            const unsigned long long kj = L.keys[j];
            rank[0] += (int)(kj < my[0]);
            rank[1] += (int)(kj < my[1]);
        }
#pragma unroll
        for (int m = 0; m < 2; ++m)
            if (tid + 256 * m < n) L.order[rank[m]] = (unsigned)my[m];
        __syncthreads();
    }

    const float4 *geom = p.ws.geom + (size_t)f * p.N * 3;
    const uint4 *rectd = p.ws.rectd + (size_t)f * p.N;
    const int *seg = p.seg + (size_t)f * p.N;
    // stage Gaussians [base, base + kChunk) of the list (the caller syncs before and after)
    auto stage = [&](int base) {
        if (tid < kChunk) {
            const int k = base + tid;
            if (k < n) {
                const unsigned id = local ? L.order[k] : sorted[k];
                const float4 g0 = geom[(size_t)id * 3], g1 = geom[(size_t)id * 3 + 1], g2 = geom[(size_t)id * 3 + 2];
                // the forward's staging (raster_project.h)
                const float2 k = raster::tile_k(g0, g1, X0f, Y0f);
                L.geo[tid] = make_float4(k.x, k.y, g0.z, g0.w);
                L.geo2[tid] = make_float4(g1.x, g1.y, g0.x, g0.y);
                L.col[tid] = make_float4(g1.z, g1.w, g2.x, 0.f);
                L.qmask[tid] = raster::quad_mask(g0, g2, X0f, Y0f);
                const uint4 rd = rectd[id];
                const int cx0 = rd.x & 0xffff, cy0 = rd.x >> 16, cx1 = rd.y & 0xffff;
                L.slot[tid] = seg[id] + (ty - cy0) * (cx1 - cx0) + (tx - cx0);
            } else {
                L.qmask[tid] = 0;
                L.slot[tid] = -1;
            }
        }
    };

    // ---- pass 1: replay
    float T = 1.0f, R = 0.f, G = 0.f, B = 0.f;
    bool done = !inimg;
    for (int base = 0; base < n; base += kChunk) {
        __syncthreads();
        if (!__syncthreads_or(!done)) break;
        stage(base);
        __syncthreads();
        const int cnt = min(kChunk, n - base);
        if (!done) {
            for (int j = 0; j < cnt; ++j) {
                if (!((L.qmask[j] >> quad) & 1)) continue;
                float u, v, araw;
                const float a = blend_alpha(L.geo[j], L.geo2[j], lx, ly, u, v, araw);
                if (a == 0.0f) continue;
                const float Tn = fmaf(-a, T, T);
                if (Tn < 1e-4f) {
                    done = true;
                    break;
                }
                const float w = a * T;
                const float4 c = L.col[j];
                R = fmaf(c.x, w, R);
                G = fmaf(c.y, w, G);
                B = fmaf(c.z, w, B);
                T = Tn;
            }
        }
    }
    const float Tfin = T;
    const size_t pid = ((size_t)f * p.H + (inimg ? py : 0)) * p.W + (inimg ? px : 0);
    if (p.debug_alpha && inimg) p.debug_alpha[pid] = 1.0f - Tfin;

    // ---- pass 2: gradients
    float4 dpix = make_float4(0.f, 0.f, 0.f, 0.f);
    if (inimg) dpix = reinterpret_cast<const float4 *>(p.grad_rgba)[pid];
    const float bgR = Tfin * p.bg[0], bgG = Tfin * p.bg[1], bgB = Tfin * p.bg[2];
    const float x_px = (float)px, y_px = (float)py;
    T = 1.0f;
    float aR = 0.f, aG = 0.f, aB = 0.f;
    done = !inimg;
    float *slots = p.slots + (size_t)f * p.slots_per_frame * kComp;
    for (int base = 0; base < n; base += kChunk) {
        __syncthreads();  // the previous round's partials have been stored
        const bool alive = __syncthreads_or(!done);
        stage(base);
        __syncthreads();
        const int cnt = min(kChunk, n - base);
        for (int j = 0; j < cnt; ++j) {  // block-uniform trip count
            float c[kComp] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            bool hit = false;
            if (alive && !done && ((L.qmask[j] >> quad) & 1)) {
                const float4 g = L.geo[j], g2 = L.geo2[j];
                float u, v, araw;
                const float a = blend_alpha(g, g2, lx, ly, u, v, araw);
                if (a != 0.0f) {
                    const float Tn = fmaf(-a, T, T);
                    if (Tn < 1e-4f) {
                        done = true;
                    } else {
                        hit = true;
                        const float w = a * T;
                        const float4 cl = L.col[j];
                        aR = fmaf(cl.x, w, aR);
                        aG = fmaf(cl.y, w, aG);
                        aB = fmaf(cl.z, w, aB);
                        const float inv = 1.0f / (1.0f - a);
                        // colour (and background) behind this Gaussian, as seen through it
                        const float bR = (R - aR) + bgR, bG = (G - aG) + bgG, bB = (B - aB) + bgB;
                        const float ga = dpix.x * (cl.x * T - bR * inv) + dpix.y * (cl.y * T - bG * inv) +
                                         dpix.z * (cl.z * T - bB * inv) + dpix.w * (Tfin * inv);
                        // alpha = min(0.99, 2^e): the clamp is passed through (upstream), d 2^e / de = 2^e ln 2
                        const float dE = ga * araw * kLn2;
                        const float dU = -2.0f * u * dE, dV = -2.0f * v * dE;
                        const float ddx = g2.z - x_px, ddy = g2.w - y_px;  // u = qa ddx + qb ddy, v = qc ddy
                        c[0] = dU * g.z;
                        c[1] = dU * g.w + dV * g2.x;
                        c[2] = dU * ddx;
                        c[3] = dU * ddy;
                        c[4] = dV * ddy;
                        c[5] = dE;
                        c[6] = dpix.x * w;
                        c[7] = dpix.y * w;
                        c[8] = dpix.z * w;
                        T = Tn;
                    }
                }
            }
            if (__any(hit)) {  // wave-uniform
#pragma unroll
                for (int k = 0; k < kComp; ++k) {
                    const float s = wave_sum_rows(c[k]);
                    if (lane == 0) L.part[wave][k][j] = s;
                }
            } else if (lane == 0) {
#pragma unroll
                for (int k = 0; k < kComp; ++k) L.part[wave][k][j] = 0.f;
            }
        }
        __syncthreads();
        // the four waves' sums in a fixed order -> the instances' slots
        for (int e = tid; e < kComp * kChunk; e += 256) {
            const int k = e / kChunk, j = e - k * kChunk;
            if (j < cnt) {
                const float s = ((L.part[0][k][j] + L.part[1][k][j]) + L.part[2][k][j]) + L.part[3][k][j];
                slots[(size_t)L.slot[j] * kComp + k] = s;
            }
        }
    }
}

// -------------------------------------------------------------------------------------------------- per Gaussian
__global__ __launch_bounds__(256) void gauss_grad_kernel(Params p) {
#pragma clang fp contract(off)
    const long long gi = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gi >= (long long)p.F * p.N) return;
    const int f = (int)(gi / p.N), i = (int)(gi - (long long)f * p.N);
    float *gm = p.g_means + gi * 3, *gr = p.g_rot + gi * 4, *gs = p.g_scale + gi * 3, *go = p.g_opac + gi,
          *gc = p.g_color + gi * 3;
    auto zero = [&]() {
        gm[0] = gm[1] = gm[2] = 0.f;
        gr[0] = gr[1] = gr[2] = gr[3] = 0.f;
        gs[0] = gs[1] = gs[2] = 0.f;
        go[0] = 0.f;
        gc[0] = gc[1] = gc[2] = 0.f;
    };
    if (*p.ws.overflow || !frame_ok(p, f)) return zero();
    const uint4 rd = p.ws.rectd[gi];
    const int area = rect_area(rd);
    if (area == 0) return zero();  // culled, or no tile of its rectangle can see it
    float d[kComp] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const float *sl = p.slots + ((size_t)f * p.slots_per_frame + p.seg[gi]) * kComp;
    for (int s = 0; s < area; ++s)
#pragma unroll
        for (int k = 0; k < kComp; ++k) d[k] += sl[(size_t)s * kComp + k];
    const float g_px = d[0], g_py = d[1], g_qa = d[2], g_qb = d[3], g_qc = d[4], g_L = d[5];

    // ---- the forward's projection: preprocess_one's stages (raster_project.h); J is restated in its operation order
    const float *vm = p.view + f * 16, *pm = p.proj + f * 16;
    const float tanx = p.tanfov[2 * f], tany = p.tanfov[2 * f + 1];
    const float *m_ = at(p.means3d, f, i), *q_ = at(p.rotations, f, i), *s_ = at(p.scales, f, i);
    const float *c_ = at(p.colors, f, i);
    const float px3 = m_[0], py3 = m_[1], pz3 = m_[2];
    const raster::ViewPoint vp = raster::view_point(vm, px3, py3, pz3);
    const float vx = vp.x, vy = vp.y, vz = vp.z;
    const raster::ClipPoint cp = raster::clip_point(pm, px3, py3, pz3);
    const float hx_ = cp.hx, hy_ = cp.hy, pw = cp.pw;
    const float r = q_[0], x = q_[1], y = q_[2], z = q_[3];
    const float sraw[3] = {s_[0], s_[1], s_[2]};
    float sact[3], sexp[3];
    const float oraw = at(p.opacities, f, i)[0];
    float opacity = oraw;
    const float craw[3] = {c_[0], c_[1], c_[2]};
    for (int k = 0; k < 3; ++k) sact[k] = sraw[k], sexp[k] = 0.f;
    if (p.apply_activations) {
        for (int k = 0; k < 3; ++k) sact[k] = raster::scale_act(sraw[k], p.scale_bias, p.scale_max, sexp[k]);
        opacity = raster::opacity_act(oraw, p.opacity_bias);
    }
    const float s0 = sact[0] * p.scale_modifier, s1 = sact[1] * p.scale_modifier, s2 = sact[2] * p.scale_modifier;
    const raster::Cov3 cv = raster::cov3d(r, x, y, z, s0, s1, s2);
    const float(&Rm)[3][3] = cv.R, (&M)[3][3] = cv.M, (&S)[3][3] = cv.S;  // M[k][a] = s_k R[a][k]; Sigma = M^T M
    const float sv[3] = {s0, s1, s2};
    const float focal_x = (float)p.W / (2.0f * tanx), focal_y = (float)p.H / (2.0f * tany);
    const float limx = 1.3f * tanx, limy = 1.3f * tany;
    const float tz = vz;
    const float txr = vx / tz, tyr = vy / tz;
    const float txc = fminf(limx, fmaxf(-limx, txr)), tyc = fminf(limy, fmaxf(-limy, tyr));
    const float tx = txc * tz, ty = tyc * tz;
    const float J00 = focal_x / tz, J02 = -(focal_x * tx) / (tz * tz);
    const float J11 = focal_y / tz, J12 = -(focal_y * ty) / (tz * tz);
    float T0[3], T1[3];
    for (int b = 0; b < 3; ++b) {
        T0[b] = J00 * vm[b * 4 + 0] + J02 * vm[b * 4 + 2];
        T1[b] = J11 * vm[b * 4 + 1] + J12 * vm[b * 4 + 2];
    }
    const raster::Cov2 cov = raster::cov2d(S, T0, T1);
    const float(&ST0)[3] = cov.ST0, (&ST1)[3] = cov.ST1;  // Sigma T0, Sigma T1
    const float ca = cov.ca + 0.3f, cb = cov.cb, cc = cov.cc + 0.3f;
    const float det = ca * cc - cb * cb;
    const float det_inv = 1.0f / det;
    const float kk = 0.5f * kLog2e;
    const raster::Conic q = raster::conic(cb, cc, det_inv);
    const float A = q.A, qa = q.qa, qb = q.qb, qc = q.qc;

    // ---- Cholesky form -> conic (A, B) -> 2D covariance (the +0.3 dilation has derivative 1)
    const float gA = g_qa * (kk / (2.0f * qa)) - g_qb * (qb / (2.0f * A));
    const float gB = g_qb * (kk / qa);
    const float d2 = det_inv * det_inv;
    const float g_ca = gA * (-cc * cc * d2) + gB * (cb * cc * d2);
    const float g_cb = gA * (2.0f * cb * cc * d2) + gB * (-(ca * cc + cb * cb) * d2);
    const float g_cc = gA * (-cb * cb * d2) + gB * (cb * ca * d2) + g_qc * (-qc / (2.0f * cc));

    // ---- 2D covariance -> Sigma and the rows T0, T1 of J W
    float gS[3][3];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) gS[a][b] = g_ca * T0[a] * T0[b] + g_cb * T0[a] * T1[b] + g_cc * T1[a] * T1[b];
    float gT0[3], gT1[3];
    for (int a = 0; a < 3; ++a) {
        gT0[a] = 2.0f * g_ca * ST0[a] + g_cb * ST1[a];
        gT1[a] = 2.0f * g_cc * ST1[a] + g_cb * ST0[a];
    }
    // Sigma = M^T M -> M -> scales, rotation matrix
    float gsv[3] = {0.f, 0.f, 0.f}, gR[3][3];
    for (int k = 0; k < 3; ++k)
        for (int a = 0; a < 3; ++a) {
            const float gM = M[k][0] * (gS[a][0] + gS[0][a]) + M[k][1] * (gS[a][1] + gS[1][a]) + M[k][2] * (gS[a][2] + gS[2][a]);
            gsv[k] += gM * Rm[a][k];
            gR[a][k] = gM * sv[k];
        }
    // rotation matrix -> quaternion (w, x, y, z), not normalised (as the forward)
    const float g_r = 2.f * (-z * gR[0][1] + y * gR[0][2] + z * gR[1][0] - x * gR[1][2] - y * gR[2][0] + x * gR[2][1]);
    const float g_x = 2.f * (y * gR[0][1] + z * gR[0][2] + y * gR[1][0] - r * gR[1][2] + z * gR[2][0] + r * gR[2][1]) -
                      4.f * x * (gR[1][1] + gR[2][2]);
    const float g_y = 2.f * (x * gR[0][1] + r * gR[0][2] + x * gR[1][0] + z * gR[1][2] - r * gR[2][0] + z * gR[2][1]) -
                      4.f * y * (gR[0][0] + gR[2][2]);
    const float g_z = 2.f * (-r * gR[0][1] + x * gR[0][2] + r * gR[1][0] + y * gR[1][2] + x * gR[2][0] + y * gR[2][1]) -
                      4.f * z * (gR[0][0] + gR[1][1]);
    gr[0] = g_r, gr[1] = g_x, gr[2] = g_y, gr[3] = g_z;
    for (int k = 0; k < 3; ++k) {
        float g = gsv[k] * p.scale_modifier;
        if (p.apply_activations)  // min(exp(s - bias), max): torch.min's gradient (split at a tie)
            g = sexp[k] < p.scale_max ? g * sexp[k] : (sexp[k] == p.scale_max ? 0.5f * g * sexp[k] : 0.f);
        gs[k] = g;
    }

    // ---- T0, T1 -> J -> view-space mean (tx, ty clamped to 1.3 tanfov: torch.clamp's gradient)
    float gJ00 = 0.f, gJ02 = 0.f, gJ11 = 0.f, gJ12 = 0.f;
    for (int b = 0; b < 3; ++b) {
        gJ00 += gT0[b] * vm[b * 4 + 0];
        gJ02 += gT0[b] * vm[b * 4 + 2];
        gJ11 += gT1[b] * vm[b * 4 + 1];
        gJ12 += gT1[b] * vm[b * 4 + 2];
    }
    const float tz2 = tz * tz, tz3 = tz2 * tz;
    const float g_tx = gJ02 * (-focal_x / tz2), g_ty = gJ12 * (-focal_y / tz2);
    float g_tz = gJ00 * (-focal_x / tz2) + gJ11 * (-focal_y / tz2) + gJ02 * (2.0f * focal_x * tx / tz3) +
                 gJ12 * (2.0f * focal_y * ty / tz3);
    const bool inx = txr >= -limx && txr <= limx, iny = tyr >= -limy && tyr <= limy;
    // tx = clamp(vx / tz) tz: d/dvx = [inside], d/dtz = clamp(vx / tz) - [inside] vx / tz (0 inside)
    const float g_vx = inx ? g_tx : 0.f, g_vy = iny ? g_ty : 0.f;
    g_tz += inx ? 0.f : g_tx * txc;
    g_tz += iny ? 0.f : g_ty * tyc;
    const float g_vz = g_tz;

    // ---- pixel-space mean -> clip space -> means3D
    const float g_ppx = g_px * 0.5f * (float)p.W, g_ppy = g_py * 0.5f * (float)p.H;
    const float g_hx = g_ppx * pw, g_hy = g_ppy * pw;
    const float g_hw = -(g_ppx * hx_ + g_ppy * hy_) * pw * pw;
    for (int k = 0; k < 3; ++k)
        gm[k] = pm[k * 4 + 0] * g_hx + pm[k * 4 + 1] * g_hy + pm[k * 4 + 3] * g_hw + vm[k * 4 + 0] * g_vx +
                vm[k * 4 + 1] * g_vy + vm[k * 4 + 2] * g_vz;

    // ---- log2(opacity), colours
    float g_op = g_L / (opacity * kLn2);
    if (p.apply_activations) g_op = g_op * (opacity * (1.0f - opacity));
    go[0] = g_op;
    for (int k = 0; k < 3; ++k) {
        float g = d[6 + k];
        if (p.apply_activations && !(craw[k] >= 0.0f && craw[k] <= 1.0f)) g = 0.f;  // clamp(c, 0, 1)
        gc[k] = g;
    }
}

}  // namespace raster_bwd
}  // namespace amav

using namespace amav;
using namespace amav::raster_bwd;

static size_t backward_bytes(int F, int N, long long max_frame, size_t *seg_off) {
    Carver c(nullptr);
    c.take<int>((size_t)F * N);
    const size_t s = c.total();
    c.take<float>((size_t)F * (size_t)max_frame * kComp);
    if (seg_off) *seg_off = s;
    return c.total();
}

extern "C" size_t amav_rasterize_backward_bytes(int F, int N, int64_t max_frame_instances) {
    if (F <= 0 || N <= 0 || max_frame_instances < 0) return 0;
    return backward_bytes(F, N, max_frame_instances, nullptr);
}

extern "C" int amav_rasterize_backward(const amav_raster_args *a, const amav_raster_backward_args *b, void *stream_) {
    AMAV_REQUIRE(a != nullptr, "amav_rasterize_backward: forward args is NULL");
    AMAV_REQUIRE(b != nullptr, "amav_rasterize_backward: backward args is NULL");
    AMAV_REQUIRE(a->num_frames > 0 && a->num_gaussians > 0 && a->height > 0 && a->width > 0,
                 "amav_rasterize_backward: bad sizes F=%d N=%d H=%d W=%d", a->num_frames, a->num_gaussians, a->height,
                 a->width);
    AMAV_REQUIRE(a->means3d.ptr && a->rotations.ptr && a->scales.ptr && a->opacities.ptr && a->colors.ptr,
                 "amav_rasterize_backward: NULL Gaussian attribute");
    AMAV_REQUIRE(a->viewmatrix && a->projmatrix && a->tanfov, "amav_rasterize_backward: NULL camera");
    AMAV_REQUIRE(a->workspace != nullptr, "amav_rasterize_backward: workspace is NULL");
    AMAV_REQUIRE(a->instance_capacity >= 0, "amav_rasterize_backward: negative instance_capacity");
    AMAV_REQUIRE(!a->antialiasing, "amav_rasterize_backward: antialiasing has no backward");
    AMAV_REQUIRE(a->wire == nullptr, "amav_rasterize_backward: a forward with a wire output has no backward");
    AMAV_REQUIRE(!a->clamp_output, "amav_rasterize_backward: the forward must be unclamped (clamp_output = 0)");
    AMAV_REQUIRE(b->grad_rgba && b->grad_means3d && b->grad_rotations && b->grad_scales && b->grad_opacities &&
                     b->grad_colors,
                 "amav_rasterize_backward: NULL gradient pointer");
    AMAV_REQUIRE((reinterpret_cast<uintptr_t>(b->grad_rgba) & 15) == 0, "amav_rasterize_backward: grad_rgba not 16-B aligned");
    AMAV_REQUIRE(b->scratch != nullptr, "amav_rasterize_backward: scratch is NULL");
    AMAV_REQUIRE(b->max_frame_instances >= 0, "amav_rasterize_backward: negative max_frame_instances");
    const int F = a->num_frames, N = a->num_gaussians, H = a->height, W = a->width;
    const int gx = (W + kTile - 1) / kTile, gy = (H + kTile - 1) / kTile;
    AMAV_REQUIRE(gx < 65536 && gy < 65536 && F <= 65535, "amav_rasterize_backward: image or frame count too large");
    const long long cap_per_frame = a->instance_capacity / F;
    AMAV_REQUIRE(b->max_frame_instances <= cap_per_frame,
                 "amav_rasterize_backward: the forward overflowed its workspace (%lld instances in a frame, room for %lld)",
                 (long long)b->max_frame_instances, cap_per_frame);
    const raster::WorkspaceView ws = raster::workspace_view(a->workspace, F, N, H, W, a->instance_capacity);
    if (a->workspace_bytes < ws.bytes)
        return fail(AMAV_ERR_WORKSPACE, "amav_rasterize_backward: workspace %zu < required %zu", a->workspace_bytes, ws.bytes);
    size_t seg_off = 0;
    const size_t need = backward_bytes(F, N, b->max_frame_instances, &seg_off);
    if (b->scratch_bytes < need)
        return fail(AMAV_ERR_WORKSPACE, "amav_rasterize_backward: scratch %zu < required %zu", b->scratch_bytes, need);

    Params p;
    p.F = F, p.N = N, p.H = H, p.W = W, p.gx = gx, p.gy = gy, p.T = gx * gy;
    p.means3d = a->means3d, p.rotations = a->rotations, p.scales = a->scales, p.opacities = a->opacities;
    p.colors = a->colors;
    p.view = a->viewmatrix, p.proj = a->projmatrix, p.tanfov = a->tanfov;
    p.bg[0] = a->bg[0], p.bg[1] = a->bg[1], p.bg[2] = a->bg[2];
    p.scale_modifier = a->scale_modifier;
    p.apply_activations = a->apply_activations;
    p.scale_bias = a->scale_bias, p.scale_max = a->scale_max, p.opacity_bias = a->opacity_bias;
    p.ws = ws;
    p.grad_rgba = b->grad_rgba;
    p.g_means = b->grad_means3d, p.g_rot = b->grad_rotations, p.g_scale = b->grad_scales;
    p.g_opac = b->grad_opacities, p.g_color = b->grad_colors;
    p.debug_alpha = b->debug_alpha;
    p.slots_per_frame = b->max_frame_instances;
    p.seg = static_cast<int *>(b->scratch);
    p.slots = reinterpret_cast<float *>(static_cast<char *>(b->scratch) + seg_off);

    hipStream_t stream = static_cast<hipStream_t>(stream_);
    // pixels of empty tiles are never visited: their replay alpha is 0
    if (p.debug_alpha && zero_async(p.debug_alpha, (size_t)F * H * W * sizeof(float), stream) != hipSuccess)
        return fail(AMAV_ERR_LAUNCH, "amav_rasterize_backward: debug_alpha clear failed");
    seg_kernel<<<F, 1024, 0, stream>>>(p);
    tile_grad_kernel<<<dim3((unsigned)p.T, (unsigned)F), 256, 0, stream>>>(p);
    const long long total = (long long)F * N;
    gauss_grad_kernel<<<(unsigned)((total + 255) / 256), 256, 0, stream>>>(p);
    return check_launch("amav_rasterize_backward");
}
