// SMPL-X mesh overlay (the demo's second clip: draw_smplx_on_image / SimpleMeshRenderer.render_mesh,
// src/utils/graphic_utils.py:782-944, there pyrender on an offscreen GL context): a z-buffered triangle rasterizer with
// flat shading and a composite over the rendered frames, for a whole batch of frames per call.
//
//   fill      keys [F,H,W] = all ones, counters = 0
//   project   one thread per (frame, vertex): camera-space z, and (u, v) snapped to 1/256 px as int32
//   setup     one thread per (frame, face): drops, culling, shade; small bounding boxes are rasterized here, the
//             others are appended to the frame's deferred list
//   large     one wave per deferred face, lanes stride over the pixel centres of its bounding box
//   resolve   one thread per pixel: the winner's shade or the frame's RGB
//
// Coverage is exact int64 arithmetic on the snapped coordinates (top-left fill rule); the z-buffer is the integer
// atomicMin over (depth bits << 32) | face of project_zbuffer_kernel (splat.hip): order-independent, so the two tiers
// and any batching give the same bits.  include/amav.h has the contract, DESIGN.md section 4.21 the reasoning.
#include "amav_common.h"

namespace amav {
namespace mesh {

constexpr int kGuard = 1 << 22;     // snapped units: 16384 px
constexpr int kMaxExtent = 16384;   // H, W: pixel centres stay within the guard band
constexpr int kLargeBlocks = 32;    // x 4 waves per frame stride over the deferred list

// Edge functions e_k(px, py) = A px + B py + C of one face, oriented so that the interior is where all three are
// positive, with the fill rule folded in: C holds -1 for an edge that does not own the centres lying exactly on it, so
// "covered" is e_k >= 0 for all k and e_k + bias_k is the exact edge value (the barycentric numerator of vertex k).
struct Tri {
    long long A[3], B[3], C[3];
    int bias[3];
    float area, iz[3];  // doubled area (positive), 1 / z of the three vertices
    int c0, r0, bw, count;  // clipped box of pixel centres: first column / row, width, number of centres
};

// x, y: snapped coordinates, |.| <= 2^22; z: camera-space depth of the vertices.  False for a face of zero area.
__device__ __forceinline__ bool tri_setup(const int x[3], const int y[3], const float z[3], long long area2, int H,
                                          int W, Tri &t) {
    if (area2 == 0) return false;
    const long long s = area2 > 0 ? 1 : -1;
#pragma unroll
    for (int k = 0; k < 3; ++k) {  // edge a -> b opposite vertex k
        const int a = (k + 1) % 3, b = (k + 2) % 3;
        const long long A = -s * ((long long)y[b] - y[a]), B = s * ((long long)x[b] - x[a]);
        // the interior is where e grows: to the right of the edge (A > 0: a left edge) or, for a horizontal edge, below
        // it (B > 0 with y down: a top edge)
        const bool owns = A > 0 || (A == 0 && B > 0);
        t.A[k] = A;
        t.B[k] = B;
        t.bias[k] = owns ? 0 : 1;
        t.C[k] = -(A * x[a] + B * y[a]) - t.bias[k];
        t.iz[k] = 1.0f / z[k];
    }
    t.area = (float)(s * area2);
    const int xmin = min(x[0], min(x[1], x[2])), xmax = max(x[0], max(x[1], x[2]));
    const int ymin = min(y[0], min(y[1], y[2])), ymax = max(y[0], max(y[1], y[2]));
    // centres 256 c + 128 inside [min, max]: c from ceil((min - 128) / 256) to floor((max - 128) / 256)
    const int c0 = max(0, (xmin + 127) >> 8), c1 = min(W - 1, (xmax - 128) >> 8);
    const int r0 = max(0, (ymin + 127) >> 8), r1 = min(H - 1, (ymax - 128) >> 8);
    t.c0 = c0;
    t.r0 = r0;
    t.bw = c1 - c0 + 1;
    t.count = (c1 >= c0 && r1 >= r0) ? t.bw * (r1 - r0 + 1) : 0;
    return true;
}

// Centres start, start + stride, ... of the face's box: the one coverage and depth routine of both tiers.
__device__ __forceinline__ void raster_box(const Tri &t, unsigned face, int W, unsigned long long *__restrict__ zbuf,
                                           int start, int stride) {
#pragma clang fp contract(off)  // the same fp32 operations wherever this is inlined: both tiers give the same bits
    for (int i = start; i < t.count; i += stride) {
        const int r = t.r0 + i / t.bw, c = t.c0 + i % t.bw;
        const long long px = 256ll * c + 128, py = 256ll * r + 128;
        const long long e0 = t.A[0] * px + t.B[0] * py + t.C[0];
        const long long e1 = t.A[1] * px + t.B[1] * py + t.C[1];
        const long long e2 = t.A[2] * px + t.B[2] * py + t.C[2];
        if ((e0 | e1 | e2) < 0) continue;
        const float b0 = (float)(e0 + t.bias[0]) / t.area, b1 = (float)(e1 + t.bias[1]) / t.area,
                    b2 = (float)(e2 + t.bias[2]) / t.area;
        const float z = 1.0f / ((b0 * t.iz[0] + b1 * t.iz[1]) + b2 * t.iz[2]);
        atomicMin(&zbuf[(size_t)r * W + c], ((unsigned long long)__float_as_uint(z) << 32) | face);
    }
}

__device__ __forceinline__ long long doubled_area(const int x[3], const int y[3]) {
    return ((long long)x[1] - x[0]) * ((long long)y[2] - y[0]) - ((long long)x[2] - x[0]) * ((long long)y[1] - y[0]);
}

__global__ __launch_bounds__(256) void fill_kernel(size_t npix, unsigned long long *__restrict__ keys, int F,
                                                   int *__restrict__ counters, int *__restrict__ out_status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < npix) keys[i] = ~0ull;
    if (i < (size_t)3 * F) counters[i] = 0;  // list lengths [F], then status [F,2]
    if (out_status && i < (size_t)2 * F) out_status[i] = 0;
}

__global__ __launch_bounds__(256) void project_kernel(int V, const float *__restrict__ vertices,
                                                      const float *__restrict__ transl, const float *__restrict__ Ks,
                                                      const float *__restrict__ Es, float *__restrict__ zcam,
                                                      int *__restrict__ screen, int *__restrict__ out_screen) {
#pragma clang fp contract(off)  // plain fp32 operations in source order, as project_zbuffer_kernel
    const int v = blockIdx.x * blockDim.x + threadIdx.x, f = blockIdx.y;
    if (v >= V) return;
    const size_t at = (size_t)f * V + v;
    const float *p = vertices + at * 3, *E = Es + (size_t)f * 16, *K = Ks + (size_t)f * 9;
    float wx = p[0], wy = p[1], wz = p[2];
    if (transl) {
        wx += transl[f * 3 + 0];
        wy += transl[f * 3 + 1];
        wz += transl[f * 3 + 2];
    }
    const float X = E[0] * wx + E[1] * wy + E[2] * wz + E[3];
    const float Y = E[4] * wx + E[5] * wy + E[6] * wz + E[7];
    const float Z = E[8] * wx + E[9] * wy + E[10] * wz + E[11];
    const float u = K[0] * X / Z + K[2], w = K[4] * Y / Z + K[5];
    // far outside the guard band (or not a number, behind the camera) pins to +-2^30: setup drops such a face
    const float lim = 1073741824.0f;
    const int su = (int)rintf(fminf(fmaxf(u * 256.0f, -lim), lim)), sv = (int)rintf(fminf(fmaxf(w * 256.0f, -lim), lim));
    zcam[at] = Z;
    screen[at * 2 + 0] = su;
    screen[at * 2 + 1] = sv;
    if (out_screen) {
        out_screen[at * 2 + 0] = su;
        out_screen[at * 2 + 1] = sv;
    }
}

__global__ __launch_bounds__(256) void setup_kernel(int V, int T, int H, int W, const int *__restrict__ faces,
                                                    const float *__restrict__ vertices, const float *__restrict__ Es,
                                                    const float *__restrict__ zcam, const int *__restrict__ screen,
                                                    float znear, int cull, int small_box, float k0, float k1, float k2,
                                                    float *__restrict__ shade, float *__restrict__ out_shade,
                                                    int *__restrict__ list, int *__restrict__ counts,
                                                    int *__restrict__ status, unsigned long long *__restrict__ zbuf) {
    const int face = blockIdx.x * blockDim.x + threadIdx.x, f = blockIdx.y;
    if (face >= T) return;
    const size_t sat = ((size_t)f * T + face) * 3;
    float sh[3] = {0.0f, 0.0f, 0.0f};
    bool keep = false;
    Tri t;
    t.count = 0;
    const int id[3] = {faces[face * 3 + 0], faces[face * 3 + 1], faces[face * 3 + 2]};
    if ((unsigned)id[0] < (unsigned)V && (unsigned)id[1] < (unsigned)V && (unsigned)id[2] < (unsigned)V) {
        const float *zc = zcam + (size_t)f * V;
        const int *sc = screen + (size_t)f * V * 2;
        float pz[3];
        int x[3], y[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            pz[k] = zc[id[k]];
            x[k] = sc[(size_t)id[k] * 2 + 0];
            y[k] = sc[(size_t)id[k] * 2 + 1];
        }
        if (!(pz[0] >= znear && pz[1] >= znear && pz[2] >= znear)) {
            atomicAdd(&status[f * 2 + 0], 1);
        } else if (max(max(abs(x[0]), abs(x[1])), max(max(abs(x[2]), abs(y[0])), max(abs(y[1]), abs(y[2])))) > kGuard) {
            atomicAdd(&status[f * 2 + 1], 1);
        } else {
            const long long area2 = doubled_area(x, y);
            const bool front = area2 < 0;
            if ((front || !cull) && tri_setup(x, y, pz, area2, H, W, t)) {
                keep = true;
                // flat shade in camera space; the headlight l = (0, 0, -1), so n . l = -n_z (n reversed for a back face).
                // The edges p_k - p_0 are taken as E (v_k - v_0): the world-space difference is exact to an ulp of the
                // EDGE (transl and E's translation cancel), where p_k - p_0 from the projected points carries the
                // rounding of the whole camera-space position, which tilts the normal of a sliver face visibly
                const float *w = vertices + (size_t)f * V * 3, *E = Es + (size_t)f * 16;
                const float *w0 = w + (size_t)id[0] * 3, *w1 = w + (size_t)id[1] * 3, *w2 = w + (size_t)id[2] * 3;
                const float dax = w1[0] - w0[0], day = w1[1] - w0[1], daz = w1[2] - w0[2];
                const float dbx = w2[0] - w0[0], dby = w2[1] - w0[1], dbz = w2[2] - w0[2];
                const float ax = E[0] * dax + E[1] * day + E[2] * daz, ay = E[4] * dax + E[5] * day + E[6] * daz,
                            az = E[8] * dax + E[9] * day + E[10] * daz;
                const float bx = E[0] * dbx + E[1] * dby + E[2] * dbz, by = E[4] * dbx + E[5] * dby + E[6] * dbz,
                            bz = E[8] * dbx + E[9] * dby + E[10] * dbz;
                const float nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
                const float len = sqrtf(nx * nx + ny * ny + nz * nz);
                const float ndotl = len > 0.0f ? fmaxf(0.0f, (front ? -nz : nz) / len) : 0.0f;
                sh[0] = fminf(1.0f, k0 * ndotl);
                sh[1] = fminf(1.0f, k1 * ndotl);
                sh[2] = fminf(1.0f, k2 * ndotl);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        shade[sat + c] = sh[c];
        if (out_shade) out_shade[sat + c] = sh[c];
    }
    if (!keep || t.count == 0) return;
    if (t.count <= small_box) {
        raster_box(t, (unsigned)face, W, zbuf + (size_t)f * H * W, 0, 1);
    } else {
        const int slot = atomicAdd(&counts[f], 1);  // every face appends at most once: slot < T
        list[(size_t)f * T + slot] = face;
    }
}

__global__ __launch_bounds__(256) void large_kernel(int V, int T, int H, int W, const int *__restrict__ faces,
                                                    const float *__restrict__ zcam, const int *__restrict__ screen,
                                                    const int *__restrict__ list, const int *__restrict__ counts,
                                                    unsigned long long *__restrict__ zbuf) {
    const int f = blockIdx.y;
    const int n = min(counts[f], T);
    const int wave = blockIdx.x * (blockDim.x / kWave) + (threadIdx.x / kWave), lane = threadIdx.x % kWave;
    const int waves = gridDim.x * (blockDim.x / kWave);
    const float *zc = zcam + (size_t)f * V;
    const int *sc = screen + (size_t)f * V * 2;
    for (int k = wave; k < n; k += waves) {
        const int face = list[(size_t)f * T + k];  // appended by setup_kernel: ids in range, not dropped, area != 0
        int x[3], y[3];
        float z[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int id = faces[face * 3 + j];
            x[j] = sc[(size_t)id * 2 + 0];
            y[j] = sc[(size_t)id * 2 + 1];
            z[j] = zc[id];
        }
        Tri t;
        if (tri_setup(x, y, z, doubled_area(x, y), H, W, t))
            raster_box(t, (unsigned)face, W, zbuf + (size_t)f * H * W, lane, kWave);
    }
}

__global__ __launch_bounds__(256) void resolve_kernel(size_t npix, size_t frame_pixels, int T,
                                                      const unsigned long long *__restrict__ keys,
                                                      const float *__restrict__ shade, const float *__restrict__ frames,
                                                      int channels, float bg0, float bg1, float bg2,
                                                      float *__restrict__ rgb, float *__restrict__ depth,
                                                      int *__restrict__ face_index) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const unsigned long long key = keys[i];
    float r = bg0, g = bg1, b = bg2, z = 0.0f;
    int face = -1;
    if (key != ~0ull) {
        face = (int)(unsigned)key;
        z = __uint_as_float((unsigned)(key >> 32));
        const float *s = shade + ((i / frame_pixels) * T + face) * 3;
        r = s[0], g = s[1], b = s[2];
    } else if (frames) {
        const float *p = frames + i * channels;
        r = p[0], g = p[1], b = p[2];
    }
    rgb[i * 3 + 0] = r;
    rgb[i * 3 + 1] = g;
    rgb[i * 3 + 2] = b;
    if (depth) depth[i] = z;
    if (face_index) face_index[i] = face;
}

struct Slabs {
    unsigned long long *keys;
    float *zcam, *shade;
    int *screen, *list, *counters;
    size_t bytes;
};

Slabs carve(void *workspace, int F, int V, int T, int H, int W) {
    Carver c(workspace);
    Slabs s;
    s.keys = c.take<unsigned long long>((size_t)F * H * W);
    s.zcam = c.take<float>((size_t)F * V);
    s.screen = c.take<int>((size_t)F * V * 2);
    s.shade = c.take<float>((size_t)F * T * 3);
    s.list = c.take<int>((size_t)F * T);
    s.counters = c.take<int>((size_t)F * 3);
    s.bytes = c.total();
    return s;
}

bool sizes_ok(int F, int V, int T, int H, int W) {
    return F > 0 && V > 0 && T > 0 && H > 0 && W > 0 && H <= kMaxExtent && W <= kMaxExtent && F <= 65535 &&
           (long long)F * H * W <= (1ll << 38) && (long long)T * 3 < (1ll << 31);
}

}  // namespace mesh
}  // namespace amav

using namespace amav;
using namespace amav::mesh;

extern "C" size_t amav_mesh_overlay_workspace_bytes(int F, int V, int T, int H, int W) {
    if (!sizes_ok(F, V, T, H, W)) return 0;
    return carve(nullptr, F, V, T, H, W).bytes;
}

extern "C" int amav_mesh_overlay(const amav_mesh_overlay_args *a, void *stream_) {
    AMAV_REQUIRE(a != nullptr, "amav_mesh_overlay: args is NULL");
    const int F = a->num_frames, V = a->num_verts, T = a->num_faces, H = a->height, W = a->width;
    AMAV_REQUIRE(sizes_ok(F, V, T, H, W),
                 "amav_mesh_overlay: bad sizes (F=%d V=%d T=%d H=%d W=%d; all positive, H and W <= 16384, F <= 65535)", F, V,
                 T, H, W);
    AMAV_REQUIRE(a->vertices && a->faces && a->K && a->E && a->out_rgb && a->workspace, "amav_mesh_overlay: NULL pointer");
    AMAV_REQUIRE(!a->frames || a->frame_channels == 3 || a->frame_channels == 4,
                 "amav_mesh_overlay: frame_channels %d, expected 3 or 4", a->frame_channels);
    AMAV_REQUIRE(a->znear > 0.0f, "amav_mesh_overlay: znear must be positive");
    const uintptr_t words = reinterpret_cast<uintptr_t>(a->vertices) | reinterpret_cast<uintptr_t>(a->faces) |
                            reinterpret_cast<uintptr_t>(a->transl) | reinterpret_cast<uintptr_t>(a->K) |
                            reinterpret_cast<uintptr_t>(a->E) | reinterpret_cast<uintptr_t>(a->frames) |
                            reinterpret_cast<uintptr_t>(a->out_rgb) | reinterpret_cast<uintptr_t>(a->out_depth) |
                            reinterpret_cast<uintptr_t>(a->out_face_index) | reinterpret_cast<uintptr_t>(a->out_screen) |
                            reinterpret_cast<uintptr_t>(a->out_status) | reinterpret_cast<uintptr_t>(a->out_shade);
    AMAV_REQUIRE((words & 3) == 0 && aligned16(a->workspace),
                 "amav_mesh_overlay: misaligned pointer (tensors 4-byte, workspace 16-byte aligned)");
    const size_t need = amav_mesh_overlay_workspace_bytes(F, V, T, H, W);
    if (a->workspace_bytes < need)
        return fail(AMAV_ERR_WORKSPACE, "amav_mesh_overlay: workspace %zu < required %zu", a->workspace_bytes, need);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const Slabs s = carve(a->workspace, F, V, T, H, W);
    int *counts = s.counters, *status = a->out_status ? a->out_status : s.counters + F;
    const size_t npix = (size_t)F * H * W;
    const size_t fill = npix > (size_t)3 * F ? npix : (size_t)3 * F;
    const int small_box = a->small_box < 0 ? AMAV_MESH_SMALL_BOX : a->small_box;
    fill_kernel<<<blocks_for((long long)fill), 256, 0, stream>>>(npix, s.keys, F, s.counters, a->out_status);
    project_kernel<<<dim3(blocks_for(V), (unsigned)F), 256, 0, stream>>>(V, a->vertices, a->transl, a->K, a->E, s.zcam,
                                                                         s.screen, a->out_screen);
    setup_kernel<<<dim3(blocks_for(T), (unsigned)F), 256, 0, stream>>>(
        V, T, H, W, a->faces, a->vertices, a->E, s.zcam, s.screen, a->znear, a->cull_backfaces, small_box, a->shade_k[0], a->shade_k[1],
        a->shade_k[2], s.shade, a->out_shade, s.list, counts, status, s.keys);
    large_kernel<<<dim3(kLargeBlocks, (unsigned)F), 256, 0, stream>>>(V, T, H, W, a->faces, s.zcam, s.screen, s.list,
                                                                      counts, s.keys);
    resolve_kernel<<<blocks_for((long long)npix), 256, 0, stream>>>(npix, (size_t)H * W, T, s.keys, s.shade, a->frames,
                                                                    a->frame_channels, a->background[0], a->background[1],
                                                                    a->background[2], a->out_rgb, a->out_depth,
                                                                    a->out_face_index);
    return check_launch("amav_mesh_overlay");
}
