/*
 * amav.h -- C ABI of libamav_hip.so: the MI355X (gfx950) kernels of the audio-driven avatar rendering hot path.
 *
 * The reference (liubingqi7/audio-motion-avatar) has no FFI layer: its native work is reached through
 * third-party Python wheels.  Each entry point below replaces one of those call sites (cited per function,
 * paths relative to the reference root) and is what a ctypes binding on the reference side would bind
 * (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - Every pointer named *_dev / documented "device" is a caller-owned HIP device pointer (a torch tensor's
 *     data_ptr()).  The library never allocates, frees or retains device memory: scratch is a caller-provided
 *     workspace sized by the matching *_workspace_bytes() query.
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream).  All work is enqueued
 *     on it; no call synchronises unless documented.  No hipMalloc / hipFree / host sync on the hot path, so every
 *     launch function may be captured into a hipGraph.
 *   - Return value: 0 = AMAV_OK, negative = error; amav_last_error() returns a thread-local message.
 *   - All floating-point data is IEEE fp32; indices are int32 unless stated.
 *   - Thread-safe for distinct streams/workspaces; no mutable global state.
 *   - The Python binding (audio-motion-avatar_amd/_lib.py) is generated from this file at import.  Keep to the forms
 *     used here -- `typedef struct amav_x {...} amav_x;`, plain prototypes, integer #defines -- and to the *_dev suffix:
 *     a typed pointer parameter is bound as a device address only when its name ends in _dev (any other `float *` /
 *     `int32_t *` parameter is a host out-parameter); what the parser does not recognise fails the import.
 */
#ifndef AMAV_H
#define AMAV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AMAV_OK 0
#define AMAV_ERR_INVALID_ARG (-1)
#define AMAV_ERR_LAUNCH (-2)
#define AMAV_ERR_WORKSPACE (-3)
#define AMAV_ERR_NO_DEVICE (-4)

#define AMAV_TILE 16          /* rasterizer tile edge, pixels (fixed by the algorithm being replaced) */
#define AMAV_GAUSS_STRIDE 16  /* floats per packed Gaussian record written by amav_triplane_sample_decode */

const char *amav_version(void);
const char *amav_last_error(void);
/* Number of visible HIP devices, or a negative error.  Does not create a context on a device. */
int amav_device_count(void);
/* Process-wide arithmetic selection, effective from the next call on (the environment variables AMAV_ATTN / AMAV_LBS give
 * the defaults; there is no reference counterpart: the reference computes these products in library fp32).
 *   name "attn": "fp16" (fp16 x 2 split products, default) | "bf16" (bf16 x 3) | "f32" (exact products on the fp32 MFMA)
 *   name "lbs":  "split" (fp16 x 2 split blend product, default) | "f32" (fp32 MFMA)
 * value "default" returns to the environment's choice.  Not to be changed while calls of that entry point are in
 * flight on another thread (a call reads it more than once: workspace layout, then launch). */
int amav_set_option(const char *name, const char *value);

/* Timing events for callers without a HIP binding of their own (thin hipEvent wrappers; elapsed synchronises). */
int amav_event_create(void **event);
int amav_event_destroy(void *event);
int amav_event_record(void *event, void *stream);
int amav_event_elapsed_ms(void *start, void *stop, float *ms);

/* One per-Gaussian (or per-point) attribute: element (f, i) lives at ptr[f * frame_stride + i * elem_stride].
 * frame_stride = 0 broadcasts one set of Gaussians to every frame (render_multi_view, renderer.py:431-445). */
typedef struct amav_attr {
    const float *ptr;
    int64_t frame_stride; /* in floats */
    int32_t elem_stride;  /* in floats */
    int32_t _pad;
} amav_attr;

/* ------------------------------------------------------------------------------------------------------------
 * Camera.  Replaces the per-frame host code of render_one (src/models/renderer.py:486-510) and
 * getWorld2View2_torch / getProjectionMatrix_torch / focal2fov_torch (src/utils/graphic_utils.py:67-78,103-145):
 * K [F,3,3], E [F,4,4] (row-major, device) -> viewmatrix [F,16] = E^T, projmatrix [F,16] = (K_ndc E)^T (both as
 * the rasterizer reads them: column-major), tanfov [F,2] = (W/(2fx), H/(2fy)), campos [F,3].  No host sync.
 */
int amav_camera_from_intrinsics(int num_frames, const float *K_dev, const float *E_dev, int height, int width,
                                float znear, float zfar, float *viewmatrix_dev, float *projmatrix_dev,
                                float *tanfov_dev, float *campos_dev, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Gaussian tile rasterizer, forward, all frames of a shard in one call.
 * Replaces GaussianRasterizer.forward of diff_gaussian_rasterization as called at src/models/renderer.py:555-566
 * (preprocess, per-tile binning, per-tile (depth, index) sort, 16x16-tile front-to-back alpha compositing) and,
 * with apply_activations = 1, the torch ops of renderer.py:532-547,568 that surround it.
 */
typedef struct amav_raster_args {
    int32_t num_frames, num_gaussians, height, width;
    amav_attr means3d;   /* 3 floats: world position */
    amav_attr rotations; /* 4 floats: unit quaternion (w,x,y,z); NOT normalised here (renderer.py:333 did it) */
    amav_attr scales;    /* 3 floats */
    amav_attr opacities; /* 1 float  */
    amav_attr colors;    /* 3 floats (colors_precomp; colours from SH coefficients come from amav_sh_colors below) */
    const float *viewmatrix; /* device [F,16] */
    const float *projmatrix; /* device [F,16] */
    const float *tanfov;     /* device [F,2]  */
    float bg[3];             /* background colour (renderer.py:512-514: white by default) */
    float scale_modifier;    /* renderer.py:522: 1.0 */
    /* 1: scales = min(exp(s - scale_bias), scale_max), opacities = sigmoid(o - opacity_bias),
     *    colors = clamp(c, 0, 1) are applied on load (renderer.py:532-533,547 with SCALE_BIAS 3.9, cap 0.1,
     *    OPACITY_BIAS 0.0).  0: inputs are already activated (the op-level GaussianRasterizer contract). */
    int32_t apply_activations;
    float scale_bias, scale_max, opacity_bias;
    int32_t antialiasing; /* renderer.py:529: False */
    int32_t clamp_output; /* 1: clamp RGB to [0,1] (renderer.py:568) */
    /* outputs (device).  out_rgba is required: [F,H,W,4] = (R,G,B,alpha = 1 - T_final), pixel-interleaved so a tile
     * row is one 256-byte run.  out_inv_depth [F,H,W] and out_radii [F,N] (int32) may be NULL. */
    float *out_rgba;
    float *out_inv_depth;
    int32_t *out_radii;
    /* scratch */
    void *workspace;
    size_t workspace_bytes;
    int64_t instance_capacity; /* instances the workspace was sized for; each frame owns capacity / F of them */
    /* optional hipEvent_t pair (amav_event_create) recorded on `stream` right before / after the blend kernel, so a
     * caller can time the dominant kernel live (bench.py roofline); NULL = off */
    void *profile_start_event;
    void *profile_stop_event;
    /* diagnostic only: device buffer of num_frames * tiles * 6 uint64 that receives per-tile-wave clock stamps
     * (start, ranges read, sorted, blended, stored) and the list length; NULL in production */
    void *debug_stamps;
    /* optional: the tile-sparse wire buffer of the frame exchange (amav_frames_wire_bytes(F, H, W, wire_capacity_tiles)
     * bytes, 16-byte aligned), written by the rasterizer itself: every tile that holds a Gaussian is stored (uint8 RGB,
     * quantised as amav_frames_to_rgb8 does, of the clamped colour), the others are background -- the result of
     * amav_frames_pack_tiles with the rasterizer's tile counts as hint, without the pass over the fp32 frames.  Needs
     * clamp_output = 1.  Tiles beyond the capacity are dropped and header.count > capacity tells the receivers
     * (amav_frames_unpack_tiles raises its status flag).  NULL = off. */
    void *wire;
    size_t wire_bytes;
    int64_t wire_capacity_tiles;
} amav_raster_args;

size_t amav_rasterize_workspace_bytes(int num_frames, int num_gaussians, int height, int width,
                                      int64_t instance_capacity);
int amav_rasterize_forward(const amav_raster_args *args, void *stream);
/* Synchronises `stream`, then reports the last forward on this workspace: the total instance count, the largest
 * per-frame count, and whether some frame exceeded its region (instance_capacity / num_frames instances each), in
 * which case the outputs are invalid and the caller must retry with instance_capacity >= num_frames *
 * *max_frame_instances.  The only rasterizer call that waits on the device. */
int amav_rasterize_status(const void *workspace, int64_t *total_instances, int64_t *max_frame_instances,
                          int32_t *overflow, void *stream);

/* Gaussian tile rasterizer, backward: diff_gaussian_rasterization's backward (the reference's stage-2 training,
 * src/models/lightning_model_wrapper.py:132-156) for the forward that `fwd` describes, which must be the LAST
 * amav_rasterize_forward on fwd->workspace, with the same inputs, sizes and settings (the backward reads its tile
 * lists and blend records).  Not supported: antialiasing, a decoding or wire forward.
 * Gradients of the five Gaussian inputs, dense [F,N,width] fp32 (frame stride 0 inputs get one row per frame; the
 * caller sums them).  grad_rgba is dL/d out_rgba [F,H,W,4] of an UNCLAMPED forward (clamp_output = 0): alpha is
 * differentiable, inv_depth and the background are not.  The min(0.99, .) clamp of alpha is passed through (upstream's
 * convention); the tanfov clamp of the view-space mean and the activations (apply_activations) are differentiated as
 * torch autograd does.  Deterministic: no float atomics, bitwise the same gradients from run to run.
 * scratch: amav_rasterize_backward_bytes(F, N, max_frame_instances) bytes, max_frame_instances = the largest per-frame
 * instance count amav_rasterize_status reported for that forward (a larger value is fine).  A forward that overflowed
 * (max_frame_instances > instance_capacity / F) is refused.  No host synchronisation. */
typedef struct amav_raster_backward_args {
    const float *grad_rgba;        /* device [F,H,W,4] */
    float *grad_means3d;           /* device [F,N,3] */
    float *grad_rotations;         /* device [F,N,4] */
    float *grad_scales;            /* device [F,N,3] */
    float *grad_opacities;         /* device [F,N,1] */
    float *grad_colors;            /* device [F,N,3] */
    int64_t max_frame_instances;   /* from amav_rasterize_status after the forward */
    void *scratch;
    size_t scratch_bytes;
    /* optional, device [F,H,W]: 1 - T_final of the backward's replay of the blend (equals the forward's alpha channel
     * bit for bit); NULL = off */
    float *debug_alpha;
} amav_raster_backward_args;
size_t amav_rasterize_backward_bytes(int num_frames, int num_gaussians, int64_t max_frame_instances);
int amav_rasterize_backward(const amav_raster_args *fwd, const amav_raster_backward_args *bwd, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * View-dependent colours from spherical-harmonic coefficients: the SH branch of render_one (src/models/renderer.py:
 * 540-545 with eval_sh, src/utils/graphic_utils.py:707-762), which the reference's own 3-channel colour head never
 * reaches but a caller with 3 * (degree+1)^2 colour channels does.  For every frame f and Gaussian i
 *     d = (p - campos[f]) / |p - campos[f]|,   colours[f,i,c] = max(sum_k B_k(d) * sh[k][c] + 0.5, 0)
 * with the real SH basis of degree 0..4 in the reference's order and signs; there is no clamp at 1.  The result is what
 * amav_raster_args.colors takes with apply_activations = 0.  A Gaussian exactly at the camera centre gives NaN, as in
 * the reference (the rasterizer culls it at the near plane).
 * amav_sh_colors_backward: grad_sh[f,i,k*3+c] = gate * grad_colors[f,i,c] * B_k(d) with gate = (the value before the
 * clamp > 0), replayed with the forward's own arithmetic; coefficients k >= (degree+1)^2 are written as zeros, so the
 * buffer needs no initialisation.  grad_means3d (may be NULL) goes through d(d)/d(p) = (I - d d^T) / |p - campos|.
 * Both gradients are dense rows per frame: a frame-stride-0 input gets one row per frame and the caller sums them, as
 * for amav_rasterize_backward.  campos gets no gradient.
 * No workspace, no allocation, no host synchronisation, no atomics: bitwise the same results from run to run.
 * Refused (AMAV_ERR_INVALID_ARG, before any launch): negative counts, degree outside 0..4, num_coeffs < (degree+1)^2, an
 * element stride below the attribute's width, a NULL required pointer.  num_frames = 0 or num_gaussians = 0 return 0. */
typedef struct amav_sh_args {
    int32_t num_frames, num_gaussians, degree, num_coeffs; /* degree 0..4; num_coeffs stored per Gaussian >= (degree+1)^2 */
    amav_attr means3d;   /* 3 floats */
    amav_attr sh;        /* 3 * num_coeffs floats, coefficient-major: coefficient k, channel c at k * 3 + c (the layout of
                            colors.reshape(N,-1,3) at renderer.py:541 and of upstream's shs [N,K,3]) */
    const float *campos; /* device [F,3], from amav_camera_from_intrinsics */
} amav_sh_args;
int amav_sh_colors(const amav_sh_args *a, float *colors_dev, void *stream);
int amav_sh_colors_backward(const amav_sh_args *a, const float *grad_colors_dev, float *grad_sh_dev,
                            float *grad_means3d_dev, void *stream);

/* amav_triplane_sample_decode_indexed + amav_rasterize_forward in one call: the packed Gaussian records are decoded
 * from the inputs below into the buffer the attributes of `args` view -- which must be the packed views
 * (xyz|opacity|rot|scale|color at float offsets 0, 3, 4, 8, 12, element stride 16) of ONE contiguous [F,N,16] buffer,
 * 16-B aligned -- and then rasterised.  Same records, frames, instance counts and workspace as the two calls.  For
 * shards of many frames whose binning block keeps its records in LDS (no out_radii, images up to 255 x 255 tiles, N
 * small enough) the decode runs inside the per-frame binning block and the records are not read back; otherwise the
 * two launches are enqueued.  No allocation and no host synchronisation (HIP-graph capturable). */
typedef struct amav_decode_source {
    int32_t resolution, num_verts;  /* R of the projected planes, V of the posed vertices */
    const float *proj;              /* [F,3,R,R,16] from amav_triplane_project(_region), 16-B aligned */
    const float *vertices;          /* [F,V,3] posed vertices */
    const int32_t *idx4;            /* [N,4] subdivision table, 16-B aligned */
    const float *transl;            /* [F,3] or NULL */
    float radius;
    const float *head_w_point;      /* [16,4], 16-B aligned */
} amav_decode_source;
int amav_rasterize_decode_forward(const amav_raster_args *args, const amav_decode_source *src, void *stream);

/* Rendered frames -> on-wire format of the multi-GPU exchange: fp32 RGBA [pixels,4] -> uint8 RGB [pixels,3] with the
 * reference's own quantisation (src/main2.py:351: (frame * 255).astype(uint8), truncating). num_pixels % 4 == 0. */
int amav_frames_to_rgb8(int64_t num_pixels, const float *rgba_dev, uint8_t *out_rgb8_dev, void *stream);

/* Tile-sparse form of the same exchange (lossless): an avatar frame is mostly background, so only the 16x16 tiles
 * that differ from the background colour are put on the wire.  One wire buffer per rank:
 *   int32 header[16] = {magic, stored tiles, capacity, F, tiles per frame, H, W, background as 0x00BBGGRR, 0...}
 *   int32 stored tiles per frame [F]
 *   int32 slot of every tile [F * tiles per frame]   (-1: background; else index into the payload)
 *   uint8 payload [capacity][16*16*3]                (16-byte aligned; tiles in (frame, tile) order)
 * amav_frames_wire_bytes: size of such a buffer (0 on bad arguments).
 * amav_frames_pack_tiles: fp32 RGBA frames [F,H,W,4] -> wire (quantised as amav_frames_to_rgb8 does); tiles beyond
 *   `capacity_tiles` are dropped and header[1] > header[2] tells every receiver.  capacity 0 only counts.
 *   tile_hint (optional, int32 [F * tiles per frame]): zero = the caller knows the tile is pure background, e.g.
 *   amav_rasterize_tile_counts (a tile without Gaussians); with a hint the frames are read for the stored tiles only.
 * amav_frames_unpack_tiles: `num_buffers` gathered wire buffers (rank r at wire_all + r * wire_stride) -> dense uint8
 *   RGB [num_buffers * F, H, W, 3]; status[0] |= 1 if any buffer was truncated or is not a wire buffer (the caller
 *   re-packs with more room, as with the rasterizer's instance capacity).  No host synchronisation in either call.
 * amav_frames_unpack_tiles_delta: the same into an output buffer that is REUSED from step to step (width % 16 == 0).
 *   tile_state int32 [num_buffers * F * tiles per frame] belongs to that output buffer and records what every tile
 *   of it holds: the background word 0x00BBGGRR it was last cleared to, or -1 (rendered pixels / unknown -- a fresh
 *   buffer's state is all -1).  Only the tiles stored on the wire, and the tiles that are background now but do not
 *   hold this background yet, are written; the state is updated in the same launch. */
/* Per-tile Gaussian list lengths of the last amav_rasterize_forward on this workspace, int32 [F * tiles per frame]
 * (frame-major, tiles row-major; all ones after an instance-capacity overflow).  Same sizes as the forward call. */
int amav_rasterize_tile_counts(const void *workspace, int num_frames, int num_gaussians, int height, int width,
                               int64_t instance_capacity, int32_t *out_counts_dev, void *stream);
size_t amav_frames_wire_bytes(int num_frames, int height, int width, int64_t capacity_tiles);
int amav_frames_pack_tiles(int num_frames, int height, int width, const float *rgba_dev, const float *background_host3,
                           const int32_t *tile_hint_dev, int64_t capacity_tiles, void *wire_dev, size_t wire_bytes,
                           void *stream);
int amav_frames_unpack_tiles(int num_buffers, int num_frames, int height, int width, int64_t capacity_tiles,
                             const void *wire_all_dev, size_t wire_stride, uint8_t *out_rgb8_dev, int32_t *status_dev,
                             void *stream);
int amav_frames_unpack_tiles_delta(int num_buffers, int num_frames, int height, int width, int64_t capacity_tiles,
                                   const void *wire_all_dev, size_t wire_stride, uint8_t *out_rgb8_dev,
                                   int32_t *tile_state_dev, int32_t *status_dev, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * SMPL-X forward + linear blend skinning for F frames.
 * Replaces smplx.SMPLX.forward -> smplx.lbs.lbs as called at src/models/renderer.py:261-274 (no transl;
 * use_pca=False).  Model constants are immutable device tables prepared once by the host mirror
 * (audio-motion-avatar_amd/body_model.py) from the SMPL-X arrays:
 *   v_template [V,3]; blend [ceil(V/32), KB, 3, 32] with KB = n_coeff + (J-1)*9: for every tile of 32 vertices (the
 *   last one zero padded) the KB blend rows as x / y / z planes, rows 0..n_coeff-1 = shape + expression directions,
 *   then posedirs; 16-byte aligned; j_template [J,3] = J_regressor v_template; j_dirs [J*3, n_coeff] = J_regressor applied to
 *   the shape directions; parents [J]; skin_idx / skin_w [V, skin_k]: the non-zero LBS weights of each vertex in
 *   ascending joint order, padded with weight 0.
 */
typedef struct amav_body_tables {
    int32_t num_verts, num_joints, num_coeffs, skin_k;
    const float *v_template;
    const float *blend;
    const float *j_template;
    const float *j_dirs;
    const int32_t *parents;
    const int32_t *skin_idx;
    const float *skin_w;
    const void *blend_split; /* amav_lbs_prepare_blend_split's buffer, or NULL (the blend product then runs on fp32 MFMA) */
} amav_body_tables;

/* The blend table as two fp16 parts (scaled by one power of two) in the fragment order of the 16-bit MFMA: with it
 * amav_lbs_forward computes the [F, KB] x [KB, 3V] blend product as three fp16 partial products per fp32 product with
 * fp32 accumulation (the fp32 result to 2^-22, 3x faster than on fp32 MFMA; every frame's features get their own
 * power-of-two scale).  Prepare once per model into a 256-byte aligned device buffer of amav_lbs_blend_split_bytes and
 * put its address into tables->blend_split (`blend` must stay valid too: short batches use it).  AMAV_LBS=f32 in the
 * environment ignores blend_split. */
size_t amav_lbs_blend_split_bytes(const amav_body_tables *tables);
int amav_lbs_prepare_blend_split(const amav_body_tables *tables, void *out_dev, size_t out_bytes, void *stream);

size_t amav_lbs_workspace_bytes(int num_frames, const amav_body_tables *tables);
/* full_pose [F, J*3] axis-angle (pose_mean already added), coeffs [F, n_coeff] (betas then expression).
 * out_vertices [F,V,3]; out_joint_transforms [F,J,12] (rows of the 3x4 rest-pose-removed transforms) may be NULL. */
int amav_lbs_forward(int num_frames, const amav_body_tables *tables, const float *full_pose_dev,
                     const float *coeffs_dev, float *out_vertices_dev, float *out_joint_transforms_dev,
                     void *workspace, size_t workspace_bytes, void *stream);

/* The same with the pose and the coefficients as the caller of the SMPL-X layer holds them -- the keyword arguments of
 * renderer.py:261-272 (global_orient, body_pose, jaw_pose, leye_pose, reye_pose, left_hand_pose, right_hand_pose / betas,
 * expression) -- concatenated in the given order as the first kernel loads them, plus smplx's `full_pose += pose_mean`:
 * what smplx does with torch.cat / add / torch.cat (three launches) in front of the joint chain.  Part p holds
 * pose_joints[p] axis-angle triples per frame, pose_stride[p] floats apart between frames; the joint counts must add up
 * to tables->num_joints and the coefficient counts to tables->num_coeffs.  pose_mean [J*3] may be NULL. */
typedef struct amav_pose_parts {
    int32_t num_pose_parts;  /* 1..8 */
    int32_t num_coeff_parts; /* 1..4 */
    const float *pose[8];
    int32_t pose_joints[8];
    int64_t pose_stride[8];
    const float *pose_mean;
    const float *coeff[4];
    int32_t coeff_count[4];
    int64_t coeff_stride[4];
} amav_pose_parts;
int amav_lbs_forward_parts(int num_frames, const amav_body_tables *tables, const amav_pose_parts *parts,
                           float *out_vertices_dev, float *out_joint_transforms_dev, void *workspace,
                           size_t workspace_bytes, void *stream);

/* Densify + subset of the posed vertices (src/models/renderer.py:276-288: pytorch3d SubdivideMeshes applied to the
 * posed mesh once or twice, then a vertex subset) as one baked table of 4 base-vertex ids per output point:
 *   point n = 1/2 * ( 1/2 * (v[a0] + v[b0]) + 1/2 * (v[a1] + v[b1]) ),   idx[n] = (a0, b0, a1, b1)
 * which is the midpoint-of-midpoints order subdivision evaluates in; an original vertex repeats its id four times
 * and a level-1 midpoint repeats its pair (halving and adding equal values is exact, so all three cases are
 * bit-identical to the sequential subdivision). */
int amav_points_gather(int num_frames, int num_verts, int num_points, const float *vertices_dev,
                       const int32_t *idx_dev, float *out_points_dev, void *stream);

/* SMPL-X LBS, backward: given grad_vertices = dL/d vertices [F,V,3] of amav_lbs_forward_parts (or amav_lbs_forward: one
 * pose part, one coefficient part, no pose_mean), the gradients of the concatenated pose and coefficients:
 *   grad_full_pose [F, J*3] (the pose_mean term passes the gradient through: it is also the gradient of every pose part's
 *   columns) and grad_coeffs [F, n_coeff] (betas, then expression).  Both contiguous, overwritten.
 * The derivative is that of the forward as oracle.lbs.lbs states it (Rodrigues with angle = ||r + 1e-8||, the kinematic
 * chain, the pose-corrective and shape blend, the skinning), whichever forward kernel produced the vertices.
 * skin_offsets [J+1] / skin_verts / skin_weights [skin_offsets[J]]: the skinning weights transposed -- for every joint
 * its vertices in ascending order with their non-zero weights (body_model.build_skin_transpose).
 * Deterministic: no float atomics; every sum has a fixed order that depends on V, J and the tables only, so gradients
 * are bitwise the same from run to run and a frame's gradients do not depend on the other frames of the call.
 * scratch: amav_lbs_backward_bytes(F, tables) bytes, 16-B aligned (0 = bad arguments).  Refused with an error code
 * before any launch: NULL pointers, F <= 0, bad tables, parts that do not add up to J joints and n_coeff coefficients,
 * scratch too small or misaligned.  No allocation and no host synchronisation. */
typedef struct amav_lbs_backward_args {
    int32_t num_frames;
    const amav_body_tables *tables;
    const amav_pose_parts *parts;   /* exactly those of the forward */
    const float *grad_vertices;     /* [F,V,3] contiguous */
    float *grad_full_pose;          /* [F,J*3] */
    float *grad_coeffs;             /* [F,n_coeff] */
    const int32_t *skin_offsets;    /* [J+1] */
    const int32_t *skin_verts;      /* [skin_offsets[J]] */
    const float *skin_weights;      /* [skin_offsets[J]] */
    void *scratch;
    size_t scratch_bytes;
} amav_lbs_backward_args;
size_t amav_lbs_backward_bytes(int num_frames, const amav_body_tables *tables);
int amav_lbs_backward(const amav_lbs_backward_args *args, void *stream);

/* amav_points_gather, backward: grad_vertices [F,V,3] (overwritten) from grad_points [F,N,3].  Every slot of idx[n]
 * carries 1/4 of point n's gradient to its vertex.  csr_offsets [V+1] / csr_entries [4N]: the gather table transposed --
 * for every vertex the ids of the points whose slots name it, ascending, once per slot (ops.points_gather_csr); a vertex
 * no point names gets exactly +0.  One thread per (frame, vertex) sums in that order: deterministic, no atomics. */
int amav_points_gather_backward(int num_frames, int num_verts, int num_points, const float *grad_points_dev,
                                const int32_t *csr_offsets_dev, const int32_t *csr_entries_dev,
                                float *grad_vertices_dev, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Triplane decode: F.grid_sample x 3 planes + the five Gaussian heads + construct_gaussians
 * (src/models/renderer.py:136,158,165-181,292-346), restructured for HBM: because the heads are linear in the
 * sampled features and bilinear sampling is linear in the texels, each texel is projected through the head
 * weights ONCE (amav_triplane_project: streams the [C, 3R^2] token slab exactly once, coalesced) and the points
 * then sample the 16-channel projected planes (amav_triplane_sample_decode).
 *
 * head_w_plane: device [3, C, 16]: head_w_plane[p][c][o] = Wcat[o][3 + p*C + c] where Wcat [14, 3C+3] stacks the
 * head weights in the output order below (rows 14,15 zero).  head_w_point: device [16,4]: columns 0..2 =
 * Wcat[o][0..2] (the xyz inputs), column 3 = bias.  Output channel order o (= packed record layout):
 *   0-2 xyz_offset, 3 opacity | 4-7 rotation (w,x,y,z) | 8-10 scaling, 11 pad | 12-14 shs, 15 pad.
 */
int amav_triplane_project(int num_frames, int channels, int resolution, const float *tokens_dev,
                          int64_t tokens_frame_stride, const float *head_w_plane_dev, float *out_proj_dev,
                          void *stream);
/* The same, restricted to the texels the sampling can touch: boxes [F,6] = {min x, y, z, max x, y, z} of the points
 * (amav_points_bbox of the point set handed to amav_triplane_sample_decode, or of the posed vertices the subdivision
 * table of amav_triplane_sample_decode_indexed averages: a midpoint lies inside the box of its ends in floating point
 * too), radius as in the sampling call.  Every tap address the sampling kernels form for a point inside the box --
 * including the clamped addresses of zero-padded taps -- lies inside the projected rectangle (each step of
 * p -> texel is monotonic), so the decoded Gaussians are bit-identical; texels outside are left unwritten.  The avatar
 * covers a fifth to a third of each plane, and the token slab is the largest stream of the path.  boxes = NULL: all. */
int amav_triplane_project_region(int num_frames, int channels, int resolution, const float *tokens_dev,
                                 int64_t tokens_frame_stride, const float *head_w_plane_dev, float *out_proj_dev,
                                 const float *boxes_dev, float radius, void *stream);
/* boxes [F,6] = per frame {min x, y, z, max x, y, z} of points [F,N,3]; a frame holding a NaN gets the infinite box. */
int amav_points_bbox(int num_frames, int num_points, const float *points_dev, float *out_boxes_dev, void *stream);
/* points [F,N,3]; transl [F,3] or NULL; proj [F,3,R,R,16] from amav_triplane_project.
 * out_gaussians [F,N,16] packed records: xyz = p + offset + transl, opacity (raw logit) | rot (normalised) |
 * scale (raw), 0 | color = sigmoid(shs), 0.   (renderer.py:333-344) */
int amav_triplane_sample_decode(int num_frames, int num_points, int resolution, const float *proj_dev,
                                const float *points_dev, const float *transl_dev, float radius,
                                const float *head_w_point_dev, float *out_gaussians_dev, void *stream);
/* The same with amav_points_gather fused in: the N points are gathered from the posed vertices [F,V,3] through the
 * baked subdivision table idx [N,4] (identical operation order, so identical bits), saving the [F,N,3] round trip. */
int amav_triplane_sample_decode_indexed(int num_frames, int num_points, int resolution, int num_verts,
                                        const float *proj_dev, const float *vertices_dev, const int32_t *idx_dev,
                                        const float *transl_dev, float radius, const float *head_w_point_dev,
                                        float *out_gaussians_dev, void *stream);
/* Triplane decode, backward: gradients of the packed records that amav_triplane_project(_region) +
 * amav_triplane_sample_decode produced (the reference's stage-2 training reaches the five gaussian_decoder heads and the
 * triplane tokens through them, src/models/renderer.py:136-181), given grad_records = dL/d records [F,N,16].  The
 * padding channels 11 and 15 take no gradient; F.normalize (eps 1e-12) and the sigmoid are differentiated as torch
 * autograd does, and so are clamp(p / radius) and grid_sample (bilinear, align_corners=False, zero padding) for the points.
 *   tokens, proj, boxes, radius, head weights, points: exactly those of the forward (proj is its output, kept).
 *   Region contract: with boxes (R % 4 == 0) only the rectangle of each frame's plane the forward projected is read from
 *   the slab -- the unprojected texels may hold anything, NaN included -- and grad_tokens is written everywhere, exact
 *   zeros outside it; nothing from outside reaches grad_head_w_plane.
 *   Outputs: grad_tokens [F,C,3R^2] contiguous, grad_head_w_plane [3,C,16], grad_head_w_point [16,4] (overwritten,
 *   not accumulated); grad_points [F,N,3] and grad_transl [F,3] optional (NULL = not wanted).
 * Deterministic: no float atomics; every sum has a fixed order, so gradients are bitwise the same from run to run, and
 * grad_tokens, grad_points and grad_transl of a frame do not depend on the other frames of the call (each texel sums its
 * taps in point order).  scratch: amav_triplane_decode_backward_bytes(F, N, C, R) bytes, 16-B aligned (0 = bad sizes).
 * Refused with an error code before any launch: NULL pointers, sizes <= 0, F > 65535, C > 1024 (the plane's weights
 * are staged in 64 KiB of LDS), radius <= 0, misaligned buffers, a tokens frame stride below C 3R^2, scratch too small.
 * No allocation and no host synchronisation. */
typedef struct amav_triplane_decode_backward_args {
    int32_t num_frames, num_points, channels, resolution;
    float radius;
    const float *tokens;            /* [F,C,3R^2], unit stride along texels, frame stride below */
    int64_t tokens_frame_stride;    /* floats */
    const float *head_w_plane;      /* [3,C,16], 16-B aligned */
    const float *head_w_point;      /* [16,4], 16-B aligned */
    const float *points;            /* [F,N,3] */
    const float *proj;              /* [F,3,R,R,16] of the forward, 16-B aligned */
    const float *boxes;             /* [F,6] given to amav_triplane_project_region, or NULL (whole planes) */
    const float *grad_records;      /* [F,N,16], 16-B aligned */
    float *grad_tokens;             /* [F,C,3R^2], 16-B aligned */
    float *grad_head_w_plane;       /* [3,C,16] */
    float *grad_head_w_point;       /* [16,4] */
    float *grad_points;             /* [F,N,3] or NULL */
    float *grad_transl;             /* [F,3] or NULL */
    void *scratch;
    size_t scratch_bytes;
} amav_triplane_decode_backward_args;
size_t amav_triplane_decode_backward_bytes(int num_frames, int num_points, int channels, int resolution);
int amav_triplane_decode_backward(const amav_triplane_decode_backward_args *args, void *stream);
/* Plain Renderer.sample_from_triplane (renderer.py:292-317): element (f,p,c,h,w) of the planes lives at
 * planes[f*frame_stride + p*plane_stride + c*chan_stride + h*R + w] (so both the [F,3,C,R,R] tensor and the
 * [F,C,(3 R R)] token layout are addressable); points [F,N,3] -> features [F,N,3C] in (plane, channel) order. */
int amav_triplane_sample_features(int num_frames, int num_points, int channels, int resolution,
                                  const float *planes_dev, int64_t frame_stride, int64_t plane_stride,
                                  int64_t chan_stride, const float *points_dev, float radius,
                                  float *out_features_dev, void *stream);
/* amav_triplane_sample_features, backward (training through the point refiner, whose input features are these samples):
 * given grad_out = dL/d features [F,N,3C],
 *   grad_planes (f, plane, c, y, x), written at grad_planes[f*grad_frame_stride + plane*grad_plane_stride +
 *     c*grad_chan_stride + y*R + x] = sum over the frame's taps on that texel of w * grad_out[f,n,plane*C+c].  EVERY element
 *     is written (exact zeros where no tap lands); out-of-plane taps are skipped, as the forward's zero padding does.
 *   grad_points [F,N,3]: the bilinear weights' derivative as torch's grid_sampler backward takes it (out-of-plane taps
 *     count with value 0), * R / 2, through clamp(p / radius, -1, 1) (gradient where -1 <= p / radius <= 1, zero beyond),
 *     / radius; each coordinate collects from the two planes that sample it.  Needs the forward's planes and strides.
 * Either output may be NULL (not wanted); the other one's bits do not change.  One kernel pair serves every C.
 * Deterministic: no float atomics.  A texel sums its taps in a fixed order (the four base cells that reach it, rows then
 * columns; points ascending inside a cell; the order comes from a stable counting sort of the frame's points), a point
 * its channels ascending in four interleaved runs: bitwise the same from run to run, and a frame's gradients do not
 * depend on the other frames of the call.
 * scratch: amav_triplane_sample_features_backward_bytes(F, N, C, R) bytes, 16-B aligned (0 = bad sizes); only
 * grad_planes uses it.  Refused with an error code before any launch: NULL args / points / grad_out / both outputs /
 * planes with grad_points / scratch with grad_planes, sizes <= 0, F > 65535, R > 4096, C > 64 * 21845, radius <= 0,
 * grad_planes strides that make elements overlap (plane and channel stride below R^2, frame stride below 3 C R^2),
 * negative planes strides, a misaligned or too small scratch.  No allocation and no host synchronisation. */
typedef struct amav_triplane_sample_backward_args {
    int32_t num_frames, num_points, channels, resolution;
    float radius;
    const float *planes;            /* as given to amav_triplane_sample_features; NULL allowed without grad_points */
    int64_t planes_frame_stride, planes_plane_stride, planes_chan_stride; /* floats */
    const float *points;            /* [F,N,3] */
    const float *grad_out;          /* [F,N,3C] */
    float *grad_planes;             /* strided as below, or NULL */
    int64_t grad_frame_stride, grad_plane_stride, grad_chan_stride;       /* floats */
    float *grad_points;             /* [F,N,3] or NULL */
    void *scratch;
    size_t scratch_bytes;
} amav_triplane_sample_backward_args;
size_t amav_triplane_sample_features_backward_bytes(int num_frames, int num_points, int channels, int resolution);
int amav_triplane_sample_features_backward(const amav_triplane_sample_backward_args *args, void *stream);

/* Window cutting of the windowed triplane upsampler (TriplaneUpsampler.forward_tokens_windowed under autograd): K square
 * windows of size x size out of x [F,C,h,w].  Window k belongs to frame frame[k] and has its top-left corner at
 * (oy[k], ox[k]) in source coordinates; a corner may be negative and a window may reach past h / w.
 *   out [K,C,size,size] = x[frame[k], c, oy[k] + i, ox[k] + j], exact zeros where that lies outside the source (or
 *   frame[k] outside [0, F)).  Every element is written.  K = 0 or C = 0: nothing to do. */
int amav_windows_cut(int num_frames, int channels, int height, int width, const float *x_dev, int num_windows, int size,
                     const int32_t *frame_dev, const int32_t *oy_dev, const int32_t *ox_dev, float *out_dev,
                     void *stream);
/* Its transpose: grad_x[f,c,y,x] = sum over the windows k of frame f that cover (y, x) of
 * grad_windows[k, c, y - oy_k, x - ox_k].  The corners lie on a lattice, oy = a * step + off_y and ox = b * step + off_x
 * with 0 <= a < lattice_rows, 0 <= b < lattice_cols; lattice [F, lattice_rows, lattice_cols] int32 holds the window index
 * at each position, or -1 (each window at one position; an index >= num_windows is never read).  A gather: one thread
 * owns one element of grad_x, walks the <= ceil(size / step)^2 positions whose window covers it and adds them in
 * ascending window index.  No float atomics: bitwise the same on every run.  Elements no window covers get +0.0; every
 * element of grad_x [F,C,h,w] is written.
 * Both refuse (AMAV_ERR_INVALID_ARG, before any launch) negative counts, size <= 0, step <= 0, h * w or size^2 beyond
 * 2^31 - 1, a lattice whose corners leave the int32 range, and a NULL pointer to a non-empty array.  Element offsets are
 * 64-bit.  No allocation and no host synchronisation. */
int amav_windows_cut_backward(int num_frames, int channels, int height, int width, int num_windows, int size,
                              const float *grad_windows_dev, int step, int off_y, int off_x, int lattice_rows,
                              int lattice_cols, const int32_t *lattice_dev, float *grad_x_dev, void *stream);

/* 3x3 convolution, stride 1, over K independent cells in channels-last layout: the two tile stages of the windowed
 * triplane upsampler (three nn.Conv2d(C, C, 3, padding=1) per UpsampleBlock, src/models/renderer.py:348-375) without the
 * mosaic image the library needed.  x [K,h,w,Cin] -> out [K,H,W,Cout], fp32, zero padding of 1 around every cell; an
 * implicit GEMM of K H W rows, Cout columns and a contraction of 9 Cin on the 16-bit MFMA pipe: both operands as two fp16
 * parts scaled by one power of two each, three partial products per fp32 product, fp32 accumulation (the arithmetic of
 * amav_subm_pair_gemm_split).  The weights' exponent is in the prepared buffer's header; the activations' comes from the
 * largest magnitude of the operand after the prologue, found by one sweep inside the call (into the workspace).
 *
 * amav_conv3x3_weights_split_bytes: size of the prepared weights (256-byte header + 9 cin cout x 2 fp16); 0 = channels
 *   that are not positive multiples of 32.
 * amav_conv3x3_prepare_weights_split: weights [cout,cin,3,3] (torch's layout), out_scale NULL or [cout]: weight
 *   [co,:,:,:] is multiplied by out_scale[co] before the split (an eval-mode BatchNorm behind the convolution folds
 *   into it).  out: 256-byte aligned, out_bytes >= the size above (else AMAV_ERR_WORKSPACE).
 * amav_conv3x3_cells, in the order the operand is built:
 *   upsample_input   x is [K,H/2,W/2,Cin] and tap (y + dy, x + dx) reads input texel ((y + dy) >> 1, (x + dx) >> 1): a
 *                    nearest x2 folded into the gather.  H and W must be even.
 *   in_scale, in_shift  [Cin], both or neither: the prologue relu(in_scale x + in_shift) on every texel read.
 *   zeros            a tap outside the cell, [0,H) x [0,W) at the OUTPUT resolution, reads 0; with origin int32 [K,2]
 *                    (the cell's first texel (y, x) in plane coordinates at the output level; may be negative) so does a
 *                    tap whose plane position is outside [0, extent) on either axis.  Both are zeros of the
 *                    convolution's operand: they apply after the prologue (a padded tap is 0, not relu(in_shift)).
 *   epilogue         out = acc (+ bias [Cout]) -> max(., 0) if relu_out -> + residual [K,H,W,Cout] if given.
 * workspace: amav_conv3x3_workspace_bytes() bytes, 16-byte aligned.  Refused with an error code before any launch: NULL
 * args / x / weights_split / out, sizes <= 0, channels that are not multiples of 32, odd H or W with upsample_input,
 * in_scale without in_shift (or the reverse), origin with extent <= 0, misaligned x / in_scale / in_shift, a
 * weights_split_bytes or workspace below the required size (AMAV_ERR_WORKSPACE).  Element offsets are 64-bit.  No float
 * atomics: bitwise the same on every run.  No allocation and no host synchronisation. */
typedef struct amav_conv3x3_args {
    int64_t cells;                   /* K */
    int32_t height, width;           /* H, W of the output */
    int32_t cin, cout;
    int32_t upsample_input, relu_out;
    int32_t extent;                  /* plane size at the output level; read only with origin_dev */
    const float *x_dev;              /* [K,H,W,Cin], or [K,H/2,W/2,Cin] with upsample_input */
    const void *weights_split_dev;   /* from amav_conv3x3_prepare_weights_split */
    size_t weights_split_bytes;
    const float *in_scale_dev, *in_shift_dev; /* [Cin] or NULL */
    const int32_t *origin_dev;       /* [K,2] or NULL */
    const float *bias_dev;           /* [Cout] or NULL */
    const float *residual_dev;       /* [K,H,W,Cout] or NULL */
    float *out_dev;                  /* [K,H,W,Cout] */
    void *workspace_dev;
    size_t workspace_bytes;
} amav_conv3x3_args;
size_t amav_conv3x3_weights_split_bytes(int cin, int cout);
size_t amav_conv3x3_workspace_bytes(void);
int amav_conv3x3_prepare_weights_split(int cin, int cout, const float *weights_dev, const float *out_scale_dev,
                                       void *out_dev, size_t out_bytes, void *stream);
int amav_conv3x3_cells(const amav_conv3x3_args *args, void *stream);

/* Backward of amav_conv3x3_cells.  With Z = inside o relu(in_scale up(x) + in_shift) the forward's operand (prologue and
 * up optional; `inside`: the cell's zero padding and the plane rule), y = conv(Z, W) + bias, out = relu(y) if relu_out,
 * and g = grad_out [K,H,W,Cout]:
 *   ga           = g where out > 0 with relu_out (the gate reads out_dev, the forward's saved result; a forward that also
 *                  added a residual cannot be gated from it, so the two do not combine), else g.  grad_residual = g.
 *   grad_bias    [Cout] = column sum of ga.
 *   gZ           = the same 3x3 cell convolution of ga (the cell's own zero padding, no prologue, no plane rule) with the
 *                  weights W'[ci,co,a,b] = W[co,ci,2-a,2-b]: amav_conv3x3_cells' kernel on weights_split_t_dev from
 *                  amav_conv3x3_prepare_weights_split_transposed, ga built while the operand is staged; the sweep for
 *                  its exponent sees ga.
 *   grad_x       [K,h,w,Cin] = in_scale * pool(gZ m), m = inside o [in_scale up(x) + in_shift > 0]; pool adds the 2 x 2
 *                  fine texels of a coarse one in row-major order (upsample_input only).
 *   grad_in_scale, grad_in_shift [Cin] = column sums of gZ m up(x) and of gZ m.
 *   grad_weight  [Cout,Cin,3,3] (torch's layout) = sum over all texels of ga[co] Z[ci] shifted by the tap: a split-product
 *                  MFMA GEMM over K H W texels.  Split-K: the (cell, tile) pairs are cut into `wgrad_slices` contiguous
 *                  ranges (0: a heuristic that fills the CUs within 64 MiB of workspace; at most 4096), each range
 *                  writes its own partial, a second kernel adds the partials in ascending order.
 * Every sum has a fixed order and nothing is accumulated with atomics: bitwise the same on every run.  A NULL gradient
 * pointer skips that gradient's work; grad_in_scale and grad_in_shift come together and need the prologue.
 * amav_conv3x3_backward_workspace_bytes: the workspace this call needs (it depends on which gradients are asked for and
 * on the slice count); 0 = the arguments would be refused.  Refused with an error code before any launch: everything
 * amav_conv3x3_cells refuses, NULL grad_out, relu_out without out_dev, misaligned grad_out / out / gradients, a slice
 * count outside [0, 4096], no gradient asked for at all, a workspace below the required size (AMAV_ERR_WORKSPACE).
 * Element offsets are 64-bit.  No allocation and no host synchronisation.
 * amav_conv3x3_prepare_weights_split_transposed: weights [cout,cin,3,3] -> the prepared weights of the data gradient
 * (amav_conv3x3_weights_split_bytes(cout, cin) bytes, 256-byte aligned). */
typedef struct amav_conv3x3_backward_args {
    int64_t cells;                   /* K */
    int32_t height, width;           /* H, W of the output */
    int32_t cin, cout;
    int32_t upsample_input, relu_out;
    int32_t extent;
    int32_t wgrad_slices;            /* 0 = heuristic */
    const float *x_dev;              /* the forward's x */
    const void *weights_split_t_dev; /* from amav_conv3x3_prepare_weights_split_transposed; read for grad_x / in_scale */
    size_t weights_split_t_bytes;
    const float *in_scale_dev, *in_shift_dev;
    const int32_t *origin_dev;
    const float *out_dev;            /* the forward's result [K,H,W,Cout]; read only with relu_out */
    const float *grad_out_dev;       /* [K,H,W,Cout] */
    float *grad_x_dev;               /* [K,h,w,Cin] or NULL */
    float *grad_weight_dev;          /* [Cout,Cin,3,3] or NULL */
    float *grad_bias_dev;            /* [Cout] or NULL */
    float *grad_in_scale_dev, *grad_in_shift_dev; /* [Cin], both or neither */
    void *workspace_dev;
    size_t workspace_bytes;
} amav_conv3x3_backward_args;
int amav_conv3x3_prepare_weights_split_transposed(int cin, int cout, const float *weights_dev, void *out_dev,
                                                  size_t out_bytes, void *stream);
size_t amav_conv3x3_backward_workspace_bytes(const amav_conv3x3_backward_args *args, int wgrad_slices);
int amav_conv3x3_cells_backward(const amav_conv3x3_backward_args *args, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Image loss of the two training steps: L1 and SSIM (src/utils/loss_utils.py:18-19, 24-84) of N images of H x W x C,
 * forward and backward.  SSIM uses the reference's separable 11-tap window, zero padding of 5 (taps outside the image
 * contribute 0, the window is not renormalised), C1 = 0.01^2, C2 = 0.03^2.
 *
 * Both images are read in place: element (n, y, x, c) of a view lives at
 * ptr[n * image_stride + y * row_stride + x * pixel_stride + c * channel_stride] (strides in floats, 64-bit offsets), so
 * a [..., :3] view of an RGBA frame, a planar [N,C,H,W] target and a contiguous [N,H,W,C] tensor need no copy. */
typedef struct amav_image_view {
    const float *ptr;
    int64_t image_stride, row_stride, pixel_stride, channel_stride; /* floats */
} amav_image_view;
/* The 11 taps of the 1-D window, as fp32 (losses.gaussian(11, 1.5)): the 2-D window is their outer product. */
typedef struct amav_image_loss_window {
    float taps[11];
} amav_image_loss_window;
/* Bytes of the forward's workspace (one pair of partial sums per 16 x 16 tile and image); 0 for an empty problem or
 * negative counts. */
size_t amav_image_loss_workspace_bytes(int num_images, int height, int width);
/* sums [2,N]: sums[n] = sum over image n of |x - y|, sums[N + n] = sum over image n of the SSIM map.  One workgroup per
 * tile writes its pair of partial sums to its own workspace slot and a second kernel adds an image's slots in a fixed
 * order: no float atomics, bitwise the same on every run.
 * maps: NULL, or [3,N,H,W,C] (contiguous) receiving per element the derivatives of the SSIM map with respect to the
 * window means E[x^2], E[xy] and mu_x, which amav_image_loss_backward reads.  With NULL nothing of that size is written.
 * workspace: amav_image_loss_workspace_bytes(N, H, W) bytes; NULL or too small: AMAV_ERR_WORKSPACE. */
int amav_image_loss_forward(int num_images, int height, int width, int channels, const amav_image_view *x,
                            const amav_image_view *y, const amav_image_loss_window *window, float *sums_dev,
                            float *maps_dev, void *workspace_dev, size_t workspace_bytes, void *stream);
/* grad_x [N,H,W,C] (contiguous; every element written exactly once) =
 *   grad_l1[n] * sign(x - y) + grad_ssim[n] * (conv(d_m1) + 2 x conv(d_e11) + y conv(d_e12))
 * with conv the same zero-padded window over the forward's maps, sign(0) = 0, and grad_l1 / grad_ssim [N] the gradients
 * of the per-image sums, read on the device.  The target y gets no gradient.  A gather: no atomics, deterministic.
 * All three entry points refuse (AMAV_ERR_INVALID_ARG, before any launch) negative counts, channels outside 1..4, a
 * per-image H * W * C beyond 2^31 - 1 and NULL pointers; N = 0, H = 0 or W = 0 is an empty problem (AMAV_OK, no pointer
 * is looked at).  No allocation and no host synchronisation. */
int amav_image_loss_backward(int num_images, int height, int width, int channels, const amav_image_view *x,
                             const amav_image_view *y, const amav_image_loss_window *window, const float *maps_dev,
                             const float *grad_l1_dev, const float *grad_ssim_dev, float *grad_x_dev, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Stage-1 identity encoder: the point <-> triplane-cell reductions of
 * SMPLXTriplaneEncoder and the point -> pixel feature lookup, deterministic segment reductions.
 * Replaces torch_scatter.scatter_max / scatter_mean as used at src/models/triplane_net.py:226-244 and the pytorch3d
 * point rasterizer + index_put of points_projection (src/utils/graphic_utils.py:275-331).
 *   order [B,3,N] (amav_cell_max) / [B,N] (amav_cell_mean): point ids sorted by cell (stable); seg [.., cells + 1]:
 *   offsets of every cell's run in `order`; cell_of [B,3,N]: cell of every point per plane.
 * amav_cell_max:    cellmax [B,3,cells,C] = per-cell channel-wise maximum of feat [B,N,C] (0 for an empty cell)
 * amav_cell_gather: out [B,N,C] = cellmax[plane 0] + cellmax[plane 1] + cellmax[plane 2] at the point's cells
 *                   (pool_local, triplane_net.py:226-238)
 * amav_cell_mean:   out_planes [B,C,cells] = per-cell mean of feat [B,N,C], summed in ascending point id, 0 if empty
 *                   (generate_plane_features, triplane_net.py:240-244)
 * amav_points_project: points [B,N,3] (world), w2c [B,4,4] row-major, intrinsics [B,3,3] (OpenCV pixels), features
 *   [B,C,H,W] -> out [B,N,C]: z-buffer of discs of radius_px around the projected points (pixel centres at +0.5);
 *   a point that is the nearest one at some pixel takes the features of the LAST such pixel in (y, x) order, every
 *   other point zeros. */
int amav_cell_max(int batch, int num_points, int channels, int cells, const float *feat_dev, const int32_t *order_dev,
                  const int32_t *seg_dev, float *cellmax_dev, void *stream);
int amav_cell_gather(int batch, int num_points, int channels, int cells, const float *cellmax_dev,
                     const int32_t *cell_of_dev, float *out_dev, void *stream);
int amav_cell_mean(int batch, int num_points, int channels, int cells, const float *feat_dev, const int32_t *order_dev,
                   const int32_t *seg_dev, float *out_planes_dev, void *stream);
size_t amav_points_project_workspace_bytes(int batch, int num_points, int height, int width);
int amav_points_project(int batch, int num_points, int channels, int height, int width, const float *points_dev,
                        const float *w2c_dev, const float *intrinsics_dev, const float *features_dev, float radius_px,
                        float *out_dev, void *workspace, size_t workspace_bytes, void *stream);

/* Backwards of the three stage-1 ops (training stage 1, lightning_model_wrapper.py:82-170).  No
 * float atomics, every sum in a fixed order: bitwise reproducible and independent of how frames are batched.
 * amav_cell_max_backward: grad_feat [B,N,C] (overwritten) of amav_cell_max + amav_cell_gather, given grad_out [B,N,C]
 *   and the forward's feat, order, seg and cell_of.  For every plane p, the whole gradient of a cell's maximum, S_p =
 *   sum of grad_out over the cell's points in ascending point id, goes to the ONE point that holds the maximum (the
 *   lowest point id among ties: a sequential scan with a strict >), as torch_scatter's scatter_max backward routes it;
 *   grad_feat = (v_0 + v_1) + v_2.  workspace: amav_cell_max_backward_workspace_bytes(B, C, cells) bytes (0 = bad
 *   sizes): the arg and S tables [B,3,cells,C].
 * amav_cell_mean_backward: grad_feat [B,N,C] of amav_cell_mean, given grad_planes [B,C,cells] and the forward's order
 *   and seg: grad_feat[n][c] = grad_planes[c][cell(n)] / count(cell(n)), one fp32 division.  Every row is written once
 *   provided order is a permutation of the point ids with seg[cells] = N (as the forward's segments are).
 * amav_points_project_backward: grad_features [B,C,H,W] (overwritten) of amav_points_project w.r.t. its features, given
 *   grad_out [B,N,C] and the forward's WORKSPACE, unchanged since that call: the backward reads its z-buffer (the first
 *   B*H*W uint64 keys, (depth bits << 32) | point id, all ones where no point covers the pixel).  index_put's backward:
 *   every pixel a point wins takes that point's gradient row (also the won pixels whose features the forward
 *   discarded), 0 where no point won.  Points, w2c and intrinsics get no gradient (the selection is piecewise
 *   constant). */
size_t amav_cell_max_backward_workspace_bytes(int batch, int channels, int cells);
int amav_cell_max_backward(int batch, int num_points, int channels, int cells, const float *feat_dev,
                           const int32_t *order_dev, const int32_t *seg_dev, const int32_t *cell_of_dev,
                           const float *grad_out_dev, float *grad_feat_dev, void *workspace, size_t workspace_bytes,
                           void *stream);
int amav_cell_mean_backward(int batch, int num_points, int channels, int cells, const int32_t *order_dev,
                            const int32_t *seg_dev, const float *grad_planes_dev, float *grad_feat_dev, void *stream);
int amav_points_project_backward(int batch, int num_points, int channels, int height, int width,
                                 const float *grad_out_dev, const void *forward_workspace, size_t workspace_bytes,
                                 float *grad_features_dev, void *stream);

/* Stage-1 image features sampled from the token grid.  ImageFeature resizes a [Gh,Gw,Cg] grid
 * bilinearly to the image, concatenates RGB and lets amav_points_project look up one pixel per visible point; these two
 * entry points evaluate the resize at those pixels only and gather the gradient straight back into the grid, so neither
 * the [B,3+Cg,H,W] tensor nor its gradient exists.
 * amav_points_project_grid: points, w2c, intrinsics, radius_px and the selection exactly as amav_points_project (the
 *   same two kernels; the same workspace, amav_points_project_workspace_bytes: z-buffer keys first, then pixel_of);
 *   rgb [B,3,H,W]; grid [B,Gh,Gw,Cg] channels-last (the layout of the reducing Linear's output) -> out [B,N,3+Cg].  For a
 *   point that claims pixel (y, x): channels 0..2 = rgb[b,:,y,x] copied, channel 3 + c = the grid resized as
 *   F.interpolate(mode="bilinear", align_corners=False) defines it, at (y, x).  A point that claims nothing: zeros.
 *   Per axis (pixel i of `size`, G nodes), all in fp32, in this order, no contraction:
 *     scale = (float)G / (float)size;  s = scale * ((float)i + 0.5f) - 0.5f;  s = s < 0 ? 0 : s;
 *     i0 = min((int)s, G - 1);  i1 = i0 + (i0 < G - 1);  l = s - (float)i0;  h = 1 - l
 *   value = hy * (hx * g00 + lx * g01) + ly * (hx * g10 + lx * g11), g_yx = grid[b, iy_y, ix_x, c].
 * amav_points_project_grid_backward: given grad_out [B,N,3+Cg] and the forward's WORKSPACE, unchanged since that call,
 *   grad_grid [B,Gh,Gw,Cg] (every element overwritten) and, unless grad_rgb is NULL, grad_rgb [B,3,H,W] (overwritten).
 *   The gradient of the dense path: index_put's backward credits every pixel a point WINS (not only the claimed one), so
 *     grad_grid[b,j,i,c] = sum over the pixels p whose z-buffer winner n is valid, and over those of p's corners 00, 01,
 *                          10, 11 that are node (j, i), of w_corner(p) * grad_out[b,n,3+c]
 *   with w_00 = hy * hx, w_01 = hy * lx, w_10 = ly * hx, w_11 = ly * lx (one fp32 product), each term one fp32 product
 *   w * g added to the running fp32 sum, starting from 0, in ascending pixel index y * W + x and, within a pixel, corners
 *   in the order 00, 01, 10, 11.  In the clamped first and last half-cell of an axis i0 == i1 and both weights reach the
 *   same node as two separate terms.  A node no won pixel reaches (also: every node of a down-sampled axis that no
 *   pixel maps to) is exactly 0.  grad_rgb[b,:,y,x] = grad_out[b,winner(y,x),0:3], 0 where no point won.  No float
 *   atomics; the order depends on neither B nor the launch geometry: bitwise reproducible, and B frames equal B calls.
 * Both refuse, before any launch: sizes <= 0, B > 65535, H * W >= 2^31, Gh * Gw >= 2^31 (AMAV_ERR_INVALID_ARG), NULL
 * pointers (grad_rgb excepted), and a workspace that is NULL or smaller than amav_points_project_workspace_bytes
 * (AMAV_ERR_WORKSPACE; the forward reports a NULL workspace as a NULL pointer, as amav_points_project does). */
int amav_points_project_grid(int batch, int num_points, int height, int width, int grid_height, int grid_width,
                             int grid_channels, const float *points_dev, const float *w2c_dev,
                             const float *intrinsics_dev, const float *rgb_dev, const float *grid_dev, float radius_px,
                             float *out_dev, void *workspace, size_t workspace_bytes, void *stream);
int amav_points_project_grid_backward(int batch, int num_points, int height, int width, int grid_height, int grid_width,
                                      int grid_channels, const float *grad_out_dev, const void *forward_workspace,
                                      size_t workspace_bytes, float *grad_grid_dev, float *grad_rgb_dev, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Self-attention of the audio transformer (diffusers Attention -> F.scaled_dot_product_attention as reached from
 * src/models/transformers.py:329-336): softmax(Q K^T * scale) V, fp32 in/out, no mask.  q,k,v,out: [B, S, H*D] with
 * row stride `row_stride` floats (so a fused QKV projection output can be passed without a copy); D must be 64.  The key
 * sweep may be split over several workgroups for load balance; their partial softmax states and the split K / V
 * operands live in the caller's workspace.
 *
 * The products are fp32-equivalent sums of low-precision partial products on the 16-bit MFMA pipe (1.1e-7 max abs
 * against fp64 at the reference shape; the library's fp32 SDPA: 4.8e-7): by default two fp16 parts per operand, three
 * partial products, every operand pre-scaled by a power of two taken from its magnitude -- measured by a pre-pass over
 * q, k, v (amav_selfattn_forward), or handed over by a caller that can PROVE upper bounds of |q|, |k|, |v|
 * (amav_selfattn_forward_bounded with all three > 0; a bound the data exceeds by more than 2x overflows fp16).  The
 * process-wide switch AMAV_ATTN=bf16 selects three bf16 parts / six partial products (no scaling involved),
 * AMAV_ATTN=f32 the exact-product fp32 MFMA kernel (v_mfma_f32_32x32x2_f32).
 */
size_t amav_selfattn_workspace_bytes(int batch, int seq_len, int heads, int head_dim);
int amav_selfattn_forward(int batch, int seq_len, int heads, int head_dim, const float *q_dev, const float *k_dev,
                          const float *v_dev, int64_t row_stride, float *out_dev, int64_t out_row_stride,
                          float scale, void *workspace, size_t workspace_bytes, void *stream);
int amav_selfattn_forward_bounded(int batch, int seq_len, int heads, int head_dim, const float *q_dev,
                                  const float *k_dev, const float *v_dev, int64_t row_stride, float *out_dev,
                                  int64_t out_row_stride, float scale, float q_bound, float k_bound, float v_bound,
                                  void *workspace, size_t workspace_bytes, void *stream);
/* The same, with the result ALSO (or, when the key range is split over workgroups, ONLY) written as the fp16 x 2 activation
 * operand of the projection that follows (amav_split_operand's AMAV_SPLIT_FP16X2 layout, rows of [h2 | h1 | h1] with K =
 * heads * head_dim, x 2^split_scale_exp = h1 + h2): diffusers' to_out after the attention (transformers.py:329-336, 448).
 * out_split_dev [batch * seq_len, 3 K] fp16, 16-byte aligned; out_dev rows dense (out_row_stride = K) -- whether out_dev is
 * written depends on the key split the kernel chooses, so a caller that passes out_split must not read it.  NULL: as above. */
int amav_selfattn_forward_split_out(int batch, int seq_len, int heads, int head_dim, const float *q_dev, const float *k_dev,
                                    const float *v_dev, int64_t row_stride, float *out_dev, int64_t out_row_stride,
                                    float scale, float q_bound, float k_bound, float v_bound, void *out_split_dev,
                                    int split_scale_exp, void *workspace, size_t workspace_bytes, void *stream);
/* The forward of the differentiable path: as amav_selfattn_forward (measured operand scales, same workspace size), and
 * the row log-sum-exp lse_dev [B, H, S] fp32 in natural units, lse[b,h,i] = ln sum_j exp(scale q_i . k_j), which
 * amav_selfattn_backward recomputes the probabilities from.  out_dev equals amav_selfattn_forward's bit for bit.  Built
 * for the default fp16 x 2 kernel only: refused (AMAV_ERR_INVALID_ARG) when attn = bf16 | f32 is selected. */
int amav_selfattn_forward_lse(int batch, int seq_len, int heads, int head_dim, const float *q_dev, const float *k_dev,
                              const float *v_dev, int64_t row_stride, float *out_dev, int64_t out_row_stride, float scale,
                              float *lse_dev, void *workspace, size_t workspace_bytes, void *stream);
/* Self-attention backward (flash-attention-2 form): from the forward's q, k, v (row stride
 * row_stride, as the forward reads them), its output out_dev, its lse_dev and dout_dev = dLoss/d out ([B, S, H*D], row
 * stride dout_row_stride), writes dq | dk | dv into dqkv_dev [B, S, 3*H*D] (row stride dqkv_row_stride >= 3*H*D; columns
 * past 3*H*D untouched): the gradient of a fused q/k/v projection's output.  Deterministic bit for bit (fixed-order sums,
 * no atomics); exact fp32 products on v_mfma_f32_32x32x2_f32.  D must be 64; q/k/v/out/dout/dqkv 16-byte aligned, row
 * strides multiples of 4 floats.  workspace: amav_selfattn_backward_workspace_bytes(B, S, H, D) bytes (0 = bad sizes). */
size_t amav_selfattn_backward_workspace_bytes(int batch, int seq_len, int heads, int head_dim);
int amav_selfattn_backward(int batch, int seq_len, int heads, int head_dim, const float *q_dev, const float *k_dev,
                           const float *v_dev, int64_t row_stride, const float *out_dev, int64_t out_row_stride,
                           const float *lse_dev, const float *dout_dev, int64_t dout_row_stride, float *dqkv_dev,
                           int64_t dqkv_row_stride, float scale, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Cross-attention of the stage-1 encoder (diffusers Attention with encoder_hidden_states, as reached from
 * BasicTransformerBlock.attn2: the fusion network's 3*32^2 + 80 = 3152 queries and the SMPL-X predictor's 80 queries
 * over the 4096 Sapiens tokens, 8 heads x 64): softmax(Q K^T * scale) V, fp32 in/out, no mask, any q_len and kv_len.
 * q [B, q_len, H*D] with row stride q_row_stride; k, v [B, kv_len, H*D] sharing kv_row_stride (so the halves of a fused
 * k | v projection output can be passed without a copy); out [B, q_len, H*D] with out_row_stride; D must be 64.
 *
 * Always the fp16 x 2 kernels of the self-attention above (two fp16 parts per operand, three partial products,
 * operands pre-scaled by powers of two from the measured max |q| over the B*q_len rows and max |k|, |v| over the
 * B*kv_len rows), WHATEVER the attn option / AMAV_ATTN selects: the bf16 x 3 and fp32 kernels are self-attention only.
 * With q_len = kv_len and one row stride the results equal amav_selfattn_forward_lse's bit for bit.
 * lse_dev: NULL, or the row log-sum-exp [B, H, q_len] in natural units, which amav_crossattn_backward needs.
 * amav_crossattn_key_split: the number of key slices a call takes (>= 1; 0 = bad sizes); above 1 the slices' partial
 * softmax states pass through the workspace.  workspace: amav_crossattn_workspace_bytes bytes (0 = bad sizes).
 * Pointers 16-byte aligned (lse 4), row strides multiples of 4 floats and >= H*D, scale finite, H, B <= 65535. */
size_t amav_crossattn_workspace_bytes(int batch, int q_len, int kv_len, int heads, int head_dim);
int amav_crossattn_key_split(int batch, int q_len, int kv_len, int heads);
int amav_crossattn_forward(int batch, int q_len, int kv_len, int heads, int head_dim, const float *q_dev,
                           int64_t q_row_stride, const float *k_dev, const float *v_dev, int64_t kv_row_stride,
                           float *out_dev, int64_t out_row_stride, float scale, float *lse_dev, void *workspace,
                           size_t workspace_bytes, void *stream);
/* Cross-attention backward (the flash-attention-2 form of amav_selfattn_backward with two row sets): from the forward's
 * q, k, v, out_dev, lse_dev and dout_dev = dLoss/d out ([B, q_len, H*D]) writes dq into dq_dev [B, q_len, >= H*D] and
 * dk | dv into dkv_dev [B, kv_len, >= 2*H*D] (the gradient of a fused k | v projection's output; columns past the row
 * width untouched).  Deterministic bit for bit (fixed-order sums, no atomics), batch items independent; exact fp32
 * products on v_mfma_f32_32x32x2_f32.  Same alignment and stride rules; dkv_row_stride >= 2*H*D.
 * workspace: amav_crossattn_backward_workspace_bytes(B, q_len, H, D) bytes (0 = bad sizes). */
size_t amav_crossattn_backward_workspace_bytes(int batch, int q_len, int heads, int head_dim);
int amav_crossattn_backward(int batch, int q_len, int kv_len, int heads, int head_dim, const float *q_dev,
                            int64_t q_row_stride, const float *k_dev, const float *v_dev, int64_t kv_row_stride,
                            const float *out_dev, int64_t out_row_stride, const float *lse_dev, const float *dout_dev,
                            int64_t dout_row_stride, float *dq_dev, int64_t dq_row_stride, float *dkv_dev,
                            int64_t dkv_row_stride, float scale, void *workspace, size_t workspace_bytes, void *stream);

/* The two backwards above on fp16 x 2 split products ("split arithmetic"): the same three
 * passes, arguments, strides, alignment rules and errors, with all seven products on v_mfma_f32_32x32x16_f16 -- two
 * fp16 parts per operand, three partial products per fp32 product, fp32 sums.  Q, K, V and dO are scaled by powers of
 * two from their measured call-wide maxima, P by 2^14 and dS by a power of two from the proven bound |dS_ij| <=
 * 2 max_i |dO_i|_2 max_j |v_j|_2; the maxima are reduced on the device into a header in the workspace (integer atomicMax
 * on bit patterns: order-independent).  Deterministic bit for bit; because the scales are measured per call, a batch of
 * two is not bitwise two single calls.  No float atomics, no host synchronisation, HIP-graph capturable.
 * workspace: the matching ..._split_workspace_bytes (header + delta; 0 = bad sizes). */
size_t amav_selfattn_backward_split_workspace_bytes(int batch, int seq_len, int heads, int head_dim);
int amav_selfattn_backward_split(int batch, int seq_len, int heads, int head_dim, const float *q_dev, const float *k_dev,
                                 const float *v_dev, int64_t row_stride, const float *out_dev, int64_t out_row_stride,
                                 const float *lse_dev, const float *dout_dev, int64_t dout_row_stride, float *dqkv_dev,
                                 int64_t dqkv_row_stride, float scale, void *workspace, size_t workspace_bytes,
                                 void *stream);
size_t amav_crossattn_backward_split_workspace_bytes(int batch, int q_len, int heads, int head_dim);
int amav_crossattn_backward_split(int batch, int q_len, int kv_len, int heads, int head_dim, const float *q_dev,
                                  int64_t q_row_stride, const float *k_dev, const float *v_dev, int64_t kv_row_stride,
                                  const float *out_dev, int64_t out_row_stride, const float *lse_dev,
                                  const float *dout_dev, int64_t dout_row_stride, float *dq_dev, int64_t dq_row_stride,
                                  float *dkv_dev, int64_t dkv_row_stride, float scale, void *workspace,
                                  size_t workspace_bytes, void *stream);

/* Operand of an fp32-equivalent nn.Linear (src/models/transformers.py:70-84, 448, 505: the to_q/k/v, to_out and
 * feed-forward projections) computed as ONE low-precision GEMM with fp32 accumulation over operands split into parts
 * and concatenated along K.  x [rows, k] fp32 (row stride in floats, k a multiple of 8) -> out [rows, parts * k]:
 *   AMAV_SPLIT_BF16X3  x = x1 + x2 + x3 (bf16 each); activations (weights = 0) [x3 x2 x1 x2 x1 x1], weights (weights = 1)
 *                      [w1 w2 w3 w1 w2 w1]: A' B'^T = the six partial products x_i w_j^T with i + j <= 4 (K' = 6 k).
 *                      Any finite input; scale_exp is ignored.
 *   AMAV_SPLIT_FP16X2  x 2^scale_exp = h1 + h2 (fp16 each); activations [h2 h1 h1], weights [g1 g2 g1]: A' B'^T =
 *                      h2 g1 + h1 g2 + h1 g1 (K' = 3 k, half the matrix work).  The caller picks scale_exp from a bound
 *                      on |x| so that |x| 2^scale_exp <= 32768 (no overflow) and typical values keep their residual out
 *                      of fp16's subnormals, and multiplies the product by 2^-(scale_exp_a + scale_exp_w). */
#define AMAV_SPLIT_BF16X3 0
#define AMAV_SPLIT_FP16X2 1
int amav_split_operand(int64_t rows, int k, const float *x_dev, int64_t x_row_stride, int weights, int format,
                       int scale_exp, void *out_dev, void *stream);

/* The AMAV_SPLIT_BF16X3 operand of x^T, for the products whose contraction runs over the ROWS of an fp32 tensor: both
 * backward products of a linear layer (dW = g^T x over the rows of g and x, dx = g W over the rows
 * of W).  x [rows, k] fp32, the same rules on k, stride and alignment as amav_split_operand.  With
 * Rp = amav_split_transposed_rows(rows) = rows rounded up to a multiple of 8 (0 for rows <= 0):
 *   out_t_dev     [k, 6 Rp] bf16: part p of column c at out_t[c, p Rp : p Rp + rows], the Rp - rows entries after it
 *                 written as +0; part order as amav_split_operand ([x3 x2 x1 x2 x1 x1] for weights = 0, [x1 x2 x3 x1 x2 x1]
 *                 for weights = 1) and the same three-way split, so every part equals that kernel's bit for bit.
 *   out_rows_dev  NULL, or [rows, 6 k] bf16: the ACTIVATION operand of x from the same read, bit-identical to
 *                 amav_split_operand(..., weights = 0, AMAV_SPLIT_BF16X3, ...) whatever `weights` is (a backward needs its
 *                 upstream gradient in both forms).
 * One kernel, no atomics, no workspace. */
int64_t amav_split_transposed_rows(int64_t rows);
int amav_split_operand_transposed(int64_t rows, int k, const float *x_dev, int64_t x_row_stride, int weights,
                                  void *out_rows_dev /* may be NULL */, void *out_t_dev, void *stream);

/* GEGLU gate of the transformer feed-forward (src/models/transformers.py:484-508, exact-erf GELU):
 * proj [rows, 2*inner] (row stride in floats) -> [rows, inner] = proj[:, :inner] * gelu(proj[:, inner:]).
 * bias [2*inner] (may be NULL) is added to proj first: the projection's bias when its GEMM ran without one.
 * The result goes to exactly one of out (fp32) and out_split (the AMAV_SPLIT_FP16X2 activation operand [rows, 3*inner]
 * of the output projection, pre-scaled by 2^split_scale_exp); the other is NULL. */
int amav_geglu(int64_t rows, int inner, const float *proj_dev, int64_t proj_row_stride, const float *bias_dev,
               float *out_dev, void *out_split_dev, int split_scale_exp, void *stream);

/* Residual adds + LayerNorm of BasicTransformerBlock (src/models/transformers.py:292-399) in one pass over [rows, dim]
 * (dim in {256, 512, 768, 1024}):  h = ((add + add_bias) + hidden);  h = (batch_row[row / rows_per_batch] + h);
 * hidden_out = h;  norm = LayerNorm(h) * weight + bias.  `add` [rows, dim], `add_bias` [dim] (the bias of the projection
 * that produced `add`, when its GEMM ran without one) and `batch_row` [batches, dim] may be NULL; hidden_out may alias
 * hidden.  The normalised rows go to exactly one of out_norm (fp32 [rows, dim]) and out_norm_split (the activation
 * operand of amav_split_operand in split_format / split_scale_exp, for the projection that follows); the other is
 * NULL. */
int amav_add_layernorm(int64_t rows, int dim, int64_t rows_per_batch, const float *add_dev, const float *add_bias_dev,
                       const float *batch_row_dev, const float *hidden_dev, float *hidden_out_dev,
                       const float *weight_dev, const float *bias_dev, float eps, float *out_norm_dev,
                       void *out_norm_split_dev, int split_format, int split_scale_exp, void *stream);

/* Backwards of the two row kernels above and the column sum their bias-like gradients need
 * (csrc/attention_rows_backward.hip).  Deterministic bit for bit: no atomics, every sum in a fixed
 * order that depends on the sizes alone.  Kernel launches only, no host synchronisation; all buffers 16-byte aligned, row
 * strides in floats and multiples of 4.
 *
 * amav_rows_colsum     out [groups, cols] : out[g, c] = sum of x[r, c] over the rows_per_group rows of group g
 *                      (groups = rows / rows_per_group, which must divide; cols a multiple of 4).  Two stages: the rows
 *                      of a group in consecutive chunks of 16 (the last may be shorter; no chunk straddles a group), each
 *                      summed in ascending row order; then a group's chunk partials added in ascending order.  workspace:
 *                      amav_rows_colsum_workspace_bytes(rows, cols, rows_per_group) bytes (0 = bad sizes).
 * amav_geglu_backward  with h = proj[:, :inner] + bias_h and g = proj[:, inner:] + bias_g (bias [2*inner] may be NULL),
 *                      recomputed from proj: dproj [rows, 2*inner] = (dout gelu(g) | dout h (Phi(g) + g phi(g))), exact
 *                      erf.  Nothing else of the forward is needed; the bias gradient is amav_rows_colsum(dproj), one group.
 * amav_add_layernorm_backward  h [rows, dim] = the forward's hidden_out, dim in {256, 512, 768, 1024}.  mean and rstd are
 *                      recomputed as the forward computes them; with xhat = (h - mean) rstd and t = dnorm * weight:
 *                        dh = dhidden_out + rstd (t - mean_c(t) - xhat mean_c(t xhat))         [rows, dim]
 *                        dweight[c] = sum_r dnorm xhat,  dbias[c] = sum_r dnorm                 [dim] each
 *                      both in amav_rows_colsum's order with one group (a wave keeps the partials of its 16 rows in
 *                      registers: dnorm is read once).  dnorm / dhidden_out [rows, dim] may be NULL (= zero); without dnorm
 *                      dweight and dbias are +0.  dh must not alias an input.  The forward's other operands follow from
 *                      dh: d add = d hidden = dh, d batch_row = amav_rows_colsum(dh, rows_per_group = rows_per_batch),
 *                      d add_bias = amav_rows_colsum(dh, one group).  workspace:
 *                      amav_add_layernorm_backward_workspace_bytes(rows, dim) bytes (0 = bad sizes). */
size_t amav_rows_colsum_workspace_bytes(int64_t rows, int cols, int64_t rows_per_group);
int amav_rows_colsum(int64_t rows, int cols, const float *x_dev, int64_t x_row_stride, int64_t rows_per_group,
                     float *out_dev, void *workspace, size_t workspace_bytes, void *stream);
int amav_geglu_backward(int64_t rows, int inner, const float *proj_dev, int64_t proj_row_stride, const float *bias_dev,
                        const float *dout_dev, float *dproj_dev, int64_t dproj_row_stride, void *stream);
size_t amav_add_layernorm_backward_workspace_bytes(int64_t rows, int dim);
int amav_add_layernorm_backward(int64_t rows, int dim, const float *h_dev, const float *weight_dev, float eps,
                                const float *dnorm_dev, const float *dhidden_out_dev, float *dh_dev, float *dweight_dev,
                                float *dbias_dev, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Stage-1 TriplaneDownsampler (src/models/triplane_net.py:411-451: two ConvNeXtBlocks and Conv2d(C, C, 4, stride s,
 * padding 1)): everything of it that is not a matrix product (csrc/convnext.hip).  fp32, planes
 * channels-last [planes, height, width, channels] with planes = frames x 3; deterministic bit for bit (no atomics, every
 * sum in an order fixed by the sizes alone), planes independent of each other; kernel launches only; all buffers 16-byte
 * aligned.  Results that feed a projection go to exactly one of an fp32 buffer and out_split, the ACTIVATION operand of
 * amav_split_operand in split_format / split_scale_exp (the rule of amav_add_layernorm); the other is NULL.
 *
 * amav_dwconv7_layernorm   ConvNeXtBlock's dwconv -> permute -> norm (:414-424).  y = depthwise 7x7 convolution of x
 *                      (padding 3, taps outside the plane read zero; dw_weight [channels, 49], nn.Conv2d's [C,1,7,7]) +
 *                      dw_bias: bias first, then the taps in (ky, kx) order, one fma each.  out [planes*height*width,
 *                      channels] = LayerNorm over the channels of y (two-pass mean / variance, eps as given; the
 *                      reference uses 1e-6) * ln_weight + ln_bias.  y_dev: NULL, or [planes, height, width, channels],
 *                      receives y -- what the backward reads.  channels: a multiple of 64 in [64, 512].
 * ..._backward         from x, the stored y and dnorm = dLoss/d out [planes*height*width, channels]: LayerNorm backward
 *                      with mean and rstd recomputed as the forward computes them (amav_add_layernorm_backward's
 *                      formulas), then dx = the same stencil over dy with the flipped kernel, d_dw_weight [channels, 49],
 *                      d_dw_bias, d_ln_weight, d_ln_bias [channels].  The four parameter gradients are two-stage sums
 *                      in amav_rows_colsum's scheme: LayerNorm's over chunks of 16 rows (ascending rows, then ascending
 *                      chunks); the depthwise ones over the 8 x 8 pixel tiles of the stencil (inside a tile row-major,
 *                      two rows per wave, then the four waves in order; then the tiles ascending over plane, tile row,
 *                      tile column).  dx of a plane does not depend on the other planes of the call.  workspace:
 *                      amav_dwconv7_layernorm_backward_workspace_bytes bytes (0 = bad sizes).
 * amav_gelu_bias       ConvNeXtBlock's act (:417, exact erf): out [rows, inner] = gelu(proj + bias); proj [rows, inner]
 *                      with row stride proj_row_stride floats (a multiple of 4), bias [inner] may be NULL; inner a
 *                      multiple of 4 (of 8 for a split operand).
 * ..._backward         dproj = dout (Phi(g) + g phi(g)) with g = proj + bias recomputed; the bias gradient is
 *                      amav_rows_colsum(dproj), one group.
 * amav_patch4_gather   the im2col of the strided convolution: out [planes*Ho*Wo, 16*channels], column (4 ky + kx) *
 *                      channels + c of window (k, oy, ox) = x[k, oy*stride - 1 + ky, ox*stride - 1 + kx, c], +0 outside
 *                      the plane; Ho = (height - 2) / stride + 1, Wo likewise.  The convolution is out times the weight
 *                      permuted to [C_out, ky, kx, C_in].  stride >= 2, height, width >= 2, channels a multiple of 4 (of 8
 *                      for a split operand).
 * ..._backward         the transpose: dx [planes, height, width, channels] = the sum of dcols over the at most
 *                      ceil(4 / stride)^2 windows that cover the pixel, in ascending window index; +0 where no window
 *                      does (stride > 4, or rows / columns past the last window). */
int amav_dwconv7_layernorm(int planes, int height, int width, int channels, const float *x_dev,
                           const float *dw_weight_dev, const float *dw_bias_dev, const float *ln_weight_dev,
                           const float *ln_bias_dev, float eps, float *y_dev /* may be NULL */, float *out_dev,
                           void *out_split_dev, int split_format, int split_scale_exp, void *stream);
size_t amav_dwconv7_layernorm_backward_workspace_bytes(int planes, int height, int width, int channels);
int amav_dwconv7_layernorm_backward(int planes, int height, int width, int channels, const float *x_dev,
                                    const float *y_dev, const float *dw_weight_dev, const float *ln_weight_dev, float eps,
                                    const float *dnorm_dev, float *dx_dev, float *d_dw_weight_dev, float *d_dw_bias_dev,
                                    float *d_ln_weight_dev, float *d_ln_bias_dev, void *workspace, size_t workspace_bytes,
                                    void *stream);
int amav_gelu_bias(int64_t rows, int inner, const float *proj_dev, int64_t proj_row_stride, const float *bias_dev,
                   float *out_dev, void *out_split_dev, int split_format, int split_scale_exp, void *stream);
int amav_gelu_bias_backward(int64_t rows, int inner, const float *proj_dev, int64_t proj_row_stride, const float *bias_dev,
                            const float *dout_dev, float *dproj_dev, int64_t dproj_row_stride, void *stream);
int amav_patch4_gather(int planes, int height, int width, int channels, int stride, const float *x_dev, float *out_dev,
                       void *out_split_dev, int split_format, int split_scale_exp, void *stream);
int amav_patch4_gather_backward(int planes, int height, int width, int channels, int stride, const float *dcols_dev,
                                float *dx_dev, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Point refiner: the sparse / serialised operators of the reference's
 * PointTransformerV3 (src/models/point_transformer/pointtransformer_v3.py:81-145,328-499,618-759; point_encoder.py:25-40;
 * called from src/models/renderer.py:143-151) over a batch of CLOUDS (one per frame; n = all their points, a
 * cloud's points contiguous).  Replaces spconv.SubMConv3d (hash-table submanifold convolution), torch_scatter.segment_csr
 * and the padded-patch softmax attention.  Deterministic semantics (oracle/ptv3.py header): per-cloud
 * grid origin / depth / patch size, stable sorts, a voxel is seen by its neighbours through its lowest row.
 *
 * amav_cloud_voxelize   grid [n,3] = floor(resolution * p) - per-cloud minimum; cloud_depth [clouds] = bit length of
 *                       the cloud's largest grid coordinate; bounds [clouds,6] int32 scratch.     (point_encoder.py:33)
 * amav_cloud_codes      keys [4,n] int64 = cloud << 48 | code for the orders z, z-trans, hilbert, hilbert-trans
 *                       (serialization/default.py:10-27, z_order.py:86-118, hilbert.py:93-190); a stable sort of a row
 *                       orders every cloud at once.
 * amav_cloud_neighbors  nbr [n, ksize^3] int32: row gathered by tap (a,b,c) (offset (a,b,c) - ksize/2 on x,y,z), -1
 *                       where the voxel is empty; centre tap = the row itself.  sorted_keys / order: the z-order keys
 *                       ascending and the rows in that order; cloud_start [clouds+1] int32.         (spconv SubMConv3d)
 * amav_subm_pair_gemm   the convolution's products, only where a voxel exists: pairs grouped by tap (tap_start [taps+1]
 *                       int32), pair p of tap t: products[p] [cout] = feat[pair_src[p]] [cin] x weights[t] [cin][cout]
 *                       (weights [taps,cin,cout]); tile_start [taps+1] int32 = prefix sum of ceil(pairs of tap / 128),
 *                       tiles = its last entry; cin, cout multiples of 32.  fp32 MFMA.
 * amav_subm_pair_gemm_split  the same products as three fp16 partial products per fp32 product on the 16-bit MFMA pipe
 *                       (fp32 accumulation, the fp32 result to 2^-22): weights_split = the buffer of
 *                       amav_subm_prepare_weights_split (weights as two fp16 parts scaled by one power of two, in MFMA
 *                       fragment order; prepare once per layer into 256-byte aligned memory of
 *                       amav_subm_weights_split_bytes); feat [n_rows, cin] is scaled by one power of two from its largest
 *                       magnitude, measured by a pre-pass into scratch16 (16 bytes of device memory).
 * amav_subm_pair_sum    out [n,cout] = bias + sum over taps (ascending) of products[pair_of[i][tap]] (pair_of [n,taps]
 *                       int32, -1: no voxel); bias may be NULL.
 * amav_patch_attention  out [n, heads*head_dim] = softmax(q k^T * scale) v inside patches of a serialised order.
 *                       qkv [n, 3*heads*head_dim] (q | k | v, head-major inside each); order [n] int64 rows in serialised
 *                       order; patch_desc [patches,4] int32 = {first sorted position, K, own, 0}: slot j of the patch is
 *                       sorted position first + j for j < own and first + j - K otherwise (a cloud's last patch borrows
 *                       the tail of the one before, pointtransformer_v3.py:419-432); only slots < own are stored.
 *                       head_dim in {16, 32, 64}; max_patch = largest K.                (pointtransformer_v3.py:449-499)
 * amav_cluster_max      out [clusters,C] = gelu(scale * max over rows members[seg[j]..seg[j+1]) of x + shift)
 *                       (segment_csr 'max' + BatchNorm(eval) + GELU, pointtransformer_v3.py:693-719)
 * amav_bn_gelu          out = gelu(x * scale + shift), [rows, C]                                    (:785-788,738-744)
 * amav_unpool_merge     skip = gelu(x * scale + shift); sum = skip + up[cluster[row]]               (:748-755)
 * amav_rows_norm        out_sum = base + (weight_a ? LayerNorm_a(x) : x); out_norm = LayerNorm_b(out_sum), rows of
 *                       channels in {32, 64, 128, 256, 512}: `feat + cpe(...)` + norm1 and `feat + attn` + norm2 of a
 *                       Block in one pass each (:595-609); weight_a / bias_a may both be NULL.
 */
int amav_cloud_voxelize(int64_t n, int clouds, const float *points_dev, const int32_t *cloud_of_dev, float resolution,
                        int32_t *grid_dev, int32_t *cloud_depth_dev, int32_t *bounds_dev, void *stream);
int amav_cloud_codes(int64_t n, const int32_t *grid_dev, const int32_t *cloud_of_dev, const int32_t *cloud_depth_dev,
                     int64_t *keys_dev, void *stream);
int amav_cloud_neighbors(int64_t n, int ksize, const int32_t *grid_dev, const int32_t *cloud_of_dev,
                         const int32_t *cloud_depth_dev, const int32_t *cloud_start_dev, const int64_t *sorted_keys_dev,
                         const int64_t *order_dev, int32_t *nbr_dev, void *stream);
int amav_subm_pair_gemm(int64_t pairs, int tiles, int taps, int cin, int cout, const float *feat_dev,
                        const int32_t *pair_src_dev, const int32_t *tap_start_dev, const int32_t *tile_start_dev,
                        const float *weights_dev, float *products_dev, void *stream);
size_t amav_subm_weights_split_bytes(int taps, int cin, int cout);
int amav_subm_prepare_weights_split(int taps, int cin, int cout, const float *weights_dev, void *out_dev,
                                    size_t out_bytes, void *stream);
int amav_subm_pair_gemm_split(int64_t pairs, int tiles, int taps, int cin, int cout, int64_t n_rows,
                              const float *feat_dev, const int32_t *pair_src_dev, const int32_t *tap_start_dev,
                              const int32_t *tile_start_dev, const void *weights_split_dev, void *scratch16_dev,
                              float *products_dev, void *stream);
int amav_subm_pair_sum(int64_t n, int taps, int cout, const float *products_dev, const int32_t *pair_of_dev,
                       const float *bias_dev, float *out_dev, void *stream);
int amav_patch_attention(int patches, int max_patch, int heads, int head_dim, const float *qkv_dev,
                         const int64_t *order_dev, const int32_t *patch_desc_dev, float *out_dev, float scale,
                         void *stream);
int amav_cluster_max(int64_t clusters, int channels, const float *x_dev, const int64_t *members_dev,
                     const int64_t *seg_dev, const float *scale_dev, const float *shift_dev, float *out_dev, void *stream);
int amav_bn_gelu(int64_t rows, int channels, const float *x_dev, const float *scale_dev, const float *shift_dev,
                 float *out_dev, void *stream);
int amav_rows_norm(int64_t rows, int channels, const float *x_dev, const float *base_dev, const float *weight_a_dev,
                   const float *bias_a_dev, const float *weight_b_dev, const float *bias_b_dev, float eps,
                   float *out_sum_dev, float *out_norm_dev, void *stream);
int amav_unpool_merge(int64_t rows, int channels, const float *x_dev, const float *scale_dev, const float *shift_dev,
                      const float *up_dev, const int64_t *cluster_dev, float *skip_dev, float *sum_dev, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Backward of the point refiner's operators (csrc/cloud_backward.hip).  Deterministic: no atomics,
 * every sum in a fixed order; exact fp32 products on the matrix pipe.  No entry point synchronises with the host.
 *
 * amav_patch_attention_lse   amav_patch_attention that also writes lse [n, heads]: the log-sum-exp (natural units) of
 *                       every own query row's scaled scores.  out is amav_patch_attention's bit for bit.
 * amav_patch_attention_backward  grad_qkv [n, 3*heads*head_dim] (dq | dk | dv, point order, fully overwritten) from qkv,
 *                       the forward's out and lse and grad_out [n, heads*head_dim].  A row is a query of one patch; as a key
 *                       it can also sit in a borrowed slot of its cloud's last patch: dk / dv = own patch's part + the
 *                       borrowing patch's part, added in that order.  workspace:
 *                       amav_patch_attention_backward_workspace_bytes(n, heads, head_dim) bytes (0 = bad sizes).
 * amav_subm_pair_sum_csr  out [n, channels] (+)= sum over r in [src_start[i], src_start[i+1]) with
 *                       pair_lo <= src_pairs[r] < pair_lo + pair_count of products[src_pairs[r] - pair_lo]: the transposed
 *                       ordered sum of the convolution (products = amav_subm_pair_gemm of grad_out with pair_dst as the
 *                       gather index and the per-tap transposed weights [taps, cout, cin]).  src_pairs [P] int32 = stable
 *                       sort of pair_src (a row's pairs ascend), src_start [n+1] int32.  accumulate != 0 adds to out: a
 *                       sweep over consecutive pair ranges adds in the order of one call over all pairs.
 * amav_subm_pair_wgrad  grad_weights [taps, cin, cout] = per tap, sum over its pairs of feat[pair_src[p]]^T (x)
 *                       grad_out[pair_dst[p]]; zeros for a tap without pairs.  Split over slices of `chunk` pairs (a
 *                       multiple of 128) of one tap: slice_start [taps+1] int32 = prefix sum of ceil(pairs of tap / chunk),
 *                       slices = its last entry; partial matrices go to the workspace
 *                       (amav_subm_pair_wgrad_workspace_bytes(slices, cin, cout), 0 = bad sizes) and are added in slice
 *                       order.  cin, cout multiples of 32.
 * amav_cluster_max_backward  backward of amav_cluster_max: grad_z [clusters, C] = grad_out * gelu'(x_max * scale + shift),
 *                       x_max [clusters, C] the raw maxima (the scale / shift gradients are column sums of grad_z * x_max
 *                       and grad_z); grad_x [n, C]: grad_z * scale on the first member, in segment order, that attains the
 *                       maximum, zero on every other row of the segment (every row is written once).
 * amav_cluster_sum      out [clusters, C] = sum of x[members[r]] over r in [seg[j], seg[j+1]) in that order: the backward
 *                       of the up[cluster] gather of amav_unpool_merge.
 */
int amav_patch_attention_lse(int patches, int max_patch, int heads, int head_dim, const float *qkv_dev,
                             const int64_t *order_dev, const int32_t *patch_desc_dev, float *out_dev, float *lse_dev,
                             float scale, void *stream);
size_t amav_patch_attention_backward_workspace_bytes(int64_t n, int heads, int head_dim);
int amav_patch_attention_backward(int64_t n, int patches, int max_patch, int heads, int head_dim, const float *qkv_dev,
                                  const int64_t *order_dev, const int32_t *patch_desc_dev, const float *out_dev,
                                  const float *lse_dev, const float *grad_out_dev, float *grad_qkv_dev, float scale,
                                  void *workspace, size_t workspace_bytes, void *stream);
int amav_subm_pair_sum_csr(int64_t n, int channels, const float *products_dev, int64_t pair_lo, int64_t pair_count,
                           const int32_t *src_start_dev, const int32_t *src_pairs_dev, int accumulate, float *out_dev,
                           void *stream);
size_t amav_subm_pair_wgrad_workspace_bytes(int slices, int cin, int cout);
int amav_subm_pair_wgrad(int64_t pairs, int slices, int chunk, int taps, int cin, int cout, const float *feat_dev,
                         const float *grad_out_dev, const int32_t *pair_src_dev, const int32_t *pair_dst_dev,
                         const int32_t *tap_start_dev, const int32_t *slice_start_dev, float *grad_weights_dev,
                         void *workspace, size_t workspace_bytes, void *stream);
int amav_cluster_max_backward(int64_t clusters, int channels, const float *x_dev, const int64_t *members_dev,
                              const int64_t *seg_dev, const float *scale_dev, const float *shift_dev,
                              const float *grad_out_dev, float *grad_x_dev, float *grad_z_dev, float *x_max_dev,
                              void *stream);
int amav_cluster_sum(int64_t clusters, int channels, const float *x_dev, const int64_t *members_dev, const int64_t *seg_dev,
                     float *out_dev, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Train-mode BatchNorm of the point refiner (csrc/cloud_norm.hip): the statistics of a batch of
 * rows, the backward through them, and the pooling maximum on its own (in pooling the BatchNorm follows the maximum,
 * pointtransformer_v3.py:693-719, so its statistics are over the pooled rows).  fp32, kernel launches only, no host
 * synchronisation, no atomics; every sum in an order fixed by (rows, channels): a call is deterministic bit for bit.
 * channels: a multiple of 4.  rows >= 2 (one value per channel has no batch statistics; torch refuses it too).
 * The train-mode forward is amav_bn_gelu / amav_unpool_merge with scale = weight * rstd, shift = bias - mean * scale.
 *
 * amav_bn_batch_stats   mean [C], var [C] (biased: divided by rows) of the columns of x [rows, C].  Rows are cut into
 *                       chunks of 64; a chunk is summed about its own first row (the pivot) and becomes (count, mean, M2);
 *                       chunks are merged with the pairwise update of Chan, Golub & LeVeque, so a large common offset of a
 *                       column costs no digits and a constant column has var = 0 exactly.  workspace:
 *                       amav_bn_batch_stats_workspace_bytes(rows, channels) bytes (0 = bad sizes; one size serves this
 *                       entry and the backward, whose fp64 partial sums are the larger need).
 * amav_bn_gelu_train_backward  backward of y = gelu(xhat * weight + bias), xhat = (x - mean) * rstd, through the batch
 *                       statistics.  With g = grad_out * gelu'(xhat * weight + bias) (exact erf, recomputed):
 *                       grad_bias [C] = sum of g, grad_weight [C] = sum of g * xhat,
 *                       grad_x [rows, C] = weight * rstd * (g - grad_bias / rows - xhat * grad_weight / rows).
 *                       One pass over x and grad_out makes the column sums, a second pass makes grad_x.  The sums are
 *                       accumulated in fp64 (grad_bias / grad_weight are their roundings) and grad_x is evaluated in fp64
 *                       about the column means of g and of xhat, then rounded once: every column of grad_x sums to zero
 *                       to 2^-24 of its absolute sum at any row count, two rows included.  workspace:
 *                       amav_bn_batch_stats_workspace_bytes(rows, channels) bytes.
 * amav_cluster_max_raw  out [clusters, C] = max over rows members[seg[j] .. seg[j+1]) of x: amav_cluster_max without scale,
 *                       shift and GELU.
 * amav_cluster_max_route  grad_x [n, C] from grad_max [clusters, C]: the whole gradient to the first member, in segment
 *                       order, that attains the maximum, zero on every other row of the segment (amav_cluster_max_backward's
 *                       rule; every row of a segment is written once).
 */
size_t amav_bn_batch_stats_workspace_bytes(int64_t rows, int channels);
int amav_bn_batch_stats(int64_t rows, int channels, const float *x_dev, float *mean_dev, float *var_dev, void *workspace,
                        size_t workspace_bytes, void *stream);
int amav_bn_gelu_train_backward(int64_t rows, int channels, const float *x_dev, const float *mean_dev, const float *rstd_dev,
                                const float *weight_dev, const float *bias_dev, const float *grad_out_dev, float *grad_x_dev,
                                float *grad_weight_dev, float *grad_bias_dev, void *workspace, size_t workspace_bytes,
                                void *stream);
int amav_cluster_max_raw(int64_t clusters, int channels, const float *x_dev, const int64_t *members_dev,
                         const int64_t *seg_dev, float *out_dev, void *stream);
int amav_cluster_max_route(int64_t clusters, int channels, const float *x_dev, const int64_t *members_dev,
                           const int64_t *seg_dev, const float *grad_max_dev, float *grad_x_dev, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Library GEMM of the fp16 x 2 split projections: out[rows, n] fp32 = alpha * a[rows, k3] x
 * w[n, k3]^T with fp16 operands and fp32 accumulation -- the three partial products of an fp32-equivalent nn.Linear
 * (src/models/transformers.py:70-84, 448, 505) concatenated along K.  hipBLASLt does the arithmetic; `algo_index` names
 * one of its kernels (as found by amav_gemm_split_fp16_tune for this shape on this library build), -1 or an index the
 * library does not accept selects its own heuristic's choice; -2 runs this library's own kernel instead (n % 128 == 0,
 * k3 = 3 K with K % 32 == 0, operands laid out [h2 | h1 | h1] and [g1 | g2 | g1]: it reads the first two thirds and issues
 * the three partial products itself; correct, 70-80 % of the tuned library kernels' speed, not on the product path).  `workspace` may be NULL for kernels that need none.
 * amav_gemm_split_fp16_tune synchronises: it times every kernel of the library on the given operands (`repeats` runs
 * each; with `copies` > 1 the three buffers hold that many consecutive operand sets and run i uses set i % copies, which
 * times a kernel as it runs inside the step, not out of a hot L2) and reports the fastest one's index and time next to
 * the heuristic choice's time.
 * amav_gemm_library_version: the library build the indices belong to. */
int amav_gemm_split_fp16(int64_t rows, int n, int k3, const void *a_fp16, const void *w_fp16, float alpha, float *out_dev,
                         int algo_index, void *workspace, size_t workspace_bytes, void *stream);
int amav_gemm_split_fp16_tune(int64_t rows, int n, int k3, const void *a_fp16, const void *w_fp16, float *out_dev, void *workspace,
                              size_t workspace_bytes, int repeats, int copies, int32_t *best_index, float *best_ms,
                              float *heuristic_ms, void *stream);
const char *amav_gemm_library_version(void);

/* ------------------------------------------------------------------------------------------------------------
 * The tail of a training step (csrc/optimizer.hip): Lightning's clip of the global L2 norm of all
 * gradients (trainer_factory.py:44-45, gradient_clip_val = 1.0 -> torch.nn.utils.clip_grad_norm_) and torch.optim.Adam's
 * update (lightning_model_wrapper.py:366-382, 642-658), over any number of fp32 tensors in three launches.  No atomics,
 * no host synchronisation, every sum in an order fixed by the tables: a call is deterministic bit for bit.
 *
 * Tables (device memory, written by the caller, never read on the host -- the contract below is the caller's):
 *   tensors [num_tensors] amav_optim_tensor: the four addresses of a tensor (4-byte aligned is enough; 16-byte aligned
 *                         addresses take the 16-byte path), its element count and the index of its amav_optim_group.
 *   chunks  [num_chunks]  amav_optim_chunk: elements [start, min(start + chunk, numel)) of tensor `tensor`.  The chunks
 *                         partition every tensor (no element twice: two chunks of one update must not overlap), ordered
 *                         by (tensor, start); a tensor of 0 elements has no chunk.  One work-group handles one chunk;
 *                         with more than 2048 chunks work-group b takes chunks b, b + 2048, ... .  A chunk whose tensor,
 *                         start or group index is out of range is skipped by the kernels (it adds 0 to the norm).
 * `chunk` (elements, > 0) is the caller's choice: it sets the granularity of the work and of the partial sums.
 *
 * amav_grad_norm_clip   partial[c] (fp64 [num_chunks], `partial_dev`) = the sum of grad^2 over chunk c, accumulated in
 *                       fp64 from exact fp64 squares: per lane in element order, a shuffle tree inside the wave, the 4 waves
 *                       in order.  Then one work-group adds the partials (fp64; lane l takes l, l + 256, ... in order, then
 *                       the same tree) and writes norm_dev[0] = (float)sqrt(sum) and
 *                       norm_dev[1] = min(1, max_norm / (norm_dev[0] + 1e-6f)) in fp32 (clip_grad_norm_'s coefficient; a NaN
 *                       norm gives a NaN coefficient, as torch.clamp does).  num_tensors == 0 or num_chunks == 0: no table is
 *                       needed and norm_dev = {0, 1}.
 * amav_adam_step        per element, fp32, with h = groups[tensor.group] and c = *coef_dev (NULL: 1):
 *                           g = grad * c;  if (h.weight_decay != 0) g += h.weight_decay * param
 *                           exp_avg    += h.one_minus_beta1 * (g - exp_avg)
 *                           exp_avg_sq  = h.beta2 * exp_avg_sq + h.one_minus_beta2 * g * g
 *                           param      -= h.step_size * (exp_avg / (sqrt(exp_avg_sq) * h.inv_sqrt_bc2 + h.eps))
 *                       torch.optim.Adam's single-tensor formula (eps outside the bias-corrected root).  `groups` is a HOST
 *                       array of num_groups <= AMAV_OPTIM_MAX_GROUPS entries, passed to the kernel by value: the caller
 *                       computes step_size = lr / (1 - beta1^t) and inv_sqrt_bc2 = 1 / sqrt(1 - beta2^t) in double per step
 *                       and nothing has to be uploaded.  grad is only read (the clipped gradient is never stored), unless
 *                       zero_grad != 0: then the same pass stores zeros to it.  28 bytes of traffic per element (32 with
 *                       zero_grad) after the norm's 4.  The version counters of the tensors are the caller's to bump.
 */
#define AMAV_OPTIM_MAX_GROUPS 16
typedef struct amav_optim_tensor {
    float *param;
    float *grad;
    float *exp_avg;
    float *exp_avg_sq;
    int64_t numel;
    int32_t group;
    int32_t reserved;
} amav_optim_tensor;
typedef struct amav_optim_chunk {
    int64_t start;
    int32_t tensor;
    int32_t reserved;
} amav_optim_chunk;
typedef struct amav_optim_group {
    float step_size;    /* lr / (1 - beta1^t) */
    float inv_sqrt_bc2; /* 1 / sqrt(1 - beta2^t) */
    float beta1;
    float beta2;
    float one_minus_beta1;
    float one_minus_beta2;
    float eps;
    float weight_decay;
} amav_optim_group;
int amav_grad_norm_clip(const void *tensors_dev, int num_tensors, const void *chunks_dev, int num_chunks, int chunk,
                        float max_norm, void *partial_dev, float *norm_dev, void *stream);
int amav_adam_step(const void *tensors_dev, int num_tensors, const void *chunks_dev, int num_chunks, int chunk,
                   const amav_optim_group *groups, int num_groups, const float *coef_dev, int zero_grad, void *stream);

/* The data-parallel step ("Data-parallel step"): the gradients of every tensor, scaled, into one
 * bucket that a collective averages in place; the two entry points above then run from a second table whose grad
 * addresses point into the bucket.  Same tables, same chunk rules, same skip of out-of-range entries as above.
 *
 * amav_grads_pack           bucket[offsets[t] + i] = scale * tensors[t].grad[i] for every element of every chunk: one
 *                           correctly rounded fp32 multiply.  A tensor whose grad is NULL contributes zeros (the parameter
 *                           was not used on this rank).  zero_source != 0: store 0 to grad[i] after reading it.
 *                           offsets_dev: int64 [num_tensors], in elements.  A chunk is skipped when its tensor index or
 *                           start is out of range, or when offsets[t] is negative or offsets[t] + numel exceeds
 *                           bucket_numel.  Only elements [offsets[t], offsets[t] + numel) are written, never the gaps
 *                           between tensors; the bucket overlaps no gradient.  16-byte loads and stores where the chunk's
 *                           first element is 16-byte aligned in the gradient and in the bucket (ops.bucket_offsets keeps
 *                           the bucket side aligned).  8 bytes of traffic per element, 12 with zero_source.  Nothing to
 *                           pack (num_tensors == 0 or num_chunks == 0): returns 0 without a launch or a table.
 * amav_tensors_fingerprint  out_dev[0] (uint64) = the sum over all elements of all chunks of the element's 32 bits,
 *                           zero-extended to 64 bits, modulo 2^64, of the array `which`: 0 param, 1 grad, 2 exp_avg,
 *                           3 exp_avg_sq; a NULL address contributes 0.  partial_dev: uint64 [num_chunks], one sum per
 *                           chunk, which one work-group then adds.  num_tensors == 0 or num_chunks == 0: out_dev[0] = 0,
 *                           no table and no partial_dev needed.  Equal fingerprints do not prove equal arrays: the sum does
 *                           not see two elements swapped.
 * Neither uses atomics.
 */
int amav_grads_pack(const void *tensors_dev, int num_tensors, const void *chunks_dev, int num_chunks, int chunk,
                    const int64_t *offsets_dev, float *bucket_dev, int64_t bucket_numel, float scale, int zero_source,
                    void *stream);
int amav_tensors_fingerprint(const void *tensors_dev, int num_tensors, const void *chunks_dev, int num_chunks, int chunk,
                             int which, void *partial_dev, void *out_dev, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * SMPL-X mesh overlay: the demo's second clip (src/main2.py:213-220,296-303; draw_smplx_on_image and
 * SimpleMeshRenderer.render_mesh, src/utils/graphic_utils.py:782-944, there pyrender on an offscreen GL context with one
 * scene and one host round trip per frame).  A z-buffered triangle rasterizer with flat shading and a composite over
 * the rendered frames, a whole batch of frames per call.
 *
 * Conventions of amav_points_project: E [F,4,4] row-major world-to-camera (OpenCV: x right, y down, z forward), K
 * [F,3,3] in pixels, the centre of pixel (r, c) at (c + 0.5, r + 0.5).  Five launches on the caller's stream:
 *   fill     every key of the [F,H,W] uint64 z-buffer to all ones, the counters to 0
 *   project  one thread per (frame, vertex): p_cam = E (v + transl_f), u = fx x / z + cx, v = fy y / z + cy, snapped to
 *            1/256 px as int32 fixed point (round to nearest even); everything downstream works on the snapped integers
 *   setup    one thread per (frame, face).  A face with a vertex at z < znear is dropped and counted in status[f][0]
 *            (no clipping at the near plane); otherwise a face with a snapped |u| or |v| above 2^22 units (16384 px) is
 *            dropped and counted in status[f][1] (with that guard the edge functions stay below 2^48 in int64).  A face
 *            with a vertex id outside [0, V) or with zero doubled area is skipped without a count.  Front faces have a
 *            NEGATIVE doubled area (x1-x0)(y2-y0) - (x2-x0)(y1-y0) in pixel coordinates: SMPL-X's outward,
 *            counter-clockwise-from-outside faces as the OpenCV camera sees them.  cull_backfaces != 0 drops the others;
 *            0 keeps them with their normal reversed.  Shade, per channel: min(1, shade_k[c] * max(0, n . l)) with n the
 *            unit normal of the face in camera space (from the edges E (v_k - v_0): the differences are taken in world
 *            space, where they do not cancel) and l = (0, 0, -1) the camera's headlight (pyrender's
 *            metallic-roughness diffuse term at metallic 0, roughness 1 is shade_k = 0.96 * base_color * intensity / pi;
 *            its specular lobe is left out).  A face whose clipped bounding box holds at most small_box pixel centres is
 *            rasterized by its thread; the others go to a per-frame list (integer atomicAdd, capacity T)
 *   large    a fixed grid of waves strides over that list (its length is read on the device): one wave per face, the
 *            lanes stride over the pixel centres of the box
 *   resolve  one thread per pixel: the winner's shade, or the frame's RGB (the background colour without frames)
 * Coverage is exact: int64 edge functions at (256 c + 128, 256 r + 128) with the top-left fill rule (a centre exactly on
 * an edge belongs to the face only if the interior lies to the right of the edge, or below a horizontal one), so two
 * faces that share an edge never both own a pixel and never both miss it.  Depth is perspective-correct, z = 1 / sum
 * b_i / z_i with b_i the edge value over the doubled area in fp32; the pixel keeps the smallest key
 * (bits(z) << 32) | face under integer atomicMin: nearest face, lowest id on exact ties, independent of the order the
 * faces arrive in.  No float atomics: results are bitwise reproducible and a frame does not depend on the others of
 * the batch.  Every check below is made before the first launch; no allocation, no host synchronisation. */
#define AMAV_MESH_SMALL_BOX 256
typedef struct amav_mesh_overlay_args {
    int32_t num_frames, num_verts, num_faces, height, width;
    int32_t frame_channels;    /* floats per pixel of `frames`: 3 or 4 (ignored without frames) */
    int32_t cull_backfaces;
    int32_t small_box;         /* pixel centres a face's own thread may visit; < 0: AMAV_MESH_SMALL_BOX; 0: every face
                                  takes the large tier */
    const float *vertices;     /* [F,V,3] world */
    const int32_t *faces;      /* [T,3] */
    const float *transl;       /* [F,3] added to every vertex of the frame, or NULL */
    const float *K;            /* [F,3,3] */
    const float *E;            /* [F,4,4] */
    const float *frames;       /* [F,H,W,frame_channels] contiguous; NULL: composite over `background` */
    float background[3];
    float shade_k[3];
    float znear;               /* > 0 */
    float *out_rgb;            /* [F,H,W,3] */
    float *out_depth;          /* [F,H,W] camera-space z in metres, 0 where no face covers the pixel; or NULL */
    int32_t *out_face_index;   /* [F,H,W], -1 where no face covers the pixel; or NULL */
    int32_t *out_screen;       /* [F,V,2] the snapped (u, v) in 1/256 px; or NULL */
    int32_t *out_status;       /* [F,2] faces dropped at the near plane / at the guard band; or NULL */
    float *out_shade;          /* [F,T,3] the shade of every rasterized face, 0 for a dropped one; or NULL */
    void *workspace;           /* 16-byte aligned */
    size_t workspace_bytes;
} amav_mesh_overlay_args;
/* 8 F H W (keys) + 12 F V (camera z, snapped coordinates) + 16 F T (shade, list) + 12 F (counters), every slab rounded up to
 * 256 bytes; 0 on a non-positive size, H or W above 16384, F above 65535 or F H W above 2^38. */
size_t amav_mesh_overlay_workspace_bytes(int num_frames, int num_verts, int num_faces, int height, int width);
int amav_mesh_overlay(const amav_mesh_overlay_args *args, void *stream);

/* Motion-JPEG output (csrc/jpeg.hip): a batch of frames [F,H,W] -> baseline sequential JPEG (SOF0, 8 bit, YCbCr, JFIF),
 * one complete file per frame (SOI, APP0, DQT x 2, SOF0, DHT x 4, DRI, SOS, entropy-coded data with RSTn, EOI), packed
 * back to back.  frames_dev: fp32 RGBA [F,H,W,4] (frames_are_rgba_f32 = 1, 16-byte aligned; quantised first as
 * amav_frames_to_rgb8 does: clamp, x 255, truncate) or uint8 RGB [F,H,W,3] (0); both give the same bytes for the same
 * image.  1 <= H, W <= 65535.
 * Arithmetic, all fp32: Y = 0.299 R + 0.587 G + 0.114 B, Cb = -0.168736 R - 0.331264 G + 0.5 B + 128,
 * Cr = 0.5 R - 0.418688 G - 0.081312 B + 128, not rounded; AMAV_JPEG_420 (MCU 16x16, blocks Y Y Y Y Cb Cr, chroma = mean
 * of each 2x2) or AMAV_JPEG_444 (MCU 8x8, blocks Y Cb Cr); a partial MCU replicates the last column / row; level shift
 * -128; separable orthonormal 8x8 DCT-II; level = nearest integer of coefficient / table entry; tables = T.81 Annex K
 * scaled by quality 1..100 with libjpeg's rule (s = 5000 / q below 50, else 200 - 2 q; (base s + 50) / 100 in 1..255);
 * the Annex K Huffman tables.
 * restart_rows: MCU rows per restart interval (DRI + RST0..RST7 cycling; the DC predictors reset, every interval is
 * byte aligned); 0 = no restarts.  restart_rows x MCUs per row must fit DRI's 16 bits.
 * tile_hint_dev (optional, int32 [F * ceil(H/16) * ceil(W/16)], as amav_frames_pack_tiles takes it): zero = the caller
 * knows that 16x16 tile holds nothing but background_host3 (rgb in [0,1], quantised like the frames); such an MCU takes
 * the levels of a constant block, computed once by the same code, without its pixels being read.
 *
 * amav_jpeg_num_blocks: 8x8 blocks of the batch (0 = rejected sizes).
 * amav_jpeg_coefficients: the transform stage alone: int16 levels [F, blocks in MCU-interleaved scan order, 64 zigzag]
 *   into levels_dev (16-byte aligned, levels_bytes >= 128 x blocks).  workspace: AMAV_JPEG_HINT_WORKSPACE bytes, needed
 *   with a tile hint only.
 * amav_jpeg_stream_bound: bytes the stream can need at worst (0 = rejected sizes); amav_jpeg_workspace_bytes: the
 *   workspace of amav_jpeg_encode (levels + per-interval sizes and offsets; 0 = rejected sizes).
 * amav_jpeg_encode: stream_out_dev [capacity] receives the frames; frame f is bytes frame_offsets[f] ..
 *   frame_offsets[f + 1] (int64 [F + 1], device).  Nothing is written at or beyond `capacity`; when the stream needs more,
 *   status[0] |= 1 (int32, device, zeroed by the caller) and frame_offsets[F] still holds the size that was needed: the
 *   convention of the wire format and of the rasterizer's instance capacity.  Transform, entropy pass that sizes every
 *   interval, scan, entropy pass that writes: no host synchronisation, no float atomics, the same bytes on every run.
 * Refused with an error code before any launch: quality outside 1..100, an unknown subsampling, sizes outside
 * 1..65535 or F <= 0, more than 2^31 - 1 blocks, a negative restart_rows or an interval beyond 65535 MCUs, a NULL
 * required pointer, a hint without background, a misaligned buffer, a negative capacity, and a levels buffer or
 * workspace that is NULL or too small (AMAV_ERR_WORKSPACE). */
#define AMAV_JPEG_420 420
#define AMAV_JPEG_444 444
#define AMAV_JPEG_HINT_WORKSPACE 384
int64_t amav_jpeg_num_blocks(int num_frames, int height, int width, int subsampling);
size_t amav_jpeg_stream_bound(int num_frames, int height, int width, int subsampling, int restart_rows);
size_t amav_jpeg_workspace_bytes(int num_frames, int height, int width, int subsampling, int restart_rows);
int amav_jpeg_coefficients(int num_frames, int height, int width, const void *frames_dev, int frames_are_rgba_f32,
                           int quality, int subsampling, const int32_t *tile_hint_dev, const float *background_host3,
                           void *levels_dev, size_t levels_bytes, void *workspace_dev, size_t workspace_bytes,
                           void *stream);
int amav_jpeg_encode(int num_frames, int height, int width, const void *frames_dev, int frames_are_rgba_f32, int quality,
                     int subsampling, int restart_rows, const int32_t *tile_hint_dev, const float *background_host3,
                     uint8_t *stream_out_dev, int64_t capacity, int64_t *frame_offsets_dev, int32_t *status_dev,
                     void *workspace_dev, size_t workspace_bytes, void *stream);

/* Motion-JPEG input (csrc/jpeg_decode.hip): the inverse of the above.  One call decodes num_frames baseline JPEG frames
 * (SOF0, 8 bit, one interleaved sequential scan) that share height, width and sampling: AMAV_JPEG_444 (3 components,
 * MCU 8x8, blocks Y Cb Cr), AMAV_JPEG_420 (3 components, MCU 16x16, blocks Y Y Y Y Cb Cr) or AMAV_JPEG_GRAY (1 component,
 * MCU 8x8).  The frames lie anywhere (unaligned) in stream_dev [stream_bytes]; the host has parsed their headers into
 * one amav_jpeg_frame record per frame (records_dev: the records back to back on the device, 8-byte aligned), so
 * quantisation tables, Huffman tables and the restart interval are per frame.  A record's scan range is clamped to the
 * stream buffer on the device, table indices are masked: no record makes a kernel read or write out of bounds.
 *   markers  one wave per frame searches [scan_begin, scan_end) byte-parallel for FF D0..D7 (RSTn) and FF D9 (EOI) up to
 *            the first EOI.  In entropy-coded data an FF is followed by 00 (a stuffed byte) or belongs to a marker or to
 *            the fill bytes FF FF.. before one, so a marker code preceded by FF is a marker.  Interval k starts after
 *            marker k - 1 and ends at marker k; the offsets are written in stream order (ballot + prefix count, no
 *            atomics).  status[f] = AMAV_JPEG_STATUS_MARKERS unless EOI was found, the markers number
 *            ceil(MCUs / restart_interval) (1 without DRI) and RSTn counts 0..7 cyclically; else 0.
 *   entropy  one lane per restart interval (a frame without DRI is one lane's work: correct, and slow).  The frame's
 *            DHT pairs are expanded per workgroup into 9-bit lookup tables in LDS (longer codes: the canonical
 *            first-code / count comparison per length).  Per interval: DC predictors = 0; per block DC category +
 *            extend, then AC run / size with ZRL and EOB.  Reads stay inside the interval's byte range, writes inside
 *            its own blocks.  An invalid code, a run past coefficient 63 or data that ends inside a symbol zeroes that
 *            block and the interval's remaining blocks and sets AMAV_JPEG_STATUS_ENTROPY in status[f]; an interval
 *            whose start the marker search did not find is zero levels.  Other intervals and frames are unaffected.
 *            Levels: int16 [F, blocks, 64], MCU-interleaved scan order, zigzag: the layout of amav_jpeg_coefficients.
 *   pixels   coefficient = level x table entry; separable orthonormal 8x8 inverse DCT in fp32; + 128; clamp to
 *            [0, 255], not rounded, per component sample.  4:2:0 chroma is upsampled on its ceil(H/2) x ceil(W/2) plane
 *            with the triangle filter: 3/4 of the nearer sample and 1/4 of the farther one, vertically then
 *            horizontally, neighbours clamped at the plane's edge, nothing rounded in between.  R = Y + 1.402 Cr',
 *            G = Y - 0.344136 Cb' - 0.714136 Cr', B = Y + 1.772 Cb' with Cb' = Cb - 128, Cr' = Cr - 128; rounded to
 *            nearest, clamped to 0..255.  One component: R = G = B = Y.  AMAV_JPEG_HWC_U8: uint8 [F,H,W,3];
 *            AMAV_JPEG_CHW_F32: fp32 [F,3,H,W] holding exactly uint8 / 255.0f.
 * amav_jpeg_decode_levels runs the first two stages (levels_dev 16-byte aligned, levels_bytes >= 128 x blocks);
 * amav_jpeg_decode all three.  status_dev: int32 [F], written by the call (no need to zero it).  Workspace:
 * amav_jpeg_decode_workspace_bytes (levels_only != 0 for amav_jpeg_decode_levels); 0 = rejected sizes.  No allocation,
 * no host synchronisation, no memset, no float atomics; the same bytes on every run, and a frame does not depend on the
 * others of the batch.  Refused with an error code before any launch: F outside 1..65535, H or W outside 1..65535, more
 * than 2^31 - 1 blocks, an unknown sampling or layout, a NULL or misaligned pointer, a negative stream_bytes, and an
 * output, levels buffer or workspace that is too small (AMAV_ERR_WORKSPACE). */
#define AMAV_JPEG_GRAY 400
#define AMAV_JPEG_HWC_U8 0
#define AMAV_JPEG_CHW_F32 1
#define AMAV_JPEG_STATUS_MARKERS 1
#define AMAV_JPEG_STATUS_ENTROPY 2
typedef struct amav_jpeg_frame {
    int64_t scan_begin, scan_end; /* bytes of stream_dev: first byte after SOS .. end of the frame (EOI included) */
    int32_t restart_interval;     /* MCUs per interval (DRI); 0 = none */
    int32_t reserved;
    uint8_t quant[192];           /* [component][zigzag position]: the component's DQT entries as the file has them */
    uint8_t dc_counts[48];        /* [component][length - 1]: codes of length 1..16 of the component's DC table */
    uint8_t dc_values[48];        /* [component][16] */
    uint8_t ac_counts[48];
    uint8_t ac_values[768];       /* [component][256] */
} amav_jpeg_frame;
size_t amav_jpeg_decode_workspace_bytes(int num_frames, int height, int width, int sampling, int levels_only);
int amav_jpeg_decode_levels(int num_frames, int height, int width, int sampling, const uint8_t *stream_dev,
                            int64_t stream_bytes, const void *records_dev, void *levels_dev, size_t levels_bytes,
                            int32_t *status_dev, void *workspace_dev, size_t workspace_bytes, void *stream);
int amav_jpeg_decode(int num_frames, int height, int width, int sampling, const uint8_t *stream_dev, int64_t stream_bytes,
                     const void *records_dev, int layout, void *out_dev, size_t out_bytes, int32_t *status_dev,
                     void *workspace_dev, size_t workspace_bytes, void *stream);

/* Training-clip frame preparation (csrc/frame_prep.hip): what the reference's dataset does to every frame on the CPU
 * (src/datasets/dataset_speech_vid.py:170-252, pad_image :319-331), for num_frames frames of one size H x W per call.
 *   frames_dev  uint8 (frames_are_f32 = 0; the value is byte / 255.0f) or fp32, read in place at element
 *               f frame_stride_f + c frame_stride_c + y frame_stride_y + x frame_stride_x (strides in elements): the
 *               decoder's [F,H,W,3] and [F,3,H,W], or any view of them.  The strides inside a frame (c, y, x) are not
 *               negative and one frame's view spans fewer than 2^31 elements; the frame stride is free.
 *   masks_dev   uint8 (byte / 255.0f) or fp32 in [0,1] at f mask_stride_f + y mask_stride_y + x mask_stride_x; NULL =
 *               all ones.
 *   images_dev  fp32 [F,3,Hp,Wp]: ones, and at (offset_y, offset_x) the frame composited over white,
 *               image * mask + (1 - mask), each operator rounded to fp32 on its own (:184, pad_image).
 *   boxes_dev   int32 [F,5]: y_min, y_max, x_min, x_max (inclusive, as finally used) and max_size.  The bounding box of
 *               mask != 0 grows by extent / 5 (= int(extent * 0.2)), is clamped to H - 1, W - 1, made square around its
 *               centre with crop_size // 2 and clamped again (:195-216).  It is found in frame coordinates and applied to
 *               the padded image as it is, as the reference does.  An empty mask: the whole padded image.
 *               max_size = max(y_max - y_min, x_max - x_min) + 1.
 *   cropped_dev fp32 [F,3,S,S], S = crop_side: the crop, centred in a square of ones of side max_size ((max_size - w) / 2
 *               columns on the left, (max_size - h) / 2 rows on top, :227-244), resized with torch's bilinear,
 *               align_corners=True: scale = float(max_size - 1) / float(S - 1) (0 for S = 1), src = scale * dst,
 *               i0 = (int)src, i1 = min(i0 + 1, max_size - 1), w1 = src - i0, w0 = 1 - w1,
 *               value = h0 (w0 p00 + w1 p01) + h1 (w0 p10 + w1 p11), fp32, nothing contracted.  The taps are composited
 *               on the fly, so images_dev is not read.  max_size == S takes the same path with scale 1 (the square image
 *               itself; the reference skips its resize there and returns the crop before squaring).  With mean_host3 /
 *               std_host3 (both or neither) the stored value is (value - mean[c]) / std[c], an IEEE division.
 * Each output is optional (NULL = not produced, its buffer is not touched).  At most three launches on `stream` (images
 * + box table initialisation, box reduction with integer atomicMin / atomicMax, cropped); no allocation, no memset, no
 * float atomics, no host synchronisation; the same bits on every run.  workspace: amav_frames_prepare_workspace_bytes
 * (0 = rejected F), needed when cropped_dev or boxes_dev is given.  Refused with an error code before any launch: NULL
 * frames, F outside 1..16384, H, W, Hp, Wp or crop_side outside 1..65535, Hp < H or Wp < W, offsets that put the frame
 * outside the padded image, a flag other than 0 / 1, a negative or too large stride inside a frame, mean without std,
 * a std of zero, a misaligned buffer (images, cropped, workspace: 16 bytes), and an output buffer or workspace that is
 * too small (AMAV_ERR_WORKSPACE). */
size_t amav_frames_prepare_workspace_bytes(int num_frames);
int amav_frames_prepare(int num_frames, int height, int width, const void *frames_dev, int frames_are_f32,
                        int64_t frame_stride_f, int64_t frame_stride_c, int64_t frame_stride_y, int64_t frame_stride_x,
                        const void *masks_dev, int masks_are_f32, int64_t mask_stride_f, int64_t mask_stride_y,
                        int64_t mask_stride_x, int padded_height, int padded_width, int offset_y, int offset_x,
                        int crop_side, const float *mean_host3, const float *std_host3, float *images_dev,
                        size_t images_bytes, float *cropped_dev, size_t cropped_bytes, int32_t *boxes_dev,
                        size_t boxes_bytes, void *workspace_dev, size_t workspace_bytes, void *stream);

/* PNG input (csrc/png_decode.hip, csrc/png_inflate_core.h): the reference's dataset stores its frames and masks as PNG
 * (imgs_png/%05d.png, samurai_seg/%05d.png); they are inflated, unfiltered and converted on the device, bit for bit what
 * PIL's Image.open(...).convert("RGB") / .convert("L") give.
 *
 * amav_inflate decodes num_streams DEFLATE streams (RFC 1951), one wave each.  Stream n lies at bytes [in_begin, in_end)
 * of stream_dev [stream_bytes], unaligned; its output goes to out_dev [out_bytes] at out_begin, at most out_capacity
 * bytes (unaligned as well; nothing is written outside [out_begin, out_begin + out_capacity), and both ranges are clamped
 * to their buffers on the device, so no record makes the kernel read or write out of bounds).  wrapper 0: raw DEFLATE;
 * 1: zlib (RFC 1950): CMF / FLG are checked (method 8, window <= 32 KiB, the mod-31 check), a preset dictionary (FDICT)
 * is refused by status, and the 4 Adler-32 bytes after the last block are neither read nor VERIFIED.  Bytes after the
 * final block are ignored.  produced_dev: int64 [N], bytes written; status_dev: int32 [N], written by the call:
 *   AMAV_PNG_STATUS_INFLATE  a reserved block type (3); a stored block whose LEN is not ~NLEN; HLIT above 286 or HDIST
 *                            above 30; over-subscribed code lengths (an incomplete set is accepted, its unused codes are
 *                            "not in the set"); a repeat code 16 with nothing before it, or a repeat that runs past
 *                            HLIT + HDIST (it may cross from one into the other); a code not in the set; literal/length
 *                            symbol 286 / 287 or distance symbol 30 / 31; a distance that reaches before the start of
 *                            the output; input that ends before the final block's end-of-block (or inside a stored
 *                            block); a bad zlib header or FDICT.  Decoding stops there; produced = the bytes so far.
 *   AMAV_PNG_STATUS_SIZE     the stream would produce more than out_capacity bytes: decoding stops before the symbol
 *                            that would pass it.
 * workspace: amav_inflate_workspace_bytes (0 = rejected count; one 256-byte granule, the kernel keeps its state in LDS).
 * This entry point stands on its own so that the entropy stage can be held to an independent decoder on any stream.
 *
 * amav_png_decode decodes num_frames frames of one height and width; colour type and bit depth are per frame
 * (amav_png_frame, records_dev: back to back, 8-byte aligned).  The host has joined a frame's IDAT payloads into one zlib
 * stream at [zlib_begin, zlib_end) of stream_dev and put its PLTE bytes (3 x palette_entries) at palette_at.
 *   inflate   into workspace, H x (1 + rowbytes) bytes per frame, rowbytes = ceil(W x channels x depth / 8), channels
 *             1, 3, 1, 2, 4 for colour types 0, 2, 3, 4, 6; the workspace is sized for 4 bytes per pixel
 *             (amav_png_decode_workspace_bytes; 0 = rejected sizes).  AMAV_PNG_STATUS_INFLATE as above;
 *             AMAV_PNG_STATUS_SIZE also when the stream ends with fewer bytes than the frame needs.
 *   unfilter  per row by its filter byte, on bytes, with bpp = max(1, channels x depth / 8): 0 None; 1 Sub, + the byte bpp
 *             to the left; 2 Up, + the byte above; 3 Average, + floor((left + above) / 2); 4 Paeth, + whichever of left,
 *             above, above-left is nearest to left + above - above-left (ties in that order); all mod 256, bytes outside
 *             the image are 0.  A filter byte above 4 sets AMAV_PNG_STATUS_FILTER and the row is taken as filter 0.
 *   convert   pixels of fewer than 8 bits are unpacked after the filter, most significant bits first.  AMAV_PNG_RGB:
 *             colour type 2 as it is; 6: alpha dropped; 0 / 4: R = G = B = grey, a grey of depth d < 8 scaled by
 *             255 / (2^d - 1); 3: the PLTE entry.  AMAV_PNG_L: 0 / 4: grey; 2 / 6 / 3:
 *             (19595 R + 38470 G + 7471 B + 0x8000) >> 16.  tRNS, gAMA and the like never reach the device.  A palette
 *             index at or beyond palette_entries is (0, 0, 0) and is not flagged.  absent != 0: no stream; the frame is
 *             all 255 (a missing mask file).  A record whose colour type / depth pair the standard does not allow, or
 *             depth 16, is flagged INFLATE | SIZE and not decoded.
 *   out_dev   AMAV_JPEG_HWC_U8: uint8 [F,H,W,3] (RGB) / [F,H,W] (L); AMAV_JPEG_CHW_F32: fp32 [F,3,H,W] / [F,1,H,W] holding
 *             exactly uint8 / 255.0f.
 * A frame flagged INFLATE or SIZE is not unfiltered and its pixels are 0; a frame flagged FILTER alone is decoded with
 * filter 0 on the offending rows.  Either way only that frame's output is written; the other frames are not affected.  Two launches, no allocation, no memset, no float atomics, no host synchronisation; the same bytes on every
 * run.  Interlaced and 16-bit files are not decoded (png.parse_png refuses them).
 * Refused with an error code before any launch: amav_inflate: num_streams outside 1..65535, a NULL pointer, a negative
 * stream_bytes or out_bytes, misaligned records, produced (8) or status (4), a NULL, misaligned (16) or short workspace
 * (AMAV_ERR_WORKSPACE).  amav_png_decode: F outside 1..65535, H or W outside 1..16384, an unknown mode or layout, NULL
 * stream, records, status or out, a negative stream_bytes, misaligned records (8), status (4) or fp32 out (4), and an
 * output buffer or workspace that is too small, NULL or not 16-byte aligned (AMAV_ERR_WORKSPACE). */
#define AMAV_PNG_RGB 0
#define AMAV_PNG_L 1
#define AMAV_PNG_STATUS_INFLATE 1
#define AMAV_PNG_STATUS_SIZE 2
#define AMAV_PNG_STATUS_FILTER 4
typedef struct amav_inflate_stream {
    int64_t in_begin, in_end;        /* bytes of stream_dev */
    int64_t out_begin, out_capacity; /* bytes of out_dev */
    int32_t wrapper;                 /* 0 raw, 1 zlib */
    int32_t reserved;
} amav_inflate_stream;
typedef struct amav_png_frame {
    int64_t zlib_begin, zlib_end; /* bytes of stream_dev: the frame's IDAT payloads, joined */
    int64_t palette_at;           /* byte of stream_dev where the PLTE entries lie (colour type 3) */
    int32_t color_type, bit_depth, palette_entries, absent;
} amav_png_frame;
size_t amav_inflate_workspace_bytes(int num_streams);
int amav_inflate(int num_streams, const uint8_t *stream_dev, int64_t stream_bytes, const void *records_dev, uint8_t *out_dev,
                 int64_t out_bytes, int64_t *produced_dev, int32_t *status_dev, void *workspace_dev, size_t workspace_bytes,
                 void *stream);
size_t amav_png_decode_workspace_bytes(int num_frames, int height, int width);
int amav_png_decode(int num_frames, int height, int width, const uint8_t *stream_dev, int64_t stream_bytes,
                    const void *records_dev, int mode, int layout, void *out_dev, size_t out_bytes, int32_t *status_dev,
                    void *workspace_dev, size_t workspace_bytes, void *stream);

/* PNG output (csrc/png_encode.hip, csrc/png_deflate_core.h): everything the reference writes to disk as a picture is a PNG
 * (vutils.save_image sheets, plt.imsave frame dumps, the dataset's imgs_png / samurai_seg); the frames are converted,
 * filtered, deflated and framed on the device.
 *
 * amav_deflate is the counterpart of amav_inflate: num_streams byte ranges [in_begin, in_end) of in_dev [in_bytes] become
 * num_streams DEFLATE streams (RFC 1951), raw (wrapper 0) or zlib-wrapped (1: 78 01 in front, the Adler-32 behind), each
 * written to out_dev [out_bytes] from out_begin, never at or past out_begin + out_capacity.  Both ranges are clamped to
 * their buffers on the device.  produced_dev: int64 [N], the bytes the stream needs; status_dev: int32 [N], written by
 * the call: 0, or AMAV_PNG_STATUS_SIZE when the stream needs more than out_capacity (what fits, the stream's start, is
 * written; produced says how much room to come back with), or AMAV_PNG_STATUS_TABLE (below).
 *   pieces    a stream is cut into pieces of AMAV_DEFLATE_PIECE input bytes, one wave each, so a frame is compressed by
 *             as many waves as it has pieces.  A piece is coded with no reference across its start.  It ends on a byte
 *             boundary: a stored piece by itself, a Huffman piece with an empty stored block (00 00 00 ff ff); the last
 *             piece carries BFINAL instead.  The pieces back to back are one stream for any decoder.  An empty range is
 *             one empty piece.
 *   matches   LDS hash of 3-byte prefixes (4096 entries), 64 consecutive positions a step.  A position is compared with
 *             the newest position of an EARLIER step that has its hash and with the byte before it (runs); the longer
 *             match wins, the nearer on a tie; a 3-byte match farther than 4096 is dropped.  Positions of one step that
 *             share a hash leave the largest position in the table (an integer max), so the bytes do not depend on lane
 *             timing.  The parse is greedy and walked wave-uniformly: a match is taken wherever one starts.
 *   coding    literal/length and distance histograms in LDS; code lengths of at most 15 bits (7 for the code-length
 *             code): the lanes rank the symbols by frequency, one lane runs the linear in-place minimum-redundancy
 *             construction on the sorted list and moves codes up until the Kraft sum is one; the header is run-length
 *             coded with 16 / 17 / 18.  A piece without a match sends one unused distance code of one bit, a piece with
 *             one used distance code sends it with one bit.  The piece is then sized exactly as stored (5 + n bytes),
 *             fixed and dynamic, each with the empty stored block it needs, and the smallest is kept (stored, then fixed,
 *             on ties; a piece with fewer than two literal/length symbols is never dynamic).  So a stream never exceeds
 *             input + 5 bytes per piece + 6 for the wrapper.
 *   two runs  the pieces are run twice, as amav_jpeg_encode runs its entropy stage: once for sizes and Adler-32 sums
 *             (sum of bytes; sum of (n - i) x byte i), then one thread per stream lays them back to back and joins the
 *             sums (b += n a + s2, a += s1 mod 65521), then once more to write.  A piece's bytes are put together in LDS
 *             (integer OR of each token's bits at its prefix-summed bit offset) and leave in one pass.
 * workspace: amav_deflate_workspace_bytes(num_streams, in_bytes) holds the tables of in_bytes / AMAV_DEFLATE_PIECE +
 * num_streams pieces, which covers any ranges that do not overlap; a stream whose pieces no longer fit the table (ranges
 * that overlap) is not coded: AMAV_PNG_STATUS_TABLE, produced 0.  No allocation, no memset, no float atomics, no host
 * synchronisation; the same bytes on every run, and the bytes of csrc/png_deflate_core.h compiled for the host
 * (tools/png_deflate_host.cpp).
 *
 * amav_png_encode writes num_frames frames of one height and width as num_frames complete PNG files (8 bit, not
 * interlaced; no alpha, palette or 16-bit output), back to back in stream_out_dev [capacity]: frame f is bytes
 * [frame_offsets_dev[f], frame_offsets_dev[f + 1]) (int64 [F + 1]).  frames_dev is read in place:
 *   AMAV_PNG_IN_RGBA_F32  fp32 [F,H,W,4], alpha dropped      colour type 2
 *   AMAV_PNG_IN_CHW_F32   fp32 [F,3,H,W]                     colour type 2
 *   AMAV_PNG_IN_RGB_U8    uint8 [F,H,W,3]                    colour type 2
 *   AMAV_PNG_IN_GREY_U8   uint8 [F,H,W]                      colour type 0
 *   AMAV_PNG_IN_GREY_F32  fp32 [F,H,W]                       colour type 0
 * fp32 -> level: AMAV_PNG_ROUND_NEAREST is torchvision's save_image, x.mul(255).add_(0.5).clamp_(0, 255) truncated: the
 * product and the sum are rounded to fp32 separately (no fused multiply-add), so the level equals the torch expression
 * bit for bit; AMAV_PNG_ROUND_TRUNCATE is amav_frames_to_rgb8's clamp to [0, 1], x 255, truncated.  NaN -> 0.
 *   filter    one wave per scanline writes filter byte + filtered row into the workspace.  filter 0..4 (None, Sub, Up,
 *             Average, Paeth) for every row, or AMAV_PNG_FILTER_ADAPTIVE: all five per row, the smallest sum of the
 *             residuals' absolute values as signed bytes wins, the lowest filter number on ties.  The previous row is
 *             converted from the image again, so rows and pieces stay independent.
 *   deflate   as above over each frame's H x (1 + W x channels) filtered bytes, zlib-wrapped.
 *   container signature, IHDR, ONE IDAT CHUNK PER PIECE (the first holds the zlib header, the last the Adler-32), IEND.
 *             Each wave computes its chunk's CRC-32 over the staged bytes in parallel: every lane runs the register over
 *             its run of the chunk, lane 0 joins the 64 registers (register x x^(8 len) + next, modulo the polynomial).
 * status_dev: int32 [F]: 0, or AMAV_PNG_STATUS_SIZE for a frame that ends behind the capacity; frame_offsets_dev holds the
 * needed sizes either way, and nothing is written at or past the capacity.  amav_png_stream_bound: a capacity that always
 * suffices (every piece stored); amav_png_encode_workspace_bytes: filtered bytes + piece tables; both 0 for rejected
 * sizes or layout.  Six launches, no allocation, no memset, no float atomics, no host synchronisation; the same bytes on
 * every run.
 * Refused with an error code before any launch: amav_deflate: num_streams outside 1..65535, a NULL pointer, a negative
 * in_bytes or out_bytes, misaligned records, produced (8) or status (4), a NULL, misaligned (16) or short workspace
 * (AMAV_ERR_WORKSPACE).  amav_png_encode: F outside 1..65535, H or W outside 1..16384, an unknown layout, filter or
 * rounding, NULL frames, stream, frame_offsets or status, a negative capacity, misaligned fp32 frames (4), frame_offsets
 * (8) or status (4), and a workspace that is too small, NULL or not 16-byte aligned (AMAV_ERR_WORKSPACE). */
#define AMAV_DEFLATE_PIECE 8192
#define AMAV_PNG_STATUS_TABLE 8
#define AMAV_PNG_IN_RGBA_F32 0
#define AMAV_PNG_IN_CHW_F32 1
#define AMAV_PNG_IN_RGB_U8 2
#define AMAV_PNG_IN_GREY_U8 3
#define AMAV_PNG_IN_GREY_F32 4
#define AMAV_PNG_FILTER_ADAPTIVE 5
#define AMAV_PNG_ROUND_NEAREST 0
#define AMAV_PNG_ROUND_TRUNCATE 1
typedef struct amav_deflate_stream {
    int64_t in_begin, in_end;        /* bytes of in_dev */
    int64_t out_begin, out_capacity; /* bytes of out_dev */
    int32_t wrapper;                 /* 0 raw, 1 zlib */
    int32_t reserved;
} amav_deflate_stream;
size_t amav_deflate_workspace_bytes(int num_streams, int64_t in_bytes);
int amav_deflate(int num_streams, const uint8_t *in_dev, int64_t in_bytes, const void *records_dev, uint8_t *out_dev,
                 int64_t out_bytes, int64_t *produced_dev, int32_t *status_dev, void *workspace_dev, size_t workspace_bytes,
                 void *stream);
int64_t amav_png_stream_bound(int num_frames, int height, int width, int layout);
size_t amav_png_encode_workspace_bytes(int num_frames, int height, int width, int layout);
int amav_png_encode(int num_frames, int height, int width, const void *frames_dev, int layout, int filter, int rounding,
                    uint8_t *stream_out_dev, int64_t capacity, int64_t *frame_offsets_dev, int32_t *status_dev,
                    void *workspace_dev, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * The SMPL-X parameter term of the two training steps (csrc/smplx_params.hip): the decoder's
 * rot6d -> axis-angle conversion and losses.smplx_param_loss, one forward and one backward launch each.
 *
 * amav_rot6d_to_axis_angle: aa [n,3] (contiguous) = matrix_to_axis_angle(rotation_6d_to_matrix(d6)) of
 * smplx_decoder.py, branch for branch: Gram-Schmidt with F.normalize's max(||x||, 1e-12), the four quaternion
 * candidates of sqrt(max(., 0)), the one with the largest |q| divided by 2 max(|q|, 0.1), flipped to w >= 0,
 * angle = 2 atan2(||xyz||, w), and xyz / (sin(angle / 2) / angle) with the series 1/2 - angle^2 / 48 below 1e-6.
 * Row i of d6 is the six floats at d6[i * row_stride] (floats; a [B,55,6] view of a wider buffer is read in place).
 * amav_rot6d_to_axis_angle_backward: grad_d6 [n,6] (contiguous) for grad_aa [n,3]; the forward is recomputed from d6,
 * nothing is saved, and every branch (candidate, flip, small angle, the clamps' gates, the zero derivative of the
 * square root of a non-positive number) is the one the forward takes on the same d6.
 * Both refuse a negative n and NULL pointers (AMAV_ERR_INVALID_ARG, before any launch); n = 0 is AMAV_OK and no
 * pointer is looked at.  No allocation and no host synchronisation. */
int amav_rot6d_to_axis_angle(int n, const float *d6_dev, int64_t row_stride, float *aa_dev, void *stream);
int amav_rot6d_to_axis_angle_backward(int n, const float *d6_dev, int64_t row_stride, const float *grad_aa_dev,
                                      float *grad_d6_dev, void *stream);
/* One term of the parameter loss: `frames` blocks of `per_frame` consecutive items, frame f of pred starting at
 * pred[f * pred_stride] (floats), of gt at gt[f * gt_stride].  An item is one float for betas, expression and transl
 * and a rotation vector of three floats for the seven rotation keys.  So body_pose = aa[:, 1:22] of the decoder's
 * [F,55,3] (per_frame 21, pred_stride 165) and a contiguous [B,T,21,3] target (gt_stride 63) are read in place.
 * pred = gt = NULL: the term is absent and its parts are 0; so is a term with frames = 0 or per_frame = 0. */
#define AMAV_SMPLX_TERMS 10
#define AMAV_SMPLX_PARTS 12
typedef struct amav_smplx_term {
    const float *pred, *gt;
    int frames, per_frame;
    int64_t pred_stride, gt_stride; /* floats */
} amav_smplx_term;
/* term[0] betas, term[1..7] global_orient, body_pose, left_hand_pose, right_hand_pose, jaw_pose, leye_pose, reye_pose
 * (losses.ROTATION_KEYS), term[8] expression, term[9] transl */
typedef struct amav_smplx_terms {
    amav_smplx_term term[10];
} amav_smplx_terms;
/* grad[k]: NULL (no gradient wanted), or [frames, per_frame] items of term k, contiguous */
typedef struct amav_smplx_grads {
    float *grad[10];
} amav_smplx_grads;
/* Bytes of the forward's workspace: 0 while one workgroup does the whole sum (no term above 4096 items, which covers
 * every training size), else twelve doubles per workgroup (16-byte aligned); 0 as well for terms the forward
 * refuses. */
size_t amav_smplx_param_loss_workspace_bytes(const amav_smplx_terms *terms);
/* parts [12], the means of losses.smplx_param_loss in this order: betas_mse, betas_prior, the seven *_geo parts,
 * expression_l1, expression_prior, transl_smoothl1.  Geodesic part: the mean over rows of
 * acos(clamp((tr(Rp^T Rg) - 1) / 2, -0.999, 0.999)) with R = I + sin K + (1 - cos) K K of r / angle,
 * angle = ||r + 1e-8|| (1 - cos evaluated as 2 sin^2(angle / 2)); smooth-L1 with beta = 1.  Inputs and parts are fp32;
 * the arithmetic and the sums in between run in double (so do the conversion's above), the sums in a fixed order with
 * no atomics: bitwise the same on every run.  workspace: NULL is fine while the query returns 0, else
 * AMAV_ERR_WORKSPACE when it is NULL or too small. */
int amav_smplx_param_loss_forward(const amav_smplx_terms *terms, float *parts_dev, void *workspace_dev,
                                  size_t workspace_bytes, void *stream);
/* grads->grad[k] = d(sum over p of grad_parts[p] * parts[p]) / d(pred of term k), every element written exactly once;
 * grad_parts [12] is read on the device.  The gates are the forward's: the clamp passes the gradient where
 * -0.999 <= cos <= 0.999 and nowhere else, sign(0) = 0 for the L1 part, smooth-L1 is quadratic where |d| < 1.  The
 * targets get no gradient.  All three entry points refuse (AMAV_ERR_INVALID_ARG, before any launch) NULL terms /
 * parts / grads, negative counts, one NULL pointer of a pair and terms beyond 2^30 - 1 floats.  No allocation and no
 * host synchronisation. */
int amav_smplx_param_loss_backward(const amav_smplx_terms *terms, const float *grad_parts_dev,
                                   const amav_smplx_grads *grads, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* AMAV_H */
