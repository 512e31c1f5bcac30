"""Tensor-level wrappers over the C ABI (include/amav.h).  torch is used for device memory and streams only.

Every function requires CUDA(HIP) float32 tensors and raises on anything else: there is no CPU path.
"""
import copy
import ctypes
import math
import os

import torch

from . import _lib
from ._lib import (AmavError, Attr, BodyTables, Conv3x3Args, Conv3x3BackwardArgs, DecodeSource, ImageLossWindow, ImageView, LbsBackwardArgs, PoseParts,
                   RasterArgs, RasterBackwardArgs, TriplaneDecodeBackwardArgs, TriplaneSampleBackwardArgs, check)

OptimTensor, OptimChunk, OptimGroup = (_lib.STRUCTS["amav_optim_" + n] for n in ("tensor", "chunk", "group"))

SCALE_BIAS = 3.9    # src/models/renderer.py:428
OPACITY_BIAS = 0.0  # src/models/renderer.py:429
SCALE_MAX = 0.1     # src/models/renderer.py:532
TILE = _lib.DEFINES["AMAV_TILE"]                   # rasterizer tile edge, pixels
GAUSS_STRIDE = _lib.DEFINES["AMAV_GAUSS_STRIDE"]   # floats per packed Gaussian record
SPLIT_BF16X3, SPLIT_FP16X2 = _lib.DEFINES["AMAV_SPLIT_BF16X3"], _lib.DEFINES["AMAV_SPLIT_FP16X2"]
# channel offsets inside a packed record
REC_XYZ, REC_OPACITY, REC_ROT, REC_SCALE, REC_COLOR = 0, 3, 4, 8, 12


def tensor_version(t: torch.Tensor) -> int:
    """Version counter of a tensor for "has it been modified in place" cache keys, or -1 for inference tensors (created
    under torch.inference_mode(): they track no version -- reading `_version` raises -- and cannot be modified outside
    it, so identity + storage address identify their contents)."""
    return -1 if t.is_inference() else t._version


def set_option(name: str, value: str):
    """Process-wide arithmetic selection (include/amav.h, amav_set_option): attn = fp16 | bf16 | f32, lbs = split | f32,
    value "default" = the environment's choice.  The projections' GEMM format is the host-side AMAV_GEMM variable."""
    check(_lib.lib().amav_set_option(name.encode(), value.encode()), "amav_set_option")


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _call(name, *args):
    """Entry point `name` with `args` and the current stream as its last argument; a non-zero return code raises."""
    check(getattr(_lib.lib(), name)(*args, _stream()), name)


def _scratch(query, device, *sizes, rejected=None):
    """uint8 device buffer of the size the *_bytes entry point `query` reports for `sizes`.  0 bytes = the library
    refused them: the error names the entry point and `rejected` (the sizes as text; None: "the tables" and the
    library's own message)."""
    nbytes = getattr(_lib.lib(), query)(*sizes)
    if nbytes == 0:
        raise AmavError(f"{query} rejected " + (rejected or "the tables: " + _lib.lib().amav_last_error().decode()))
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def tile_count(height, width) -> int:
    """Tiles of one frame: the rasterizer's and the frame exchange's grid of AMAV_TILE x AMAV_TILE pixels."""
    return ((int(height) + TILE - 1) // TILE) * ((int(width) + TILE - 1) // TILE)


def _need(t: torch.Tensor, name: str, dtype=torch.float32):
    if not isinstance(t, torch.Tensor):
        raise AmavError(f"{name}: expected a torch.Tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise AmavError(f"{name}: tensor is on {t.device}; this package only runs on an MI355X (HIP) device")
    if t.dtype != dtype:
        raise AmavError(f"{name}: dtype {t.dtype}, expected {dtype}")
    return t


def _contig(t, name, dtype=torch.float32):
    t = _need(t, name, dtype)
    return t if t.is_contiguous() else t.contiguous()


def _attr(t: torch.Tensor, name: str, width: int) -> Attr:
    """[F,N,width] tensor (any frame/element strides, unit stride on the last axis) -> amav_attr."""
    _need(t, name)
    if t.dim() != 3 or t.shape[2] != width:
        raise AmavError(f"{name}: expected [F,N,{width}], got {tuple(t.shape)}")
    if width > 1 and t.stride(2) != 1:
        t = t.contiguous()
    return Attr(t.data_ptr(), t.stride(0), t.stride(1), 0), t


class Event:
    """hipEvent through the C ABI (bench.py times the blend kernel with a pair of these)."""

    def __init__(self):
        h = ctypes.c_void_p()
        check(_lib.lib().amav_event_create(ctypes.byref(h)), "amav_event_create")
        self.handle = h

    def record(self):
        _call("amav_event_record", self.handle)

    def elapsed_ms(self, stop) -> float:
        ms = ctypes.c_float(0)
        check(_lib.lib().amav_event_elapsed_ms(self.handle, stop.handle, ctypes.byref(ms)), "amav_event_elapsed_ms")
        return ms.value

    def __del__(self):
        try:
            _lib.lib().amav_event_destroy(self.handle)
        except Exception:
            pass


# --------------------------------------------------------------------------------------------------------- camera
def camera_from_intrinsics(K, E, height, width, znear=0.01, zfar=100.0):
    """K [F,3,3], E [F,4,4] -> (viewmatrix [F,16], projmatrix [F,16], tanfov [F,2], campos [F,3]); no host sync.

    Replaces src/models/renderer.py:486-510 (which costs >= 6 host syncs per frame in the reference).
    """
    K = _contig(K.reshape(-1, 3, 3), "K")
    E = _contig(E.reshape(-1, 4, 4), "E")
    F = K.shape[0]
    if E.shape[0] != F:
        raise AmavError(f"camera: {F} intrinsics vs {E.shape[0]} extrinsics")
    dev = K.device
    view = torch.empty(F, 16, device=dev)
    proj = torch.empty(F, 16, device=dev)
    tanfov = torch.empty(F, 2, device=dev)
    campos = torch.empty(F, 3, device=dev)
    _call("amav_camera_from_intrinsics", F, K.data_ptr(), E.data_ptr(), int(height), int(width), znear, zfar,
          view.data_ptr(), proj.data_ptr(), tanfov.data_ptr(), campos.data_ptr())
    return view, proj, tanfov, campos


# ----------------------------------------------------------------------------------------------------- rasterizer
class RasterWorkspace:
    """Caller-owned scratch of the rasterizer for one problem size (reusable across calls and hipGraph-safe)."""

    def __init__(self, num_frames, num_gaussians, height, width, instance_capacity, device):
        self.key = (num_frames, num_gaussians, height, width)
        self.capacity = int(instance_capacity)
        self.buffer = _scratch("amav_rasterize_workspace_bytes", device, *self.key, self.capacity,
                               rejected=f"{self.key} capacity={self.capacity}")

    def tile_counts(self, out=None):
        """Per-tile Gaussian list lengths of the last forward, int32 [F * tiles] (no host sync)."""
        F, N, H, W = self.key
        n = F * tile_count(H, W)
        if out is None:
            out = torch.empty(n, dtype=torch.int32, device=self.buffer.device)
        _call("amav_rasterize_tile_counts", self.buffer.data_ptr(), F, N, H, W, self.capacity, out.data_ptr())
        return out

    def status(self):
        """(total_instances, overflowed) of the last forward.  Synchronises the current stream."""
        total, _, over = self.status_full()
        return total, over

    def status_full(self):
        """(total_instances, max_instances_of_a_frame, overflowed).  Synchronises the current stream."""
        total, mx, over = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int32(0)
        _call("amav_rasterize_status", self.buffer.data_ptr(), ctypes.byref(total), ctypes.byref(mx),
              ctypes.byref(over))
        return total.value, mx.value, bool(over.value)


# A list of (Event, Event) pairs: every rasterize() call pops one and records it around its blend kernel (bench.py).
PROFILE_EVENTS = None
# diagnostic: int64 CUDA tensor [F*tiles, 6] that receives the blend kernel's per-tile clock stamps (tools/)
DEBUG_STAMPS = None


def default_instance_capacity(num_frames, num_gaussians, per_gaussian=16):
    return int(num_frames) * int(num_gaussians) * per_gaussian


def decode_bin_enabled():
    """AMAV_DECODE_BIN (default 1): rasterize(decode=...) decodes inside the rasterizer's binning block where that
    applies (amav_rasterize_decode_forward); 0 = the decode and the rasterizer as two launches."""
    return os.environ.get("AMAV_DECODE_BIN", "1") != "0"


_GAUSSIAN_WIDTHS = (("means3d", 3), ("rotations", 4), ("scales", 3), ("opacities", 1), ("colors", 3))


def _use_workspace(args, ws):
    args.workspace, args.workspace_bytes, args.instance_capacity = ws.buffer.data_ptr(), ws.buffer.numel(), ws.capacity


def _raster_args(gaussians, camera, height, width, bg, scale_modifier, apply_activations, workspace):
    """The part of amav_raster_args that rasterize() and rasterize_backward() fill alike: sizes, the five attributes,
    camera, background, activations and workspace (None: a new one of the default capacity).
    -> (args, the tensors it points into: attributes, then camera; the workspace)."""
    args, keep = RasterArgs(), []
    for (name, w), t in zip(_GAUSSIAN_WIDTHS, gaussians):
        attr, t = _attr(t, name, w)
        setattr(args, name, attr)
        keep.append(t)
    F, N = keep[0].shape[0], keep[0].shape[1]
    for (name, _), t in zip(_GAUSSIAN_WIDTHS[1:], keep[1:]):
        if t.shape[0] != F or t.shape[1] != N:
            raise AmavError(f"{name}: shape {tuple(t.shape)} does not match means3d [F={F},N={N},3]")
    H, W = int(height), int(width)
    if workspace is None:
        workspace = RasterWorkspace(F, N, H, W, default_instance_capacity(F, N), keep[0].device)
    elif workspace.key != (F, N, H, W):
        raise AmavError(f"workspace was sized for {workspace.key}, call is {(F, N, H, W)}")
    for name, t, cols in zip(("viewmatrix", "projmatrix", "tanfov"), camera, (16, 16, 2)):
        keep.append(_contig(t.reshape(F, cols), name))
        setattr(args, name, keep[-1].data_ptr())
    args.num_frames, args.num_gaussians, args.height, args.width = F, N, H, W
    args.bg = (ctypes.c_float * 3)(*[float(b) for b in bg])
    args.scale_modifier = float(scale_modifier)
    args.apply_activations = int(bool(apply_activations))
    args.scale_bias, args.scale_max, args.opacity_bias = SCALE_BIAS, SCALE_MAX, OPACITY_BIAS
    _use_workspace(args, workspace)
    return args, keep, workspace


def rasterize(means3d, rotations, scales, opacities, colors, viewmatrix, projmatrix, tanfov, height, width,
              bg=(1.0, 1.0, 1.0), apply_activations=False, scale_modifier=1.0, antialiasing=False, clamp_output=False,
              want_inv_depth=False, want_radii=False, workspace=None, check_overflow=True, out_rgba=None,
              profile_events=None, wire=None, decode=None, fuse_decode=None):
    """Batched tile rasterizer.  Gaussian attributes are [F,N,*] (frame stride 0 = shared across frames).

    Returns dict(rgba [F,H,W,4], inv_depth [F,H,W] | None, radii [F,N] | None, workspace).
    With check_overflow the call synchronises once to read the instance count and transparently retries with a
    larger workspace; without it the caller must consult workspace.status() before trusting the output.
    `wire`: (uint8 buffer, capacity in tiles) -- the rasterizer also writes the frame exchange's tile-sparse wire buffer
    (include/amav.h, amav_raster_args.wire; needs clamp_output): what frames_pack_tiles would produce from these frames
    with the tile counts as hint, without the extra pass.
    `decode`: a decode_source() whose `out` buffer the five attributes view.  The packed records are decoded into it
    first: with fuse_decode (None = decode_bin_enabled()) by the rasterizer's own launch (amav_rasterize_decode_forward,
    again on an overflow retry), else by triplane_sample_decode_indexed ahead of it.  Same records and frames either way.
    """
    args, keep, workspace = _raster_args((means3d, rotations, scales, opacities, colors),
                                         (viewmatrix, projmatrix, tanfov), height, width, bg, scale_modifier,
                                         apply_activations, workspace)
    means3d, dev = keep[0], keep[0].device
    F, N, H, W = workspace.key
    if out_rgba is None:
        out_rgba = torch.empty(F, H, W, 4, device=dev)
    else:
        _need(out_rgba, "out_rgba")
        if tuple(out_rgba.shape) != (F, H, W, 4) or not out_rgba.is_contiguous():
            raise AmavError(f"out_rgba must be contiguous [F,H,W,4] = {(F, H, W, 4)}")
    inv_depth = torch.empty(F, H, W, device=dev) if want_inv_depth else None
    radii = torch.empty(F, N, dtype=torch.int32, device=dev) if want_radii else None
    args.antialiasing, args.clamp_output = int(bool(antialiasing)), int(bool(clamp_output))
    args.out_rgba = out_rgba.data_ptr()
    args.out_inv_depth = inv_depth.data_ptr() if inv_depth is not None else None
    args.out_radii = radii.data_ptr() if radii is not None else None
    if DEBUG_STAMPS is not None:
        args.debug_stamps = DEBUG_STAMPS.data_ptr()
    if wire is not None:
        buf, cap = wire
        if buf.dtype != torch.uint8 or not buf.is_cuda or not buf.is_contiguous():
            raise AmavError("rasterize: wire must be a contiguous uint8 device buffer")
        args.wire, args.wire_bytes, args.wire_capacity_tiles = buf.data_ptr(), buf.numel(), int(cap)

    fused = False
    if decode is not None:
        if means3d.data_ptr() != decode["out"].data_ptr():
            raise AmavError("rasterize: with decode=..., the Gaussian attributes must be views of decode['out']")
        fused = decode_bin_enabled() if fuse_decode is None else bool(fuse_decode)
        if not fused:
            d = decode
            triplane_sample_decode_indexed(d["proj"], d["vertices"], d["idx4"], d["transl"], d["radius"],
                                           d["head_w_point"], out=d["out"])

    def launch(ws):
        _use_workspace(args, ws)
        ev = profile_events
        if ev is None and PROFILE_EVENTS:
            ev = PROFILE_EVENTS.pop(0)
        start, stop = (ev[0].handle, ev[1].handle) if ev is not None else (None, None)
        args.profile_start_event, args.profile_stop_event = start, stop
        if fused:
            _call("amav_rasterize_decode_forward", ctypes.byref(args), ctypes.byref(decode["struct"]))
        else:
            _call("amav_rasterize_forward", ctypes.byref(args))

    launch(workspace)
    if check_overflow:
        total, max_frame, over = workspace.status_full()
        if over:  # every frame owns capacity / F instances: size the retry by the fullest frame
            workspace = RasterWorkspace(F, N, H, W, F * max_frame, dev)
            launch(workspace)
            total, max_frame, over = workspace.status_full()
            if over:
                raise AmavError(f"rasterizer overflowed twice (instances={total}, fullest frame {max_frame})")
        # the largest per-frame instance count: what rasterize_backward sizes its partial sums by
        return dict(rgba=out_rgba, inv_depth=inv_depth, radii=radii, workspace=workspace, max_frame=max_frame)
    return dict(rgba=out_rgba, inv_depth=inv_depth, radii=radii, workspace=workspace)


def rasterize_backward(means3d, rotations, scales, opacities, colors, viewmatrix, projmatrix, tanfov, height, width,
                       grad_rgba, workspace, max_frame, bg=(1.0, 1.0, 1.0), apply_activations=False, scale_modifier=1.0,
                       want_alpha=False):
    """Gradients of the rasterizer (amav_rasterize_backward) for the LAST rasterize() on `workspace`, which must have run
    on these inputs with clamp_output=False and check_overflow=True (`max_frame` = its result's "max_frame").

    grad_rgba = dL/d rgba [F,H,W,4].  Returns dict(means3d, rotations, scales, opacities, colors): dense [F,N,width]
    gradients (a frame-stride-0 input gets one row per frame), and with want_alpha the replay's 1 - T_final [F,H,W]
    ("alpha"; bit-identical to the forward's alpha channel).  No host sync.
    """
    args, keep, _ = _raster_args((means3d, rotations, scales, opacities, colors), (viewmatrix, projmatrix, tanfov),
                                 height, width, bg, scale_modifier, apply_activations, workspace)
    F, N, H, W = workspace.key
    grad_rgba = _contig(grad_rgba, "grad_rgba")
    if tuple(grad_rgba.shape) != (F, H, W, 4):
        raise AmavError(f"grad_rgba must be [F,H,W,4] = {(F, H, W, 4)}, got {tuple(grad_rgba.shape)}")
    dev = keep[0].device
    grads = {k: torch.empty(F, N, w, device=dev) for k, w in _GAUSSIAN_WIDTHS}
    alpha = torch.empty(F, H, W, device=dev) if want_alpha else None
    scratch = _scratch("amav_rasterize_backward_bytes", dev, F, N, int(max_frame),
                       rejected=f"F={F} N={N} max_frame={max_frame}")
    b = RasterBackwardArgs()
    b.grad_rgba = grad_rgba.data_ptr()
    b.grad_means3d, b.grad_rotations = grads["means3d"].data_ptr(), grads["rotations"].data_ptr()
    b.grad_scales, b.grad_opacities = grads["scales"].data_ptr(), grads["opacities"].data_ptr()
    b.grad_colors = grads["colors"].data_ptr()
    b.max_frame_instances = int(max_frame)
    b.scratch, b.scratch_bytes = scratch.data_ptr(), scratch.numel()
    b.debug_alpha = alpha.data_ptr() if alpha is not None else None
    _call("amav_rasterize_backward", ctypes.byref(args), ctypes.byref(b))
    if want_alpha:
        grads["alpha"] = alpha
    return grads


class _Rasterize(torch.autograd.Function):
    """rasterize() with diff_gaussian_rasterization's backward.  The Function owns its workspace and keeps it in ctx:
    the backward reads the forward's tile lists and blend records from it, which a later forward must not overwrite."""

    @staticmethod
    def forward(ctx, means3d, rotations, scales, opacities, colors, viewmatrix, projmatrix, tanfov, settings):
        s = settings
        F, N = means3d.shape[0], means3d.shape[1]
        ws = RasterWorkspace(F, N, s["height"], s["width"], default_instance_capacity(F, N), means3d.device)
        out = rasterize(means3d, rotations, scales, opacities, colors, viewmatrix, projmatrix, tanfov, s["height"],
                        s["width"], bg=s["bg"], apply_activations=s["apply_activations"],
                        scale_modifier=s["scale_modifier"], clamp_output=False, want_inv_depth=s["want_inv_depth"],
                        want_radii=s["want_radii"], workspace=ws, check_overflow=True)
        ctx.workspace, ctx.max_frame, ctx.settings = out["workspace"], out["max_frame"], s
        ctx.save_for_backward(means3d, rotations, scales, opacities, colors, viewmatrix, projmatrix, tanfov)
        empty = means3d.new_empty(0)
        inv_depth = out["inv_depth"] if out["inv_depth"] is not None else empty
        radii = out["radii"] if out["radii"] is not None else empty.to(torch.int32)
        ctx.mark_non_differentiable(inv_depth, radii)
        return out["rgba"], inv_depth, radii

    @staticmethod
    def backward(ctx, grad_rgba, _grad_inv_depth, _grad_radii):
        means3d, rotations, scales, opacities, colors, viewmatrix, projmatrix, tanfov = ctx.saved_tensors
        s = ctx.settings
        if grad_rgba is None:
            grad_rgba = torch.zeros(means3d.shape[0], s["height"], s["width"], 4, device=means3d.device)
        g = rasterize_backward(means3d, rotations, scales, opacities, colors, viewmatrix, projmatrix, tanfov,
                               s["height"], s["width"], grad_rgba.float(), ctx.workspace, ctx.max_frame, bg=s["bg"],
                               apply_activations=s["apply_activations"], scale_modifier=s["scale_modifier"])
        need = ctx.needs_input_grad
        out = [g[k] if need[i] else None for i, k in enumerate(("means3d", "rotations", "scales", "opacities", "colors"))]
        return (*out, None, None, None, None)


def rasterize_differentiable(means3d, rotations, scales, opacities, colors, viewmatrix, projmatrix, tanfov, height,
                             width, bg=(1.0, 1.0, 1.0), apply_activations=False, scale_modifier=1.0, antialiasing=False,
                             clamp_output=False, want_inv_depth=False, want_radii=False, workspace=None, **unsupported):
    """rasterize() as a torch.autograd.Function: the rgba output (RGB and alpha) is differentiable with respect to the
    five Gaussian attributes (amav_rasterize_backward); inv_depth and radii are not, nor are the camera and `bg`.

    The images equal rasterize()'s with the same arguments bit for bit: the kernel runs unclamped and clamp_output is
    applied here with torch.clamp (exact either way), so the clamp's backward is torch's.  The call owns its workspace
    (no `workspace=`) and synchronises once for the overflow check.  Not differentiable, and refused:
    antialiasing, and rasterize()'s `decode` / `wire` / `out_rgba` / `profile_events` arguments.
    """
    if workspace is not None:
        raise NotImplementedError("rasterize_differentiable owns its workspace (the backward reads the forward's); "
                                  "do not pass workspace=")
    if antialiasing:
        raise NotImplementedError("the rasterizer has no backward for antialiasing=True")
    bad = sorted(k for k, v in unsupported.items() if v is not None)
    if bad:
        raise NotImplementedError(f"rasterize_differentiable does not support {', '.join(bad)}")
    settings = dict(height=int(height), width=int(width), bg=tuple(float(b) for b in bg),
                    apply_activations=bool(apply_activations), scale_modifier=float(scale_modifier),
                    want_inv_depth=bool(want_inv_depth), want_radii=bool(want_radii))
    rgba, inv_depth, radii = _Rasterize.apply(means3d, rotations, scales, opacities, colors, viewmatrix, projmatrix,
                                                 tanfov, settings)
    if clamp_output:
        rgba = torch.cat([rgba[..., :3].clamp(0.0, 1.0), rgba[..., 3:]], dim=-1)
    return dict(rgba=rgba, inv_depth=inv_depth if want_inv_depth else None, radii=radii if want_radii else None,
                workspace=None)


# ------------------------------------------------------------------------------------- spherical-harmonic colours
SH_MAX_DEGREE = 4


def _sh_args(means3d, sh, campos, degree, who):
    """means3d [F,N,3], sh [F,N,3*K] or [F,N,K,3] (any frame / element strides, unit stride on the last axis; frame
    stride 0 = one set for every frame), campos [F,3] -> (amav_sh_args, the tensors it points into, F, N, K)."""
    degree = int(degree)
    if not 0 <= degree <= SH_MAX_DEGREE:
        raise AmavError(f"{who}: degree {degree} outside 0..{SH_MAX_DEGREE}")
    _need(sh, f"{who}: sh")
    if sh.dim() == 4:
        if sh.shape[3] != 3:
            raise AmavError(f"{who}: sh {tuple(sh.shape)}; expected [F,N,K,3] or [F,N,3*K]")
        if sh.stride(3) != 1 or sh.stride(2) != 3:
            sh = sh.contiguous()
        sh = sh.as_strided((sh.shape[0], sh.shape[1], sh.shape[2] * 3), (sh.stride(0), sh.stride(1), 1))
    if sh.dim() != 3 or sh.shape[2] % 3 != 0 or sh.shape[2] == 0:
        raise AmavError(f"{who}: sh {tuple(sh.shape)}; expected [F,N,K,3] or [F,N,3*K]")
    K = sh.shape[2] // 3
    if K < (degree + 1) ** 2:
        raise AmavError(f"{who}: {K} coefficients per channel; degree {degree} needs (degree+1)^2 = {(degree + 1) ** 2}")
    args = _lib.ShArgs()
    args.sh, sh = _attr(sh, f"{who}: sh", 3 * K)
    args.means3d, means3d = _attr(means3d, f"{who}: means3d", 3)
    F, N = means3d.shape[0], means3d.shape[1]
    if sh.shape[0] != F or sh.shape[1] != N:
        raise AmavError(f"{who}: sh {tuple(sh.shape)} does not match means3d [F={F},N={N},3]")
    campos = _contig(campos, f"{who}: campos")
    if campos.numel() != F * 3:
        raise AmavError(f"{who}: campos {tuple(campos.shape)}, expected [F={F},3]")
    args.campos = campos.data_ptr()
    args.num_frames, args.num_gaussians, args.degree, args.num_coeffs = F, N, degree, K
    return args, (means3d, sh, campos), F, N, K


def sh_colors(means3d, sh, campos, degree):
    """View-dependent colours [F,N,3] = clamp_min(eval_sh(degree, sh, dir) + 0.5, 0), dir = (p - campos) / |p - campos|:
    the SH branch of render_one (src/models/renderer.py:540-545) for all frames in one launch (amav_sh_colors).
    means3d [F,N,3]; sh [F,N,K,3] or [F,N,3*K] with K >= (degree+1)^2 (coefficient-major, read in place; frame stride 0
    shares one set among the frames); campos [F,3] (camera_from_intrinsics).  No clamp at 1, no host sync."""
    args, keep, F, N, _ = _sh_args(means3d, sh, campos, degree, "sh_colors")
    colors = torch.empty(F, N, 3, device=keep[0].device)
    _call("amav_sh_colors", ctypes.byref(args), colors.data_ptr())
    return colors


def sh_colors_backward(means3d, sh, campos, degree, grad_colors, want_means3d=True, grad_sh=None):
    """Gradients of sh_colors (amav_sh_colors_backward) for grad_colors = dL/d colours [F,N,3]: (grad_sh [F,N,3*K],
    grad_means3d [F,N,3] | None), dense rows per frame (a frame-stride-0 input gets one row per frame; the caller sums
    them).  Coefficients beyond (degree+1)^2 get exact zeros; campos gets no gradient.  One launch, deterministic.
    `grad_sh`: a contiguous [F,N,3*K] buffer to write into (every element is written; it needs no initialisation)."""
    args, keep, F, N, K = _sh_args(means3d, sh, campos, degree, "sh_colors_backward")
    grad_colors = _contig(grad_colors, "sh_colors_backward: grad_colors")
    if tuple(grad_colors.shape) != (F, N, 3):
        raise AmavError(f"sh_colors_backward: grad_colors {tuple(grad_colors.shape)}, expected {(F, N, 3)}")
    dev = keep[0].device
    if grad_sh is None:
        grad_sh = torch.empty(F, N, 3 * K, device=dev)
    else:
        _need(grad_sh, "sh_colors_backward: grad_sh")
        if tuple(grad_sh.shape) != (F, N, 3 * K) or not grad_sh.is_contiguous():
            raise AmavError(f"sh_colors_backward: grad_sh must be contiguous [F,N,3*K] = {(F, N, 3 * K)}")
    grad_means3d = torch.empty(F, N, 3, device=dev) if want_means3d else None
    _call("amav_sh_colors_backward", ctypes.byref(args), grad_colors.data_ptr(), grad_sh.data_ptr(),
          grad_means3d.data_ptr() if want_means3d else None)
    return grad_sh, grad_means3d


class _ShColors(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3d, sh, campos, degree):
        ctx.save_for_backward(means3d, sh, campos)
        ctx.degree = degree
        return sh_colors(means3d, sh, campos, degree)

    @staticmethod
    def backward(ctx, grad_colors):
        means3d, sh, campos = ctx.saved_tensors
        grad_sh, grad_means3d = sh_colors_backward(means3d, sh, campos, ctx.degree, grad_colors.float(),
                                                   want_means3d=ctx.needs_input_grad[0])
        return grad_means3d, (grad_sh.view(sh.shape) if ctx.needs_input_grad[1] else None), None, None


def sh_colors_differentiable(means3d, sh, campos, degree):
    """sh_colors() as a torch.autograd.Function, differentiable in sh and means3d (campos gets no gradient).  Expanded
    (frame-stride-0) views are taken as they are: the Function returns one gradient row per frame and autograd's own
    expand backward sums them over the frames."""
    _sh_args(means3d, sh, campos, degree, "sh_colors_differentiable")
    return _ShColors.apply(means3d, sh, campos, int(degree))


def frames_to_rgb8(rgba, out=None):
    """fp32 RGBA [...,4] (contiguous) -> uint8 RGB [...,3], truncating like src/main2.py:351."""
    rgba = _need(rgba, "rgba")
    if not rgba.is_contiguous() or rgba.shape[-1] != 4:
        raise AmavError("frames_to_rgb8: need a contiguous [...,4] tensor")
    shape = tuple(rgba.shape[:-1]) + (3,)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=rgba.device)
    elif tuple(out.shape) != shape or out.dtype != torch.uint8 or not out.is_contiguous():
        raise AmavError(f"frames_to_rgb8: out must be contiguous uint8 {shape}")
    _call("amav_frames_to_rgb8", rgba.numel() // 4, rgba.data_ptr(), out.data_ptr())
    return out


def frames_wire_bytes(F, H, W, capacity_tiles):
    n = _lib.lib().amav_frames_wire_bytes(int(F), int(H), int(W), int(capacity_tiles))
    if n == 0:
        raise AmavError(f"frames_wire_bytes: bad sizes F={F} H={H} W={W} capacity={capacity_tiles}")
    return int(n)


def frames_pack_tiles(rgba, capacity_tiles, bg=(1.0, 1.0, 1.0), wire=None, tile_hint=None):
    """fp32 RGBA [F,H,W,4] -> tile-sparse wire buffer (uint8 tensor, include/amav.h).  No host sync; use
    frames_wire_count() (which synchronises) to read how many tiles were stored.  `tile_hint`: int32 [F*tiles], zero
    where the caller knows the tile is background (RasterWorkspace.tile_counts())."""
    rgba = _need(rgba, "rgba")
    if rgba.dim() != 4 or rgba.shape[-1] != 4 or not rgba.is_contiguous() or rgba.dtype != torch.float32:
        raise AmavError("frames_pack_tiles: need a contiguous fp32 [F,H,W,4] tensor")
    F, H, W = (int(x) for x in rgba.shape[:3])
    need = frames_wire_bytes(F, H, W, capacity_tiles)
    if wire is None:
        wire = torch.empty(need, dtype=torch.uint8, device=rgba.device)
    elif wire.dtype != torch.uint8 or not wire.is_contiguous() or wire.numel() < need:
        raise AmavError(f"frames_pack_tiles: wire must be a contiguous uint8 buffer of >= {need} bytes")
    bg3 = (ctypes.c_float * 3)(*[float(c) for c in bg])
    hint_ptr = None
    if tile_hint is not None:
        tile_hint = _need(tile_hint, "tile_hint", torch.int32)
        if not tile_hint.is_contiguous() or tile_hint.numel() != F * tile_count(H, W):
            raise AmavError("frames_pack_tiles: tile_hint must be a contiguous int32 [F * tiles] tensor")
        hint_ptr = tile_hint.data_ptr()
    _call("amav_frames_pack_tiles", F, H, W, rgba.data_ptr(), bg3, hint_ptr, int(capacity_tiles), wire.data_ptr(),
          wire.numel())
    return wire


def frames_wire_count(wire):
    """(stored tiles, capacity) of a packed wire buffer; synchronises."""
    head = wire[:16].view(torch.int32).cpu()
    return int(head[1]), int(head[2])


def frames_unpack_tiles(wire_all, num_buffers, F, H, W, capacity_tiles, out=None, status=None, state=None):
    """`num_buffers` gathered wire buffers (a uint8 tensor [num_buffers, stride]) -> uint8 RGB [num_buffers*F,H,W,3].
    `status` (int32 [1], accumulated) becomes non-zero when a sender had to drop tiles.

    `state` (int32 [num_buffers * F * tiles], made by frames_tile_state()) selects the differential form for an `out`
    buffer that is reused from step to step: only stored tiles and tiles that must return to background are written
    (include/amav.h, amav_frames_unpack_tiles_delta); `state` belongs to `out` and is updated in place."""
    wire_all = _need(wire_all, "wire_all", torch.uint8)
    if wire_all.dtype != torch.uint8 or not wire_all.is_contiguous() or wire_all.dim() != 2 or \
            wire_all.shape[0] != num_buffers:
        raise AmavError("frames_unpack_tiles: wire_all must be a contiguous uint8 [num_buffers, stride] tensor")
    dev = wire_all.device
    if out is None:
        if state is not None:
            raise AmavError("frames_unpack_tiles: `state` describes a buffer the caller keeps: pass it as `out`")
        out = torch.empty(num_buffers * F, H, W, 3, dtype=torch.uint8, device=dev)
    elif tuple(out.shape) != (num_buffers * F, H, W, 3) or out.dtype != torch.uint8 or not out.is_contiguous():
        raise AmavError(f"frames_unpack_tiles: out must be contiguous uint8 {(num_buffers * F, H, W, 3)}")
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
    if state is not None:
        tiles = num_buffers * F * tile_count(H, W)
        state = _need(state, "state", torch.int32)
        if state.numel() != tiles or not state.is_contiguous():
            raise AmavError(f"frames_unpack_tiles: state must be a contiguous int32 tensor of {tiles} entries")
        _call("amav_frames_unpack_tiles_delta", int(num_buffers), int(F), int(H), int(W), int(capacity_tiles),
              wire_all.data_ptr(), wire_all.shape[1], out.data_ptr(), state.data_ptr(), status.data_ptr())
        return out, status
    _call("amav_frames_unpack_tiles", int(num_buffers), int(F), int(H), int(W), int(capacity_tiles),
          wire_all.data_ptr(), wire_all.shape[1], out.data_ptr(), status.data_ptr())
    return out, status


DELTA_UNPACK_MAX_TILES = 64 * 1024 // 4 - 16 * 128  # amav_frames_unpack_tiles_delta keeps (T + 16 * 128) ints in LDS


def frames_delta_unpack_supported(H, W) -> bool:
    """Whether amav_frames_unpack_tiles_delta accepts frames of this size (width a multiple of 16 and a per-frame tile
    table that fits its 64 KiB of LDS: 14 336 tiles -- the reference's 1296 x 2304 frames have 11 664, a 3840 x 2160
    frame 32 400)."""
    return W % TILE == 0 and tile_count(H, W) <= DELTA_UNPACK_MAX_TILES


def frames_tile_state(num_buffers, F, H, W, device):
    """Fresh per-tile state of a reusable dense output buffer for the differential unpack: every tile unknown (-1)."""
    if not frames_delta_unpack_supported(H, W):
        raise AmavError(f"frames_tile_state: {H}x{W} frames are outside the differential unpack's limits "
                        "(use frames_unpack_tiles without `state`)")
    return torch.full((num_buffers * F * tile_count(H, W),), -1, dtype=torch.int32, device=device)


# ----------------------------------------------------------------------------------------------------------- JPEG
JPEG_SUBSAMPLING = {"420": _lib.DEFINES["AMAV_JPEG_420"], "444": _lib.DEFINES["AMAV_JPEG_444"]}


def _jpeg_args(frames, subsampling, tile_hint, background, who):
    """(frames, F, H, W, is_rgba_f32, subsampling code, hint pointer, background) of a JPEG call: fp32 RGBA [F,H,W,4]
    or uint8 RGB [F,H,W,3], contiguous, on the device."""
    if not isinstance(frames, torch.Tensor) or not frames.is_cuda:
        raise AmavError(f"{who}: frames must be a tensor on the HIP device")
    rgba = frames.dtype == torch.float32
    if frames.dim() != 4 or not frames.is_contiguous() or frames.dtype not in (torch.float32, torch.uint8) or \
            frames.shape[-1] != (4 if rgba else 3):
        raise AmavError(f"{who}: need contiguous fp32 RGBA [F,H,W,4] or uint8 RGB [F,H,W,3] frames, got "
                        f"{frames.dtype} {tuple(frames.shape)}")
    if str(subsampling) not in JPEG_SUBSAMPLING:
        raise AmavError(f"{who}: unknown subsampling {subsampling!r} (420 or 444)")
    F, H, W = (int(x) for x in frames.shape[:3])
    hint_ptr, bg3 = None, None
    if tile_hint is not None:
        tile_hint = _need(tile_hint, "tile_hint", torch.int32)
        if not tile_hint.is_contiguous() or tile_hint.numel() != F * tile_count(H, W):
            raise AmavError(f"{who}: tile_hint must be a contiguous int32 [F * tiles] tensor")
        hint_ptr = tile_hint.data_ptr()
        bg3 = (ctypes.c_float * 3)(*[float(c) for c in (background if background is not None else (1.0, 1.0, 1.0))])
    return frames, F, H, W, int(rgba), JPEG_SUBSAMPLING[str(subsampling)], hint_ptr, bg3


def jpeg_coefficients(frames, quality=90, subsampling="420", tile_hint=None, background=None):
    """The encoder's transform stage alone: frames -> int16 levels [F, blocks per frame, 64] (blocks in MCU-interleaved
    scan order, coefficients in zigzag order; include/amav.h has the arithmetic).  `tile_hint` / `background` as in
    frames_pack_tiles (background defaults to white)."""
    frames, F, H, W, rgba, sub, hint_ptr, bg3 = _jpeg_args(frames, subsampling, tile_hint, background, "jpeg_coefficients")
    blocks = int(_lib.lib().amav_jpeg_num_blocks(F, H, W, sub))
    if blocks == 0:
        raise AmavError(f"jpeg_coefficients: sizes F={F} H={H} W={W} are outside the encoder's limits")
    levels = torch.empty(F, blocks // F, 64, dtype=torch.int16, device=frames.device)
    ws = torch.empty(_lib.DEFINES["AMAV_JPEG_HINT_WORKSPACE"], dtype=torch.uint8, device=frames.device)
    _call("amav_jpeg_coefficients", F, H, W, frames.data_ptr(), rgba, int(quality), sub, hint_ptr, bg3,
          levels.data_ptr(), levels.numel() * 2, ws.data_ptr(), ws.numel())
    return levels


def jpeg_stream_bound(F, H, W, subsampling="420", restart_rows=1):
    n = _lib.lib().amav_jpeg_stream_bound(int(F), int(H), int(W), JPEG_SUBSAMPLING[str(subsampling)], int(restart_rows))
    if n == 0:
        raise AmavError(f"jpeg_stream_bound: bad sizes F={F} H={H} W={W} restart_rows={restart_rows}")
    return int(n)


def jpeg_encode_into(frames, stream, quality=90, subsampling="420", restart_rows=1, tile_hint=None, background=None,
                     capacity=None, frame_offsets=None, status=None):
    """One amav_jpeg_encode call into the caller's uint8 `stream` buffer (its first `capacity` bytes; default: all of
    it).  Returns (frame_offsets int64 [F+1], status int32 [1]) on the device; no host synchronisation.  status != 0:
    the stream needed frame_offsets[F] > capacity bytes, and nothing at or beyond the capacity was written."""
    frames, F, H, W, rgba, sub, hint_ptr, bg3 = _jpeg_args(frames, subsampling, tile_hint, background, "jpeg_encode")
    if not isinstance(stream, torch.Tensor) or stream.dtype != torch.uint8 or not stream.is_contiguous() or \
            stream.device != frames.device:
        raise AmavError("jpeg_encode: stream must be a contiguous uint8 tensor on the frames' device")
    capacity = stream.numel() if capacity is None else int(capacity)
    if not 0 <= capacity <= stream.numel():
        raise AmavError(f"jpeg_encode: capacity {capacity} outside the {stream.numel()}-byte stream buffer")
    if frame_offsets is None:
        frame_offsets = torch.empty(F + 1, dtype=torch.int64, device=frames.device)
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=frames.device)
    ws = _scratch("amav_jpeg_workspace_bytes", frames.device, F, H, W, sub, int(restart_rows),
                  rejected=f"F={F} H={H} W={W} restart_rows={restart_rows}")
    _call("amav_jpeg_encode", F, H, W, frames.data_ptr(), rgba, int(quality), sub, int(restart_rows), hint_ptr, bg3,
          stream.data_ptr(), capacity, frame_offsets.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel())
    return frame_offsets, status


def jpeg_encode(frames, quality=90, subsampling="420", restart_rows=1, tile_hint=None, background=None, capacity=None):
    """Frames (fp32 RGBA [F,H,W,4] as the rasterizer leaves them, or uint8 RGB [F,H,W,3]) -> baseline JPEG, one complete
    file per frame, packed back to back: (stream uint8 [bytes] on the device, frame_offsets int64 [F+1] on the host);
    frame f is stream[frame_offsets[f]:frame_offsets[f + 1]].

    `capacity` (default: the raw rgb24 size F*H*W*3) is the buffer the first attempt encodes into; when the stream does
    not fit, the call is repeated once at amav_jpeg_stream_bound.  Reading frame_offsets (the size) back is the call's
    single host synchronisation; jpeg_encode_into() is the form without any."""
    F, H, W = (int(x) for x in frames.shape[:3])
    kw = dict(quality=quality, subsampling=subsampling, restart_rows=restart_rows, tile_hint=tile_hint, background=background)
    capacity = F * H * W * 3 if capacity is None else int(capacity)
    stream = torch.empty(capacity, dtype=torch.uint8, device=frames.device)
    offsets = jpeg_encode_into(frames, stream, **kw)[0].cpu()
    if int(offsets[-1]) > capacity:  # what status[0] flags on the device
        stream = torch.empty(jpeg_stream_bound(F, H, W, subsampling, restart_rows), dtype=torch.uint8, device=frames.device)
        offsets = jpeg_encode_into(frames, stream, **kw)[0].cpu()
        if int(offsets[-1]) > stream.numel():
            raise AmavError(f"jpeg_encode: {int(offsets[-1])} bytes exceed the worst-case bound {stream.numel()}")
    return stream[:int(offsets[-1])], offsets


JPEG_SAMPLING = dict(JPEG_SUBSAMPLING, gray=_lib.DEFINES["AMAV_JPEG_GRAY"])  # what the decoder takes
JPEG_LAYOUTS = {"hwc_u8": _lib.DEFINES["AMAV_JPEG_HWC_U8"], "chw_f32": _lib.DEFINES["AMAV_JPEG_CHW_F32"]}
JPEG_STATUS_MARKERS, JPEG_STATUS_ENTROPY = _lib.DEFINES["AMAV_JPEG_STATUS_MARKERS"], _lib.DEFINES["AMAV_JPEG_STATUS_ENTROPY"]
JpegFrame = _lib.STRUCTS["amav_jpeg_frame"]


class _FrameRecords:
    """The per-frame records of one decode call: `table`, a uint8 tensor holding F records of the struct `Frame` back to
    back (on the host until .to(device)), and the height and width the frames share."""
    Frame = None

    def __init__(self, table, height, width):
        size = ctypes.sizeof(self.Frame)
        if not isinstance(table, torch.Tensor) or table.dtype != torch.uint8 or table.dim() != 1 or table.numel() == 0 or \
                table.numel() % size:
            raise AmavError(f"{type(self).__name__}: the table must be a uint8 tensor of whole {size}-byte records")
        self.table, self.height, self.width = table, int(height), int(width)

    @property
    def num_frames(self):
        return self.table.numel() // ctypes.sizeof(self.Frame)

    def to(self, device):
        moved = copy.copy(self)
        moved.table = self.table.to(device)
        return moved


class JpegRecords(_FrameRecords):
    """F amav_jpeg_frame records and the geometry the frames share.  mjpeg.frame_records() builds one from parsed
    headers."""
    Frame = JpegFrame

    def __init__(self, table, height, width, sampling):
        if str(sampling) not in JPEG_SAMPLING:
            raise AmavError(f"JpegRecords: unknown sampling {sampling!r} (420, 444 or gray)")
        super().__init__(table, height, width)
        self.sampling = str(sampling)


def _byte_stream(stream, who):
    if not isinstance(stream, torch.Tensor) or not stream.is_cuda or stream.dtype != torch.uint8 or stream.dim() != 1 or \
            stream.stride(0) != 1:
        raise AmavError(f"{who}: stream must be a uint8 vector on the HIP device")
    return stream


def _status_words(status, n, device, who):
    if status is None:
        return torch.empty(n, dtype=torch.int32, device=device)
    if not isinstance(status, torch.Tensor) or status.dtype != torch.int32 or status.device != device or \
            not status.is_contiguous() or status.numel() != n:
        raise AmavError(f"{who}: status must be a contiguous int32 [{n}] tensor on the stream's device")
    return status


def _out_like(out, shape, dtype, device, who, source="stream"):
    """`out` after its checks, or a fresh tensor in its place: contiguous, of `dtype` and `shape` (None: a vector of any
    length, which the caller supplies) on `device`."""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    ok = isinstance(out, torch.Tensor) and out.dtype == dtype and out.device == device
    if ok and shape is None:
        ok = out.dim() == 1 and out.stride(0) == 1
    elif ok:
        ok = tuple(out.shape) == shape and out.is_contiguous()
    if not ok:
        what = "a uint8 vector" if shape is None else f"a contiguous {dtype} {shape} tensor"
        raise AmavError(f"{who}: out must be {what} on the {source}'s device")
    return out


def _jpeg_decode_args(stream, records, status, who):
    if not isinstance(records, JpegRecords):
        raise AmavError(f"{who}: records must be an ops.JpegRecords")
    _byte_stream(stream, who)
    table = records.table
    if table.device != stream.device or not table.is_contiguous():
        raise AmavError(f"{who}: the record table must be contiguous on the stream's device (records.to(device))")
    F = records.num_frames
    return F, records.height, records.width, JPEG_SAMPLING[records.sampling], _status_words(status, F, stream.device, who)


def jpeg_decode_levels(stream, records, status=None):
    """The decoder's marker search and entropy decode alone: (int16 levels [F, blocks per frame, 64] in the layout of
    jpeg_coefficients, status int32 [F]), both on the device; no host synchronisation."""
    F, H, W, sampling, status = _jpeg_decode_args(stream, records, status, "jpeg_decode_levels")
    ws = _scratch("amav_jpeg_decode_workspace_bytes", stream.device, F, H, W, sampling, 1, rejected=f"F={F} H={H} W={W}")
    mcu = 16 if records.sampling == "420" else 8
    blocks = -(-H // mcu) * -(-W // mcu) * {"420": 6, "444": 3, "gray": 1}[records.sampling]
    levels = torch.empty(F, blocks, 64, dtype=torch.int16, device=stream.device)
    _call("amav_jpeg_decode_levels", F, H, W, sampling, stream.data_ptr(), stream.numel(), records.table.data_ptr(),
          levels.data_ptr(), levels.numel() * 2, status.data_ptr(), ws.data_ptr(), ws.numel())
    return levels, status


def jpeg_decode(stream, records, layout="chw_f32", out=None, status=None):
    """Baseline JPEG frames lying in the device byte vector `stream` -> (frames, status), both on the device, without a
    host synchronisation.  layout "hwc_u8": uint8 RGB [F,H,W,3]; "chw_f32": fp32 [F,3,H,W] holding exactly uint8 / 255
    (include/amav.h has the arithmetic).  status int32 [F]: 0, or JPEG_STATUS_MARKERS | JPEG_STATUS_ENTROPY for a
    damaged frame, whose undecodable blocks are zero levels; the other frames are not affected."""
    F, H, W, sampling, status = _jpeg_decode_args(stream, records, status, "jpeg_decode")
    if layout not in JPEG_LAYOUTS:
        raise AmavError(f"jpeg_decode: unknown layout {layout!r} (hwc_u8 or chw_f32)")
    shape, dtype = ((F, H, W, 3), torch.uint8) if layout == "hwc_u8" else ((F, 3, H, W), torch.float32)
    out = _out_like(out, shape, dtype, stream.device, "jpeg_decode")
    ws = _scratch("amav_jpeg_decode_workspace_bytes", stream.device, F, H, W, sampling, 0, rejected=f"F={F} H={H} W={W}")
    _call("amav_jpeg_decode", F, H, W, sampling, stream.data_ptr(), stream.numel(), records.table.data_ptr(),
          JPEG_LAYOUTS[layout], out.data_ptr(), out.numel() * out.element_size(), status.data_ptr(), ws.data_ptr(),
          ws.numel())
    return out, status


# ------------------------------------------------------------------------------------------------------------ PNG
PNG_MODES = {"rgb": _lib.DEFINES["AMAV_PNG_RGB"], "l": _lib.DEFINES["AMAV_PNG_L"]}
PNG_STATUS_INFLATE, PNG_STATUS_SIZE, PNG_STATUS_FILTER = (_lib.DEFINES["AMAV_PNG_STATUS_" + n] for n in ("INFLATE", "SIZE", "FILTER"))
PngFrame = _lib.STRUCTS["amav_png_frame"]


class PngRecords(_FrameRecords):
    """F amav_png_frame records and the height and width the frames share.  png.frame_records() builds one."""
    Frame = PngFrame


def _flate(entry, query, data, records, out, status, who, *query_sizes, source="stream"):
    """What inflate() and deflate() share: the [N,5] rows become 40-byte records, go up in one copy, and one call of
    `entry` runs over them with the scratch that `query`(N, *query_sizes) asks for."""
    _byte_stream(data, who)
    if not isinstance(records, torch.Tensor) or records.dtype != torch.int64 or records.dim() != 2 or records.shape[1] != 5 or \
            records.shape[0] == 0:
        raise AmavError(f"{who}: records must be an int64 [N,5] tensor (in_begin, in_end, out_begin, out_capacity, wrapper)")
    host = records.cpu() if records.is_cuda else records
    N = host.shape[0]
    if out is None:
        out = torch.empty(max(1, int((host[:, 2] + host[:, 3]).max())), dtype=torch.uint8, device=data.device)
    out = _out_like(out, None, torch.uint8, data.device, who, source)
    table = torch.zeros(N, ctypes.sizeof(_lib.STRUCTS[entry + "_stream"]) // 8, dtype=torch.int64)
    table[:, :4] = host[:, :4]
    table[:, 4] = host[:, 4] & 0xFFFFFFFF  # wrapper (int32) + reserved
    table = table.to(data.device)
    status = _status_words(status, N, data.device, who)
    produced = torch.empty(N, dtype=torch.int64, device=data.device)
    ws = _scratch(query, data.device, N, *query_sizes, rejected=f"{N} streams")
    _call(entry, N, data.data_ptr(), data.numel(), table.data_ptr(), out.data_ptr(), out.numel(), produced.data_ptr(),
          status.data_ptr(), ws.data_ptr(), ws.numel())
    return out, produced, status


def inflate(stream, records, out=None, status=None):
    """DEFLATE streams lying in the device byte vector `stream` -> (out, produced, status), all on the device.  With
    records on the host there is no host synchronisation (the table goes up in one copy); records given on the device
    are read back first, which is one.  records: int64 [N,5], one row per stream: in_begin, in_end (bytes
    of `stream`), out_begin, out_capacity (bytes of `out`), wrapper (0 raw, 1 zlib; the Adler-32 is not verified).
    out: the uint8 vector written into (default: a fresh one that just holds every row's range; the bytes between the
    ranges are not touched).  produced int64 [N]: bytes written per stream; status int32 [N]: 0, or PNG_STATUS_INFLATE /
    PNG_STATUS_SIZE (include/amav.h has the rules)."""
    return _flate("amav_inflate", "amav_inflate_workspace_bytes", stream, records, out, status, "inflate")


def png_decode(stream, records, mode="rgb", layout="hwc_u8", out=None, status=None):
    """PNG frames whose joined IDAT streams (and palettes) lie in the device byte vector `stream` -> (frames, status),
    both on the device, without a host synchronisation.  mode "rgb" / "l": PIL's convert("RGB") / convert("L"), bit for
    bit.  layout "hwc_u8": uint8 [F,H,W,3] / [F,H,W]; "chw_f32": fp32 [F,3,H,W] / [F,1,H,W] holding exactly uint8 / 255.
    status int32 [F]: 0, or PNG_STATUS_INFLATE | PNG_STATUS_SIZE | PNG_STATUS_FILTER for a damaged frame (its pixels
    are 0 unless FILTER is the only bit); the other frames are not affected."""
    if not isinstance(records, PngRecords):
        raise AmavError("png_decode: records must be an ops.PngRecords")
    _byte_stream(stream, "png_decode")
    table = records.table
    if table.device != stream.device or not table.is_contiguous():
        raise AmavError("png_decode: the record table must be contiguous on the stream's device (records.to(device))")
    if mode not in PNG_MODES:
        raise AmavError(f"png_decode: unknown mode {mode!r} (rgb or l)")
    if layout not in JPEG_LAYOUTS:
        raise AmavError(f"png_decode: unknown layout {layout!r} (hwc_u8 or chw_f32)")
    F, H, W = records.num_frames, records.height, records.width
    status = _status_words(status, F, stream.device, "png_decode")
    if layout == "hwc_u8":
        shape, dtype = ((F, H, W, 3) if mode == "rgb" else (F, H, W)), torch.uint8
    else:
        shape, dtype = (F, 3 if mode == "rgb" else 1, H, W), torch.float32
    out = _out_like(out, shape, dtype, stream.device, "png_decode")
    ws = _scratch("amav_png_decode_workspace_bytes", stream.device, F, H, W, rejected=f"F={F} H={H} W={W}")
    _call("amav_png_decode", F, H, W, stream.data_ptr(), stream.numel(), table.data_ptr(), PNG_MODES[mode],
          JPEG_LAYOUTS[layout], out.data_ptr(), out.numel() * out.element_size(), status.data_ptr(), ws.data_ptr(), ws.numel())
    return out, status


PNG_STATUS_TABLE = _lib.DEFINES["AMAV_PNG_STATUS_TABLE"]
DEFLATE_PIECE = _lib.DEFINES["AMAV_DEFLATE_PIECE"]
PNG_FILTERS = {"none": 0, "sub": 1, "up": 2, "average": 3, "paeth": 4, "adaptive": _lib.DEFINES["AMAV_PNG_FILTER_ADAPTIVE"]}
PNG_ROUNDINGS = {"nearest": _lib.DEFINES["AMAV_PNG_ROUND_NEAREST"], "truncate": _lib.DEFINES["AMAV_PNG_ROUND_TRUNCATE"]}


def deflate_bound(nbytes, wrapper=True):
    """The most bytes deflate() makes of `nbytes` input bytes: every piece stored."""
    return int(nbytes) + 5 * max(1, -(-int(nbytes) // DEFLATE_PIECE)) + (6 if wrapper else 0)


def deflate(data, records, out=None, status=None):
    """Byte ranges of the device byte vector `data` -> DEFLATE streams: (out, produced, status), all on the device; the
    mirror of inflate().  With records on the host there is no host synchronisation; records given on the device are
    read back first, which is one.  records: int64 [N,5], one row per stream: in_begin, in_end (bytes of `data`),
    out_begin, out_capacity (bytes of `out`), wrapper (0 raw, 1 zlib).  out: the uint8 vector written into (default: a
    fresh one that just holds every row's range).  produced int64 [N]: the bytes each stream needs; status int32 [N]: 0,
    PNG_STATUS_SIZE (produced > out_capacity; the part that fits was written) or PNG_STATUS_TABLE (ranges that overlap
    beyond the piece table; include/amav.h has the rules)."""
    return _flate("amav_deflate", "amav_deflate_workspace_bytes", data, records, out, status, "deflate",
                  _byte_stream(data, "deflate").numel(), source="data")


def _png_frames(frames, who):
    """(frames, F, H, W, layout code) of a PNG encode call: fp32 RGBA [F,H,W,4], fp32 [F,3,H,W], uint8 RGB [F,H,W,3],
    or uint8 / fp32 grey [F,H,W]; contiguous, on the device.  An fp32 [F,3,H,4] tensor is taken as RGBA."""
    if not isinstance(frames, torch.Tensor) or not frames.is_cuda:
        raise AmavError(f"{who}: frames must be a tensor on the HIP device")
    d = _lib.DEFINES
    layout = None
    if frames.is_contiguous() and frames.dtype == torch.float32:
        if frames.dim() == 4 and frames.shape[-1] == 4:
            layout, (F, H, W) = d["AMAV_PNG_IN_RGBA_F32"], frames.shape[:3]
        elif frames.dim() == 4 and frames.shape[1] == 3:
            layout, (F, H, W) = d["AMAV_PNG_IN_CHW_F32"], (frames.shape[0], frames.shape[2], frames.shape[3])
        elif frames.dim() == 3:
            layout, (F, H, W) = d["AMAV_PNG_IN_GREY_F32"], frames.shape
    elif frames.is_contiguous() and frames.dtype == torch.uint8:
        if frames.dim() == 4 and frames.shape[-1] == 3:
            layout, (F, H, W) = d["AMAV_PNG_IN_RGB_U8"], frames.shape[:3]
        elif frames.dim() == 3:
            layout, (F, H, W) = d["AMAV_PNG_IN_GREY_U8"], frames.shape
    if layout is None:
        raise AmavError(f"{who}: need contiguous fp32 RGBA [F,H,W,4], fp32 [F,3,H,W], uint8 RGB [F,H,W,3] or uint8 / fp32 "
                        f"grey [F,H,W] frames, got {frames.dtype} {tuple(frames.shape)}")
    return frames, int(F), int(H), int(W), layout


def png_stream_bound(F, H, W, channels=3):
    layout = _lib.DEFINES["AMAV_PNG_IN_RGB_U8" if channels == 3 else "AMAV_PNG_IN_GREY_U8"]
    n = _lib.lib().amav_png_stream_bound(int(F), int(H), int(W), layout)
    if n == 0:
        raise AmavError(f"png_stream_bound: bad sizes F={F} H={H} W={W}")
    return int(n)


def png_encode_into(frames, stream, filter="adaptive", rounding="nearest", capacity=None, frame_offsets=None, status=None):
    """One amav_png_encode call into the caller's uint8 `stream` buffer (its first `capacity` bytes; default: all of it).
    Returns (frame_offsets int64 [F+1], status int32 [F]) on the device; no host synchronisation.  status[f] != 0: frame
    f ends behind the capacity (frame_offsets still holds the sizes needed), and nothing at or beyond the capacity was
    written."""
    frames, F, H, W, layout = _png_frames(frames, "png_encode")
    if filter not in PNG_FILTERS:
        raise AmavError(f"png_encode: unknown filter {filter!r} ({', '.join(PNG_FILTERS)})")
    if rounding not in PNG_ROUNDINGS:
        raise AmavError(f"png_encode: unknown rounding {rounding!r} (nearest or truncate)")
    if not isinstance(stream, torch.Tensor) or stream.dtype != torch.uint8 or not stream.is_contiguous() or \
            stream.device != frames.device:
        raise AmavError("png_encode: stream must be a contiguous uint8 tensor on the frames' device")
    capacity = stream.numel() if capacity is None else int(capacity)
    if not 0 <= capacity <= stream.numel():
        raise AmavError(f"png_encode: capacity {capacity} outside the {stream.numel()}-byte stream buffer")
    if frame_offsets is None:
        frame_offsets = torch.empty(F + 1, dtype=torch.int64, device=frames.device)
    status = _status_words(status, F, frames.device, "png_encode")
    ws = _scratch("amav_png_encode_workspace_bytes", frames.device, F, H, W, layout, rejected=f"F={F} H={H} W={W}")
    _call("amav_png_encode", F, H, W, frames.data_ptr(), layout, PNG_FILTERS[filter], PNG_ROUNDINGS[rounding],
          stream.data_ptr(), capacity, frame_offsets.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel())
    return frame_offsets, status


def png_encode(frames, filter="adaptive", rounding="nearest", capacity=None):
    """Frames (fp32 RGBA [F,H,W,4] as the rasterizer leaves them, fp32 [F,3,H,W], uint8 RGB [F,H,W,3], or uint8 / fp32
    grey [F,H,W]) -> PNG, one complete file per frame, packed back to back: (stream uint8 [bytes] on the device,
    frame_offsets int64 [F+1] on the host); frame f is stream[frame_offsets[f]:frame_offsets[f + 1]].  `rounding`
    "nearest" is torchvision's save_image (x * 255 + 0.5, clamped, truncated), "truncate" frames_to_rgb8's rule.

    `capacity` (default: half the raw size, at least 4 KiB) is the buffer the first attempt encodes into; when the
    stream does not fit, the call is repeated once at amav_png_stream_bound.  Reading frame_offsets (the size) back is
    the call's single host synchronisation; png_encode_into() is the form without any."""
    frames, F, H, W, layout = _png_frames(frames, "png_encode")
    channels = 1 if frames.dim() == 3 else 3
    capacity = max(4096, F * H * W * channels // 2) if capacity is None else int(capacity)
    stream = torch.empty(max(1, capacity), dtype=torch.uint8, device=frames.device)
    offsets = png_encode_into(frames, stream, filter, rounding, capacity=capacity)[0].cpu()
    if int(offsets[-1]) > capacity:  # what status flags on the device
        stream = torch.empty(png_stream_bound(F, H, W, channels), dtype=torch.uint8, device=frames.device)
        offsets = png_encode_into(frames, stream, filter, rounding)[0].cpu()
        if int(offsets[-1]) > stream.numel():
            raise AmavError(f"png_encode: {int(offsets[-1])} bytes exceed the worst-case bound {stream.numel()}")
    return stream[:int(offsets[-1])], offsets


def padded_size(height, width, pad_ratio):
    """pad_image's geometry (src/datasets/dataset_speech_vid.py:319-327), in Python doubles as there:
    (Hp, Wp, offset_y, offset_x)."""
    hp, wp = int(height * (1 + pad_ratio)), int(width * (1 + pad_ratio))
    return hp, wp, (hp - height) // 2, (wp - width) // 2


def _frame_view(t, name, channels):
    """Element strides (f, [c,] y, x) of a decoder-layout tensor or a view of one: uint8 [F,H,W(,3)] or fp32 [F(,3),H,W]."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype not in (torch.uint8, torch.float32):
        raise AmavError(f"{name}: expected a uint8 or float32 tensor on the HIP device")
    if t.dim() != 3 + channels:
        raise AmavError(f"{name}: expected {3 + channels} dimensions, got {tuple(t.shape)}")
    if not channels:
        return tuple(t.shape), t.stride()
    if t.dtype == torch.uint8:
        t = t.permute(0, 3, 1, 2)  # [F,H,W,3] read as [F,3,H,W]
    if t.shape[1] != 3:
        raise AmavError(f"{name}: expected uint8 [F,H,W,3] or float32 [F,3,H,W], got {tuple(t.shape)}")
    return (t.shape[0], t.shape[2], t.shape[3]), t.stride()


def prepare_frames(frames, masks=None, pad_ratio=0.0, crop_size=1024, normalize=None, images=True, cropped=True,
                   out_images=None, out_cropped=None):
    """The image half of the reference dataset's __getitem__ (src/datasets/dataset_speech_vid.py:184-252) for a whole clip
    in one amav_frames_prepare call, without a host synchronisation: (images, cropped, boxes).

    frames: uint8 [F,H,W,3] or fp32 [F,3,H,W] (jpeg_decode's two layouts) or a view of one; masks: uint8 or fp32 [F,H,W]
    or a view (channel 0 of a decoded grey clip: clip[..., 0]); None = all ones.
    images  fp32 [F,3,Hp,Wp], Hp = int(H * (1 + pad_ratio)): the frame over white, padded with ones  (`images`)
    cropped fp32 [F,3,crop_size,crop_size]: the mask's box grown by 20 %, squared, cropped from the padded image, padded
            to a square with ones and resized bilinearly with align_corners=True  (`cropped_images`); with
            normalize=(mean[3], std[3]) it holds (x - mean) / std, SapiensWrapper._preprocess_image's normalize
    boxes   int32 [F,5]: y_min, y_max, x_min, x_max (inclusive) and max_size
    images=False / cropped=False skip that output (None is returned in its place); out_images / out_cropped are written
    instead of fresh tensors.  Where the crop's side already equals crop_size the reference skips its resize and hands
    back the crop before squaring; this returns the square image."""
    _no_autograd("prepare_frames", frames, masks)
    (F, H, W), fs = _frame_view(frames, "frames", 1)
    ms = (0, 0, 0)
    if masks is not None:
        shape, ms = _frame_view(masks, "masks", 0)
        if shape != (F, H, W) or masks.device != frames.device:
            raise AmavError(f"prepare_frames: masks {shape} on {masks.device} do not match frames {(F, H, W)} on {frames.device}")
    Hp, Wp, oy, ox = padded_size(H, W, pad_ratio)
    S, dev = int(crop_size), frames.device

    def output(wanted, given, shape, name):
        if not wanted:
            return None  # a buffer given for it stays untouched
        if given is None:
            return torch.empty(shape, device=dev)
        if not isinstance(given, torch.Tensor) or given.dtype != torch.float32 or given.device != dev or \
                not given.is_contiguous() or tuple(given.shape) != shape:
            raise AmavError(f"prepare_frames: {name} must be a contiguous float32 {shape} tensor on the frames' device")
        return given

    if Hp < H or Wp < W or S < 1:
        raise AmavError(f"prepare_frames: pad_ratio {pad_ratio} or crop_size {crop_size} out of range")
    out_i = output(images, out_images, (F, 3, Hp, Wp), "out_images")
    out_c = output(cropped, out_cropped, (F, 3, S, S), "out_cropped")
    boxes = torch.empty(F, 5, dtype=torch.int32, device=dev)
    mean3 = std3 = None
    if normalize is not None:
        mean3, std3 = ((ctypes.c_float * 3)(*[float(v) for v in part]) for part in normalize)
    ws = _scratch("amav_frames_prepare_workspace_bytes", dev, F, rejected=f"F={F}")
    nbytes = lambda t: 0 if t is None else t.numel() * t.element_size()  # noqa: E731
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    _call("amav_frames_prepare", F, H, W, frames.data_ptr(), int(frames.dtype == torch.float32), *fs, ptr(masks),
          int(masks is not None and masks.dtype == torch.float32), *ms, Hp, Wp, oy, ox, S, mean3, std3, ptr(out_i),
          nbytes(out_i), ptr(out_c), nbytes(out_c), boxes.data_ptr(), nbytes(boxes), ws.data_ptr(), ws.numel())
    return out_i, out_c, boxes


# ------------------------------------------------------------------------------------------------------------ LBS
def body_tables_struct(tables: dict) -> BodyTables:
    """dict of device tensors prepared by body_model.BodyModel.device_tables() -> amav_body_tables."""
    t = BodyTables()
    t.num_verts, t.num_joints = tables["v_template"].shape[0], tables["parents"].shape[0]
    t.num_coeffs, t.skin_k = tables["j_dirs"].shape[1], tables["skin_idx"].shape[1]
    for k in ("v_template", "blend", "j_template", "j_dirs", "skin_w"):
        setattr(t, k, _contig(tables[k], k).data_ptr())
    for k in ("parents", "skin_idx"):
        setattr(t, k, _contig(tables[k], k, torch.int32).data_ptr())
    split = tables.get("blend_split")
    t.blend_split = None if split is None else _contig(split, "blend_split", torch.uint8).data_ptr()
    return t


def lbs_prepare_blend_split(tables: dict):
    """-> uint8 device buffer: the blend table as two scaled fp16 parts in MFMA fragment order (include/amav.h,
    amav_lbs_prepare_blend_split).  Put it into the tables dict as "blend_split": lbs_forward then runs the blend product
    on the 16-bit matrix pipe."""
    ts = body_tables_struct({k: v for k, v in tables.items() if k != "blend_split"})
    out = _scratch("amav_lbs_blend_split_bytes", tables["blend"].device, ctypes.byref(ts))
    _call("amav_lbs_prepare_blend_split", ctypes.byref(ts), out.data_ptr(), out.numel())
    return out


def lbs_forward(tables: dict, full_pose, coeffs, want_transforms=False):
    """full_pose [F, J*3], coeffs [F, n_coeff] -> vertices [F,V,3] (and A [F,J,12]).  renderer.py:261-274."""
    full_pose = _contig(full_pose, "full_pose")
    coeffs = _contig(coeffs, "coeffs")
    F = full_pose.shape[0]
    ts = body_tables_struct(tables)
    if full_pose.shape != (F, ts.num_joints * 3) or coeffs.shape != (F, ts.num_coeffs):
        raise AmavError(f"lbs: full_pose {tuple(full_pose.shape)} / coeffs {tuple(coeffs.shape)} do not match "
                        f"J={ts.num_joints}, n_coeff={ts.num_coeffs}")
    dev = full_pose.device
    ws = _scratch("amav_lbs_workspace_bytes", dev, F, ctypes.byref(ts))
    verts = torch.empty(F, ts.num_verts, 3, device=dev)
    A = torch.empty(F, ts.num_joints, 12, device=dev) if want_transforms else None
    _call("amav_lbs_forward", F, ctypes.byref(ts), full_pose.data_ptr(), coeffs.data_ptr(), verts.data_ptr(),
          A.data_ptr() if A is not None else None, ws.data_ptr(), ws.numel())
    return (verts, A) if want_transforms else verts


def _pose_parts(ts, pose_parts, coeff_parts, pose_mean):
    """-> (amav_pose_parts, tensors it points into, F) for the SMPL-X call's pose / coefficient parts."""
    F = int(pose_parts[0].shape[0])
    pp = PoseParts()
    keep = []

    def rows(tt, name):
        _need(tt, name)
        if tt.dtype != torch.float32 or tt.dim() != 2 or tt.shape[0] != F or (tt.shape[1] > 1 and tt.stride(1) != 1):
            raise AmavError(f"lbs: {name} must be float32 [F={F}, n] with contiguous rows, got {tuple(tt.shape)} {tt.dtype}")
        if F > 1 and tt.stride(0) < tt.shape[1]:
            tt = tt.contiguous()  # broadcast rows
        keep.append(tt)
        return tt

    if not 1 <= len(pose_parts) <= 8 or not 1 <= len(coeff_parts) <= 4:
        raise AmavError(f"lbs: {len(pose_parts)} pose parts (1..8), {len(coeff_parts)} coefficient parts (1..4)")
    pp.num_pose_parts, pp.num_coeff_parts = len(pose_parts), len(coeff_parts)
    for q, part in enumerate(pose_parts):
        part = rows(part, f"pose part {q}")
        if part.shape[1] % 3:
            raise AmavError(f"lbs: pose part {q} has {part.shape[1]} columns (not axis-angle triples)")
        pp.pose[q], pp.pose_joints[q] = part.data_ptr(), part.shape[1] // 3
        pp.pose_stride[q] = part.stride(0) if F > 1 else part.shape[1]
    for q, part in enumerate(coeff_parts):
        part = rows(part, f"coefficient part {q}")
        pp.coeff[q], pp.coeff_count[q] = part.data_ptr(), part.shape[1]
        pp.coeff_stride[q] = part.stride(0) if F > 1 else part.shape[1]
    if sum(pp.pose_joints[q] for q in range(len(pose_parts))) != ts.num_joints or \
            sum(pp.coeff_count[q] for q in range(len(coeff_parts))) != ts.num_coeffs:
        raise AmavError(f"lbs: the parts do not add up to J={ts.num_joints} joints / {ts.num_coeffs} coefficients")
    if pose_mean is not None:
        pose_mean = _contig(pose_mean.reshape(-1), "pose_mean")
        if pose_mean.numel() != ts.num_joints * 3:
            raise AmavError(f"lbs: pose_mean has {pose_mean.numel()} entries, expected {ts.num_joints * 3}")
        pp.pose_mean = pose_mean.data_ptr()
        keep.append(pose_mean)
    return pp, keep, F


def lbs_forward_parts(tables: dict, pose_parts, coeff_parts, pose_mean=None, want_transforms=False):
    """lbs_forward with the pose / coefficients as the SMPL-X call's keyword arguments hold them (renderer.py:261-272):
    `pose_parts` = float32 tensors [F, joints_p * 3] (rows may be strided, elements contiguous) concatenated in order,
    `coeff_parts` likewise (betas, expression), `pose_mean` [J*3] is added to the concatenated pose (smplx's
    full_pose += pose_mean).  No torch.cat / add launches: the joint-chain kernel reads the parts."""
    ts = body_tables_struct(tables)
    pp, keep, F = _pose_parts(ts, pose_parts, coeff_parts, pose_mean)
    dev = keep[0].device
    ws = _scratch("amav_lbs_workspace_bytes", dev, F, ctypes.byref(ts))
    verts = torch.empty(F, ts.num_verts, 3, device=dev)
    A = torch.empty(F, ts.num_joints, 12, device=dev) if want_transforms else None
    _call("amav_lbs_forward_parts", F, ctypes.byref(ts), ctypes.byref(pp), verts.data_ptr(),
          A.data_ptr() if A is not None else None, ws.data_ptr(), ws.numel())
    return (verts, A) if want_transforms else verts


def lbs_backward(tables: dict, pose_parts, coeff_parts, grad_vertices, pose_mean=None):
    """Gradients of lbs_forward_parts(tables, pose_parts, coeff_parts, pose_mean) (amav_lbs_backward), given
    grad_vertices = dL/d vertices [F,V,3] -> (grad_full_pose [F, J*3], grad_coeffs [F, n_coeff]): the gradient of the
    concatenated pose (and of every pose part's columns: pose_mean passes it through) and of betas + expression.
    `tables` needs the transposed skin table (skin_t_offsets / skin_t_verts / skin_t_weights, from
    body_model.BodyModel.device_tables()).  For lbs_forward(full_pose, coeffs): pose_parts=[full_pose],
    coeff_parts=[coeffs].  Deterministic, bitwise independent of how frames are split; no host sync."""
    ts = body_tables_struct(tables)
    pp, keep, F = _pose_parts(ts, pose_parts, coeff_parts, pose_mean)
    grad_vertices = _contig(grad_vertices, "grad_vertices")
    if tuple(grad_vertices.shape) != (F, ts.num_verts, 3):
        raise AmavError(f"lbs_backward: grad_vertices {tuple(grad_vertices.shape)} != {(F, ts.num_verts, 3)}")
    if any(k not in tables for k in ("skin_t_offsets", "skin_t_verts", "skin_t_weights")):
        raise AmavError("lbs_backward: the tables lack the transposed skin table (BodyModel.device_tables())")
    dev = grad_vertices.device
    scratch = _scratch("amav_lbs_backward_bytes", dev, F, ctypes.byref(ts))
    gpose = torch.empty(F, ts.num_joints * 3, device=dev)
    gcoef = torch.empty(F, ts.num_coeffs, device=dev)
    skin = [_contig(tables["skin_t_offsets"], "skin_t_offsets", torch.int32),
            _contig(tables["skin_t_verts"], "skin_t_verts", torch.int32),
            _contig(tables["skin_t_weights"], "skin_t_weights")]
    if skin[0].numel() != ts.num_joints + 1:
        raise AmavError(f"lbs_backward: skin_t_offsets has {skin[0].numel()} entries, expected {ts.num_joints + 1}")
    a = LbsBackwardArgs()
    a.num_frames, a.tables, a.parts = F, ctypes.pointer(ts), ctypes.pointer(pp)
    a.grad_vertices, a.grad_full_pose, a.grad_coeffs = grad_vertices.data_ptr(), gpose.data_ptr(), gcoef.data_ptr()
    a.skin_offsets, a.skin_verts, a.skin_weights = (x.data_ptr() for x in skin)
    a.scratch, a.scratch_bytes = scratch.data_ptr(), scratch.numel()
    _call("amav_lbs_backward", ctypes.byref(a))
    return gpose, gcoef


class _LBSParts(torch.autograd.Function):
    """lbs_forward_parts with amav_lbs_backward as the backward: each part's gradient is its columns of the full-pose /
    coefficient gradient (autograd sums a broadcast part over the frames and scatters a strided view)."""

    @staticmethod
    def forward(ctx, settings, *parts):
        n = settings["num_pose_parts"]
        tables, mean = settings["tables"], settings["pose_mean"]
        verts = lbs_forward_parts(tables, list(parts[:n]), list(parts[n:]), pose_mean=mean)
        ctx.settings = settings
        ctx.save_for_backward(*parts)
        return verts

    @staticmethod
    def backward(ctx, grad_vertices):
        parts = ctx.saved_tensors
        n = ctx.settings["num_pose_parts"]
        if not any(ctx.needs_input_grad[1:]):
            return (None,) * (1 + len(parts))
        gpose, gcoef = lbs_backward(ctx.settings["tables"], list(parts[:n]), list(parts[n:]), grad_vertices.float(),
                                    pose_mean=ctx.settings["pose_mean"])
        out, col, ccol = [None], 0, 0
        for q, p in enumerate(parts):
            w = int(p.shape[1])
            if q < n:
                g, col = gpose[:, col:col + w], col + w
            else:
                g, ccol = gcoef[:, ccol:ccol + w], ccol + w
            out.append(g if ctx.needs_input_grad[1 + q] else None)
        return tuple(out)


def lbs_differentiable(tables: dict, pose_parts, coeff_parts, pose_mean=None):
    """lbs_forward_parts as a torch.autograd.Function: the same vertices bit for bit, with gradients to every part
    (amav_lbs_backward).  `tables` from BodyModel.device_tables() (it carries the transposed skin table)."""
    settings = dict(tables=tables, pose_mean=pose_mean, num_pose_parts=len(pose_parts))
    return _LBSParts.apply(settings, *pose_parts, *coeff_parts)


def lbs_differentiable_full(tables: dict, full_pose, coeffs):
    """lbs_forward(full_pose [F, J*3], coeffs [F, n_coeff]) as a torch.autograd.Function (pose_mean already added)."""
    return lbs_differentiable(tables, [full_pose], [coeffs])


def points_gather(vertices, idx4):
    """vertices [F,V,3], idx4 [N,4] int32 -> points [F,N,3] (baked subdivision + subset, renderer.py:276-288)."""
    vertices = _contig(vertices, "vertices")
    idx4 = _contig(idx4, "idx4", torch.int32)
    F, V, _ = vertices.shape
    N = idx4.shape[0]
    out = torch.empty(F, N, 3, device=vertices.device)
    _call("amav_points_gather", F, V, N, vertices.data_ptr(), idx4.data_ptr(), out.data_ptr())
    return out


def points_gather_csr(idx4, num_verts):
    """The gather table transposed (host-built once, like body_model.build_subdivision_table): idx4 [N,4] ->
    (offsets int32 [V+1], entries int32 [4N]) on idx4's device: for every vertex the ids of the points whose slots name
    it, ascending, once per slot.  Raises on ids outside [0, num_verts)."""
    import numpy as np

    ids = torch.as_tensor(idx4).detach().cpu().numpy().astype(np.int64).reshape(-1)
    if ids.size and (ids.min() < 0 or ids.max() >= num_verts):
        raise AmavError(f"points_gather_csr: vertex ids outside [0, {num_verts})")
    n = ids.size // 4
    order = np.argsort(ids, kind="stable")  # stable over the point-major slots: ascending point id per vertex
    entries = np.repeat(np.arange(n, dtype=np.int64), 4)[order]
    offsets = np.zeros(num_verts + 1, np.int64)
    np.cumsum(np.bincount(ids, minlength=num_verts), out=offsets[1:])
    dev = idx4.device if isinstance(idx4, torch.Tensor) else "cpu"
    return (torch.as_tensor(offsets.astype(np.int32)).to(dev), torch.as_tensor(entries.astype(np.int32)).to(dev))


def points_gather_backward(grad_points, csr, num_verts):
    """grad_points [F,N,3] -> grad_vertices [F,V,3] (amav_points_gather_backward; `csr` = points_gather_csr(idx4, V)).
    A vertex no point names gets exactly 0."""
    grad_points = _contig(grad_points, "grad_points")
    offsets = _contig(csr[0], "csr offsets", torch.int32)
    entries = _contig(csr[1], "csr entries", torch.int32)
    F, N, _ = grad_points.shape
    if offsets.numel() != num_verts + 1 or entries.numel() != 4 * N:
        raise AmavError(f"points_gather_backward: table of {offsets.numel() - 1} vertices / {entries.numel()} entries "
                        f"does not match V={num_verts}, N={N}")
    out = torch.empty(F, num_verts, 3, device=grad_points.device)
    _call("amav_points_gather_backward", F, num_verts, N, grad_points.data_ptr(), offsets.data_ptr(),
          entries.data_ptr(), out.data_ptr())
    return out


class _PointsGather(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vertices, idx4, csr_offsets, csr_entries):
        ctx.csr, ctx.num_verts = (csr_offsets, csr_entries), int(vertices.shape[1])
        return points_gather(vertices, idx4)

    @staticmethod
    def backward(ctx, grad_points):
        return points_gather_backward(grad_points.float(), ctx.csr, ctx.num_verts), None, None, None


def points_gather_differentiable(vertices, idx4, csr=None):
    """points_gather as a torch.autograd.Function (the same points bit for bit); csr = points_gather_csr(idx4, V),
    built here (one host copy of idx4) when not given."""
    if csr is None:
        csr = points_gather_csr(idx4, int(vertices.shape[1]))
    return _PointsGather.apply(vertices, idx4, csr[0], csr[1])


# ------------------------------------------------------------------------------------------------------- triplane
def pack_head_weights(weights: dict, channels: int, device, differentiable=False):
    """The five head Linear layers (renderer.py:51-55) -> (head_w_plane [3,C,16], head_w_point [16,4]).

    `weights` maps 'xyz_layer' | 'rotation_layer' | 'scaling_layer' | 'opacity_layer' | 'shs_layer' to
    (weight [out, 3C+3], bias [out]).  Output channel order = packed record layout (include/amav.h).
    differentiable=True: the same values, built from the layers' tensors without detach() (autograd carries the packed
    weights' gradients back to the layers).
    """
    C = channels
    rows = {"xyz_layer": (0, 3), "opacity_layer": (3, 1), "rotation_layer": (4, 4), "scaling_layer": (8, 3),
            "shs_layer": (12, 3)}
    for name, (o, n) in rows.items():
        w = weights[name][0]
        if tuple(w.shape) != (n, 3 * C + 3):
            raise AmavError(f"{name}.weight has shape {tuple(w.shape)}, expected {(n, 3 * C + 3)}")
    if differentiable:
        zw, zb = torch.zeros(1, 3 * C + 3, device=device), torch.zeros(1, device=device)
        parts = [(weights[k][0], weights[k][1]) for k in ("xyz_layer", "opacity_layer", "rotation_layer", "scaling_layer")]
        parts += [(zw, zb), (weights["shs_layer"][0], weights["shs_layer"][1]), (zw, zb)]  # record rows 11, 15: pad
        Wcat = torch.cat([w.to(device=device, dtype=torch.float32) for w, _ in parts])
        bias = torch.cat([b.to(device=device, dtype=torch.float32) for _, b in parts])
    else:
        Wcat = torch.zeros(16, 3 * C + 3, device=device)
        bias = torch.zeros(16, device=device)
        for name, (o, n) in rows.items():
            w, b = weights[name]
            Wcat[o:o + n] = w.detach().to(device=device, dtype=torch.float32)
            bias[o:o + n] = b.detach().to(device=device, dtype=torch.float32)
    w_plane = Wcat[:, 3:].reshape(16, 3, C).permute(1, 2, 0).contiguous()  # [3, C, 16]
    w_point = torch.cat([Wcat[:, :3], bias[:, None]], dim=1).contiguous()   # [16, 4]
    return w_plane, w_point


def points_bbox(points):
    """points [F,N,3] -> [F,6] = per frame (min xyz, max xyz); a frame with a NaN gets the infinite box."""
    points = _contig(points, "points")
    if points.dim() != 3 or points.shape[-1] != 3:
        raise AmavError(f"points_bbox: expected [F,N,3], got {tuple(points.shape)}")
    F, N = int(points.shape[0]), int(points.shape[1])
    out = torch.empty(F, 6, device=points.device)
    _call("amav_points_bbox", F, N, points.data_ptr(), out.data_ptr())
    return out


def triplane_project(tokens, head_w_plane, resolution, region=None, out=None):
    """tokens [F, C, 3*R*R] (reference token layout, renderer.py:85-91) -> projected planes [F,3,R,R,16].
    `region` = (boxes [F,6] from points_bbox, radius): only the texels that sampling points inside the boxes can touch
    are projected (include/amav.h, amav_triplane_project_region); the others are left unwritten (of `out`, when given)."""
    _need(tokens, "tokens")
    if tokens.dim() != 3 or tokens.stride(2) != 1 or tokens.stride(1) != tokens.shape[2]:
        tokens = tokens.contiguous()
    F, C, S = tokens.shape
    R = int(resolution)
    if S != 3 * R * R:
        raise AmavError(f"tokens last dim {S} != 3*R*R = {3 * R * R}")
    head_w_plane = _contig(head_w_plane, "head_w_plane")
    if tuple(head_w_plane.shape) != (3, C, 16):
        raise AmavError(f"head_w_plane {tuple(head_w_plane.shape)} != {(3, C, 16)}")
    if out is None:
        out = torch.empty(F, 3, R, R, 16, device=tokens.device)
    elif tuple(out.shape) != (F, 3, R, R, 16) or not out.is_contiguous() or out.dtype != torch.float32 or not out.is_cuda:
        raise AmavError(f"triplane_project: out must be a contiguous float32 device tensor {(F, 3, R, R, 16)}")
    boxes, radius = None, 1.0
    if region is not None:
        boxes, radius = region
        boxes = _contig(boxes, "region boxes")
        if tuple(boxes.shape) != (F, 6) or not float(radius) > 0.0:
            raise AmavError(f"triplane_project: region boxes {tuple(boxes.shape)} != {(F, 6)} or radius {radius} <= 0")
    _call("amav_triplane_project_region", F, C, R, tokens.data_ptr(), tokens.stride(0), head_w_plane.data_ptr(),
          out.data_ptr(), boxes.data_ptr() if boxes is not None else None, float(radius))
    return out


def _decode_out(out, F, N, device):
    if out is None:
        return torch.empty(F, N, GAUSS_STRIDE, device=device)
    _need(out, "out")
    if tuple(out.shape) != (F, N, GAUSS_STRIDE) or not out.is_contiguous():
        raise AmavError(f"out must be contiguous {(F, N, GAUSS_STRIDE)}, got {tuple(out.shape)}")
    return out


def triplane_sample_decode(proj, points, transl, radius, head_w_point, out=None):
    """proj [F,3,R,R,16], points [F,N,3], transl [F,3] | None -> packed Gaussians [F,N,16]."""
    proj = _contig(proj, "proj")
    points = _contig(points, "points")
    head_w_point = _contig(head_w_point, "head_w_point")
    F, _, R, _, _ = proj.shape
    N = points.shape[1]
    if points.shape[0] != F:
        raise AmavError(f"points has {points.shape[0]} frames, proj has {F}")
    if transl is not None:
        transl = _contig(transl.reshape(F, 3), "transl")
    out = _decode_out(out, F, N, proj.device)
    _call("amav_triplane_sample_decode", F, N, R, proj.data_ptr(), points.data_ptr(),
          transl.data_ptr() if transl is not None else None, float(radius), head_w_point.data_ptr(), out.data_ptr())
    return out


def triplane_sample_decode_indexed(proj, vertices, idx4, transl, radius, head_w_point, out=None):
    """triplane_sample_decode with points_gather fused in: vertices [F,V,3] + idx4 [N,4] instead of points."""
    proj = _contig(proj, "proj")
    vertices = _contig(vertices, "vertices")
    idx4 = _contig(idx4, "idx4", torch.int32)
    head_w_point = _contig(head_w_point, "head_w_point")
    F, _, R, _, _ = proj.shape
    if vertices.shape[0] != F:
        raise AmavError(f"vertices has {vertices.shape[0]} frames, proj has {F}")
    V, N = vertices.shape[1], idx4.shape[0]
    if transl is not None:
        transl = _contig(transl.reshape(F, 3), "transl")
    out = _decode_out(out, F, N, proj.device)
    _call("amav_triplane_sample_decode_indexed", F, N, R, V, proj.data_ptr(), vertices.data_ptr(), idx4.data_ptr(),
          transl.data_ptr() if transl is not None else None, float(radius), head_w_point.data_ptr(), out.data_ptr())
    return out


def decode_source(proj, vertices, idx4, transl, radius, head_w_point, out=None):
    """The inputs of triplane_sample_decode_indexed, checked and held for rasterize(decode=...), which decodes them into
    `out` (packed [F,N,16], allocated here if None) as part of the rasterizer's launch sequence."""
    proj = _contig(proj, "proj")
    vertices = _contig(vertices, "vertices")
    idx4 = _contig(idx4, "idx4", torch.int32)
    head_w_point = _contig(head_w_point, "head_w_point")
    F, _, R, _, _ = proj.shape
    if vertices.shape[0] != F:
        raise AmavError(f"vertices has {vertices.shape[0]} frames, proj has {F}")
    V, N = vertices.shape[1], idx4.shape[0]
    if transl is not None:
        transl = _contig(transl.reshape(F, 3), "transl")
    out = _decode_out(out, F, N, proj.device)
    st = DecodeSource()
    st.resolution, st.num_verts = R, V
    st.proj, st.vertices, st.idx4 = proj.data_ptr(), vertices.data_ptr(), idx4.data_ptr()
    st.transl = transl.data_ptr() if transl is not None else None
    st.radius, st.head_w_point = float(radius), head_w_point.data_ptr()
    return dict(proj=proj, vertices=vertices, idx4=idx4, transl=transl, radius=float(radius), head_w_point=head_w_point,
                out=out, struct=st)


def triplane_decode_backward(tokens, head_w_plane, head_w_point, points, proj, grad_records, radius, boxes=None,
                             want_points=True, want_transl=True):
    """Gradients of triplane_project(tokens, head_w_plane, R, region=(boxes, radius) or None) followed by
    triplane_sample_decode(proj, points, transl, radius, head_w_point) (amav_triplane_decode_backward).

    `proj` is that forward's output, kept; grad_records = dL/d records [F,N,16].  Returns dict(tokens [F,C,3R^2],
    head_w_plane [3,C,16], head_w_point [16,4], points [F,N,3] or None, transl [F,3] or None).  With boxes, the slab is
    read only inside the projected rectangles and d tokens is exactly 0 outside them.  Deterministic; no host sync.
    """
    _need(tokens, "tokens")
    if tokens.dim() != 3 or tokens.stride(2) != 1 or tokens.stride(1) != tokens.shape[2]:
        tokens = tokens.contiguous()
    F, C, S = tokens.shape
    proj = _contig(proj, "proj")
    R = int(proj.shape[2])
    if tuple(proj.shape) != (F, 3, R, R, 16) or S != 3 * R * R:
        raise AmavError(f"proj {tuple(proj.shape)} does not match tokens {tuple(tokens.shape)}")
    head_w_plane = _contig(head_w_plane, "head_w_plane")
    head_w_point = _contig(head_w_point, "head_w_point")
    points = _contig(points, "points")
    grad_records = _contig(grad_records, "grad_records")
    N = int(points.shape[1])
    if tuple(head_w_plane.shape) != (3, C, 16) or tuple(head_w_point.shape) != (16, 4):
        raise AmavError(f"head weights {tuple(head_w_plane.shape)}, {tuple(head_w_point.shape)} != (3,{C},16), (16,4)")
    if tuple(points.shape) != (F, N, 3) or tuple(grad_records.shape) != (F, N, GAUSS_STRIDE):
        raise AmavError(f"points {tuple(points.shape)} / grad_records {tuple(grad_records.shape)} do not match F={F}")
    if boxes is not None:
        boxes = _contig(boxes, "boxes")
        if tuple(boxes.shape) != (F, 6):
            raise AmavError(f"boxes {tuple(boxes.shape)} != {(F, 6)}")
    dev = tokens.device
    out = dict(tokens=torch.empty(F, C, S, device=dev), head_w_plane=torch.empty(3, C, 16, device=dev),
               head_w_point=torch.empty(16, 4, device=dev),
               points=torch.empty(F, N, 3, device=dev) if want_points else None,
               transl=torch.empty(F, 3, device=dev) if want_transl else None)
    scratch = _scratch("amav_triplane_decode_backward_bytes", dev, F, N, C, R, rejected=f"F={F} N={N} C={C} R={R}")
    a = TriplaneDecodeBackwardArgs()
    a.num_frames, a.num_points, a.channels, a.resolution, a.radius = F, N, C, R, float(radius)
    a.tokens, a.tokens_frame_stride = tokens.data_ptr(), tokens.stride(0)
    a.head_w_plane, a.head_w_point = head_w_plane.data_ptr(), head_w_point.data_ptr()
    a.points, a.proj = points.data_ptr(), proj.data_ptr()
    a.boxes = boxes.data_ptr() if boxes is not None else None
    a.grad_records = grad_records.data_ptr()
    a.grad_tokens, a.grad_head_w_plane = out["tokens"].data_ptr(), out["head_w_plane"].data_ptr()
    a.grad_head_w_point = out["head_w_point"].data_ptr()
    a.grad_points = out["points"].data_ptr() if want_points else None
    a.grad_transl = out["transl"].data_ptr() if want_transl else None
    a.scratch, a.scratch_bytes = scratch.data_ptr(), scratch.numel()
    _call("amav_triplane_decode_backward", ctypes.byref(a))
    return out


class _TriplaneDecode(torch.autograd.Function):
    """triplane_project (region) + triplane_sample_decode with amav_triplane_decode_backward as the backward.  The
    projected planes and region boxes of the forward are kept for it."""

    @staticmethod
    def forward(ctx, tokens, w_plane, w_point, points, transl, settings):
        R, radius = settings["resolution"], settings["radius"]
        boxes = points_bbox(points) if settings["region"] else None
        proj = triplane_project(tokens, w_plane, R, region=(boxes, radius) if boxes is not None else None)
        out = triplane_sample_decode(proj, points, transl, radius, w_point)
        ctx.settings, ctx.has_transl = settings, transl is not None
        ctx.save_for_backward(tokens, w_plane, w_point, points, proj, boxes)
        return out

    @staticmethod
    def backward(ctx, grad_records):
        tokens, w_plane, w_point, points, proj, boxes = ctx.saved_tensors
        need = ctx.needs_input_grad
        g = triplane_decode_backward(tokens, w_plane, w_point, points, proj, grad_records.float(),
                                     ctx.settings["radius"], boxes=boxes, want_points=need[3],
                                     want_transl=ctx.has_transl and need[4])
        return (g["tokens"] if need[0] else None, g["head_w_plane"] if need[1] else None,
                g["head_w_point"] if need[2] else None, g["points"] if need[3] else None,
                g["transl"] if ctx.has_transl and need[4] else None, None)


def triplane_decode_differentiable(tokens, w_plane, w_point, points, transl, resolution, radius, region=True):
    """The fused triplane decode as a torch.autograd.Function: tokens [F,C,3R^2], head weights (pack_head_weights,
    differentiable=True), points [F,N,3], transl [F,3] or None -> packed records [F,N,16], equal bit for bit to
    triplane_project(region) + triplane_sample_decode.  Gradients reach tokens, both weight blocks, points and transl
    (amav_triplane_decode_backward).  region=True projects (and differentiates) only the texels the points can sample."""
    F = tokens.shape[0]
    if transl is not None:
        transl = transl.reshape(F, 3)
    settings = dict(resolution=int(resolution), radius=float(radius), region=bool(region))
    return _TriplaneDecode.apply(tokens, w_plane, w_point, points, transl, settings)


def triplane_sample_features(planes, points, radius):
    """planes [F,3,C,R,R] (any strides with unit stride along W and R along H), points [F,N,3] -> [F,N,3C]."""
    _need(planes, "planes")
    points = _contig(points, "points")
    F, P, C, R, R2 = planes.shape
    if P != 3 or R != R2:
        raise AmavError(f"planes must be [F,3,C,R,R], got {tuple(planes.shape)}")
    if planes.stride(4) != 1 or planes.stride(3) != R:
        planes = planes.contiguous()
    N = points.shape[1]
    out = torch.empty(F, N, 3 * C, device=planes.device)
    _call("amav_triplane_sample_features", F, N, C, R, planes.data_ptr(), planes.stride(0), planes.stride(1),
          planes.stride(2), points.data_ptr(), float(radius), out.data_ptr())
    return out



def triplane_sample_features_backward(planes, points, grad_out, radius, want_planes=True, want_points=True):
    """Gradients of triplane_sample_features(planes, points, radius) given grad_out [F,N,3C]
    (amav_triplane_sample_features_backward).  Returns (grad_planes or None, grad_points or None).  grad_planes has the
    shape of `planes` and, for a dense `planes` (the renderer's permuted view of the token slab included), its strides:
    autograd's way back to the tokens is then a view.  Every element is written.  Deterministic; no host sync."""
    _need(planes, "planes")
    points = _contig(points, "points")
    grad_out = _contig(grad_out, "grad_out")
    F, P, C, R, R2 = planes.shape
    if P != 3 or R != R2:
        raise AmavError(f"planes must be [F,3,C,R,R], got {tuple(planes.shape)}")
    if planes.stride(4) != 1 or planes.stride(3) != R:
        planes = planes.contiguous()
    N = points.shape[1]
    if tuple(points.shape) != (F, N, 3) or tuple(grad_out.shape) != (F, N, 3 * C):
        raise AmavError(f"points {tuple(points.shape)} / grad_out {tuple(grad_out.shape)} do not match planes "
                        f"{tuple(planes.shape)}")
    dev = planes.device
    g_planes = g_points = scratch = None
    a = TriplaneSampleBackwardArgs()
    a.num_frames, a.num_points, a.channels, a.resolution, a.radius = F, N, C, R, float(radius)
    a.planes = planes.data_ptr()
    a.planes_frame_stride, a.planes_plane_stride, a.planes_chan_stride = planes.stride(0), planes.stride(1), planes.stride(2)
    a.points, a.grad_out = points.data_ptr(), grad_out.data_ptr()
    if want_planes:
        g_planes = torch.empty_like(planes)  # keeps a dense input's strides
        if g_planes.stride(4) != 1 or g_planes.stride(3) != R or min(g_planes.stride()[:3]) < R * R:
            g_planes = torch.empty(F, 3, C, R, R, device=dev)
        scratch = _scratch("amav_triplane_sample_features_backward_bytes", dev, F, N, C, R,
                           rejected=f"F={F} N={N} C={C} R={R}")
        a.grad_planes = g_planes.data_ptr()
        a.grad_frame_stride, a.grad_plane_stride, a.grad_chan_stride = g_planes.stride(0), g_planes.stride(1), g_planes.stride(2)
        a.scratch, a.scratch_bytes = scratch.data_ptr(), scratch.numel()
    if want_points:
        g_points = torch.empty(F, N, 3, device=dev)
        a.grad_points = g_points.data_ptr()
    if want_planes or want_points:
        _call("amav_triplane_sample_features_backward", ctypes.byref(a))
    return g_planes, g_points


class _TriplaneSampleFeatures(torch.autograd.Function):
    """triplane_sample_features (the unchanged forward kernels) with amav_triplane_sample_features_backward."""

    @staticmethod
    def forward(ctx, planes, points, radius):
        ctx.radius = radius
        ctx.save_for_backward(planes, points)
        return triplane_sample_features(planes, points, radius)

    @staticmethod
    def backward(ctx, grad_out):
        planes, points = ctx.saved_tensors
        g_planes, g_points = triplane_sample_features_backward(planes, points, grad_out.float(), ctx.radius,
                                                               want_planes=ctx.needs_input_grad[0],
                                                               want_points=ctx.needs_input_grad[1])
        return g_planes, g_points, None


def triplane_sample_features_differentiable(planes, points, radius):
    """triplane_sample_features as a torch.autograd.Function: the same output bit for bit; gradients reach `planes`
    (through any view it is, e.g. the token slab) and `points`, each only when it requires grad."""
    return _TriplaneSampleFeatures.apply(planes, points, float(radius))


# ------------------------------------------------------------------------------- window cutting (windowed upsampler)
def windows_lattice(frame, oy, ox, step, off_y, off_x, num_frames, rows, cols):
    """The lattice the transpose walks: (step, off_y, off_x, table) with table int32 [F, rows, cols] holding the index of
    the window whose corner is (a * step + off_y, b * step + off_x), or -1.  frame / oy / ox: integer tensors [K] on one
    device; the corners must lie on the lattice (not checked: no host sync)."""
    step = int(step)
    table = torch.full((int(num_frames), int(rows), int(cols)), -1, dtype=torch.int32, device=frame.device)
    if frame.numel():
        a = torch.div(oy.long() - int(off_y), step, rounding_mode="floor")
        b = torch.div(ox.long() - int(off_x), step, rounding_mode="floor")
        table[frame.long(), a, b] = torch.arange(frame.numel(), dtype=torch.int32, device=frame.device)
    return step, int(off_y), int(off_x), table


def _windows_cut_torch(x, frame, oy, ox, size, lattice):
    """windows_cut as pad / unfold / advanced index (any dtype and device; host sync: the extent of the corners)."""
    step, off_y, off_x, _ = lattice
    F, C, h, w = x.shape
    K = frame.numel()
    if K == 0:
        return x.new_zeros(0, C, size, size)
    oy, ox = oy.long(), ox.long()
    top, left = max(0, -int(oy.min())), max(0, -int(ox.min()))
    bottom, right = max(0, int(oy.max()) + size - h), max(0, int(ox.max()) + size - w)
    xp = torch.nn.functional.pad(x, (left, right, top, bottom)) if top or left or bottom or right else x
    ry, rx = (off_y + top) % step, (off_x + left) % step      # first lattice row / column inside the padded source
    wv = xp[:, :, ry:].unfold(2, size, step).permute(0, 1, 2, 4, 3)
    wv = wv[..., rx:].unfold(4, size, step)                                     # [F,C,ky,size,kx,size]
    return wv[frame.long(), :, (oy + top - ry) // step, :, (ox + left - rx) // step, :]


def _windows_index(t, name, K):
    t = _contig(t, name, torch.int32)
    if t.numel() != K:
        raise AmavError(f"{name}: {t.numel()} entries for {K} windows")
    return t


def windows_cut(x, frame, oy, ox, size):
    """x [F,C,h,w], frame / oy / ox int32 [K] -> [K,C,size,size]: window k is x[frame[k], :, oy[k]:oy[k]+size,
    ox[k]:ox[k]+size], zeros where it lies outside the source (amav_windows_cut)."""
    x = _contig(x, "x")
    F, C, h, w = x.shape
    K = frame.numel()
    frame, oy, ox = (_windows_index(t, n, K) for t, n in ((frame, "frame"), (oy, "oy"), (ox, "ox")))
    out = torch.empty(K, C, int(size), int(size), device=x.device)
    _call("amav_windows_cut", F, C, h, w, x.data_ptr(), K, int(size), frame.data_ptr(), oy.data_ptr(), ox.data_ptr(),
          out.data_ptr())
    return out


def windows_cut_backward(grad_windows, lattice, shape):
    """grad_windows [K,C,size,size] -> grad_x of `shape` = (F,C,h,w) (amav_windows_cut_backward): every element is the
    sum of the windows that cover it, in ascending window index; `lattice` = windows_lattice(...).  Deterministic."""
    grad_windows = _contig(grad_windows, "grad_windows")
    step, off_y, off_x, table = lattice
    table = _contig(table, "lattice table", torch.int32)
    F, C, h, w = (int(v) for v in shape)
    K, Cw, size, size2 = grad_windows.shape
    if Cw != C or size != size2 or table.dim() != 3 or table.shape[0] != F:
        raise AmavError(f"windows_cut_backward: grad_windows {tuple(grad_windows.shape)} / lattice {tuple(table.shape)} "
                        f"do not match x {(F, C, h, w)}")
    out = torch.empty(F, C, h, w, device=grad_windows.device)
    _call("amav_windows_cut_backward", F, C, h, w, K, size, grad_windows.data_ptr(), int(step), int(off_y), int(off_x),
          table.shape[1], table.shape[2], table.data_ptr(), out.data_ptr())
    return out


class _WindowsCut(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, frame, oy, ox, size, step, off_y, off_x, table):
        ctx.lattice, ctx.shape = (step, off_y, off_x, table), tuple(x.shape)
        return windows_cut(x, frame, oy, ox, size)

    @staticmethod
    def backward(ctx, grad_windows):
        return (windows_cut_backward(grad_windows.float(), ctx.lattice, ctx.shape),) + (None,) * 8


def windows_cut_differentiable(x, frame, oy, ox, size, lattice):
    """windows_cut under autograd: the HIP cut and its transpose (a gather over `lattice` = windows_lattice(...): no
    atomics) for tensors on the device.  CPU tensors -- the upsampler's host tests; the library has no CPU path -- go
    through the pad / unfold / index formulation and torch's own autograd: the same values exactly (a cut copies)."""
    if not x.is_cuda:
        return _windows_cut_torch(x, frame, oy, ox, int(size), lattice)
    return _WindowsCut.apply(x, frame, oy, ox, int(size), *lattice)


# ------------------------------------------------------------------------------------------------------ image loss
IMAGE_LOSS_WINDOW = 11   # the only window the kernels are built for (loss_utils.py:44)
_image_loss_taps = None


def _image_loss_window():
    """The fp32 taps of losses.gaussian(11, 1.5): the very numbers create_window multiplies together."""
    global _image_loss_taps
    if _image_loss_taps is None:
        from .losses import gaussian
        taps = gaussian(IMAGE_LOSS_WINDOW, 1.5).float().tolist()
        _image_loss_taps = ImageLossWindow((ctypes.c_float * IMAGE_LOSS_WINDOW)(*taps))
    return _image_loss_taps


def _image_pair(x, y, what):
    """x, y [N,H,W,C] float32 on the device, any strides (both are read in place) -> (views, N, H, W, C)."""
    _need(x, f"{what}: x")
    _need(y, f"{what}: y")
    if x.dim() != 4 or x.shape != y.shape:
        raise AmavError(f"{what}: expected x and y [N,H,W,C] of one shape, got {tuple(x.shape)} and {tuple(y.shape)}")
    if not 1 <= x.shape[3] <= 4:
        raise AmavError(f"{what}: {x.shape[3]} channels; 1 to 4 are supported")
    return (ImageView(x.data_ptr(), *x.stride()), ImageView(y.data_ptr(), *y.stride())), *x.shape


def image_loss_sums(x, y, want_grad):
    """x, y [N,H,W,C] (C = 1..4, any strides: a [..., :3] view of RGBA frames or a permuted planar target is read in
    place) -> (sums [2,N], maps): sums[0] = per-image sum of |x - y|, sums[1] = per-image sum of the SSIM map of
    losses.ssim (11-tap window, zero padding), by amav_image_loss_forward: one tile kernel and a fixed-order reduction,
    bitwise the same on every run.  maps [3,N,H,W,C] is what image_loss_backward needs, or None without want_grad
    (then nothing of that size is allocated)."""
    (vx, vy), N, H, W, C = _image_pair(x, y, "image_loss_sums")
    if N == 0 or H == 0 or W == 0:
        return torch.zeros(2, N, device=x.device), (torch.empty(3, N, H, W, C, device=x.device) if want_grad else None)
    sums = torch.empty(2, N, device=x.device)
    maps = torch.empty(3, N, H, W, C, device=x.device) if want_grad else None
    ws = _scratch("amav_image_loss_workspace_bytes", x.device, N, H, W, rejected=f"N={N} H={H} W={W}")
    _call("amav_image_loss_forward", N, H, W, C, ctypes.byref(vx), ctypes.byref(vy), ctypes.byref(_image_loss_window()),
          sums.data_ptr(), maps.data_ptr() if want_grad else None, ws.data_ptr(), ws.numel())
    return sums, maps


def image_loss_backward(x, y, maps, grad_l1, grad_ssim):
    """Gradient of image_loss_sums with respect to x, [N,H,W,C] contiguous: grad_l1 / grad_ssim [N] are the gradients of
    the per-image sums (read on the device), maps the forward's.  One launch (amav_image_loss_backward), a gather:
    deterministic.  y gets no gradient."""
    (vx, vy), N, H, W, C = _image_pair(x, y, "image_loss_backward")
    maps = _need(maps, "image_loss_backward: maps")
    if tuple(maps.shape) != (3, N, H, W, C) or not maps.is_contiguous():
        raise AmavError(f"image_loss_backward: maps {tuple(maps.shape)}, expected contiguous {(3, N, H, W, C)}")
    grad_l1, grad_ssim = _contig(grad_l1, "grad_l1"), _contig(grad_ssim, "grad_ssim")
    if grad_l1.numel() != N or grad_ssim.numel() != N:
        raise AmavError(f"image_loss_backward: {grad_l1.numel()} / {grad_ssim.numel()} gradients for {N} images")
    grad_x = torch.empty(N, H, W, C, device=x.device)
    _call("amav_image_loss_backward", N, H, W, C, ctypes.byref(vx), ctypes.byref(vy), ctypes.byref(_image_loss_window()),
          maps.data_ptr(), grad_l1.data_ptr(), grad_ssim.data_ptr(), grad_x.data_ptr())
    return grad_x


class _ImageLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, want_grad):
        sums, maps = image_loss_sums(x, y, want_grad)
        if want_grad:
            ctx.save_for_backward(x, y, maps)
        return sums[0], sums[1]

    @staticmethod
    def backward(ctx, grad_l1, grad_ssim):
        x, y, maps = ctx.saved_tensors   # an output nobody used arrives as zeros
        return image_loss_backward(x, y, maps, grad_l1.float(), grad_ssim.float()), None, None


def image_loss_differentiable(x, y):
    """x, y [N,H,W,C] -> (l1_sum [N], ssim_sum [N]) under autograd: one Function with two outputs, so whatever weights
    the caller puts on the two terms, the backward to x is one launch.  The target y must not require a gradient."""
    _image_pair(x, y, "image_loss_differentiable")
    if y.requires_grad and torch.is_grad_enabled():
        raise AmavError("image_loss_differentiable: the target y requires a gradient; only x receives one")
    # needs_input_grad does not see torch.no_grad(): decide here whether the derivative maps are written at all
    return _ImageLoss.apply(x, y, x.requires_grad and torch.is_grad_enabled())


# ------------------------------------------------------------------------------------- SMPL-X parameter term
SMPLX_TERM_KEYS = ("betas", "global_orient", "body_pose", "left_hand_pose", "right_hand_pose", "jaw_pose", "leye_pose",
                   "reye_pose", "expression", "transl")   # amav_smplx_terms.term[k]; 1..7 are losses.ROTATION_KEYS
SMPLX_PART_NAMES = ("betas_mse", "betas_prior") + tuple(k + "_geo" for k in SMPLX_TERM_KEYS[1:8]) + (
    "expression_l1", "expression_prior", "transl_smoothl1")
SmplxTerm, SmplxTerms, SmplxGrads = (_lib.STRUCTS["amav_smplx_" + n] for n in ("term", "terms", "grads"))
assert len(SMPLX_TERM_KEYS) == _lib.DEFINES["AMAV_SMPLX_TERMS"] and len(SMPLX_PART_NAMES) == _lib.DEFINES["AMAV_SMPLX_PARTS"]


def _rot6d_rows(d6, what):
    """d6 [..., 6] float32 on the device -> (tensor read in place, n, row stride): the leading axes must fold into one
    stride and the last be dense (a [B,55,6] view of a wider buffer is); anything else is copied."""
    _need(d6, f"{what}: d6")
    if d6.dim() < 1 or d6.shape[-1] != 6:
        raise AmavError(f"{what}: expected d6 [..., 6], got {tuple(d6.shape)}")
    rows = _fold(d6, d6.dim() - 1)
    if rows is None:
        d6 = d6.contiguous()
        rows = (d6.numel() // 6, 6)
    return d6, rows[0], rows[1]


def _fold(t, k):
    """(frames, frame stride) when axes k.. of t are dense and axes ..k fold into one stride, else None."""
    want = 1
    for size, stride in zip(reversed(t.shape[k:]), reversed(t.stride()[k:])):
        if size != 1 and stride != want:
            return None
        want *= size
    lead = [(size, stride) for size, stride in zip(t.shape[:k], t.stride()[:k]) if size != 1]
    frames = math.prod(t.shape[:k])
    if not lead or frames == 0:
        return frames, want
    for (_, outer), (size, inner) in zip(lead, lead[1:]):
        if outer != size * inner:
            return None
    return frames, lead[-1][1]


def rot6d_to_axis_angle(d6):
    """d6 [..., 6] -> axis-angle [..., 3] (contiguous): smplx_decoder.matrix_to_axis_angle(rotation_6d_to_matrix(d6))
    branch for branch, one lane per rotation, one launch (amav_rot6d_to_axis_angle)."""
    d6, n, stride = _rot6d_rows(d6, "rot6d_to_axis_angle")
    aa = torch.empty(*d6.shape[:-1], 3, device=d6.device)
    _call("amav_rot6d_to_axis_angle", n, d6.data_ptr(), stride, aa.data_ptr())
    return aa


def rot6d_to_axis_angle_backward(d6, grad_aa):
    """Gradient of rot6d_to_axis_angle with respect to d6, [..., 6] contiguous, for grad_aa [..., 3]: one launch that
    recomputes the forward from d6 (nothing is saved) and takes the forward's own branches."""
    d6, n, stride = _rot6d_rows(d6, "rot6d_to_axis_angle_backward")
    grad_aa = _contig(grad_aa, "rot6d_to_axis_angle_backward: grad_aa")
    if tuple(grad_aa.shape) != (*d6.shape[:-1], 3):
        raise AmavError(f"rot6d_to_axis_angle_backward: grad_aa {tuple(grad_aa.shape)} for d6 {tuple(d6.shape)}")
    grad_d6 = torch.empty(d6.shape, device=d6.device)
    _call("amav_rot6d_to_axis_angle_backward", n, d6.data_ptr(), stride, grad_aa.data_ptr(), grad_d6.data_ptr())
    return grad_d6


class _Rot6dToAxisAngle(torch.autograd.Function):
    @staticmethod
    def forward(ctx, d6):
        ctx.save_for_backward(d6)
        return rot6d_to_axis_angle(d6)

    @staticmethod
    def backward(ctx, grad_aa):
        return rot6d_to_axis_angle_backward(ctx.saved_tensors[0], grad_aa.float())


def rot6d_to_axis_angle_differentiable(d6):
    """rot6d_to_axis_angle under autograd (what SMPLXDecoder.forward runs with AMAV_SMPLX_PARAMS=hip)."""
    _rot6d_rows(d6, "rot6d_to_axis_angle_differentiable")
    return _Rot6dToAxisAngle.apply(d6)


def _smplx_terms(pred, gt, what):
    """pred, gt: dicts over SMPLX_TERM_KEYS (a key missing from either: the term is absent) of float32 device tensors
    of one shape per key -> (amav_smplx_terms, the tensors it points into, {key: pred shape}).  Both sides are read in
    place where one split into (frames, dense items of a frame) fits both; otherwise they are copied."""
    terms, keep, shapes = SmplxTerms(), [], {}
    for k, key in enumerate(SMPLX_TERM_KEYS):
        if key not in pred or key not in gt:
            continue
        p, g = _need(pred[key], f"{what}: pred[{key}]"), _need(gt[key], f"{what}: gt[{key}]")
        if p.shape != g.shape or p.device != g.device:
            raise AmavError(f"{what}: pred[{key}] {tuple(p.shape)} on {p.device}, gt[{key}] {tuple(g.shape)} on {g.device}")
        width = 3 if 1 <= k <= 7 else 1
        if width == 3 and (p.dim() < 1 or p.shape[-1] != 3):
            raise AmavError(f"{what}: {key} {tuple(p.shape)}: the last dimension must be 3")
        shapes[key] = p.shape
        fit = None
        for split in range(p.dim() - (width == 3) + 1):
            fp, fg = _fold(p, split), _fold(g, split)
            if fp is not None and fg is not None:
                fit = (fp[0], math.prod(p.shape[split:]) // width, fp[1], fg[1])
                break
        if fit is None:
            p, g = p.contiguous(), g.contiguous()
            fit = (1, p.numel() // width, p.numel(), g.numel())
        keep += [p, g]
        terms.term[k] = SmplxTerm(p.data_ptr(), g.data_ptr(), *fit)
    return terms, keep, shapes


def smplx_param_loss_forward(pred, gt):
    """parts [12] of losses.smplx_param_loss(pred, gt) in SMPLX_PART_NAMES order (the means; 0 for an absent key), by
    amav_smplx_param_loss_forward: one launch at the training sizes, fixed-order sums, bitwise the same on every run.
    pred[k], gt[k]: float32 device tensors of one shape, slices of the decoder's [F,55,3] included, read in place."""
    terms, keep, _ = _smplx_terms(pred, gt, "smplx_param_loss_forward")
    device = keep[0].device if keep else torch.device("cuda")
    parts = torch.empty(len(SMPLX_PART_NAMES), device=device)
    nbytes = _lib.lib().amav_smplx_param_loss_workspace_bytes(ctypes.byref(terms))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device) if nbytes else None
    _call("amav_smplx_param_loss_forward", ctypes.byref(terms), parts.data_ptr(), ws.data_ptr() if nbytes else None, nbytes)
    return parts


def smplx_param_loss_backward(pred, gt, grad_parts, wanted=None):
    """{key: gradient of sum(grad_parts * parts) with respect to pred[key], contiguous, pred[key]'s shape} for the keys
    in `wanted` (None: every present key); grad_parts [12] stays on the device.  One launch, every element written
    once, the gates replayed from the forward's arithmetic; gt gets no gradient."""
    terms, keep, shapes = _smplx_terms(pred, gt, "smplx_param_loss_backward")
    grad_parts = _contig(grad_parts, "smplx_param_loss_backward: grad_parts")
    if grad_parts.numel() != len(SMPLX_PART_NAMES):
        raise AmavError(f"smplx_param_loss_backward: {grad_parts.numel()} gradients for {len(SMPLX_PART_NAMES)} parts")
    grads, out = SmplxGrads(), {}
    for k, key in enumerate(SMPLX_TERM_KEYS):
        if key in shapes and (wanted is None or key in wanted):
            out[key] = torch.empty(shapes[key], device=grad_parts.device)
            grads.grad[k] = out[key].data_ptr()
    _call("amav_smplx_param_loss_backward", ctypes.byref(terms), grad_parts.data_ptr(), ctypes.byref(grads))
    return out


class _SmplxParamLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, keys, *tensors):
        pred, gt = dict(zip(keys, tensors[:len(keys)])), dict(zip(keys, tensors[len(keys):]))
        ctx.keys = keys
        ctx.save_for_backward(*tensors)
        return smplx_param_loss_forward(pred, gt)

    @staticmethod
    def backward(ctx, grad_parts):
        keys, tensors = ctx.keys, ctx.saved_tensors
        pred, gt = dict(zip(keys, tensors[:len(keys)])), dict(zip(keys, tensors[len(keys):]))
        wanted = [k for i, k in enumerate(keys) if ctx.needs_input_grad[1 + i]]
        grads = smplx_param_loss_backward(pred, gt, grad_parts.float(), wanted)
        return (None, *(grads.get(k) for k in keys), *(None for _ in keys))


def smplx_param_loss_differentiable(pred, gt):
    """parts [12] (SMPLX_PART_NAMES order) of losses.smplx_param_loss under autograd: one Function over every present
    key, so whatever weights the caller puts on the parts, the backward to all pred tensors is one launch that reads
    grad_parts on the device.  The targets must not require a gradient."""
    keys = tuple(k for k in SMPLX_TERM_KEYS if k in pred and k in gt)
    _smplx_terms(pred, gt, "smplx_param_loss_differentiable")
    if torch.is_grad_enabled() and any(gt[k].requires_grad for k in keys):
        raise AmavError("smplx_param_loss_differentiable: a target requires a gradient; only pred receives one")
    return _SmplxParamLoss.apply(keys, *(pred[k] for k in keys), *(gt[k] for k in keys))

# ---------------------------------------------------------------------------------------------- stage-1 reductions
def cell_segments(cell_of, cells):
    """cell_of int [..., N] (cell of every point) -> (order int32 [..., N], seg int32 [..., cells + 1]): point ids
    stably sorted by cell and the offset of every cell's run.  Plumbing (library sort / bincount), feeds the segment
    kernels below."""
    flat = cell_of.reshape(-1, cell_of.shape[-1]).long()
    order = torch.argsort(flat, dim=1, stable=True)
    counts = torch.zeros(flat.shape[0], cells, dtype=torch.long, device=flat.device)
    counts.scatter_add_(1, flat, torch.ones_like(flat))
    seg = torch.zeros(flat.shape[0], cells + 1, dtype=torch.long, device=flat.device)
    seg[:, 1:] = counts.cumsum(1)
    shape = tuple(cell_of.shape[:-1])
    return order.to(torch.int32).reshape(shape + (flat.shape[1],)), seg.to(torch.int32).reshape(shape + (cells + 1,))


def cell_pool_max(feat, cell_of, cells, segments=None):
    """pool_local (triplane_net.py:226-238): feat [B,N,C], cell_of int32 [B,3,N] -> [B,N,C]: for each of the three
    planes the channel-wise maximum over the points that share the point's cell, summed over the planes."""
    feat = _contig(feat, "feat")
    B, N, C = feat.shape
    cell_of = _contig(cell_of, "cell_of", torch.int32)
    if tuple(cell_of.shape) != (B, 3, N):
        raise AmavError(f"cell_of must be int32 [B,3,N] = {(B, 3, N)}, got {tuple(cell_of.shape)}")
    order, seg = segments if segments is not None else cell_segments(cell_of, cells)
    order, seg = _contig(order, "order", torch.int32), _contig(seg, "seg", torch.int32)
    cellmax = torch.empty(B, 3, cells, C, device=feat.device)
    out = torch.empty_like(feat)
    _call("amav_cell_max", B, N, C, int(cells), feat.data_ptr(), order.data_ptr(), seg.data_ptr(), cellmax.data_ptr())
    _call("amav_cell_gather", B, N, C, int(cells), cellmax.data_ptr(), cell_of.data_ptr(), out.data_ptr())
    return out


def cell_splat_mean(feat, cell_of, cells, segments=None):
    """generate_plane_features (triplane_net.py:240-244): feat [B,N,C], cell_of int32 [B,N] -> [B,C,cells]: per-cell
    mean of the points' features (summed in ascending point id), zero for an empty cell."""
    feat = _contig(feat, "feat")
    B, N, C = feat.shape
    cell_of = _contig(cell_of, "cell_of", torch.int32)
    if tuple(cell_of.shape) != (B, N):
        raise AmavError(f"cell_of must be int32 [B,N] = {(B, N)}, got {tuple(cell_of.shape)}")
    order, seg = segments if segments is not None else cell_segments(cell_of, cells)
    order, seg = _contig(order, "order", torch.int32), _contig(seg, "seg", torch.int32)
    out = torch.empty(B, C, cells, device=feat.device)
    _call("amav_cell_mean", B, N, C, int(cells), feat.data_ptr(), order.data_ptr(), seg.data_ptr(), out.data_ptr())
    return out


def points_project(points, w2c, intrinsics, features, radius_px):
    """points_projection (graphic_utils.py:275-331): points [B,N,3], w2c [B,4,4], intrinsics [B,3,3], features
    [B,C,H,W] -> [B,N,C] (include/amav.h, amav_points_project)."""
    return _points_project(points, w2c, intrinsics, features, radius_px)[0]


def _points_project(points, w2c, intrinsics, features, radius_px):
    """points_project -> (out, workspace): the workspace holds the z-buffer amav_points_project_backward reads."""
    points, w2c = _contig(points, "points"), _contig(w2c, "w2c")
    intrinsics, features = _contig(intrinsics, "intrinsics"), _contig(features, "features")
    B, N, _ = points.shape
    _, C, H, W = features.shape
    if features.shape[0] != B or tuple(w2c.shape) != (B, 4, 4) or tuple(intrinsics.shape) != (B, 3, 3):
        raise AmavError("points_project: batch sizes / matrix shapes do not match")
    ws = _scratch("amav_points_project_workspace_bytes", points.device, B, N, H, W, rejected=f"B={B} N={N} H={H} W={W}")
    out = torch.empty(B, N, C, device=points.device)
    _call("amav_points_project", B, N, C, H, W, points.data_ptr(), w2c.data_ptr(), intrinsics.data_ptr(),
          features.data_ptr(), float(radius_px), out.data_ptr(), ws.data_ptr(), ws.numel())
    return out, ws


def points_project_grid(points, w2c, intrinsics, rgb, grid, radius_px):
    """points_project on torch.cat([rgb, bilinear resize of grid]) without that tensor: points [B,N,3], w2c [B,4,4],
    intrinsics [B,3,3], rgb [B,3,H,W], grid [B,Gh,Gw,Cg] channels-last -> [B,N,3+Cg]; the resize is evaluated at the
    claimed pixels only (include/amav.h, amav_points_project_grid)."""
    return _points_project_grid(points, w2c, intrinsics, rgb, grid, radius_px)[0]


def _points_project_grid(points, w2c, intrinsics, rgb, grid, radius_px):
    """points_project_grid -> (out, workspace): the workspace holds the z-buffer the backward reads."""
    points, w2c, intrinsics = _contig(points, "points"), _contig(w2c, "w2c"), _contig(intrinsics, "intrinsics")
    rgb, grid = _contig(rgb, "rgb"), _contig(grid, "grid")
    if points.dim() != 3 or rgb.dim() != 4 or grid.dim() != 4:
        raise AmavError("points_project_grid: need points [B,N,3], rgb [B,3,H,W] and grid [B,Gh,Gw,Cg]")
    B, N, _ = points.shape
    H, W = rgb.shape[2:]
    _, Gh, Gw, Cg = grid.shape
    if (points.shape[2] != 3 or tuple(rgb.shape[:2]) != (B, 3) or grid.shape[0] != B or tuple(w2c.shape) != (B, 4, 4)
            or tuple(intrinsics.shape) != (B, 3, 3)):
        raise AmavError("points_project_grid: batch sizes / matrix shapes do not match")
    ws = _scratch("amav_points_project_workspace_bytes", points.device, B, N, H, W, rejected=f"B={B} N={N} H={H} W={W}")
    out = torch.empty(B, N, 3 + Cg, device=points.device)
    _call("amav_points_project_grid", B, N, H, W, Gh, Gw, Cg, points.data_ptr(), w2c.data_ptr(), intrinsics.data_ptr(),
          rgb.data_ptr(), grid.data_ptr(), float(radius_px), out.data_ptr(), ws.data_ptr(), ws.numel())
    return out, ws


def points_project_grid_backward(grad_out, workspace, grid_shape, height, width, want_rgb=False):
    """Gradients of points_project_grid given grad_out [B,N,3+Cg] and the forward's workspace -> (grad_grid
    [B,Gh,Gw,Cg], grad_rgb [B,3,H,W] or None without want_rgb): every pixel a point wins passes that point's gradient
    row through its four bilinear weights into the grid, summed per node in a fixed order
    (amav_points_project_grid_backward)."""
    grad_out = _contig(grad_out, "grad_out")
    B, N, C = grad_out.shape
    Gh, Gw, Cg = (int(v) for v in tuple(grid_shape)[-3:])
    if C != 3 + Cg or (len(grid_shape) == 4 and grid_shape[0] != B):
        raise AmavError(f"points_project_grid_backward: grad_out {tuple(grad_out.shape)} does not match a grid of "
                        f"{tuple(grid_shape)}")
    grad_grid = torch.empty(B, Gh, Gw, Cg, device=grad_out.device)
    grad_rgb = torch.empty(B, 3, int(height), int(width), device=grad_out.device) if want_rgb else None
    _call("amav_points_project_grid_backward", B, N, int(height), int(width), Gh, Gw, Cg, grad_out.data_ptr(),
          workspace.data_ptr(), workspace.numel(), grad_grid.data_ptr(), grad_rgb.data_ptr() if want_rgb else None)
    return grad_grid, grad_rgb


def cell_pool_max_backward(feat, cell_of, cells, segments, grad_out):
    """Gradient of cell_pool_max(feat, cell_of, cells, segments) w.r.t. feat, given grad_out [B,N,C]
    (amav_cell_max_backward): per plane, the cell's summed gradient goes to the one point that holds the maximum, the
    lowest point id among ties."""
    feat, grad_out = _contig(feat, "feat"), _contig(grad_out, "grad_out")
    B, N, C = feat.shape
    if tuple(grad_out.shape) != (B, N, C):
        raise AmavError(f"cell_pool_max_backward: grad_out {tuple(grad_out.shape)} != {(B, N, C)}")
    cell_of = _contig(cell_of, "cell_of", torch.int32)
    if tuple(cell_of.shape) != (B, 3, N):
        raise AmavError(f"cell_of must be int32 [B,3,N] = {(B, 3, N)}, got {tuple(cell_of.shape)}")
    order, seg = _contig(segments[0], "order", torch.int32), _contig(segments[1], "seg", torch.int32)
    ws = _scratch("amav_cell_max_backward_workspace_bytes", feat.device, B, C, int(cells),
                  rejected=f"B={B} C={C} cells={cells}")
    grad_feat = torch.empty_like(feat)
    _call("amav_cell_max_backward", B, N, C, int(cells), feat.data_ptr(), order.data_ptr(), seg.data_ptr(),
          cell_of.data_ptr(), grad_out.data_ptr(), grad_feat.data_ptr(), ws.data_ptr(), ws.numel())
    return grad_feat


def cell_splat_mean_backward(grad_planes, cells, segments, num_points):
    """Gradient of cell_splat_mean(feat, cell_of, cells, segments) w.r.t. feat [B,N,C], given grad_planes [B,C,cells]
    (amav_cell_mean_backward): every point takes its cell's gradient divided by the cell's point count."""
    grad_planes = _contig(grad_planes, "grad_planes")
    B, C, _ = grad_planes.shape
    if grad_planes.shape[2] != cells:
        raise AmavError(f"cell_splat_mean_backward: grad_planes {tuple(grad_planes.shape)} has not {cells} cells")
    order, seg = _contig(segments[0], "order", torch.int32), _contig(segments[1], "seg", torch.int32)
    if tuple(order.shape) != (B, num_points) or tuple(seg.shape) != (B, cells + 1):
        raise AmavError("cell_splat_mean_backward: segments do not match the batch / point / cell counts")
    grad_feat = torch.empty(B, num_points, C, device=grad_planes.device)
    _call("amav_cell_mean_backward", B, num_points, C, int(cells), order.data_ptr(), seg.data_ptr(),
          grad_planes.data_ptr(), grad_feat.data_ptr())
    return grad_feat


def points_project_backward(grad_out, workspace, height, width):
    """Gradient of points_project w.r.t. its features [B,C,H,W], given grad_out [B,N,C] and the forward's workspace
    (_points_project; amav_points_project_backward): every pixel a point wins takes that point's gradient row."""
    grad_out = _contig(grad_out, "grad_out")
    B, N, C = grad_out.shape
    grad = torch.empty(B, C, height, width, device=grad_out.device)
    _call("amav_points_project_backward", B, N, C, int(height), int(width), grad_out.data_ptr(), workspace.data_ptr(),
          workspace.numel(), grad.data_ptr())
    return grad


class _CellPoolMax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, cell_of, order, seg, cells):
        feat = _contig(feat, "feat")
        ctx.cells = cells
        ctx.save_for_backward(feat, cell_of, order, seg)
        return cell_pool_max(feat, cell_of, cells, (order, seg))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        feat, cell_of, order, seg = ctx.saved_tensors
        return cell_pool_max_backward(feat, cell_of, ctx.cells, (order, seg), grad_out.float()), None, None, None, None


class _CellSplatMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, cell_of, order, seg, cells):
        ctx.cells, ctx.num_points = cells, int(feat.shape[1])
        ctx.save_for_backward(order, seg)
        return cell_splat_mean(feat, cell_of, cells, (order, seg))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_planes):
        order, seg = ctx.saved_tensors
        return cell_splat_mean_backward(grad_planes.float(), ctx.cells, (order, seg), ctx.num_points), None, None, None, None


class _PointsProject(torch.autograd.Function):
    @staticmethod
    def forward(ctx, points, w2c, intrinsics, features, radius_px):
        out, ws = _points_project(points, w2c, intrinsics, features, radius_px)
        ctx.size, ctx.ws = tuple(features.shape[2:]), ws  # the z-buffer the backward reads
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        grad = points_project_backward(grad_out.float(), ctx.ws, *ctx.size) if ctx.needs_input_grad[3] else None
        return None, None, None, grad, None


class _PointsProjectGrid(torch.autograd.Function):
    @staticmethod
    def forward(ctx, points, w2c, intrinsics, rgb, grid, radius_px):
        out, ws = _points_project_grid(points, w2c, intrinsics, rgb, grid, radius_px)
        ctx.size, ctx.grid_shape, ctx.ws = tuple(rgb.shape[2:]), tuple(grid.shape), ws  # the z-buffer the backward reads
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        if not (ctx.needs_input_grad[3] or ctx.needs_input_grad[4]):
            return None, None, None, None, None, None
        grad_grid, grad_rgb = points_project_grid_backward(grad_out.float(), ctx.ws, ctx.grid_shape, *ctx.size,
                                                           want_rgb=ctx.needs_input_grad[3])
        return None, None, None, grad_rgb, grad_grid if ctx.needs_input_grad[4] else None, None


def _segments(cell_of, cells, segments):
    order, seg = segments if segments is not None else cell_segments(cell_of, cells)
    return _contig(order, "order", torch.int32), _contig(seg, "seg", torch.int32)


def cell_pool_max_differentiable(feat, cell_of, cells, segments=None):
    """cell_pool_max as a torch.autograd.Function: the same values bit for bit, differentiable in feat
    (amav_cell_max_backward: the whole gradient of a cell's maximum to the lowest point id that holds it)."""
    order, seg = _segments(cell_of, cells, segments)
    return _CellPoolMax.apply(feat, _contig(cell_of, "cell_of", torch.int32), order, seg, int(cells))


def cell_splat_mean_differentiable(feat, cell_of, cells, segments=None):
    """cell_splat_mean as a torch.autograd.Function: the same values bit for bit, differentiable in feat
    (amav_cell_mean_backward)."""
    order, seg = _segments(cell_of, cells, segments)
    return _CellSplatMean.apply(feat, _contig(cell_of, "cell_of", torch.int32), order, seg, int(cells))


def points_project_differentiable(points, w2c, intrinsics, features, radius_px):
    """points_project as a torch.autograd.Function: the same values bit for bit, differentiable in features
    (amav_points_project_backward: index_put's backward, every pixel a point wins takes that point's gradient row).
    points, w2c and intrinsics get no gradient: the selection is piecewise constant."""
    return _PointsProject.apply(points, w2c, intrinsics, features, float(radius_px))


def points_project_grid_differentiable(points, w2c, intrinsics, rgb, grid, radius_px):
    """points_project_grid as a torch.autograd.Function: the same values bit for bit, differentiable in grid and, when
    it requires grad, in rgb (amav_points_project_grid_backward: the gradient of the dense path, index_put's credit to
    every won pixel carried through the bilinear weights).  points, w2c and intrinsics get no gradient."""
    return _PointsProjectGrid.apply(points, w2c, intrinsics, rgb, grid, float(radius_px))


# ------------------------------------------------------------------------------------------------------ attention
# A list of (Event, Event) pairs: every selfattn() call pops one and records it around its kernels (bench.py)
ATTN_PROFILE_EVENTS = None


def _rows(t, name, B=None, S=None, min_width=None, width=None):
    """[B,S,C] fp32 device tensor with unit inner stride and dense batch stride, of the given sizes where given."""
    _need(t, name)
    if (t.dim() != 3 or t.stride(2) != 1 or t.stride(0) != t.shape[1] * t.stride(1)
            or (B is not None and t.shape[0] != B) or (S is not None and t.shape[1] != S)
            or (width is not None and t.shape[2] != width) or (min_width is not None and t.shape[2] < min_width)):
        want = width if width is not None else f">={min_width}" if min_width is not None else "C"
        raise AmavError(f"{name}: need [B,S,C] = [{B or 'B'},{S or 'S'},{want}] with unit inner stride and dense batch "
                        f"stride, got {tuple(t.shape)} strides {tuple(t.stride())}")
    return t


def _launchable(t):
    """t, or a contiguous copy where its layout is not one the attention entry points read in place."""
    if t.stride(2) != 1 or t.stride(0) != t.shape[1] * t.stride(1) or t.stride(1) % 4 or t.data_ptr() % 16:
        return t.contiguous()
    return t


def selfattn(q, k, v, heads, scale=None, bounds=None, split_out_exp=None):
    """softmax(q k^T * scale) v for [B,S,H*D] fp32 tensors (row stride may exceed H*D), D = 64.  bounds: (|q|, |k|, |v|)
    upper bounds the caller can prove, which spare the kernel its magnitude pre-pass (include/amav.h,
    amav_selfattn_forward_bounded); None: measured.  split_out_exp: return instead the fp16 x 2 activation operand
    [B*S, 3*H*D] of the projection that follows (split_operand(out, fmt=SPLIT_FP16X2, scale_exp=split_out_exp), written
    by the kernel's own last pass: amav_selfattn_forward_split_out)."""
    B, S, HD = _rows(q, "q").shape
    _rows(k, "k", B, S, width=HD), _rows(v, "v", B, S, width=HD)
    D = HD // heads
    if not (q.stride(1) == k.stride(1) == v.stride(1)):
        raise AmavError("selfattn: q, k, v must share their row stride")
    out = torch.empty(B, S, HD, device=q.device)
    ws = _scratch("amav_selfattn_workspace_bytes", q.device, B, S, heads, D, rejected=f"B={B} S={S} H={heads} D={D}")
    ev = ATTN_PROFILE_EVENTS.pop(0) if ATTN_PROFILE_EVENTS else None
    if ev is not None:
        ev[0].record()
    qb, kb, vb = (float(x) for x in bounds) if bounds is not None else (0.0, 0.0, 0.0)
    split = None if split_out_exp is None else _split_buffer(B * S, HD, SPLIT_FP16X2, q.device)
    _call("amav_selfattn_forward_split_out", B, S, heads, D, q.data_ptr(), k.data_ptr(), v.data_ptr(), q.stride(1),
          out.data_ptr(), HD, float(scale if scale is not None else D ** -0.5), qb, kb, vb,
          split.data_ptr() if split is not None else None, int(split_out_exp or 0), ws.data_ptr(), ws.numel())
    if ev is not None:
        ev[1].record()
    return out if split is None else split


def _qkv_views(qkv, heads):
    """[B,S,3*H*D] fused projection output (unit inner stride, dense batch stride) -> (B, S, H*D, D)."""
    B, S, C = _rows(qkv, "qkv").shape
    if C % (3 * heads):
        raise AmavError(f"qkv: need [B,S,3*H*D], got {tuple(qkv.shape)} for {heads} heads")
    return B, S, C // 3, C // (3 * heads)


def selfattn_lse(qkv, heads, scale=None):
    """amav_selfattn_forward_lse on a fused [B,S,3*H*D] qkv (read in place) -> (out [B,S,H*D], lse [B,H,S]), lse in
    natural units.  `out` equals selfattn()'s bit for bit; refused unless the default fp16 x 2 kernel is selected."""
    B, S, HD, D = _qkv_views(qkv, heads)
    out = torch.empty(B, S, HD, device=qkv.device)
    lse = torch.empty(B, heads, S, device=qkv.device)
    ws = _scratch("amav_selfattn_workspace_bytes", qkv.device, B, S, heads, D, rejected=f"B={B} S={S} H={heads} D={D}")
    p = qkv.data_ptr()
    _call("amav_selfattn_forward_lse", B, S, heads, D, p, p + 4 * HD, p + 8 * HD, qkv.stride(1), out.data_ptr(), HD,
          float(scale if scale is not None else D ** -0.5), lse.data_ptr(), ws.data_ptr(), ws.numel())
    return out, lse


def _attn_backward_split(arithmetic):
    """False for the exact-fp32 attention backward, True for the fp16 x 2 split products (amav_*attn_backward_split).
    arithmetic: "f32" | "split"; None follows AMAV_ATTN_BACKWARD (read per call, like AMAV_CROSS_ATTN; default f32)."""
    chosen = arithmetic if arithmetic is not None else os.environ.get("AMAV_ATTN_BACKWARD", "f32")
    if chosen == "f32":
        return False
    if chosen == "split":
        return True
    where = "arithmetic" if arithmetic is not None else "AMAV_ATTN_BACKWARD"
    raise AmavError(f"attention backward: {where} must be 'f32' or 'split', got {chosen!r}")


def _attn_backward_entry(kind, arithmetic):
    """(size query, entry point) of the dense backward of kind "self" | "cross" in `arithmetic` (_attn_backward_split)."""
    entry = f"amav_{kind}attn_backward" + ("_split" if _attn_backward_split(arithmetic) else "")
    return entry + "_workspace_bytes", entry


def selfattn_backward(qkv, out, lse, grad_out, heads, scale=None, grad_qkv=None, arithmetic=None):
    """amav_selfattn_backward: the gradient [B,S,3*H*D] (dq | dk | dv) of a fused qkv given the forward's out and lse
    (selfattn_lse) and grad_out = dLoss/d out.  out / grad_out: [B,S,H*D] with unit inner stride and dense batch stride;
    grad_qkv: optional [B,S,>=3*H*D] destination view (its first 3*H*D columns are written).  arithmetic: "f32" (exact
    fp32 products) or "split" (amav_selfattn_backward_split: fp16 x 2 split products); None follows AMAV_ATTN_BACKWARD."""
    sizer, entry = _attn_backward_entry("self", arithmetic)
    B, S, HD, D = _qkv_views(qkv, heads)
    _rows(out, "out", B, S, width=HD), _rows(grad_out, "grad_out", B, S, width=HD)
    lse = _contig(lse, "lse")
    if tuple(lse.shape) != (B, heads, S):
        raise AmavError(f"lse: need [B,H,S] = {(B, heads, S)}, got {tuple(lse.shape)}")
    if grad_qkv is None:
        grad_qkv = torch.empty(B, S, 3 * HD, device=qkv.device)
    _rows(grad_qkv, "grad_qkv", B, S, min_width=3 * HD)
    ws = _scratch(sizer, qkv.device, B, S, heads, D, rejected=f"B={B} S={S} H={heads} D={D}")
    p = qkv.data_ptr()
    _call(entry, B, S, heads, D, p, p + 4 * HD, p + 8 * HD, qkv.stride(1), out.data_ptr(),
          out.stride(1), lse.data_ptr(), grad_out.data_ptr(), grad_out.stride(1), grad_qkv.data_ptr(),
          grad_qkv.stride(1), float(scale if scale is not None else D ** -0.5), ws.data_ptr(), ws.numel())
    return grad_qkv


class _SelfAttn(torch.autograd.Function):
    """selfattn_lse with amav_selfattn_backward as the backward; qkv, the output and the row log-sum-exp are kept."""

    @staticmethod
    def forward(ctx, qkv, heads, scale):
        out, lse = selfattn_lse(qkv, heads, scale)
        ctx.heads, ctx.scale = heads, scale
        ctx.save_for_backward(qkv, out, lse)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        qkv, out, lse = ctx.saved_tensors
        return selfattn_backward(qkv, out, lse, _launchable(grad_out.float()), ctx.heads, ctx.scale), None, None


def selfattn_differentiable(qkv, heads, scale=None):
    """softmax(q k^T * scale) v as a torch.autograd.Function over a fused [B,S,3*H*D] qkv (q | k | v along the last axis,
    D = 64) -> [B,S,H*D]; the backward returns d qkv in the same fused layout (amav_selfattn_backward), so the gradient
    of a fused q/k/v weight is one GEMM.  Needs the default fp16 x 2 forward (set_option("attn", ...) = fp16)."""
    return _SelfAttn.apply(_launchable(qkv), int(heads), scale)


def _kv_views(kv, heads):
    """[B,Sk,2*H*D] fused k | v projection output -> (k, v) views sharing its row stride."""
    _rows(kv, "kv")
    if kv.shape[2] % (2 * heads):
        raise AmavError(f"kv: need [B,Sk,2*H*D], got {tuple(kv.shape)} for {heads} heads")
    HD = kv.shape[2] // 2
    return kv[..., :HD], kv[..., HD:]


def _crossattn(q, k, v, heads, scale, want_lse):
    _rows(q, "q")
    B, Sq, HD = q.shape
    Sk = _rows(k, "k", B=B, width=HD).shape[1]
    _rows(v, "v", B=B, S=Sk, width=HD)
    if HD % heads or k.stride(1) != v.stride(1):
        raise AmavError("crossattn: k and v must share shape and row stride, and H must divide the row width")
    D = HD // heads
    out = torch.empty(B, Sq, HD, device=q.device)
    lse = torch.empty(B, heads, Sq, device=q.device) if want_lse else None
    ws = _scratch("amav_crossattn_workspace_bytes", q.device, B, Sq, Sk, heads, D,
                  rejected=f"B={B} Sq={Sq} Sk={Sk} H={heads} D={D}")
    _call("amav_crossattn_forward", B, Sq, Sk, heads, D, q.data_ptr(), q.stride(1), k.data_ptr(), v.data_ptr(), k.stride(1),
          out.data_ptr(), HD, float(scale if scale is not None else D ** -0.5), lse.data_ptr() if want_lse else None,
          ws.data_ptr(), ws.numel())
    return out, lse


def crossattn(q, k, v, heads, scale=None):
    """softmax(q k^T * scale) v for q [B,Sq,H*D] and k, v [B,Sk,H*D] sharing shape and row stride (e.g. the halves of a
    fused k | v projection), any Sq and Sk, D = 64 -> [B,Sq,H*D] (amav_crossattn_forward).  Always the fp16 x 2 kernels,
    whatever set_option("attn", ...) selects for self-attention."""
    return _crossattn(q, k, v, heads, scale, False)[0]


def crossattn_lse(q, kv, heads, scale=None):
    """crossattn over a fused kv [B,Sk,2*H*D] (k | v, read in place) -> (out [B,Sq,H*D], lse [B,H,Sq]), lse the row
    log-sum-exp in natural units that crossattn_backward needs.  `out` equals crossattn()'s bit for bit."""
    return _crossattn(q, *_kv_views(kv, heads), heads, scale, True)


def crossattn_backward(q, kv, out, lse, grad_out, heads, scale=None, grad_q=None, grad_kv=None, arithmetic=None):
    """amav_crossattn_backward: (dq [B,Sq,H*D], dkv [B,Sk,2*H*D] = dk | dv) given the forward's out and lse
    (crossattn_lse) and grad_out = dLoss/d out.  grad_q / grad_kv: optional [B,Sq,>=H*D] / [B,Sk,>=2*H*D] destination
    views (their first H*D / 2*H*D columns are written).  arithmetic: as selfattn_backward's
    (amav_crossattn_backward_split)."""
    sizer, entry = _attn_backward_entry("cross", arithmetic)
    k, v = _kv_views(kv, heads)
    B, Sk, HD = k.shape
    Sq = _rows(q, "q", B=B, width=HD).shape[1]
    D = HD // heads
    _rows(out, "out", B, Sq, width=HD), _rows(grad_out, "grad_out", B, Sq, width=HD)
    lse = _contig(lse, "lse")
    if tuple(lse.shape) != (B, heads, Sq):
        raise AmavError(f"lse: need [B,H,Sq] = {(B, heads, Sq)}, got {tuple(lse.shape)}")
    if grad_q is None:
        grad_q = torch.empty(B, Sq, HD, device=q.device)
    if grad_kv is None:
        grad_kv = torch.empty(B, Sk, 2 * HD, device=q.device)
    _rows(grad_q, "grad_q", B, Sq, min_width=HD), _rows(grad_kv, "grad_kv", B, Sk, min_width=2 * HD)
    ws = _scratch(sizer, q.device, B, Sq, heads, D,
                  rejected=f"B={B} Sq={Sq} H={heads} D={D}")
    _call(entry, B, Sq, Sk, heads, D, q.data_ptr(), q.stride(1), k.data_ptr(), v.data_ptr(),
          kv.stride(1), out.data_ptr(), out.stride(1), lse.data_ptr(), grad_out.data_ptr(), grad_out.stride(1),
          grad_q.data_ptr(), grad_q.stride(1), grad_kv.data_ptr(), grad_kv.stride(1),
          float(scale if scale is not None else D ** -0.5), ws.data_ptr(), ws.numel())
    return grad_q, grad_kv


class _CrossAttn(torch.autograd.Function):
    """crossattn_lse with amav_crossattn_backward as the backward; q, kv, the output and the row log-sum-exp are kept."""

    @staticmethod
    def forward(ctx, q, kv, heads, scale):
        out, lse = crossattn_lse(q, kv, heads, scale)
        ctx.heads, ctx.scale = heads, scale
        ctx.save_for_backward(q, kv, out, lse)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        q, kv, out, lse = ctx.saved_tensors
        dq, dkv = crossattn_backward(q, kv, out, lse, _launchable(grad_out.float()), ctx.heads, ctx.scale)
        return dq, dkv, None, None


def crossattn_differentiable(q, kv, heads, scale=None):
    """softmax(q k^T * scale) v as a torch.autograd.Function over q [B,Sq,H*D] and a fused kv [B,Sk,2*H*D] (k | v along
    the last axis, D = 64) -> [B,Sq,H*D]; the backward returns dq and d kv in the same fused layout
    (amav_crossattn_backward), so the gradient of a fused to_k / to_v weight is one GEMM."""
    return _CrossAttn.apply(_launchable(q), _launchable(kv), int(heads), scale)


_GEMM_WS = {}


def gemm_split_fp16(a, w, alpha=1.0, algo_index=-1):
    """a [rows, k3] fp16 x w [n, k3]^T fp16 -> [rows, n] fp32 (fp32 accumulate, scaled by alpha) through hipBLASLt with
    the kernel named by `algo_index` (-1: the library's own heuristic; include/amav.h, amav_gemm_split_fp16)."""
    a, w = _need(a, "a", torch.float16), _need(w, "w", torch.float16)
    if a.dim() != 2 or w.dim() != 2 or a.shape[1] != w.shape[1] or not a.is_contiguous() or not w.is_contiguous():
        raise AmavError("gemm_split_fp16: need contiguous a [rows, k3] and w [n, k3]")
    out = torch.empty(a.shape[0], w.shape[0], device=a.device)
    ws = _GEMM_WS.get(a.device)
    if ws is None:
        ws = _GEMM_WS[a.device] = torch.empty(32 << 20, dtype=torch.uint8, device=a.device)
    _call("amav_gemm_split_fp16", a.shape[0], w.shape[0], a.shape[1], a.data_ptr(), w.data_ptr(), float(alpha),
          out.data_ptr(), int(algo_index), ws.data_ptr(), ws.numel())
    return out


def gemm_split_fp16_tune(a, w, repeats=10):
    """Times every hipBLASLt kernel on these operands (synchronises; seconds per shape) -> (best index, best ms,
    ms of the library's heuristic choice).  a [copies, rows, k3], w [copies, n, k3] (or 2-D: one set): run i uses set
    i % copies, so with several sets the kernels are timed out of MALL / HBM as inside the transformer step."""
    a, w = _need(a, "a", torch.float16), _need(w, "w", torch.float16)
    if a.dim() == 2:
        a, w = a[None], w[None]
    copies = a.shape[0]
    if w.shape[0] != copies or not a.is_contiguous() or not w.is_contiguous():
        raise AmavError("gemm_split_fp16_tune: need contiguous a [copies, rows, k3], w [copies, n, k3]")
    out = torch.empty(copies, a.shape[1], w.shape[1], device=a.device)
    a, w = a.view(-1, a.shape[-1]), w.view(-1, w.shape[-1])
    rows, n = a.shape[0] // copies, w.shape[0] // copies
    ws = torch.empty(64 << 20, dtype=torch.uint8, device=a.device)
    idx, best, heur = ctypes.c_int32(-1), ctypes.c_float(0), ctypes.c_float(0)
    _call("amav_gemm_split_fp16_tune", rows, n, a.shape[1], a.data_ptr(), w.data_ptr(), out.data_ptr(), ws.data_ptr(),
          ws.numel(), int(repeats), int(copies), ctypes.byref(idx), ctypes.byref(best), ctypes.byref(heur))
    return int(idx.value), float(best.value), float(heur.value)


def gemm_library_version() -> str:
    return _lib.lib().amav_gemm_library_version().decode()


def _split_buffer(rows, k, fmt, device):
    if fmt == SPLIT_FP16X2:
        return torch.empty(rows, 3 * k, dtype=torch.float16, device=device)
    if fmt == SPLIT_BF16X3:
        return torch.empty(rows, 6 * k, dtype=torch.bfloat16, device=device)
    raise AmavError(f"unknown split format {fmt}")


def geglu(proj, bias=None, split_exp=None):
    """proj [..., 2*inner] (contiguous, fp32) -> [..., inner] = h * gelu(g) (exact erf) with h, g the two halves of
    proj (+ bias [2*inner], when the projection's GEMM ran without it).  With split_exp the result is written as the
    fp16 x 2 activation operand [rows, 3*inner] of the next projection, pre-scaled by 2^split_exp."""
    proj = _need(proj, "proj")
    if not proj.is_contiguous() or proj.shape[-1] % 8:
        raise AmavError("geglu: need a contiguous [..., 2*inner] tensor with inner a multiple of 4")
    inner = proj.shape[-1] // 2
    rows = proj.numel() // proj.shape[-1]
    if split_exp is None:
        out = torch.empty(*proj.shape[:-1], inner, device=proj.device)
    else:
        out = _split_buffer(rows, inner, SPLIT_FP16X2, proj.device)
    bias_ptr = None if bias is None else _shaped(bias, "bias", (2 * inner,)).data_ptr()
    _call("amav_geglu", rows, inner, proj.data_ptr(), proj.shape[-1], bias_ptr,
          out.data_ptr() if split_exp is None else None, None if split_exp is None else out.data_ptr(),
          int(split_exp or 0))
    return out


def split_operand(x, weights=False, fmt=SPLIT_BF16X3, scale_exp=0):
    """x [rows, k] fp32 (unit inner stride; k a multiple of 8) -> the activation (default) or weight operand of an
    fp32-equivalent GEMM on the low-precision matrix pipe: [rows, 6 k] bf16 (SPLIT_BF16X3, any finite x) or [rows, 3 k]
    fp16 of x * 2^scale_exp (SPLIT_FP16X2; the caller bounds |x| 2^scale_exp by 32768).  include/amav.h,
    amav_split_operand."""
    x = _need(x, "x")
    if x.dim() != 2 or x.stride(1) != 1 or x.shape[1] % 8 or x.stride(0) % 4 or x.data_ptr() % 16:
        raise AmavError("split_operand: need a 16-byte aligned [rows, k] tensor, unit inner stride, k a multiple of 8")
    out = _split_buffer(x.shape[0], x.shape[1], fmt, x.device)
    _call("amav_split_operand", x.shape[0], x.shape[1], x.data_ptr(), x.stride(0), int(bool(weights)), int(fmt),
          int(scale_exp), out.data_ptr())
    return out


def split_operand_transposed(x, weights=False, also_rows=False):
    """x [rows, k] fp32 (as split_operand takes it) -> the bf16 x 3 activation (default) or weight operand of x^T,
    [k, 6 Rp] bf16 with Rp = rows rounded up to a multiple of 8: part p of column c at [c, p Rp : p Rp + rows], zeros after
    it.  With also_rows -> (split_operand(x), that operand) from one read of x; the row-major one is the ACTIVATION operand
    whatever `weights` is.  include/amav.h, amav_split_operand_transposed."""
    x = _need(x, "x")
    if x.dim() != 2 or x.stride(1) != 1 or x.shape[1] % 8 or x.stride(0) % 4 or x.data_ptr() % 16:
        raise AmavError("split_operand_transposed: need a 16-byte aligned [rows, k] tensor, unit inner stride, k a "
                        "multiple of 8")
    rows, k = x.shape
    padded = _lib.lib().amav_split_transposed_rows(rows)
    out_t = torch.empty(k, 6 * padded, dtype=torch.bfloat16, device=x.device)
    out_rows = _split_buffer(rows, k, SPLIT_BF16X3, x.device) if also_rows else None
    _call("amav_split_operand_transposed", rows, k, x.data_ptr(), x.stride(0), int(bool(weights)),
          out_rows.data_ptr() if also_rows else None, out_t.data_ptr())
    return (out_rows, out_t) if also_rows else out_t


def add_layernorm(hidden, add, batch_row, weight, bias, eps=1e-5, add_bias=None, split=None, split_exp=0):
    """hidden [B,S,dim] (contiguous), add [B,S,dim] or None (+ add_bias [dim]: the bias of the projection that produced
    it), batch_row [B,1,dim] or None -> (h = batch_row + ((add + add_bias) + hidden), LayerNorm(h) * weight + bias), two
    new tensors; with split = SPLIT_BF16X3 / SPLIT_FP16X2 the second is the activation operand of the next projection
    (split_operand's layout, pre-scaled by 2^split_exp for fp16) instead of fp32 [B,S,dim].  transformers.py:292-399."""
    hidden = _need(hidden, "hidden")
    if hidden.dim() != 3 or not hidden.is_contiguous():
        raise AmavError("add_layernorm: hidden must be a contiguous [B,S,dim] tensor")
    B, S, dim = hidden.shape
    ptr = lambda t, name, shape: None if t is None else _shaped(t, name, shape).data_ptr()
    h_out = torch.empty_like(hidden)
    out = torch.empty_like(hidden) if split is None else _split_buffer(B * S, dim, split, hidden.device)
    _call("amav_add_layernorm", B * S, dim, S, ptr(add, "add", (B, S, dim)), ptr(add_bias, "add_bias", (dim,)),
          ptr(batch_row, "batch_row", (B, 1, dim)), hidden.data_ptr(), h_out.data_ptr(),
          _shaped(weight, "weight", (dim,)).data_ptr(), _shaped(bias, "bias", (dim,)).data_ptr(), float(eps),
          out.data_ptr() if split is None else None, None if split is None else out.data_ptr(), int(split or 0),
          int(split_exp))
    return h_out, out


def _shaped(t, name, shape):
    t = _need(t, name)
    if tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise AmavError(f"{name}: expected a contiguous tensor of shape {tuple(shape)}, got {tuple(t.shape)}")
    return t


# ------------------------------------------------------------------- the row kernels under autograd
ROWS_CHUNK = 16  # rows per first-stage partial of rows_colsum and of the LayerNorm backward's dweight / dbias


def rows_colsum(x, rows_per_group=None):
    """x [rows, cols] fp32 (unit inner stride, row stride a multiple of 4, cols a multiple of 4) -> [groups, cols], the
    column sums over consecutive groups of rows_per_group rows (None: one group), in the fixed two-stage order of
    include/amav.h (chunks of ROWS_CHUNK rows ascending, then the chunk partials ascending): bit-identical between calls,
    and a batch of groups equals the groups one by one."""
    x = _need(x, "x")
    if x.dim() != 2 or x.stride(1) != 1 or x.shape[1] % 4 or x.stride(0) % 4 or x.data_ptr() % 16:
        raise AmavError("rows_colsum: need a 16-byte aligned [rows, cols] tensor, unit inner stride, cols a multiple of 4")
    rows, cols = x.shape
    per_group = rows if rows_per_group is None else int(rows_per_group)
    if rows < 1 or per_group < 1 or rows % per_group:
        raise AmavError(f"rows_colsum: rows={rows} is not a positive multiple of rows_per_group={per_group}")
    ws = _scratch("amav_rows_colsum_workspace_bytes", x.device, rows, cols, per_group,
                  rejected=f"rows={rows} cols={cols} rows_per_group={per_group}")
    out = torch.empty(rows // per_group, cols, device=x.device)
    _call("amav_rows_colsum", rows, cols, x.data_ptr(), x.stride(0), per_group, out.data_ptr(), ws.data_ptr(), ws.numel())
    return out


def geglu_backward(proj, bias, grad_out):
    """amav_geglu_backward: proj [..., 2*inner] (contiguous; + bias [2*inner] or None) as geglu() read it and grad_out
    [..., inner] -> d proj [..., 2*inner].  The bias gradient is rows_colsum of the result."""
    proj, grad_out = _need(proj, "proj"), _contig(grad_out, "grad_out")
    if not proj.is_contiguous() or proj.shape[-1] % 8:
        raise AmavError("geglu_backward: need a contiguous [..., 2*inner] tensor with inner a multiple of 4")
    inner = proj.shape[-1] // 2
    rows = proj.numel() // proj.shape[-1]
    if tuple(grad_out.shape) != tuple(proj.shape[:-1]) + (inner,):
        raise AmavError(f"grad_out: expected {tuple(proj.shape[:-1]) + (inner,)}, got {tuple(grad_out.shape)}")
    bias_ptr = None if bias is None else _shaped(bias, "bias", (2 * inner,)).data_ptr()
    grad = torch.empty_like(proj)
    _call("amav_geglu_backward", rows, inner, proj.data_ptr(), 2 * inner, bias_ptr, grad_out.data_ptr(), grad.data_ptr(),
          2 * inner)
    return grad


def add_layernorm_backward(h, weight, eps, grad_norm, grad_h):
    """amav_add_layernorm_backward: h [B,S,dim] = add_layernorm()'s first result, weight [dim], the upstream gradients of
    its two results (either may be None = zero) -> (dh [B,S,dim], dweight [dim], dbias [dim]).  dh is the gradient of
    `hidden` and of `add`; those of batch_row and add_bias are rows_colsum(dh) per batch item / over all rows."""
    h = _need(h, "h")
    if h.dim() != 3 or not h.is_contiguous():
        raise AmavError("add_layernorm_backward: h must be a contiguous [B,S,dim] tensor")
    B, S, dim = h.shape
    ptr = lambda t, name: None if t is None else _shaped(t, name, (B, S, dim)).data_ptr()
    ws = _scratch("amav_add_layernorm_backward_workspace_bytes", h.device, B * S, dim, rejected=f"rows={B * S} dim={dim}")
    dh = torch.empty_like(h)
    dweight, dbias = torch.empty(dim, device=h.device), torch.empty(dim, device=h.device)
    _call("amav_add_layernorm_backward", B * S, dim, h.data_ptr(), _shaped(weight, "weight", (dim,)).data_ptr(), float(eps),
          ptr(grad_norm, "grad_norm"), ptr(grad_h, "grad_h"), dh.data_ptr(), dweight.data_ptr(), dbias.data_ptr(),
          ws.data_ptr(), ws.numel())
    return dh, dweight, dbias


class _Geglu(torch.autograd.Function):
    """geglu (fp32 output) with amav_geglu_backward as the backward; only proj and bias are kept."""

    @staticmethod
    def forward(ctx, proj, bias):
        ctx.save_for_backward(proj, bias)
        return geglu(proj, bias=bias)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        proj, bias = ctx.saved_tensors
        grad = geglu_backward(proj, bias, grad_out.float())
        grad_bias = rows_colsum(grad.view(-1, grad.shape[-1]))[0] if bias is not None and ctx.needs_input_grad[1] else None
        return (grad if ctx.needs_input_grad[0] else None), grad_bias


def geglu_differentiable(proj, bias=None):
    """geglu(proj, bias) as a torch.autograd.Function: the same values bit for bit, gradients for proj and bias from
    amav_geglu_backward / amav_rows_colsum.  Saves proj and bias only (gelu(gate) is recomputed)."""
    return _Geglu.apply(_need(proj, "proj").contiguous(), bias)


class _AddLayerNorm(torch.autograd.Function):
    """add_layernorm (fp32 rows) with amav_add_layernorm_backward as the backward; h and weight are kept, the normalised
    rows are not."""

    @staticmethod
    def forward(ctx, hidden, add, batch_row, weight, bias, eps, add_bias):
        h, norm = add_layernorm(hidden, add, batch_row, weight, bias, eps, add_bias=add_bias)
        ctx.eps = float(eps)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(h, weight)
        return h, norm

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_h, grad_norm):
        h, weight = ctx.saved_tensors
        B, S, dim = h.shape
        ready = lambda g: None if g is None else g.float().contiguous()
        dh, dweight, dbias = add_layernorm_backward(h, weight, ctx.eps, ready(grad_norm), ready(grad_h))
        need = ctx.needs_input_grad
        rows = dh.view(B * S, dim)
        return (dh if need[0] else None, dh if need[1] else None,
                rows_colsum(rows, S).view(B, 1, dim) if need[2] else None,
                dweight if need[3] else None, dbias if need[4] else None, None,
                rows_colsum(rows)[0] if need[6] else None)


def add_layernorm_differentiable(hidden, add, batch_row, weight, bias, eps=1e-5, add_bias=None):
    """add_layernorm(...) -> (h, norm) as a torch.autograd.Function: the same values bit for bit, gradients for hidden,
    add, batch_row, weight, bias and add_bias from amav_add_layernorm_backward / amav_rows_colsum.  Saves h and weight;
    mean, rstd and the normalised rows are recomputed."""
    return _AddLayerNorm.apply(_need(hidden, "hidden").contiguous(), add if add is None else _need(add, "add").contiguous(),
                               batch_row if batch_row is None else _need(batch_row, "batch_row").contiguous(),
                               weight, bias, float(eps), add_bias)


# --------------------------------------------------- linear layers on bf16 x 3 split products under autograd
def _rows_2d(t, width):
    """t [..., width] -> a [rows, width] view (a copy where the kernels could not read it in place)."""
    t = t.reshape(-1, width)
    if t.stride(1) != 1 or t.stride(0) % 4 or t.stride(0) < width:
        t = t.contiguous()
    return t.clone() if t.data_ptr() % 16 else t


class _LinearSplit(torch.autograd.Function):
    """x W^T (+ b) and both of its backward products as bf16 x 3 split GEMMs (those named in `library`: the library's fp32
    GEMM); x and W are kept in fp32, as F.linear keeps them, and every split operand is rebuilt where it is used."""

    @staticmethod
    def forward(ctx, x, weight, bias, weight_split, weight_split_t, library):
        N, K = weight.shape
        if "forward" in library:
            y = torch.nn.functional.linear(_rows_2d(x, K), weight, bias)
        else:
            b = weight_split() if weight_split else split_operand(weight.detach(), weights=True)
            a = split_operand(_rows_2d(x, K))
            if bias is None:
                y = torch.mm(a, b.t(), out_dtype=torch.float32)
            else:
                y = torch.addmm(bias, a, b.t(), out_dtype=torch.float32)
        ctx.weight_split_t, ctx.library = weight_split_t, library
        ctx.has_bias = bias is not None
        ctx.save_for_backward(x, weight)
        return y.view(*x.shape[:-1], N)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        x, weight = ctx.saved_tensors
        N, K = weight.shape
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        g = _rows_2d(grad_out.float(), N)  # [rows, N]; an expanded gradient becomes a real one here
        grad_x = grad_w = grad_b = None
        split_x, split_w = need_x and "dgrad" not in ctx.library, need_w and "wgrad" not in ctx.library
        g_rows = g_t = None
        if split_x and split_w:
            g_rows, g_t = split_operand_transposed(g, also_rows=True)  # both forms from one read of g
        elif split_x:
            g_rows = split_operand(g)
        elif split_w:
            g_t = split_operand_transposed(g)
        if split_x:  # dx = g W: contraction over the rows of W, so W^T's weight operand [K, 6 N]
            make = ctx.weight_split_t
            wt = make() if make else split_operand_transposed(weight.detach(), weights=True)
            grad_x = torch.mm(g_rows, wt.t(), out_dtype=torch.float32).view(x.shape)
        elif need_x:
            grad_x = torch.mm(g, weight).view(x.shape)
        if split_w:  # dW = g^T x: contraction over the (padded) rows of both
            xt = split_operand_transposed(_rows_2d(x, K), weights=True)
            grad_w = torch.mm(g_t, xt.t(), out_dtype=torch.float32)
        elif need_w:
            grad_w = torch.mm(g.t(), _rows_2d(x, K))
        if ctx.has_bias and need_b:
            grad_b = rows_colsum(g)[0]
        return grad_x, grad_w, grad_b, None, None, None


LINEAR_PRODUCTS = ("forward", "dgrad", "wgrad")


def linear_split_differentiable(x, weight, bias=None, weight_split=None, weight_split_t=None, library=()):
    """F.linear(x, weight, bias) for HIP fp32 tensors (x [..., K], weight [N, K], K and N multiples of 8) as a
    torch.autograd.Function whose three products are fp32-equivalent bf16 x 3 split GEMMs:
        y  = mm(split_operand(x), split_operand(W, weights=True)^T) + b     -- transformer.linear's values, bit for bit
        dx = mm(split_operand(g), split_operand_transposed(W, weights=True)^T)
        dW = mm(split_operand_transposed(g), split_operand_transposed(x, weights=True)^T)      (K' = 6 rows)
        db = rows_colsum(g)
    with both operands of g from one read when dx and dW are both wanted, and no product for an input that needs no
    gradient.  weight_split / weight_split_t: zero-argument callables returning the two weight operands (a caller's
    cache, looked up only when the operand is needed); None builds them per call.  Always the split path for
    the sizes it accepts; `library` names the products (of LINEAR_PRODUCTS) a caller has measured slower there and wants
    as the library's fp32 GEMM inside the same Function -- transformer.train_linear's choice, () here."""
    x, weight = _need(x, "x"), _need(weight, "weight")
    if weight.dim() != 2 or x.dim() < 1 or x.shape[-1] != weight.shape[1] or x.numel() == 0:
        raise AmavError(f"linear_split_differentiable: x {tuple(x.shape)} does not match weight {tuple(weight.shape)}")
    N, K = weight.shape
    if K % 8 or N % 8:
        raise AmavError(f"linear_split_differentiable: K={K} and N={N} must be multiples of 8")
    if bias is not None:
        _shaped(bias, "bias", (N,))
    if any(f is not None and not callable(f) for f in (weight_split, weight_split_t)):
        raise AmavError("linear_split_differentiable: weight_split / weight_split_t are zero-argument callables or None")
    library = frozenset(library)
    if not library <= set(LINEAR_PRODUCTS):
        raise AmavError(f"linear_split_differentiable: unknown products {sorted(library - set(LINEAR_PRODUCTS))}")
    weight = weight if weight.is_contiguous() else weight.contiguous()
    return _LinearSplit.apply(x, weight, bias, weight_split, weight_split_t, library)


# ------------------------------------------------------------------ stage-1 TriplaneDownsampler
DWCONV_MIN_CHANNELS, DWCONV_MAX_CHANNELS = 64, 512  # amav_dwconv7_layernorm: a multiple of 64 in this range


def dwconv7_channels_ok(channels) -> bool:
    """Whether amav_dwconv7_layernorm is built for this width."""
    return DWCONV_MIN_CHANNELS <= channels <= DWCONV_MAX_CHANNELS and channels % 64 == 0


def _planes(x, name):
    x = _need(x, name)
    if x.dim() != 4 or not x.is_contiguous():
        raise AmavError(f"{name}: expected contiguous channels-last planes [K,H,W,C], got {tuple(x.shape)}")
    return x


def _split_out(rows, k, split, device):
    """(fp32 [rows, k] or None, split operand or None) for the kernels that write exactly one of them."""
    if split is None:
        return torch.empty(rows, k, device=device), None
    return None, _split_buffer(rows, k, split, device)


def dwconv7_layernorm(x, dw_weight, dw_bias, ln_weight, ln_bias, eps=1e-6, split=None, split_exp=0, want_y=False):
    """ConvNeXtBlock's dwconv -> LayerNorm (triplane_net.py:414-424) in one kernel: x [K,H,W,C] channels-last planes,
    dw_weight [C,1,7,7] (nn.Conv2d, groups=C), dw_bias / ln_weight / ln_bias [C] -> the normalised rows [K*H*W, C], fp32
    or (split = SPLIT_BF16X3 / SPLIT_FP16X2) the activation operand of the projection that follows.  want_y: also return
    y [K,H,W,C], the convolution before the norm -> (rows, y).  include/amav.h, amav_dwconv7_layernorm."""
    x = _planes(x, "x")
    K, H, W, C = x.shape
    w = _shaped(dw_weight, "dw_weight", (C, 1, 7, 7))
    out, out_split = _split_out(K * H * W, C, split, x.device)
    y = torch.empty_like(x) if want_y else None
    _call("amav_dwconv7_layernorm", K, H, W, C, x.data_ptr(), w.data_ptr(), _shaped(dw_bias, "dw_bias", (C,)).data_ptr(),
          _shaped(ln_weight, "ln_weight", (C,)).data_ptr(), _shaped(ln_bias, "ln_bias", (C,)).data_ptr(), float(eps),
          None if y is None else y.data_ptr(), None if out is None else out.data_ptr(),
          None if out_split is None else out_split.data_ptr(), int(split or 0), int(split_exp))
    rows = out if out_split is None else out_split
    return (rows, y) if want_y else rows


def dwconv7_layernorm_backward(x, y, dw_weight, ln_weight, eps, grad_norm):
    """amav_dwconv7_layernorm_backward: x, y [K,H,W,C] (the forward's input and its y), grad_norm [K*H*W, C] ->
    (dx [K,H,W,C], d dw_weight [C,1,7,7], d dw_bias [C], d ln_weight [C], d ln_bias [C])."""
    x, y = _planes(x, "x"), _planes(y, "y")
    K, H, W, C = x.shape
    if y.shape != x.shape:
        raise AmavError(f"dwconv7_layernorm_backward: y {tuple(y.shape)} does not match x {tuple(x.shape)}")
    g = _shaped(grad_norm, "grad_norm", (K * H * W, C))
    ws = _scratch("amav_dwconv7_layernorm_backward_workspace_bytes", x.device, K, H, W, C,
                  rejected=f"planes={K} height={H} width={W} channels={C}")
    dx, d_w = torch.empty_like(x), torch.empty(C, 1, 7, 7, device=x.device)
    d_b, d_lw, d_lb = (torch.empty(C, device=x.device) for _ in range(3))
    _call("amav_dwconv7_layernorm_backward", K, H, W, C, x.data_ptr(), y.data_ptr(),
          _shaped(dw_weight, "dw_weight", (C, 1, 7, 7)).data_ptr(), _shaped(ln_weight, "ln_weight", (C,)).data_ptr(),
          float(eps), g.data_ptr(), dx.data_ptr(), d_w.data_ptr(), d_b.data_ptr(), d_lw.data_ptr(), d_lb.data_ptr(),
          ws.data_ptr(), ws.numel())
    return dx, d_w, d_b, d_lw, d_lb


def _proj_rows(proj, name):
    proj = _need(proj, "proj")
    if proj.dim() < 1 or not proj.is_contiguous() or proj.shape[-1] % 4 or proj.numel() == 0:
        raise AmavError(f"{name}: need a contiguous [..., inner] tensor with inner a multiple of 4")
    return proj, proj.numel() // proj.shape[-1], proj.shape[-1]


def gelu_bias(proj, bias=None, split=None, split_exp=0):
    """proj [..., inner] (contiguous fp32; + bias [inner], when the projection's GEMM ran without it) -> gelu(proj + bias),
    exact erf: fp32 [..., inner], or with split the activation operand [rows, 6 inner] bf16 / [rows, 3 inner] fp16 of the
    next projection.  include/amav.h, amav_gelu_bias."""
    proj, rows, inner = _proj_rows(proj, "gelu_bias")
    out, out_split = _split_out(rows, inner, split, proj.device)
    _call("amav_gelu_bias", rows, inner, proj.data_ptr(), inner,
          None if bias is None else _shaped(bias, "bias", (inner,)).data_ptr(), None if out is None else out.data_ptr(),
          None if out_split is None else out_split.data_ptr(), int(split or 0), int(split_exp))
    return out.view(proj.shape) if out_split is None else out_split


def gelu_bias_backward(proj, bias, grad_out):
    """amav_gelu_bias_backward: proj (+ bias) as gelu_bias() read it and grad_out of proj's shape -> d proj.  The bias
    gradient is rows_colsum of the result."""
    proj, rows, inner = _proj_rows(proj, "gelu_bias_backward")
    grad_out = _shaped(_contig(grad_out, "grad_out"), "grad_out", proj.shape)
    grad = torch.empty_like(proj)
    _call("amav_gelu_bias_backward", rows, inner, proj.data_ptr(), inner,
          None if bias is None else _shaped(bias, "bias", (inner,)).data_ptr(), grad_out.data_ptr(), grad.data_ptr(), inner)
    return grad


def patch4_out_size(n, stride):
    """Output size of Conv2d(kernel 4, stride, padding 1) along an axis of n pixels."""
    return (int(n) - 2) // int(stride) + 1


def patch4_gather(x, stride, split=None, split_exp=0):
    """The im2col of Conv2d(C, C, 4, stride, padding 1) over channels-last planes: x [K,H,W,C] -> [K*Ho*Wo, 16*C], tap-major
    (column (4 ky + kx) C + c), zero outside the plane; fp32, or with split the activation operand of the product with
    the weight permuted to [C_out, ky, kx, C_in].  include/amav.h, amav_patch4_gather."""
    x = _planes(x, "x")
    K, H, W, C = x.shape
    if int(stride) < 2 or H < 2 or W < 2:
        raise AmavError(f"patch4_gather: stride={stride} height={H} width={W} (stride >= 2, height and width >= 2)")
    rows = K * patch4_out_size(H, stride) * patch4_out_size(W, stride)
    out, out_split = _split_out(rows, 16 * C, split, x.device)
    _call("amav_patch4_gather", K, H, W, C, int(stride), x.data_ptr(), None if out is None else out.data_ptr(),
          None if out_split is None else out_split.data_ptr(), int(split or 0), int(split_exp))
    return out if out_split is None else out_split


def patch4_gather_backward(grad_cols, shape, stride):
    """amav_patch4_gather_backward: grad_cols [K*Ho*Wo, 16*C] -> d x of `shape` = (K,H,W,C): every pixel adds the windows
    that cover it in ascending window index; exactly 0 where none does."""
    K, H, W, C = (int(s) for s in shape)
    rows = K * patch4_out_size(H, stride) * patch4_out_size(W, stride)
    g = _shaped(_contig(grad_cols, "grad_cols"), "grad_cols", (rows, 16 * C))
    dx = torch.empty(K, H, W, C, device=g.device)
    _call("amav_patch4_gather_backward", K, H, W, C, int(stride), g.data_ptr(), dx.data_ptr())
    return dx


class _DwConv7LayerNorm(torch.autograd.Function):
    """dwconv7_layernorm (fp32 rows) with amav_dwconv7_layernorm_backward as the backward; x, y and the two weights are
    kept (y is stored, not recomputed: DESIGN.md section 4.22), mean / rstd / the normalised rows are recomputed."""

    @staticmethod
    def forward(ctx, x, dw_weight, dw_bias, ln_weight, ln_bias, eps):
        rows, y = dwconv7_layernorm(x, dw_weight, dw_bias, ln_weight, ln_bias, eps, want_y=True)
        ctx.eps = float(eps)
        ctx.save_for_backward(x, y, dw_weight, ln_weight)
        return rows

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_rows):
        x, y, dw_weight, ln_weight = ctx.saved_tensors
        grads = dwconv7_layernorm_backward(x, y, dw_weight, ln_weight, ctx.eps, grad_rows.float().contiguous())
        return tuple(g if need else None for g, need in zip(grads, ctx.needs_input_grad)) + (None,)


def dwconv7_layernorm_differentiable(x, dw_weight, dw_bias, ln_weight, ln_bias, eps=1e-6):
    """dwconv7_layernorm(...) -> fp32 rows [K*H*W, C] as a torch.autograd.Function: the same values bit for bit, gradients
    for x and the four parameters from amav_dwconv7_layernorm_backward."""
    return _DwConv7LayerNorm.apply(_planes(x, "x"), dw_weight, dw_bias, ln_weight, ln_bias, float(eps))


class _GeluBias(torch.autograd.Function):
    """gelu_bias (fp32 output) with amav_gelu_bias_backward as the backward; only proj and bias are kept."""

    @staticmethod
    def forward(ctx, proj, bias):
        ctx.save_for_backward(proj, bias)
        return gelu_bias(proj, bias)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        proj, bias = ctx.saved_tensors
        grad = gelu_bias_backward(proj, bias, grad_out.float())
        grad_bias = rows_colsum(grad.view(-1, grad.shape[-1]))[0] if bias is not None and ctx.needs_input_grad[1] else None
        return (grad if ctx.needs_input_grad[0] else None), grad_bias


def gelu_bias_differentiable(proj, bias=None):
    """gelu_bias(proj, bias) as a torch.autograd.Function: the same values bit for bit, gradients for proj and bias from
    amav_gelu_bias_backward / amav_rows_colsum.  Saves proj and bias only."""
    return _GeluBias.apply(_need(proj, "proj").contiguous(), bias)


class _Patch4Gather(torch.autograd.Function):
    """patch4_gather (fp32 columns) with its transpose as the backward; nothing of the forward is kept but the shape."""

    @staticmethod
    def forward(ctx, x, stride):
        ctx.shape, ctx.stride = tuple(x.shape), int(stride)
        return patch4_gather(x, stride)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_cols):
        return patch4_gather_backward(grad_cols.float(), ctx.shape, ctx.stride), None


def patch4_gather_differentiable(x, stride):
    """patch4_gather(x, stride) -> fp32 [K*Ho*Wo, 16*C] as a torch.autograd.Function: the same values bit for bit, the
    gradient of x from amav_patch4_gather_backward."""
    return _Patch4Gather.apply(_planes(x, "x"), int(stride))


# -------------------------------------------------------------------------------------------------- point refiner
def cloud_voxelize(points, cloud_of, clouds, resolution=100.0):
    """points [n,3] fp32, cloud_of int32 [n] (ascending) -> (grid int32 [n,3] from the cloud's own origin, cloud_depth
    int32 [clouds]).  point_encoder.py:33 / pointtransformer_v3.py:98-101 per cloud."""
    points, cloud_of = _contig(points, "points"), _contig(cloud_of, "cloud_of", torch.int32)
    n = points.shape[0]
    if points.dim() != 2 or points.shape[1] != 3 or cloud_of.shape != (n,):
        raise AmavError(f"cloud_voxelize: points {tuple(points.shape)} / cloud_of {tuple(cloud_of.shape)}")
    grid = torch.empty(n, 3, dtype=torch.int32, device=points.device)
    depth = torch.empty(clouds, dtype=torch.int32, device=points.device)
    bounds = torch.empty(clouds, 6, dtype=torch.int32, device=points.device)
    _call("amav_cloud_voxelize", n, int(clouds), points.data_ptr(), cloud_of.data_ptr(), float(resolution),
          grid.data_ptr(), depth.data_ptr(), bounds.data_ptr())
    return grid, depth


def cloud_codes(grid, cloud_of, cloud_depth):
    """-> keys int64 [4,n] = cloud << 48 | code for the orders z, z-trans, hilbert, hilbert-trans."""
    grid, cloud_of = _contig(grid, "grid", torch.int32), _contig(cloud_of, "cloud_of", torch.int32)
    cloud_depth = _contig(cloud_depth, "cloud_depth", torch.int32)
    n = grid.shape[0]
    keys = torch.empty(4, n, dtype=torch.int64, device=grid.device)
    _call("amav_cloud_codes", n, grid.data_ptr(), cloud_of.data_ptr(), cloud_depth.data_ptr(), keys.data_ptr())
    return keys


def cloud_neighbors(grid, cloud_of, cloud_depth, cloud_start, sorted_keys, order, ksize):
    """-> nbr int32 [n, ksize^3]: the rows a submanifold convolution gathers (-1: empty voxel)."""
    grid, cloud_of = _contig(grid, "grid", torch.int32), _contig(cloud_of, "cloud_of", torch.int32)
    cloud_depth, cloud_start = _contig(cloud_depth, "cloud_depth", torch.int32), _contig(cloud_start, "cloud_start", torch.int32)
    sorted_keys, order = _contig(sorted_keys, "sorted_keys", torch.int64), _contig(order, "order", torch.int64)
    n = grid.shape[0]
    if sorted_keys.shape != (n,) or order.shape != (n,) or cloud_start.shape[0] != cloud_depth.shape[0] + 1:
        raise AmavError("cloud_neighbors: sorted_keys / order must be [n], cloud_start [clouds + 1]")
    nbr = torch.empty(n, ksize ** 3, dtype=torch.int32, device=grid.device)
    _call("amav_cloud_neighbors", n, int(ksize), grid.data_ptr(), cloud_of.data_ptr(), cloud_depth.data_ptr(),
          cloud_start.data_ptr(), sorted_keys.data_ptr(), order.data_ptr(), nbr.data_ptr())
    return nbr


def subm_pair_gemm(feat, pair_src, tap_start, tile_start, tiles, weights):
    """feat [n,C_in], pairs grouped by tap (pair_src int32 [P], tap_start / tile_start int32 [taps+1]), weights
    [taps,C_in,C_out] -> products [P,C_out] (include/amav.h)."""
    feat, weights = _contig(feat, "feat"), _contig(weights, "weights")
    pair_src = _contig(pair_src, "pair_src", torch.int32)
    tap_start, tile_start = _contig(tap_start, "tap_start", torch.int32), _contig(tile_start, "tile_start", torch.int32)
    taps, cin, cout = weights.shape
    if feat.shape[1] != cin or tap_start.shape != (taps + 1,) or tile_start.shape != (taps + 1,):
        raise AmavError("subm_pair_gemm: shapes do not match")
    products = torch.empty(pair_src.shape[0], cout, device=feat.device)
    _call("amav_subm_pair_gemm", pair_src.shape[0], int(tiles), taps, cin, cout, feat.data_ptr(), pair_src.data_ptr(),
          tap_start.data_ptr(), tile_start.data_ptr(), weights.data_ptr(), products.data_ptr())
    return products


def subm_prepare_weights_split(weights):
    """weights [taps,C_in,C_out] fp32 -> uint8 device buffer: two scaled fp16 parts in MFMA fragment order (include/amav.h,
    amav_subm_prepare_weights_split), the operand of subm_pair_gemm(..., weights_split=...)."""
    weights = _contig(weights, "weights")
    taps, cin, cout = weights.shape
    nbytes = _lib.lib().amav_subm_weights_split_bytes(taps, cin, cout)
    if nbytes == 0:
        raise AmavError(f"subm_prepare_weights_split: channels must be multiples of 32, got {cin} -> {cout}")
    out = torch.empty(nbytes, dtype=torch.uint8, device=weights.device)
    _call("amav_subm_prepare_weights_split", taps, cin, cout, weights.data_ptr(), out.data_ptr(), nbytes)
    return out


def subm_pair_gemm_split(feat, pair_src, tap_start, tile_start, tiles, weights_split, taps, cout):
    """subm_pair_gemm on the 16-bit matrix pipe: weights_split from subm_prepare_weights_split ([taps,C_in,cout])."""
    feat = _contig(feat, "feat")
    pair_src = _contig(pair_src, "pair_src", torch.int32)
    tap_start, tile_start = _contig(tap_start, "tap_start", torch.int32), _contig(tile_start, "tile_start", torch.int32)
    n, cin = feat.shape
    if tap_start.shape != (taps + 1,) or tile_start.shape != (taps + 1,):
        raise AmavError("subm_pair_gemm_split: shapes do not match")
    need = _lib.lib().amav_subm_weights_split_bytes(taps, cin, cout)
    if need == 0 or _need(weights_split, "weights_split", torch.uint8).numel() != need:
        raise AmavError("subm_pair_gemm_split: weights_split was not prepared for these shapes")
    products = torch.empty(pair_src.shape[0], cout, device=feat.device)
    scratch = torch.empty(4, dtype=torch.int32, device=feat.device)
    _call("amav_subm_pair_gemm_split", pair_src.shape[0], int(tiles), taps, cin, cout, n, feat.data_ptr(),
          pair_src.data_ptr(), tap_start.data_ptr(), tile_start.data_ptr(), weights_split.data_ptr(),
          scratch.data_ptr(), products.data_ptr())
    return products


def _no_autograd(name, *tensors):
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        raise AmavError(f"{name} carries no autograd: an input requires grad (call it under torch.no_grad())")


def conv3x3_prepare_weights(weight, out_scale=None):
    """torch's convolution weight [C_out,C_in,3,3] (times out_scale [C_out] per output channel when given) -> uint8 device
    buffer: two scaled fp16 parts in MFMA fragment order (include/amav.h, amav_conv3x3_prepare_weights_split), the
    `weights_split` of conv3x3_cells."""
    _no_autograd("conv3x3_prepare_weights", weight, out_scale)
    weight = _contig(weight, "weight")
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3):
        raise AmavError(f"conv3x3_prepare_weights: expected [C_out,C_in,3,3], got {tuple(weight.shape)}")
    cout, cin = weight.shape[:2]
    nbytes = _lib.lib().amav_conv3x3_weights_split_bytes(cin, cout)
    if nbytes == 0:
        raise AmavError(f"conv3x3_prepare_weights: channels must be multiples of 32, got {cin} -> {cout}")
    out = torch.empty(nbytes, dtype=torch.uint8, device=weight.device)
    _call("amav_conv3x3_prepare_weights_split", cin, cout, weight.data_ptr(),
          None if out_scale is None else _shaped(out_scale, "out_scale", (cout,)).data_ptr(), out.data_ptr(), nbytes)
    return out


def conv3x3_cells(x, weights_split, cout, bias=None, *, upsample_input=False, in_scale=None, in_shift=None, origin=None,
                  extent=0, relu_out=False, residual=None):
    """3x3 convolution (stride 1, zero padding 1) over independent channels-last cells on the 16-bit matrix pipe
    (include/amav.h, amav_conv3x3_cells): x [K,h,w,C_in] -> [K,H,W,cout], H = 2h with upsample_input (nearest x2 folded
    into the gather).  in_scale / in_shift [C_in]: relu(in_scale x + in_shift) in front; origin int32 [K,2] + extent: taps
    outside the plane read zero; bias [cout], relu_out, residual [K,H,W,cout]: the epilogue, in that order."""
    _no_autograd("conv3x3_cells", x, bias, in_scale, in_shift, residual)
    x = _contig(x, "x")
    if x.dim() != 4:
        raise AmavError(f"conv3x3_cells: x must be [K,h,w,C_in], got {tuple(x.shape)}")
    K, h, w, cin = x.shape
    H, W = (2 * h, 2 * w) if upsample_input else (h, w)
    cout = int(cout)
    need = _lib.lib().amav_conv3x3_weights_split_bytes(cin, cout)
    if need == 0 or _need(weights_split, "weights_split", torch.uint8).numel() != need:
        raise AmavError(f"conv3x3_cells: weights_split was not prepared for {cin} -> {cout} channels")
    if (in_scale is None) != (in_shift is None):
        raise AmavError("conv3x3_cells: in_scale and in_shift come together")
    a = Conv3x3Args()
    a.cells, a.height, a.width, a.cin, a.cout = K, H, W, cin, cout
    a.upsample_input, a.relu_out, a.extent = int(bool(upsample_input)), int(bool(relu_out)), int(extent)
    a.x_dev, a.weights_split_dev, a.weights_split_bytes = x.data_ptr(), weights_split.data_ptr(), need
    if in_scale is not None:
        a.in_scale_dev = _shaped(in_scale, "in_scale", (cin,)).data_ptr()
        a.in_shift_dev = _shaped(in_shift, "in_shift", (cin,)).data_ptr()
    if origin is not None:
        origin = _contig(origin, "origin", torch.int32)
        if tuple(origin.shape) != (K, 2):
            raise AmavError(f"conv3x3_cells: origin must be int32 [{K},2], got {tuple(origin.shape)}")
        a.origin_dev = origin.data_ptr()
    if bias is not None:
        a.bias_dev = _shaped(bias, "bias", (cout,)).data_ptr()
    if residual is not None:
        a.residual_dev = _shaped(residual, "residual", (K, H, W, cout)).data_ptr()
    out = torch.empty(K, H, W, cout, device=x.device)
    workspace = _scratch("amav_conv3x3_workspace_bytes", x.device)
    a.out_dev, a.workspace_dev, a.workspace_bytes = out.data_ptr(), workspace.data_ptr(), workspace.numel()
    if K == 0:
        return out
    _call("amav_conv3x3_cells", ctypes.byref(a))
    return out


def conv3x3_prepare_weights_transposed(weight):
    """torch's convolution weight [C_out,C_in,3,3] -> the prepared weights of conv3x3_cells' DATA gradient
    (amav_conv3x3_prepare_weights_split_transposed): W'[ci,co,a,b] = W[co,ci,2-a,2-b], split as conv3x3_prepare_weights."""
    _no_autograd("conv3x3_prepare_weights_transposed", weight)
    weight = _contig(weight, "weight")
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3):
        raise AmavError(f"conv3x3_prepare_weights_transposed: expected [C_out,C_in,3,3], got {tuple(weight.shape)}")
    cout, cin = weight.shape[:2]
    nbytes = _lib.lib().amav_conv3x3_weights_split_bytes(cout, cin)
    if nbytes == 0:
        raise AmavError(f"conv3x3_prepare_weights_transposed: channels must be multiples of 32, got {cin} -> {cout}")
    out = torch.empty(nbytes, dtype=torch.uint8, device=weight.device)
    _call("amav_conv3x3_prepare_weights_split_transposed", cin, cout, weight.data_ptr(), out.data_ptr(), nbytes)
    return out


def conv3x3_cells_backward(grad_out, x, weights_split_t=None, *, out=None, upsample_input=False, in_scale=None, in_shift=None,
                           origin=None, extent=0, relu_out=False, want_x=True, want_weight=True, want_bias=True,
                           want_prologue=None, wgrad_slices=0):
    """Backward of conv3x3_cells (include/amav.h, amav_conv3x3_cells_backward): grad_out [K,H,W,C_out], the forward's x
    and options, `out` the forward's result when relu_out, weights_split_t from conv3x3_prepare_weights_transposed (read
    for grad_x and the prologue's gradients).  -> (grad_x, grad_weight [C_out,C_in,3,3], grad_bias, grad_in_scale,
    grad_in_shift), None for what was not wanted (want_prologue None: wanted when there is a prologue).  wgrad_slices:
    split-K slices of the weight gradient, 0 = the library's heuristic.  Fixed summation orders: deterministic."""
    _no_autograd("conv3x3_cells_backward", grad_out, x, in_scale, in_shift, out)
    grad_out, x = _contig(grad_out, "grad_out"), _contig(x, "x")
    if x.dim() != 4 or grad_out.dim() != 4:
        raise AmavError(f"conv3x3_cells_backward: x must be [K,h,w,C_in] and grad_out [K,H,W,C_out], got {tuple(x.shape)}, "
                        f"{tuple(grad_out.shape)}")
    K, h, w, cin = x.shape
    H, W = (2 * h, 2 * w) if upsample_input else (h, w)
    cout = grad_out.shape[3]
    if tuple(grad_out.shape) != (K, H, W, cout):
        raise AmavError(f"conv3x3_cells_backward: grad_out {tuple(grad_out.shape)} does not match x {tuple(x.shape)}")
    need = _lib.lib().amav_conv3x3_weights_split_bytes(cout, cin)
    if need == 0:
        raise AmavError(f"conv3x3_cells_backward: channels must be multiples of 32, got {cin} -> {cout}")
    if (in_scale is None) != (in_shift is None):
        raise AmavError("conv3x3_cells_backward: in_scale and in_shift come together")
    want_prologue = in_scale is not None if want_prologue is None else bool(want_prologue)
    if want_prologue and in_scale is None:
        raise AmavError("conv3x3_cells_backward: want_prologue without a prologue")
    if not (want_x or want_weight or want_bias or want_prologue):
        raise AmavError("conv3x3_cells_backward: no gradient asked for")
    a = Conv3x3BackwardArgs()
    a.cells, a.height, a.width, a.cin, a.cout = K, H, W, cin, cout
    a.upsample_input, a.relu_out, a.extent, a.wgrad_slices = int(bool(upsample_input)), int(bool(relu_out)), int(extent), int(wgrad_slices)
    a.x_dev, a.grad_out_dev = x.data_ptr(), grad_out.data_ptr()
    if want_x or want_prologue:
        if weights_split_t is None or _need(weights_split_t, "weights_split_t", torch.uint8).numel() != need:
            raise AmavError(f"conv3x3_cells_backward: weights_split_t was not prepared for {cin} -> {cout} channels")
        a.weights_split_t_dev, a.weights_split_t_bytes = weights_split_t.data_ptr(), need
    if in_scale is not None:
        a.in_scale_dev = _shaped(in_scale, "in_scale", (cin,)).data_ptr()
        a.in_shift_dev = _shaped(in_shift, "in_shift", (cin,)).data_ptr()
    if origin is not None:
        origin = _contig(origin, "origin", torch.int32)
        if tuple(origin.shape) != (K, 2):
            raise AmavError(f"conv3x3_cells_backward: origin must be int32 [{K},2], got {tuple(origin.shape)}")
        a.origin_dev = origin.data_ptr()
    if relu_out:
        if out is None:
            raise AmavError("conv3x3_cells_backward: relu_out needs the forward's out")
        a.out_dev = _shaped(out, "out", (K, H, W, cout)).data_ptr()
    dev = x.device
    grad_x = torch.empty(K, h, w, cin, device=dev) if want_x else None
    grad_weight = torch.empty(cout, cin, 3, 3, device=dev) if want_weight else None
    grad_bias = torch.empty(cout, device=dev) if want_bias else None
    grad_scale = torch.empty(cin, device=dev) if want_prologue else None
    grad_shift = torch.empty(cin, device=dev) if want_prologue else None
    result = (grad_x, grad_weight, grad_bias, grad_scale, grad_shift)
    if K == 0:
        for t in result[1:]:
            if t is not None:
                t.zero_()
        return result
    for field, t in zip(("grad_x_dev", "grad_weight_dev", "grad_bias_dev", "grad_in_scale_dev", "grad_in_shift_dev"), result):
        if t is not None:
            setattr(a, field, t.data_ptr())
    nbytes = _lib.lib().amav_conv3x3_backward_workspace_bytes(ctypes.byref(a), int(wgrad_slices))
    if nbytes == 0:
        raise AmavError("amav_conv3x3_backward_workspace_bytes rejected the call: " + _lib.lib().amav_last_error().decode())
    workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    a.workspace_dev, a.workspace_bytes = workspace.data_ptr(), nbytes
    _call("amav_conv3x3_cells_backward", ctypes.byref(a))
    return result


class _Conv3x3Cells(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, in_scale, in_shift, residual, origin, upsample_input, extent, relu_out):
        x = _contig(x, "x")
        out = conv3x3_cells(x, conv3x3_prepare_weights(weight), weight.shape[0], bias, upsample_input=upsample_input,
                            in_scale=in_scale, in_shift=in_shift, origin=origin, extent=extent, relu_out=relu_out,
                            residual=residual)
        ctx.options = dict(upsample_input=upsample_input, extent=extent, relu_out=relu_out)
        ctx.origin = origin
        ctx.save_for_backward(x, weight, in_scale, in_shift, out if relu_out else None)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        x, weight, in_scale, in_shift, out = ctx.saved_tensors
        need = ctx.needs_input_grad
        grad_out = grad_out.float().contiguous()
        grads = [None] * 5
        if any(need[:5]):
            data = need[0] or need[3] or need[4]
            grads = conv3x3_cells_backward(
                grad_out, x, conv3x3_prepare_weights_transposed(weight) if data else None, out=out, in_scale=in_scale,
                in_shift=in_shift, origin=ctx.origin, want_x=need[0], want_weight=need[1], want_bias=need[2],
                want_prologue=need[3] or need[4], **ctx.options)
        gx, gw, gb, gs, gt = grads
        return (gx, gw, gb, gs if need[3] else None, gt if need[4] else None, grad_out if need[5] else None, None, None,
                None, None)


def conv3x3_cells_differentiable(x, weight, bias=None, *, upsample_input=False, in_scale=None, in_shift=None, origin=None,
                                 extent=0, relu_out=False, residual=None):
    """conv3x3_cells under autograd, over the plain fp32 weight [C_out,C_in,3,3]: the forward prepares the split weights
    and runs the HIP kernel, the backward is conv3x3_cells_backward (the same kernel on the transposed, flipped weights
    for the data gradient, a split-product MFMA GEMM for the weight gradient, fixed-order column sums for bias and
    prologue; deterministic).  Gradients flow to x, weight, bias, in_scale, in_shift and residual, to those that require
    them.  relu_out together with residual is refused: the backward gates on the saved output's sign."""
    if relu_out and residual is not None:
        raise AmavError("conv3x3_cells_differentiable: relu_out together with residual is not differentiable here "
                        "(the ReLU's gate is read from the saved output)")
    _need(x, "x"), _need(weight, "weight")
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3) or x.dim() != 4 or weight.shape[1] != x.shape[3]:
        raise AmavError(f"conv3x3_cells_differentiable: expected x [K,h,w,C_in] and weight [C_out,C_in,3,3], got "
                        f"{tuple(x.shape)}, {tuple(weight.shape)}")
    if weight.shape[0] % 32 or weight.shape[1] % 32 or weight.shape[0] == 0 or weight.shape[1] == 0:
        raise AmavError(f"conv3x3_cells_differentiable: channels must be multiples of 32, got {weight.shape[1]} -> {weight.shape[0]}")
    return _Conv3x3Cells.apply(x, weight, bias, in_scale, in_shift, residual, origin, bool(upsample_input), int(extent),
                               bool(relu_out))


def subm_pair_sum(products, pair_of, bias=None):
    """products [P,C_out], pair_of int32 [n,taps] (-1: no voxel) -> [n,C_out] = bias + sum over taps in tap order."""
    products, pair_of = _contig(products, "products"), _contig(pair_of, "pair_of", torch.int32)
    n, taps = pair_of.shape
    cout = products.shape[1]
    out = torch.empty(n, cout, device=products.device)
    _call("amav_subm_pair_sum", n, taps, cout, products.data_ptr(), pair_of.data_ptr(),
          None if bias is None else _shaped(bias, "bias", (cout,)).data_ptr(), out.data_ptr())
    return out


def patch_attention(qkv, order, patch_desc, heads, max_patch, scale=None):
    """qkv [n, 3*C] (q | k | v), order int64 [n], patch_desc int32 [patches,4] -> [n, C] (include/amav.h)."""
    qkv, order = _contig(qkv, "qkv"), _contig(order, "order", torch.int64)
    patch_desc = _contig(patch_desc, "patch_desc", torch.int32)
    n, C3 = qkv.shape
    C = C3 // 3
    D = C // heads
    if C3 != 3 * heads * D or order.shape != (n,) or patch_desc.dim() != 2 or patch_desc.shape[1] != 4:
        raise AmavError("patch_attention: shapes do not match")
    out = torch.empty(n, C, device=qkv.device)
    _call("amav_patch_attention", patch_desc.shape[0], int(max_patch), int(heads), D, qkv.data_ptr(), order.data_ptr(),
          patch_desc.data_ptr(), out.data_ptr(), float(scale if scale is not None else D ** -0.5))
    return out


def cluster_max(x, members, seg, scale, shift):
    """x [n,C], members int64 [n] (rows grouped by cluster), seg int64 [clusters+1] -> gelu(max * scale + shift) [clusters,C]."""
    x, members, seg = _contig(x, "x"), _contig(members, "members", torch.int64), _contig(seg, "seg", torch.int64)
    C = x.shape[1]
    clusters = seg.shape[0] - 1
    out = torch.empty(clusters, C, device=x.device)
    _call("amav_cluster_max", clusters, C, x.data_ptr(), members.data_ptr(), seg.data_ptr(),
          _shaped(scale, "scale", (C,)).data_ptr(), _shaped(shift, "shift", (C,)).data_ptr(), out.data_ptr())
    return out


def bn_gelu(x, scale, shift):
    """gelu(x * scale + shift) for x [rows, C] (BatchNorm in eval mode folded to scale / shift)."""
    x = _contig(x, "x")
    rows, C = x.shape
    out = torch.empty_like(x)
    _call("amav_bn_gelu", rows, C, x.data_ptr(), _shaped(scale, "scale", (C,)).data_ptr(),
          _shaped(shift, "shift", (C,)).data_ptr(), out.data_ptr())
    return out


def unpool_merge(x, scale, shift, up, cluster):
    """-> (skip = gelu(x * scale + shift), skip + up[cluster]) for x [n,C], up [m,C], cluster int64 [n]."""
    x, up, cluster = _contig(x, "x"), _contig(up, "up"), _contig(cluster, "cluster", torch.int64)
    n, C = x.shape
    if up.shape[1] != C or cluster.shape != (n,):
        raise AmavError("unpool_merge: shapes do not match")
    skip, total = torch.empty_like(x), torch.empty_like(x)
    _call("amav_unpool_merge", n, C, x.data_ptr(), _shaped(scale, "scale", (C,)).data_ptr(),
          _shaped(shift, "shift", (C,)).data_ptr(), up.data_ptr(), cluster.data_ptr(), skip.data_ptr(),
          total.data_ptr())
    return skip, total


def rows_norm(x, base, norm_b, norm_a=None):
    """-> (s = base + (LayerNorm_a(x) if norm_a else x), LayerNorm_b(s)) for [n, C] rows, C in {32,...,512};
    norm_a / norm_b are nn.LayerNorm modules (weight, bias, eps); the kernel takes one eps, so both must have the same."""
    if norm_a is not None and float(norm_a.eps) != float(norm_b.eps):
        raise AmavError(f"rows_norm: norm_a.eps {norm_a.eps} != norm_b.eps {norm_b.eps} (amav_rows_norm takes one eps)")
    x, base = _contig(x, "x"), _contig(base, "base")
    n, C = x.shape
    if base.shape != x.shape:
        raise AmavError("rows_norm: x and base must have the same shape")
    out_sum, out_norm = torch.empty_like(x), torch.empty_like(x)
    ptr = lambda t: _shaped(t.detach(), "norm parameter", (C,)).data_ptr()
    _call("amav_rows_norm", n, C, x.data_ptr(), base.data_ptr(), None if norm_a is None else ptr(norm_a.weight),
          None if norm_a is None else ptr(norm_a.bias), ptr(norm_b.weight), ptr(norm_b.bias), float(norm_b.eps),
          out_sum.data_ptr(), out_norm.data_ptr())
    return out_sum, out_norm


# ------------------------------------------------------------------------------------- point refiner: backward
SUBM_WGRAD_CHUNK = 128            # granularity (pairs) of a split-K slice of amav_subm_pair_wgrad
SUBM_WGRAD_WORKSPACE = 64 << 20   # the slices grow in multiples of the granularity to keep the partial matrices under this
SUBM_DGRAD_BUFFER = 256 << 20     # largest per-pair product buffer of the feature gradient; larger ones are swept by taps


def patch_attention_lse(qkv, order, patch_desc, heads, max_patch, scale=None):
    """patch_attention that also returns the row log-sum-exp [n, heads] (natural units); `out` is the same bit for bit."""
    qkv, order = _contig(qkv, "qkv"), _contig(order, "order", torch.int64)
    patch_desc = _contig(patch_desc, "patch_desc", torch.int32)
    n, C3 = qkv.shape
    C = C3 // 3
    D = C // heads
    if C3 != 3 * heads * D or order.shape != (n,) or patch_desc.dim() != 2 or patch_desc.shape[1] != 4:
        raise AmavError("patch_attention_lse: shapes do not match")
    out = torch.empty(n, C, device=qkv.device)
    lse = torch.empty(n, heads, device=qkv.device)
    _call("amav_patch_attention_lse", patch_desc.shape[0], int(max_patch), int(heads), D, qkv.data_ptr(),
          order.data_ptr(), patch_desc.data_ptr(), out.data_ptr(), lse.data_ptr(),
          float(scale if scale is not None else D ** -0.5))
    return out, lse


def patch_attention_backward(qkv, order, patch_desc, out, lse, grad_out, heads, max_patch, scale=None):
    """amav_patch_attention_backward: d qkv [n, 3*C] (dq | dk | dv, point order) from the forward's out and lse
    (patch_attention_lse) and grad_out [n, C]."""
    qkv, order = _contig(qkv, "qkv"), _contig(order, "order", torch.int64)
    patch_desc = _contig(patch_desc, "patch_desc", torch.int32)
    n, C3 = qkv.shape
    C = C3 // 3
    D = C // heads
    if C3 != 3 * heads * D or order.shape != (n,) or patch_desc.dim() != 2 or patch_desc.shape[1] != 4:
        raise AmavError("patch_attention_backward: shapes do not match")
    out, grad_out, lse = _shaped(out, "out", (n, C)), _shaped(grad_out, "grad_out", (n, C)), _shaped(lse, "lse", (n, heads))
    ws = _scratch("amav_patch_attention_backward_workspace_bytes", qkv.device, n, int(heads), D,
                  rejected=f"n={n} heads={heads} D={D}")
    grad_qkv = torch.empty_like(qkv)
    _call("amav_patch_attention_backward", n, patch_desc.shape[0], int(max_patch), int(heads), D, qkv.data_ptr(),
          order.data_ptr(), patch_desc.data_ptr(), out.data_ptr(), lse.data_ptr(), grad_out.data_ptr(),
          grad_qkv.data_ptr(), float(scale if scale is not None else D ** -0.5), ws.data_ptr(), ws.numel())
    return grad_qkv


class _PatchAttention(torch.autograd.Function):
    """patch_attention_lse with amav_patch_attention_backward as the backward; qkv, the output and the lse are kept."""

    @staticmethod
    def forward(ctx, qkv, order, patch_desc, heads, max_patch, scale):
        qkv = _contig(qkv, "qkv")
        out, lse = patch_attention_lse(qkv, order, patch_desc, heads, max_patch, scale)
        ctx.settings = (heads, max_patch, scale)
        ctx.save_for_backward(qkv, order, patch_desc, out, lse)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        qkv, order, patch_desc, out, lse = ctx.saved_tensors
        heads, max_patch, scale = ctx.settings
        grad = patch_attention_backward(qkv, order, patch_desc, out, lse, grad_out.float().contiguous(), heads, max_patch,
                                        scale)
        return grad, None, None, None, None, None


def patch_attention_differentiable(qkv, order, patch_desc, heads, max_patch, scale=None):
    """patch_attention as a torch.autograd.Function: the same values bit for bit, differentiable in qkv."""
    return _PatchAttention.apply(qkv, order, patch_desc, int(heads), int(max_patch), scale)


def subm_pair_sum_csr(products, src_start, src_pairs, pair_lo=0, out=None):
    """out [n, C] (+)= per source row, the sum of products[p - pair_lo] over the row's pairs p (ascending) that lie in
    [pair_lo, pair_lo + len(products)); src_start int32 [n+1], src_pairs int32 [P].  out given: added to it."""
    products = _contig(products, "products")
    src_start, src_pairs = _contig(src_start, "src_start", torch.int32), _contig(src_pairs, "src_pairs", torch.int32)
    n, C = src_start.shape[0] - 1, products.shape[1]
    accumulate = out is not None
    if out is None:
        out = torch.empty(n, C, device=products.device)
    _shaped(out, "out", (n, C))
    _call("amav_subm_pair_sum_csr", n, C, products.data_ptr(), int(pair_lo), products.shape[0], src_start.data_ptr(),
          src_pairs.data_ptr(), int(accumulate), out.data_ptr())
    return out


def subm_wgrad_slices(tap_counts, cin, cout):
    """Host-side slice table of subm_pair_wgrad for the taps' pair counts (numpy int64 [taps]) -> (chunk, slice_start
    numpy int32 [taps+1]): slices of SUBM_WGRAD_CHUNK pairs, doubled until the partial matrices fit the workspace bound."""
    import numpy as np

    chunk = SUBM_WGRAD_CHUNK
    while True:
        per_tap = (tap_counts + chunk - 1) // chunk
        if int(per_tap.sum()) * cin * cout * 4 <= SUBM_WGRAD_WORKSPACE or int(per_tap.max()) <= 1:
            break
        chunk *= 2
    return chunk, np.concatenate([[0], np.cumsum(per_tap)]).astype(np.int32)


def subm_pair_wgrad(feat, grad_out, pair_src, pair_dst, tap_start, slice_start, slices, chunk):
    """-> [taps, C_in, C_out]: per tap, the sum over its pairs of feat[pair_src[p]]^T (x) grad_out[pair_dst[p]]
    (include/amav.h); slice_start int32 [taps+1] / slices / chunk from subm_wgrad_slices."""
    feat, grad_out = _contig(feat, "feat"), _contig(grad_out, "grad_out")
    pair_src, pair_dst = _contig(pair_src, "pair_src", torch.int32), _contig(pair_dst, "pair_dst", torch.int32)
    tap_start, slice_start = _contig(tap_start, "tap_start", torch.int32), _contig(slice_start, "slice_start", torch.int32)
    taps, cin, cout = tap_start.shape[0] - 1, feat.shape[1], grad_out.shape[1]
    if pair_dst.shape != pair_src.shape or slice_start.shape != tap_start.shape:
        raise AmavError("subm_pair_wgrad: shapes do not match")
    ws = _scratch("amav_subm_pair_wgrad_workspace_bytes", feat.device, int(slices), cin, cout,
                  rejected=f"slices={slices} C_in={cin} C_out={cout}")
    out = torch.empty(taps, cin, cout, device=feat.device)
    _call("amav_subm_pair_wgrad", pair_src.shape[0], int(slices), int(chunk), taps, cin, cout, feat.data_ptr(),
          grad_out.data_ptr(), pair_src.data_ptr(), pair_dst.data_ptr(), tap_start.data_ptr(), slice_start.data_ptr(),
          out.data_ptr(), ws.data_ptr(), ws.numel())
    return out


def subm_feat_grad(grad_out, weights_t, pairs, max_buffer_bytes=None):
    """d feat [n, C_in] of a submanifold convolution: the fp32 gather-GEMM with pair_dst as the gather index and the
    transposed weights [taps, C_out, C_in] (C_in a multiple of 32), then the ordered sum by source row.  The per-pair
    buffer is bounded by max_buffer_bytes (default SUBM_DGRAD_BUFFER): larger ones are swept over runs of taps, which
    adds every row's pairs in the same (ascending) order."""
    grad_out, weights_t = _contig(grad_out, "grad_out"), _contig(weights_t, "weights_t")
    taps, cout, cin = weights_t.shape
    limit = SUBM_DGRAD_BUFFER if max_buffer_bytes is None else int(max_buffer_bytes)
    tap_start = pairs.tap_start_host.astype("int64")
    if pairs.count * cin * 4 <= limit:
        products = subm_pair_gemm(grad_out, pairs.pair_dst, pairs.tap_start, pairs.tile_start, pairs.tiles, weights_t)
        return subm_pair_sum_csr(products, pairs.src_start, pairs.src_pairs)
    out = torch.zeros(grad_out.shape[0], cin, device=grad_out.device)
    tile_start = pairs.tile_start_host
    t0 = 0
    while t0 < taps:
        t1 = t0 + 1
        while t1 < taps and (tap_start[t1 + 1] - tap_start[t0]) * cin * 4 <= limit:
            t1 += 1
        lo, count = int(tap_start[t0]), int(tap_start[t1] - tap_start[t0])
        if count:
            products = torch.empty(count, cin, device=grad_out.device)
            rebased = (pairs.tile_start[t0:t1 + 1] - int(tile_start[t0])).contiguous()
            # the kernel addresses products by the absolute pair index: hand it the address pair `lo` would have
            _call("amav_subm_pair_gemm", count, int(tile_start[t1] - tile_start[t0]), t1 - t0, cout, cin,
                  grad_out.data_ptr(), pairs.pair_dst.data_ptr(), pairs.tap_start.data_ptr() + 4 * t0,
                  rebased.data_ptr(), weights_t.data_ptr() + 4 * t0 * cout * cin, products.data_ptr() - 4 * lo * cin)
            subm_pair_sum_csr(products, pairs.src_start, pairs.src_pairs, pair_lo=lo, out=out)
        t0 = t1
    return out


class _SubMConv(torch.autograd.Function):
    """The inference kernels of a SubMConv3d forward (conv.run_kernels) with the HIP backward of DESIGN.md section 4.12."""

    @staticmethod
    def forward(ctx, feat, weight, bias, conv, pairs):
        feat = _contig(feat, "feat")
        ctx.conv, ctx.pairs = conv, pairs
        ctx.save_for_backward(feat, weight)
        return conv.run_kernels(feat, pairs)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        feat, weight = ctx.saved_tensors
        conv, pairs = ctx.conv, ctx.pairs
        g = grad_out.float().contiguous()
        cout, cin, k = conv.out_channels, conv.in_channels, conv.kernel_size
        pad = -cin % 32
        grad_feat = grad_weight = grad_bias = None
        if ctx.needs_input_grad[0]:
            wt = weight.detach().reshape(cout, -1, cin).permute(1, 0, 2)  # [taps, C_out, C_in]
            grad_feat = subm_feat_grad(g, torch.nn.functional.pad(wt, (0, pad)) if pad else wt, pairs)
            if pad:
                grad_feat = grad_feat[:, :cin]
        if ctx.needs_input_grad[1]:
            chunk, slice_start, slices = pairs.wgrad_slices(cin + pad, cout)
            gw = subm_pair_wgrad(torch.nn.functional.pad(feat, (0, pad)) if pad else feat, g, pairs.pair_src,
                                 pairs.pair_dst, pairs.tap_start, slice_start, slices, chunk)
            grad_weight = gw[:, :cin].permute(2, 0, 1).reshape(cout, k, k, k, cin)
        if ctx.needs_input_grad[2]:
            grad_bias = g.sum(0)
        return grad_feat, grad_weight, grad_bias, None, None


def subm_conv_differentiable(feat, conv, pairs):
    """SubMConv3d (point_transformer.py) on the pairs of a level as a torch.autograd.Function: the values of the inference
    forward bit for bit (split products, or fp32 under AMAV_SUBM=f32), differentiable in feat, conv.weight and conv.bias.
    pairs: Level.pairs(k) (its backward tables are built on first use)."""
    return _SubMConv.apply(feat, conv.weight, conv.bias, conv, pairs)


def cluster_max_backward(x, members, seg, scale, shift, grad_out):
    """amav_cluster_max_backward -> (grad_x [n,C], grad_z [clusters,C], x_max [clusters,C])."""
    x, members, seg = _contig(x, "x"), _contig(members, "members", torch.int64), _contig(seg, "seg", torch.int64)
    C = x.shape[1]
    clusters = seg.shape[0] - 1
    grad_out = _shaped(grad_out, "grad_out", (clusters, C))
    grad_x = torch.empty_like(x)
    grad_z, x_max = torch.empty_like(grad_out), torch.empty_like(grad_out)
    _call("amav_cluster_max_backward", clusters, C, x.data_ptr(), members.data_ptr(), seg.data_ptr(),
          _shaped(scale, "scale", (C,)).data_ptr(), _shaped(shift, "shift", (C,)).data_ptr(), grad_out.data_ptr(),
          grad_x.data_ptr(), grad_z.data_ptr(), x_max.data_ptr())
    return grad_x, grad_z, x_max


def cluster_sum(x, members, seg):
    """x [n,C], members int64 [n], seg int64 [clusters+1] -> [clusters,C]: the segment sums, added in segment order."""
    x, members, seg = _contig(x, "x"), _contig(members, "members", torch.int64), _contig(seg, "seg", torch.int64)
    C = x.shape[1]
    clusters = seg.shape[0] - 1
    out = torch.empty(clusters, C, device=x.device)
    _call("amav_cluster_sum", clusters, C, x.data_ptr(), members.data_ptr(), seg.data_ptr(), out.data_ptr())
    return out


class _ClusterMax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, members, seg, scale, shift):
        x, scale, shift = _contig(x, "x"), _contig(scale, "scale"), _contig(shift, "shift")
        ctx.save_for_backward(x, members, seg, scale, shift)
        return cluster_max(x, members, seg, scale, shift)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        x, members, seg, scale, shift = ctx.saved_tensors
        grad_x, grad_z, x_max = cluster_max_backward(x, members, seg, scale, shift, grad_out.float().contiguous())
        return grad_x, None, None, (grad_z * x_max).sum(0), grad_z.sum(0)


def cluster_max_differentiable(x, members, seg, scale, shift):
    """cluster_max as a torch.autograd.Function: the same values bit for bit, differentiable in x, scale and shift (the
    whole gradient of a maximum to the first member, in segment order, that attains it)."""
    return _ClusterMax.apply(x, members, seg, scale, shift)


class _ClusterGather(torch.autograd.Function):
    @staticmethod
    def forward(ctx, up, cluster, members, seg):
        ctx.save_for_backward(members, seg)
        return up[cluster]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        members, seg = ctx.saved_tensors
        return cluster_sum(grad_out.float().contiguous(), members, seg), None, None, None


def cluster_gather_differentiable(up, cluster, members, seg):
    """up[cluster] whose backward is cluster_sum over the clusters' member lists (members / seg of Level.pool()) instead
    of an atomic index_add."""
    return _ClusterGather.apply(up, cluster, members, seg)


# ------------------------------------------------- point refiner: train-mode BatchNorm
BN_CHUNK_ROWS = 64  # rows per first-stage partial of bn_batch_stats and of the train backward's column sums


def refiner_bn_library():
    """AMAV_REFINER_BN=library (read per call, like AMAV_CROSS_ATTN): F.batch_norm(training=True) + F.gelu under torch
    autograd instead of the HIP statistics / backward kernels -- the comparison path of tools/bench_refiner_backward.py."""
    return os.environ.get("AMAV_REFINER_BN", "hip") == "library"


def bn_batch_stats(x):
    """x [rows, C] (rows >= 2, C a multiple of 4) -> (mean [C], var [C]): the columns' mean and biased variance
    (amav_bn_batch_stats: chunks of BN_CHUNK_ROWS rows about their first row, merged in a fixed order; bit-identical
    between calls)."""
    x = _contig(x, "x")
    if x.dim() != 2:
        raise AmavError(f"bn_batch_stats: expected [rows, C], got {tuple(x.shape)}")
    rows, C = x.shape
    ws = _scratch("amav_bn_batch_stats_workspace_bytes", x.device, rows, C,
                  rejected=f"rows={rows} C={C} (batch statistics need at least 2 rows and C a multiple of 4)")
    mean, var = torch.empty(C, device=x.device), torch.empty(C, device=x.device)
    _call("amav_bn_batch_stats", rows, C, x.data_ptr(), mean.data_ptr(), var.data_ptr(), ws.data_ptr(), ws.numel())
    return mean, var


def bn_gelu_train_backward(x, mean, rstd, weight, bias, grad_out):
    """amav_bn_gelu_train_backward: the backward of gelu(((x - mean) * rstd) * weight + bias) through the batch statistics
    -> (grad_x [rows, C], grad_weight [C], grad_bias [C])."""
    x = _contig(x, "x")
    rows, C = x.shape
    grad_out = _shaped(grad_out, "grad_out", (rows, C))
    ws = _scratch("amav_bn_batch_stats_workspace_bytes", x.device, rows, C,
                  rejected=f"rows={rows} C={C} (batch statistics need at least 2 rows and C a multiple of 4)")
    grad_x = torch.empty_like(x)
    grad_weight, grad_bias = torch.empty(C, device=x.device), torch.empty(C, device=x.device)
    vec = lambda t, name: _shaped(t, name, (C,)).data_ptr()
    _call("amav_bn_gelu_train_backward", rows, C, x.data_ptr(), vec(mean, "mean"), vec(rstd, "rstd"), vec(weight, "weight"),
          vec(bias, "bias"), grad_out.data_ptr(), grad_x.data_ptr(), grad_weight.data_ptr(), grad_bias.data_ptr(),
          ws.data_ptr(), ws.numel())
    return grad_x, grad_weight, grad_bias


def cluster_max_raw(x, members, seg):
    """x [n,C], members int64 [n] (rows grouped by cluster), seg int64 [clusters+1] -> the segment maxima [clusters,C]."""
    x, members, seg = _contig(x, "x"), _contig(members, "members", torch.int64), _contig(seg, "seg", torch.int64)
    C = x.shape[1]
    clusters = seg.shape[0] - 1
    out = torch.empty(clusters, C, device=x.device)
    _call("amav_cluster_max_raw", clusters, C, x.data_ptr(), members.data_ptr(), seg.data_ptr(), out.data_ptr())
    return out


def cluster_max_route(x, members, seg, grad_max):
    """grad_max [clusters,C] -> grad_x [n,C]: each maximum's gradient on the first member, in segment order, that attains
    it, +0 on the segment's other rows (rows that `members` does not list keep zeros)."""
    x, members, seg = _contig(x, "x"), _contig(members, "members", torch.int64), _contig(seg, "seg", torch.int64)
    C = x.shape[1]
    clusters = seg.shape[0] - 1
    grad_max = _shaped(grad_max, "grad_max", (clusters, C))
    grad_x = torch.empty_like(x) if members.shape[0] == x.shape[0] else torch.zeros_like(x)
    _call("amav_cluster_max_route", clusters, C, x.data_ptr(), members.data_ptr(), seg.data_ptr(), grad_max.data_ptr(),
          grad_x.data_ptr())
    return grad_x


def bn_train_fold(x, weight, bias, eps):
    """Train-mode BatchNorm of the rows x [rows, C] as the (scale, shift) that bn_gelu / unpool_merge take
    -> (scale, shift, mean, var_biased, rstd); nothing here is differentiable."""
    mean, var = bn_batch_stats(x)
    rstd = torch.rsqrt(var + eps)
    scale = weight.detach() * rstd
    return scale, bias.detach() - mean * scale, mean, var, rstd


class _BnGeluTrain(torch.autograd.Function):
    """gelu(BatchNorm(x)) with the batch's own statistics: bn_batch_stats + bn_gelu forward, amav_bn_gelu_train_backward
    backward.  Saves x, mean, rstd and the affine parameters (the normalised rows are recomputed)."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        x = _contig(x, "x")
        weight, bias = _contig(weight.detach(), "weight"), _contig(bias.detach(), "bias")
        scale, shift, mean, var, rstd = bn_train_fold(x, weight, bias, eps)
        ctx.save_for_backward(x, mean, rstd, weight, bias)
        ctx.mark_non_differentiable(mean, var)
        return bn_gelu(x, scale, shift), mean, var

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out, _grad_mean, _grad_var):
        x, mean, rstd, weight, bias = ctx.saved_tensors
        grad_x, grad_weight, grad_bias = bn_gelu_train_backward(x, mean, rstd, weight, bias, grad_out.float().contiguous())
        return grad_x, grad_weight, grad_bias, None


def bn_gelu_train_differentiable(x, weight, bias, eps):
    """-> (gelu(BN_batch(x)), mean [C], var_biased [C]) for x [rows, C], rows >= 2: BatchNorm1d in training mode followed by
    GELU, differentiable in x, weight and bias THROUGH the batch statistics; the two statistics outputs are not
    differentiable (they feed the running buffers).  AMAV_REFINER_BN=library: the same function by F.batch_norm + F.gelu
    under torch autograd."""
    if refiner_bn_library():
        F = torch.nn.functional
        with torch.no_grad():
            var, mean = torch.var_mean(x, 0, unbiased=False)
        return F.gelu(F.batch_norm(x, None, None, weight, bias, True, 0.0, eps)), mean, var
    return _BnGeluTrain.apply(x, weight, bias, float(eps))


class _ClusterMaxRaw(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, members, seg):
        x = _contig(x, "x")
        ctx.save_for_backward(x, members, seg)
        return cluster_max_raw(x, members, seg)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        x, members, seg = ctx.saved_tensors
        return cluster_max_route(x, members, seg, grad_out.float().contiguous()), None, None


def cluster_max_bn_train_differentiable(x, members, seg, weight, bias, eps):
    """-> (gelu(BN_batch(segment maxima of x)), mean, var_biased): SerializedPooling's max + BatchNorm + GELU in training
    mode -- raw maxima, their batch statistics, bn_gelu; the backward is the train backward followed by the routing of each
    maximum's gradient to the first member that attains it.  Differentiable in x, weight and bias."""
    return bn_gelu_train_differentiable(_ClusterMaxRaw.apply(x, members, seg), weight, bias, eps)


# ------------------------------------------------------------------------------------------ optimizer (optimizer.hip)
OPTIM_CHUNK = 16384  # elements per chunk = per work-group visit: 64 iterations of 256 lanes x 16 B in each array
OPTIM_MAX_GROUPS = _lib.DEFINES["AMAV_OPTIM_MAX_GROUPS"]


def optimizer_tables(numels, groups, chunk=OPTIM_CHUNK):
    """The two tables of amav_grad_norm_clip / amav_adam_step as host arrays (ctypes arrays of the header's structs):
    tensors[i] = (numel numels[i], group groups[i], addresses still 0) and the chunks (tensor, start) that cut every
    tensor into pieces of at most `chunk` elements, ascending by (tensor, start); a tensor of 0 elements gets no chunk.
    Pure Python: nothing here touches a device."""
    if len(numels) != len(groups):
        raise ValueError(f"optimizer_tables: {len(numels)} element counts for {len(groups)} group indices")
    if int(chunk) <= 0:
        raise ValueError(f"optimizer_tables: chunk={chunk}, expected a positive element count")
    chunk = int(chunk)
    tensors = (OptimTensor * len(numels))()
    starts = []
    for i, (n, g) in enumerate(zip(numels, groups)):
        if n < 0 or g < 0:
            raise ValueError(f"optimizer_tables: tensor {i} has numel={n} group={g}")
        tensors[i].numel, tensors[i].group = int(n), int(g)
        starts += [(i, s) for s in range(0, int(n), chunk)]
    chunks = (OptimChunk * len(starts))()
    for c, (i, s) in zip(chunks, starts):
        c.tensor, c.start = i, s
    return tensors, chunks


def optimizer_group(lr, betas, eps, weight_decay, step):
    """amav_optim_group of torch.optim.Adam's hyper-parameters at step count `step` (>= 1): the bias corrections are
    formed in double, as torch's single-tensor path forms them, and rounded once."""
    beta1, beta2 = betas
    return OptimGroup(lr / (1.0 - beta1 ** step), 1.0 / (1.0 - beta2 ** step) ** 0.5, beta1, beta2, 1.0 - beta1, 1.0 - beta2,
                      eps, weight_decay)


def optimizer_table_to_device(table, device):
    """A host table (ctypes array) -> uint8 device tensor, through a pinned staging copy that the stream reads later:
    the host does not wait (torch's pinned allocator keeps the staging block alive until the copy has run)."""
    nbytes = ctypes.sizeof(table)
    if nbytes == 0:
        return torch.empty(0, dtype=torch.uint8, device=device)
    host = torch.frombuffer(table, dtype=torch.uint8).pin_memory()
    return torch.empty(nbytes, dtype=torch.uint8, device=device).copy_(host, non_blocking=True)


def _optimizer_table(t, name, struct, count):
    t = _contig(t, name, torch.uint8)
    if t.numel() < count * ctypes.sizeof(struct):
        raise AmavError(f"{name}: {t.numel()} bytes hold fewer than {count} entries of {ctypes.sizeof(struct)} bytes")
    return t.data_ptr()


def grad_norm_clip(tensors_dev, num_tensors, chunks_dev, num_chunks, chunk, max_norm, partial=None, norm=None):
    """amav_grad_norm_clip over device tables (uint8 tensors, optimizer_table_to_device) -> norm, fp32 [2] on the device:
    norm[0] = the L2 norm of all gradients, norm[1] = min(1, max_norm / (norm[0] + 1e-6)).  No host synchronisation.
    `partial` (fp64, >= num_chunks) and `norm` are reused when given."""
    tp = _optimizer_table(tensors_dev, "tensors_dev", OptimTensor, num_tensors)
    cp = _optimizer_table(chunks_dev, "chunks_dev", OptimChunk, num_chunks)
    if partial is None:
        partial = torch.empty(max(num_chunks, 1), dtype=torch.float64, device=tensors_dev.device)
    elif _need(partial, "partial", torch.float64).numel() < num_chunks or not partial.is_contiguous():
        raise AmavError(f"partial: {partial.numel()} contiguous fp64 values needed for {num_chunks} chunks")
    norm = torch.empty(2, device=tensors_dev.device) if norm is None else _shaped(norm, "norm", (2,))
    _call("amav_grad_norm_clip", tp, num_tensors, cp, num_chunks, chunk, float(max_norm), partial.data_ptr(),
          norm.data_ptr())
    return norm


def adam_step(tensors_dev, num_tensors, chunks_dev, num_chunks, chunk, groups, coef=None, zero_grad=False):
    """amav_adam_step over device tables: one fused pass of torch.optim.Adam's update on every chunk.  groups: a sequence
    of OptimGroup (optimizer_group), indexed by the tensors' group field; coef: None (1) or a one-element fp32 device
    tensor the gradients are multiplied by on the way in (grad_norm_clip(...)[1:]); zero_grad: also store zeros to the
    gradients.  The caller bumps the version counters of what was written."""
    tp = _optimizer_table(tensors_dev, "tensors_dev", OptimTensor, num_tensors)
    cp = _optimizer_table(chunks_dev, "chunks_dev", OptimChunk, num_chunks)
    if len(groups) > OPTIM_MAX_GROUPS:
        raise AmavError(f"adam_step: {len(groups)} groups, at most {OPTIM_MAX_GROUPS}")
    table = (OptimGroup * len(groups))(*groups)
    coef_ptr = None if coef is None else _need(coef, "coef").data_ptr()
    _call("amav_adam_step", tp, num_tensors, cp, num_chunks, chunk, table, len(groups), coef_ptr, int(bool(zero_grad)))


# ------------------------------------------------------------------- the data-parallel step's bucket (optimizer.hip)
def bucket_offsets(numels, align=64):
    """Where each tensor starts in the bucket of the data-parallel step -> (offsets, total), in elements: an offset is
    the previous tensor's end rounded up to a multiple of `align`, and so is `total`.  align=64 elements = 256 bytes, the
    allocator's own granule: a tensor's first element is then 16-byte aligned in the bucket as it is in an allocation of
    its own, so whether a chunk of the norm / Adam kernels takes their 16-byte path depends on the parameter alone, and a
    step that reads its gradients from the bucket adds in the order of a step that reads them from ordinary allocations.
    Pure Python: nothing here touches a device."""
    align = int(align)
    if align < 4:
        raise ValueError(f"bucket_offsets: align={align}, expected at least 4 elements (16 bytes)")
    offsets, end = [], 0
    for i, n in enumerate(numels):
        if n < 0:
            raise ValueError(f"bucket_offsets: tensor {i} has numel={n}")
        offsets.append(end)
        end = -(-(end + int(n)) // align) * align
    return offsets, end


def grads_pack(tensors_dev, num_tensors, chunks_dev, num_chunks, chunk, offsets, bucket, scale=1.0, zero_source=False):
    """amav_grads_pack over device tables: bucket[offsets[t] + i] = scale * grad_t[i] (one rounding), zeros for a tensor
    whose grad address is NULL; zero_source: the gradients are zeroed in the same pass.  offsets: int64 device tensor
    [num_tensors] (bucket_offsets); bucket: contiguous fp32, only the tensors' own ranges are written.  No host
    synchronisation.  The caller bumps the version counters of gradients it had zeroed."""
    tp = _optimizer_table(tensors_dev, "tensors_dev", OptimTensor, num_tensors)
    cp = _optimizer_table(chunks_dev, "chunks_dev", OptimChunk, num_chunks)
    if _need(offsets, "offsets", torch.int64).numel() < num_tensors or not offsets.is_contiguous():
        raise AmavError(f"offsets: {offsets.numel()} contiguous int64 values needed for {num_tensors} tensors")
    if not _need(bucket, "bucket").is_contiguous():
        raise AmavError("bucket: expected a contiguous fp32 tensor")
    _call("amav_grads_pack", tp, num_tensors, cp, num_chunks, chunk, offsets.data_ptr(), bucket.data_ptr(), bucket.numel(),
          float(scale), int(bool(zero_source)))
    return bucket


FINGERPRINT_OF = {"param": 0, "grad": 1, "exp_avg": 2, "exp_avg_sq": 3}


def tensors_fingerprint(tensors_dev, num_tensors, chunks_dev, num_chunks, chunk, which, partial=None, out=None):
    """amav_tensors_fingerprint over device tables -> out, a 0-dim int64 device tensor holding the uint64 sum, modulo
    2^64, of the 32-bit patterns of every element of the array `which` ("param" | "grad" | "exp_avg" | "exp_avg_sq", or
    0..3).  No host synchronisation.  `partial` (int64, >= num_chunks) and `out` are reused when given.  Equal values do
    not prove equal arrays (two swapped elements give the same sum); different values prove different arrays."""
    tp = _optimizer_table(tensors_dev, "tensors_dev", OptimTensor, num_tensors)
    cp = _optimizer_table(chunks_dev, "chunks_dev", OptimChunk, num_chunks)
    which = FINGERPRINT_OF.get(which, which)
    if partial is None:
        partial = torch.empty(max(num_chunks, 1), dtype=torch.int64, device=tensors_dev.device)
    elif _need(partial, "partial", torch.int64).numel() < num_chunks or not partial.is_contiguous():
        raise AmavError(f"partial: {partial.numel()} contiguous int64 values needed for {num_chunks} chunks")
    if out is None:
        out = torch.empty((), dtype=torch.int64, device=tensors_dev.device)
    elif _need(out, "out", torch.int64).numel() != 1:
        raise AmavError(f"out: expected one int64 value, got {tuple(out.shape)}")
    _call("amav_tensors_fingerprint", tp, num_tensors, cp, num_chunks, chunk, int(which), partial.data_ptr(), out.data_ptr())
    return out


# ----------------------------------------------------------------------------------------------------- mesh overlay
MeshOverlayArgs = _lib.STRUCTS["amav_mesh_overlay_args"]
MESH_SMALL_BOX = _lib.DEFINES["AMAV_MESH_SMALL_BOX"]
MESH_DIFFUSE = 0.96  # 1 - F0 of a dielectric at l = v: pyrender's metallic-roughness diffuse weight at metallic = 0


def mesh_overlay(vertices, faces, K, E, height, width, frames=None, transl=None, base_color=(0.8, 0.8, 0.8),
                 light_intensity=5.0, znear=0.05, cull_backfaces=True, background=(1, 1, 1), want_depth=False,
                 want_face_index=False, want_screen=False, workspace=None, want_shade=False, small_box=None):
    """Flat-shaded, z-buffered triangle mesh over a batch of frames (include/amav.h, amav_mesh_overlay; DESIGN.md
    section 4.21): vertices [F,V,3] world, faces [T,3] int32 (int64 is converted), K [F,3,3], E [F,4,4] world-to-camera,
    frames fp32 [F,H,W,3|4] or None (composite over `background`), transl [F,3] or None.  Returns a dict: rgb
    [F,H,W,3]; depth [F,H,W] (0 where no face covers the pixel), face_index int32 [F,H,W] (-1 there), screen int32
    [F,V,2] (the vertices snapped to 1/256 px) and shade [F,T,3] when asked for, else None; status int32 [F,2]: the faces
    dropped at the near plane and at the guard band, left on the device.  The shade is min(1, k max(0, n . l)) with
    k = 0.96 base_color light_intensity / pi and the camera's headlight.  workspace: a uint8 tensor of at least
    amav_mesh_overlay_workspace_bytes, reused when given.  small_box: pixel centres a face's own thread may visit
    (None: AMAV_MESH_SMALL_BOX; 0 sends every face to the wave-per-face tier; the result does not depend on it)."""
    vertices = _contig(vertices, "vertices")
    if vertices.dim() != 3 or vertices.shape[2] != 3:
        raise AmavError(f"mesh_overlay: vertices {tuple(vertices.shape)}, expected [F,V,3]")
    F, V, _ = vertices.shape
    if not isinstance(faces, torch.Tensor) or not faces.is_cuda:
        raise AmavError("mesh_overlay: faces must be a tensor on the HIP device (this package only runs on an MI355X)")
    if faces.dtype == torch.int64:
        faces = faces.to(torch.int32)
    faces = _contig(faces, "faces", torch.int32)
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise AmavError(f"mesh_overlay: faces {tuple(faces.shape)}, expected [T,3]")
    T, H, W = faces.shape[0], int(height), int(width)
    K, E = _contig(K.reshape(-1, 3, 3), "K"), _contig(E.reshape(-1, 4, 4), "E")
    if K.shape[0] != F or E.shape[0] != F:
        raise AmavError(f"mesh_overlay: {F} frames of vertices, {K.shape[0]} intrinsics, {E.shape[0]} extrinsics")
    dev = vertices.device
    a = MeshOverlayArgs()
    a.num_frames, a.num_verts, a.num_faces, a.height, a.width = F, V, T, H, W
    a.cull_backfaces, a.small_box = int(bool(cull_backfaces)), -1 if small_box is None else int(small_box)
    a.vertices, a.faces, a.K, a.E = vertices.data_ptr(), faces.data_ptr(), K.data_ptr(), E.data_ptr()
    if transl is not None:
        transl = _contig(transl.reshape(-1, 3), "transl")
        if transl.shape[0] != F:
            raise AmavError(f"mesh_overlay: transl {tuple(transl.shape)}, expected [{F},3]")
        a.transl = transl.data_ptr()
    if frames is not None:
        frames = _contig(frames, "frames")
        if frames.dim() != 4 or tuple(frames.shape[:3]) != (F, H, W) or frames.shape[3] not in (3, 4):
            raise AmavError(f"mesh_overlay: frames {tuple(frames.shape)}, expected [{F},{H},{W},3|4]")
        a.frames, a.frame_channels = frames.data_ptr(), frames.shape[3]
    for c in range(3):
        a.background[c] = float(background[c])
        a.shade_k[c] = MESH_DIFFUSE * float(base_color[c]) * float(light_intensity) / math.pi
    a.znear = float(znear)
    if workspace is None:
        workspace = _scratch("amav_mesh_overlay_workspace_bytes", dev, F, V, T, H, W,
                             rejected=f"F={F} V={V} T={T} H={H} W={W}")
    else:
        workspace = _contig(workspace, "workspace", torch.uint8)
    out = {"rgb": torch.empty(F, H, W, 3, device=dev),
           "depth": torch.empty(F, H, W, device=dev) if want_depth else None,
           "face_index": torch.empty(F, H, W, dtype=torch.int32, device=dev) if want_face_index else None,
           "screen": torch.empty(F, V, 2, dtype=torch.int32, device=dev) if want_screen else None,
           "shade": torch.empty(F, T, 3, device=dev) if want_shade else None,
           "status": torch.empty(F, 2, dtype=torch.int32, device=dev)}
    a.out_rgb, a.out_status = out["rgb"].data_ptr(), out["status"].data_ptr()
    for field, key in (("out_depth", "depth"), ("out_face_index", "face_index"), ("out_screen", "screen"),
                       ("out_shade", "shade")):
        if out[key] is not None:
            setattr(a, field, out[key].data_ptr())
    a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel()
    _call("amav_mesh_overlay", ctypes.byref(a))
    return out
