"""Renderer and the splat entry points, on the HIP kernels (mirror of src/models/renderer.py).

Kept verbatim from the reference: class / function names, argument order and meaning, the `gaussians` dict keys
(`xyz, scale, rot, opacity, color, shs`, renderer.py:337-344), return shapes (`[B,T,H,W,3]` fp32 in [0,1], white
background by default) and the parameter names of `gaussian_decoder.*` / `smpl_decoder.*` (checkpoint keys).

Changed on purpose (MI355X-first):
  * all frames of a call go through ONE batched launch per stage (the reference loops over frames in Python with
    >= 6 host syncs per frame, renderer.py:475-477,501-510);
  * triplane sampling + the five heads + construct_gaussians are one fused decode (csrc/triplane.hip) that never
    materialises the [N, 3C] feature tensor; the Gaussians live in one packed [F,N,16] buffer and the dict entries
    are views into it;
  * the vertex subset is drawn once (seeded) instead of on every forward (renderer.py:287), and no stage prints or
    synchronises (renderer.py:76-82);
  * `no_point_refiner=False` runs the PTv3 point refiner (point_transformer.py, deterministic semantics of DESIGN.md
    section 4.5) between two triplane samplings, as renderer.py:136-158 does; `upsample_triplane=True` runs the
    TriplaneUpsampler through library convolutions (torch / MIOpen), then the same fused decode.
There is no CPU path: every tensor must be on the HIP device.
"""
import os

import numpy as np
import torch
import torch.nn as nn

from . import ops
from ._lib import AmavError
from .body_model import SUBDIVIDE_VERTS, BodyModel, build_subdivision_table

SUBDEVIDE_VERTS = SUBDIVIDE_VERTS  # the reference's spelling (renderer.py:14)
SCALE_BIAS = ops.SCALE_BIAS
OPACITY_BIAS = ops.OPACITY_BIAS


def _morton_order(v_template, gather_idx):
    """Order of the sampled points along a Z-order curve of their rest-pose positions.  The reference draws the
    subset in a fresh random order on every forward (renderer.py:287), so any fixed order of the same set is as
    faithful; a spatial one keeps neighbouring points (same triplane texels, same image tiles) in neighbouring lanes."""
    vt = v_template.double()
    a0, b0, a1, b1 = (gather_idx[:, k].long() for k in range(4))
    pos = ((vt[a0] + vt[b0]) * 0.5 + (vt[a1] + vt[b1]) * 0.5) * 0.5
    lo, hi = pos.min(0).values, pos.max(0).values
    q = ((pos - lo) / (hi - lo).clamp_min(1e-12) * 1023.0).long().clamp(0, 1023)
    code = torch.zeros(pos.shape[0], dtype=torch.long)
    for bit in range(10):
        for axis in range(3):
            code |= ((q[:, axis] >> bit) & 1) << (3 * bit + axis)
    return torch.argsort(code, stable=True)


def inverse_sigmoid(x):
    """src/utils/math_utils.py:7-11."""
    return torch.log(x / (1 - x)) if isinstance(x, torch.Tensor) else float(np.log(x / (1 - x)))


class _WindowTooSmall(Exception):
    """A refined point samples outside the exact region of the windowed upsampler (Renderer.forward falls back)."""


class Renderer(nn.Module):
    """The stage-2 renderer.  Its colour head and the fused decode write 3 colour channels per Gaussian, as in the
    reference, so Renderer itself always renders RGB colours; view-dependent (spherical-harmonic) colours are for callers
    that bring the coefficients themselves to render_batch / render_one / render_multi_view (args.rgb=False) or to
    GaussianRasterizer (shs=)."""

    def __init__(self, cfg=None, smpl_decoder=None):
        super().__init__()
        self.cfg = cfg
        if getattr(cfg, "differentiable_refine_points", False) and (
                getattr(cfg, "no_point_refiner", True) or not getattr(cfg, "differentiable_refiner", False)):
            raise ValueError("RendererConfig.differentiable_refine_points=True needs a trainable point refiner: set "
                             "no_point_refiner=False and differentiable_refiner=True")
        self.smplx_model = self.init_smplx_model()
        # the reference's table (renderer.py:14-18,25); `num_gaussians` overrides it (BASELINE's 50 000-Gaussian stress
        # config has no entry there)
        self.num_verts = int(getattr(self.cfg, "num_gaussians", None) or SUBDEVIDE_VERTS[self.cfg.subdivide_steps])
        self.init_smplx_subdivider(subdivide_steps=self.cfg.subdivide_steps)
        self.smpl_decoder = smpl_decoder if cfg.predict_smplx_params else None
        if getattr(cfg, "upsample_triplane", False):
            self.triplane_upsampler = TriplaneUpsampler(cfg)

        C = cfg.triplane_feature_dim
        if not getattr(cfg, "no_point_refiner", True):  # renderer.py:34-47
            from .point_transformer import PTv3Encoder

            self.point_encoder = PTv3Encoder(cfg=cfg)
            width = self.point_encoder.point_transformer.out_channels  # 256 in the reference's config
            self.point_refiner = nn.Sequential(nn.Linear(width, 256), nn.ReLU(), nn.Linear(256, 256), nn.ReLU(),
                                               nn.Linear(256, 3))
            nn.init.constant_(self.point_refiner[-1].weight, 0)
            nn.init.constant_(self.point_refiner[-1].bias, 0)
        self.gaussian_decoder = nn.Module()
        self.gaussian_decoder.xyz_layer = nn.Linear(C * 3 + 3, 3)
        self.gaussian_decoder.rotation_layer = nn.Linear(C * 3 + 3, 4)
        self.gaussian_decoder.scaling_layer = nn.Linear(C * 3 + 3, 3)
        self.gaussian_decoder.opacity_layer = nn.Linear(C * 3 + 3, 1)
        self.gaussian_decoder.shs_layer = nn.Linear(C * 3 + 3, 3)
        # reference initialisation (renderer.py:57-71)
        for layer in (self.gaussian_decoder.xyz_layer, self.gaussian_decoder.rotation_layer,
                      self.gaussian_decoder.scaling_layer, self.gaussian_decoder.opacity_layer,
                      self.gaussian_decoder.shs_layer):
            nn.init.constant_(layer.weight, 0)
            nn.init.constant_(layer.bias, 0)
        nn.init.constant_(self.gaussian_decoder.rotation_layer.bias[0], 1.0)
        nn.init.constant_(self.gaussian_decoder.scaling_layer.bias, -1.0)
        nn.init.constant_(self.gaussian_decoder.opacity_layer.bias, inverse_sigmoid(0.1))
        self._packed = None
        self._chunk_streams = []
        self.project_sampled_region = os.environ.get("AMAV_PROJECT_REGION", "1") != "0"
        self.to(cfg.device)

    # ---- body model ------------------------------------------------------------------------------------------
    def init_smplx_model(self):
        """renderer.py:206-225.  Loads SMPLX_NEUTRAL.npz from cfg.smplx_model_path when present, else the seeded
        SMPL-X-shaped synthetic body (the real model is licence-gated)."""
        return BodyModel.create(getattr(self.cfg, "smplx_model_path", None), device=self.cfg.device, num_betas=10,
                                num_expression_coeffs=self.cfg.num_expression_coeffs,
                                flat_hand_mean=self.cfg.flat_hand_mean, seed=getattr(self.cfg, "body_seed", 42))

    def init_smplx_subdivider(self, subdivide_steps=2):
        """renderer.py:227-243: max(1, steps) edge-midpoint subdivisions, baked into one gather table together with
        the vertex subset (drawn once from cfg.subset_seed instead of per forward, renderer.py:287)."""
        levels = max(1, subdivide_steps)
        table = build_subdivision_table(self.smplx_model.faces, self.smplx_model.num_verts, levels)
        g = torch.Generator().manual_seed(int(getattr(self.cfg, "subset_seed", 42)))
        if self.num_verts > table.shape[0]:
            raise ValueError(f"{self.num_verts} Gaussians requested, the mesh subdivided {levels}x has {table.shape[0]} vertices")
        idx = torch.randperm(table.shape[0], generator=g)[: self.num_verts]
        if getattr(self.cfg, "subset_order", "random") == "spatial":
            idx = idx[_morton_order(self.smplx_model.v_template.detach().cpu(), torch.as_tensor(table)[idx])]
        self.subset_index = idx  # ids into the densified vertex list (kept for tests)
        self.register_buffer("_gather_idx", torch.as_tensor(table)[idx].contiguous(), persistent=False)
        # the gather transposed, for its backward (differentiable_smplx)
        offsets, entries = ops.points_gather_csr(self._gather_idx, self.smplx_model.num_verts)
        self.register_buffer("_gather_csr_offsets", offsets, persistent=False)
        self.register_buffer("_gather_csr_entries", entries, persistent=False)

    def _posed_vertices(self, smpl_params):
        B, T = smpl_params["global_orient"].shape[:2]
        r = lambda k: smpl_params[k].reshape(B * T, -1)
        return self.smplx_model(global_orient=r("global_orient"), body_pose=r("body_pose"), betas=r("betas"),
                                left_hand_pose=r("left_hand_pose"), right_hand_pose=r("right_hand_pose"),
                                jaw_pose=r("jaw_pose"), leye_pose=r("leye_pose"), reye_pose=r("reye_pose"),
                                expression=r("expression")).vertices

    def get_smpl_vertices(self, smpl_params):
        """renderer.py:245-290: SMPL-X LBS for all B*T frames, then densify + subset.  -> [B*T, N, 3]"""
        vertices = self._posed_vertices(smpl_params)
        if self.cfg.densify_smplx_verts:
            if vertices.requires_grad:  # BodyModel's differentiable path (grad mode on, an SMPL-X tensor requires grad)
                return ops.points_gather_differentiable(vertices, self._gather_idx,
                                                        (self._gather_csr_offsets, self._gather_csr_entries))
            vertices = ops.points_gather(vertices, self._gather_idx)
        return vertices

    # ---- triplane --------------------------------------------------------------------------------------------
    def sample_from_triplane(self, triplane_features, points):
        """renderer.py:292-317: planes [B,3,C,R,R] (or unbatched), points [B,N,3] -> [B,N,3C]."""
        batched = points.ndim == 3
        if not batched:
            triplane_features, points = triplane_features[None], points[None]
        planes, points = triplane_features.float(), points.float()
        if torch.is_grad_enabled() and (planes.requires_grad or points.requires_grad):
            out = ops.triplane_sample_features_differentiable(planes, points, self.cfg.radius)
        else:
            out = ops.triplane_sample_features(planes, points, self.cfg.radius)
        return out if batched else out.squeeze(0)

    def refine_points(self, triplane_tokens, points, differentiable=False):
        """renderer.py:136-151: features at the initial points -> PTv3 -> 3-layer MLP -> points + offsets.
        tokens [F,C,3R^2], points [F,N,3] -> refined points [F,N,3].  Frames are refined in groups of
        cfg.refiner_clouds_per_pass (they do not interact; the group only bounds the working set).
        differentiable (cfg.differentiable_refine_points, under grad mode): the same kernels in the same frame groups as
        an autograd graph -- the sampling's HIP backward (ops.triplane_sample_features_differentiable) carries gradients
        to the tokens and the points, the trainable PTv3 (point_transformer.py) to its parameters and the features, torch
        to the MLP.  PTv3 gives its `points` argument no gradient: the points' comes from the residual and the sampling."""
        F, N, _ = points.shape
        R = self._plane_resolution(triplane_tokens)
        planes = triplane_tokens.view(F, triplane_tokens.shape[1], 3, R, R).permute(0, 2, 1, 3, 4)
        step = max(1, min(int(getattr(self.cfg, "refiner_clouds_per_pass", 32)),
                          int(getattr(self.cfg, "refiner_points_per_pass", 320_000)) // max(N, 1)))
        ptv3 = self.point_encoder.point_transformer
        if ptv3.batch_statistics and ptv3.training:
            step = max(F, 1)  # cfg.refiner_batch_statistics: a BatchNorm statistic is over all frames of the call
        sample = ops.triplane_sample_features_differentiable if differentiable else ops.triplane_sample_features
        refined = []
        for s in range(0, F, step):
            pts = points[s:s + step].contiguous()
            feats = sample(planes[s:s + step], pts, self.cfg.radius)
            offsets = self.point_refiner(self.point_encoder.point_transformer(pts, feats))
            refined.append(pts + offsets.view(pts.shape))
        return refined[0] if len(refined) == 1 else torch.cat(refined)

    def _head_layers(self):
        gd = self.gaussian_decoder
        return dict(xyz_layer=gd.xyz_layer, rotation_layer=gd.rotation_layer, scaling_layer=gd.scaling_layer,
                    opacity_layer=gd.opacity_layer, shs_layer=gd.shs_layer)

    def _head_weights(self, differentiable=False):
        layers = self._head_layers()
        device = self.gaussian_decoder.xyz_layer.weight.device
        if differentiable:  # packed from the live parameters on every call: never the detached cache
            return ops.pack_head_weights({k: (l.weight, l.bias) for k, l in layers.items()},
                                         self.cfg.triplane_feature_dim, device, differentiable=True)
        version = tuple((ops.tensor_version(l.weight), ops.tensor_version(l.bias), l.weight.data_ptr()) for l in layers.values())
        if self._packed is None or self._packed[0] != version:
            heads = {k: (l.weight, l.bias) for k, l in layers.items()}
            self._packed = (version, ops.pack_head_weights(heads, self.cfg.triplane_feature_dim, device))
        return self._packed[1]

    def _differentiable_smplx(self):
        return bool(getattr(self.cfg, "differentiable_smplx", False))

    def _differentiable_refine_points(self):
        return bool(getattr(self.cfg, "differentiable_refine_points", False)) and hasattr(self, "point_encoder")

    def _differentiable_upsampler(self):
        return bool(getattr(self.cfg, "differentiable_upsampler", False)) and hasattr(self, "triplane_upsampler")

    def _wants_grad(self, *tensors, smpl_params=None):
        """Gradients are recorded through the decode when grad mode is on and the tokens, a head parameter or transl
        (among `tensors`) requires grad -- with cfg.differentiable_smplx, also any tensor of `smpl_params`, with
        cfg.differentiable_refine_points, also any point_encoder / point_refiner parameter, with
        cfg.differentiable_upsampler, also any triplane_upsampler parameter; otherwise every call runs the inference
        path exactly as before."""
        if not torch.is_grad_enabled():
            return False
        if smpl_params is not None and self._differentiable_smplx():
            tensors = tensors + tuple(v for v in smpl_params.values() if isinstance(v, torch.Tensor))
        if self._differentiable_refine_points():
            tensors = tensors + tuple(self.point_encoder.parameters()) + tuple(self.point_refiner.parameters())
        if self._differentiable_upsampler():
            tensors = tensors + tuple(self.triplane_upsampler.parameters())
        return any(t is not None and t.requires_grad for t in tensors) or any(
            p.requires_grad for p in self.gaussian_decoder.parameters())

    def _refuse_under_grad(self, smpl_params):
        """Configurations with no backward are refused rather than silently dropping gradient."""
        if hasattr(self, "point_encoder") and not self._differentiable_refine_points():
            raise NotImplementedError("Renderer: the point refiner has no backward; disable gradients "
                                      "(torch.no_grad()) or use no_point_refiner=True (to train through it, set "
                                      "differentiable_refiner=True and differentiable_refine_points=True)")
        if self._differentiable_smplx():
            return
        bad = sorted(k for k, v in smpl_params.items() if k != "transl" and isinstance(v, torch.Tensor) and v.requires_grad)
        if bad:
            raise NotImplementedError(f"Renderer: SMPL-X parameters {', '.join(bad)} require grad, but LBS has no "
                                      "backward (only transl is differentiable; set differentiable_smplx=True in the "
                                      "renderer config to train through LBS)")

    def _differentiable_decode(self, triplane_tokens, points, transl, region):
        w_plane, w_point = self._head_weights(differentiable=True)
        return ops.triplane_decode_differentiable(triplane_tokens, w_plane, w_point, points, transl,
                                                  self._plane_resolution(triplane_tokens), self.cfg.radius, region=region)

    def _plane_resolution(self, triplane_tokens):
        """Resolution of the planes inside a token slab [F,C,3 R^2] (R grows 2^num_upsample_blocks when upsampled)."""
        r = int(round((triplane_tokens.shape[-1] // 3) ** 0.5))
        if 3 * r * r != triplane_tokens.shape[-1]:
            raise AmavError(f"token length {triplane_tokens.shape[-1]} is not 3 * R^2")
        return r

    def decode_gaussians(self, triplane_tokens, points, transl):
        """Fused renderer.py:136-181: tokens [F,C,3R^2], points [F,N,3], transl [F,3] -> packed [F,N,16].
        Differentiable in the tokens, the heads, points and transl when grad mode is on and one of them requires grad."""
        if self._wants_grad(triplane_tokens, points, transl):
            return self._differentiable_decode(triplane_tokens, points, transl, region=False)
        w_plane, w_point = self._head_weights()
        proj = ops.triplane_project(triplane_tokens, w_plane, self._plane_resolution(triplane_tokens))
        return ops.triplane_sample_decode(proj, points, transl, self.cfg.radius, w_point)

    def gaussians_from_tokens(self, triplane_tokens, smpl_params, out=None, side_work=None, window_plan=None,
                              defer_decode=False):
        """renderer.py:127-181 as one fused stage: tokens [F,C,3R^2] + SMPL-X params -> packed Gaussians [F,N,16].

        Everything is enqueued on the calling stream: camera set-up (`side_work`, an optional callable whose result is
        returned as a second value), LBS chain, slab projection (of the region the posed body can sample), then the
        sampling kernel with the densify + subset gather folded in.  (Round 1 ran the projection on a helper stream; measured worth nothing -- 1.148 vs
        1.137 ms per 250-frame step -- and a fork/join graph only hid the hipMemsetAsync replay fault described in
        DESIGN.md section 1.)  `window_plan`: the windowed upsampler's plan for exactly these frames (mask [F,g,g] per
        plane); refined points that leave it raise _WindowTooSmall.
        `defer_decode`: for the densified decode (no point refiner), do not launch the sampling kernel but return its
        inputs (ops.decode_source, for ops.rasterize(decode=...)) as a last value; `packed` is filled by the rasterizer.
        Other configurations decode here and return None in that place.
        Differentiable (ops.triplane_decode_differentiable; the same records) when grad mode is on and the tokens, a
        head parameter or transl requires grad (with cfg.differentiable_smplx: any SMPL-X parameter, whose gradient then
        comes from the gather and LBS backwards; with cfg.differentiable_refine_points: any point refiner parameter,
        and the points are refined by refine_points(differentiable=True)); `out`, `window_plan`, `defer_decode`, the point
        refiner without that flag and -- without differentiable_smplx -- SMPL-X parameters other than transl that require
        grad are refused then (NotImplementedError).  With cfg.differentiable_upsampler a `window_plan` is taken under grad
        too (the refined points are checked against it as on the inference path: _WindowTooSmall).
        """
        F = triplane_tokens.shape[0]
        if self._wants_grad(triplane_tokens, smpl_params["transl"], smpl_params=smpl_params):
            self._refuse_under_grad(smpl_params)
            plan_ok = self._differentiable_upsampler()  # Renderer.forward's plan of the differentiable windowed upsampler
            refused = [n for n, v in (("out", out), ("window_plan", None if plan_ok else window_plan)) if v is not None] + (
                ["defer_decode"] if defer_decode else [])
            if refused:
                raise NotImplementedError(f"gaussians_from_tokens: {', '.join(refused)} cannot be combined with gradients")
            side_result = side_work() if side_work is not None else None
            # gather = the indexed decode's own points, bit for bit; with differentiable_smplx they carry gradients to
            # the SMPL-X parameters that require grad (BodyModel + points_gather_differentiable)
            with torch.set_grad_enabled(self._differentiable_smplx()):
                points = self.get_smpl_vertices(smpl_params)
            if hasattr(self, "point_encoder"):  # cfg.differentiable_refine_points (anything else was refused above)
                points = self.refine_points(triplane_tokens, points, differentiable=True)
                if window_plan is not None and not self.triplane_upsampler.windows_contain(
                        window_plan, points.detach(), self.cfg.triplane_resolution, self.cfg.radius):
                    raise _WindowTooSmall()
            packed = self._differentiable_decode(triplane_tokens, points, smpl_params["transl"].reshape(F, 3).float(),
                                                 region=self.project_sampled_region)
            return packed if side_work is None else (packed, side_result)
        w_plane, w_point = self._head_weights()
        R = self._plane_resolution(triplane_tokens)
        side_result = side_work() if side_work is not None else None
        vertices = self._posed_vertices(smpl_params)
        transl = smpl_params["transl"].reshape(F, 3).float()

        # The slab is projected only where the frame's points can sample it: the box of the posed vertices (the
        # subdivision table averages vertices, so its points stay inside) or of the refined points; the avatar covers a
        # fifth to a third of each plane, and the slab is the largest stream of the path (ops.triplane_project).
        def project(points_like):
            region = (ops.points_bbox(points_like), self.cfg.radius) if self.project_sampled_region else None
            return ops.triplane_project(triplane_tokens, w_plane, R, region=region)

        source = None
        if hasattr(self, "point_encoder"):
            if self.cfg.densify_smplx_verts:
                vertices = ops.points_gather(vertices, self._gather_idx)
            points = self.refine_points(triplane_tokens, vertices)
            if window_plan is not None and not self.triplane_upsampler.windows_contain(
                    window_plan, points, self.cfg.triplane_resolution, self.cfg.radius):
                raise _WindowTooSmall()
            packed = ops.triplane_sample_decode(project(points), points, transl, self.cfg.radius, w_point, out=out)
        elif self.cfg.densify_smplx_verts and defer_decode:
            source = ops.decode_source(project(vertices), vertices, self._gather_idx, transl, self.cfg.radius, w_point,
                                       out=out)
            packed = source["out"]
        elif self.cfg.densify_smplx_verts:
            packed = ops.triplane_sample_decode_indexed(project(vertices), vertices, self._gather_idx, transl,
                                                        self.cfg.radius, w_point, out=out)
        else:
            packed = ops.triplane_sample_decode(project(vertices), vertices, transl, self.cfg.radius, w_point, out=out)
        if defer_decode:
            return (packed, source) if side_work is None else (packed, side_result, source)
        return packed if side_work is None else (packed, side_result)

    def render_tokens(self, triplane_tokens, smpl_params, cam_params, chunks=1, workspaces=None, check_overflow=True,
                      bg_color=None, window_plan=None, wire=None, fuse_decode=None):
        """tokens [F,C,3R^2] + SMPL-X params [B,T,...] (B*T = F) + cameras -> (rgba [F,H,W,4], packed [F,N,16]).

        The body of forward() after the SMPL-X decoder.  With `chunks` > 1 the frames are split into that many
        groups, each driven on its own HIP stream: the blend kernel is VALU-bound while LBS / projection / binning
        are memory- and latency-bound, so one group's rasterisation overlaps the next group's decode.
        `workspaces`: optional list of per-chunk RasterWorkspace objects (reused across calls; resized entries are
        written back).  With check_overflow=False the caller must check workspaces[i].status() itself.
        `window_plan`: see gaussians_from_tokens (covers all F frames; every frame group checks its own slice of it).
        `wire`: (uint8 buffer, capacity in tiles) -- the rasterizer writes the exchange's wire buffer of these F frames
        itself (ops.rasterize; dist.FrameAllGather.wire_target()); one frame group only.
        `fuse_decode` (None = ops.decode_bin_enabled(), AMAV_DECODE_BIN): with one frame group and the densified decode,
        the triplane decode runs inside the rasterizer's binning block (ops.rasterize(decode=...)); False = its own
        launch.  Same records and frames either way.
        """
        F = triplane_tokens.shape[0]
        H, W = int(self.cfg.image_size[0]), int(self.cfg.image_size[1])
        flat = {k: v.reshape(F, *v.shape[2:]) for k, v in smpl_params.items()}
        K = cam_params["intrinsic"].reshape(F, 3, 3)
        E = cam_params["extrinsic"].reshape(F, 4, 4)
        chunks = max(1, min(int(chunks), F))
        if self._wants_grad(triplane_tokens, smpl_params["transl"], smpl_params=smpl_params):
            # differentiable: separate decode launch, one frame group, then render_batch's differentiable rasterizer
            plan_ok = self._differentiable_upsampler()  # see gaussians_from_tokens
            refused = [n for n, v in (("workspaces", workspaces), ("wire", wire),
                                      ("window_plan", None if plan_ok else window_plan))
                       if v is not None] + (["chunks > 1"] if chunks > 1 else []) + (["fuse_decode"] if fuse_decode else [])
            if refused:
                raise NotImplementedError(f"render_tokens: {', '.join(refused)} cannot be combined with gradients")
            Kc, Ec = K.float(), E.float()
            packed, camera = self.gaussians_from_tokens(
                triplane_tokens, {k: v.unsqueeze(0) for k, v in flat.items()},
                side_work=lambda: ops.camera_from_intrinsics(Kc, Ec, H, W), window_plan=window_plan)
            rgba = render_batch(self.unpack_gaussians(packed), K.unsqueeze(0), E.unsqueeze(0), self.cfg, bg_color,
                                return_rgba=True, camera=camera[:3])
            return rgba.reshape(F, H, W, 4), packed
        if wire is not None and chunks != 1:
            raise AmavError("render_tokens: the wire buffer covers the whole shard; use chunks=1 with it")
        bounds = [(F * i // chunks, F * (i + 1) // chunks) for i in range(chunks)]
        dev = triplane_tokens.device
        rgba = torch.empty(F, H, W, 4, device=dev)
        packed_all = torch.empty(F, self.num_verts if self.cfg.densify_smplx_verts else self.smplx_model.num_verts,
                                 ops.GAUSS_STRIDE, device=dev)
        if workspaces is None:
            workspaces = [None] * chunks
        cur = torch.cuda.current_stream()
        while len(self._chunk_streams) < chunks - 1:
            self._chunk_streams.append(torch.cuda.Stream(device=dev))
        fuse = chunks == 1 and (ops.decode_bin_enabled() if fuse_decode is None else bool(fuse_decode))
        used = []
        try:
            for ci, (s, e) in enumerate(bounds):
                st = cur if ci == 0 else self._chunk_streams[ci - 1]
                if st is not cur:
                    st.wait_stream(cur)
                used.append(st)
                with torch.cuda.stream(st):
                    sub = {k: v[s:e].unsqueeze(0) for k, v in flat.items()}
                    Kc, Ec = K[s:e].float(), E[s:e].float()
                    plan = None if window_plan is None else [
                        dict(w, mask=None if w["mask"] is None else w["mask"][s:e]) for w in window_plan]
                    res = self.gaussians_from_tokens(
                        triplane_tokens[s:e], sub, out=packed_all[s:e],
                        side_work=lambda: ops.camera_from_intrinsics(Kc, Ec, H, W), window_plan=plan, defer_decode=fuse)
                    packed, camera, source = res if fuse else (*res, None)
                    g = self.unpack_gaussians(packed)
                    out = render_batch(g, K[s:e].unsqueeze(0), E[s:e].unsqueeze(0), self.cfg, bg_color,
                                       workspace=workspaces[ci], check_overflow=check_overflow, out_rgba=rgba[s:e],
                                       return_workspace=True, camera=camera[:3], wire=wire, decode=source,
                                       fuse_decode=fuse)
                    workspaces[ci] = out[1]
        finally:  # also on _WindowTooSmall from a later frame group: the side streams' work is joined before a re-render
            for st in used:
                if st is not cur:
                    cur.wait_stream(st)
        return rgba, packed_all

    @staticmethod
    def unpack_gaussians(packed):
        """Packed [F,N,16] records -> the reference's dict of (strided) views (renderer.py:337-344)."""
        color = packed[..., ops.REC_COLOR:ops.REC_COLOR + 3]
        return {"xyz": packed[..., ops.REC_XYZ:ops.REC_XYZ + 3], "scale": packed[..., ops.REC_SCALE:ops.REC_SCALE + 3],
                "rot": packed[..., ops.REC_ROT:ops.REC_ROT + 4],
                "opacity": packed[..., ops.REC_OPACITY:ops.REC_OPACITY + 1], "color": color, "shs": color}

    def construct_gaussians(self, gaussian_params, points, smpl_params):
        """renderer.py:319-346 for callers that computed the raw heads themselves (torch elementwise ops)."""
        rotation = torch.nn.functional.normalize(gaussian_params["rotation"], dim=-1)
        color = torch.sigmoid(gaussian_params["shs"])
        return {"xyz": points + gaussian_params["xyz_offset"] + smpl_params["transl"].reshape(-1, 1, 3),
                "scale": gaussian_params["scaling"], "rot": rotation, "opacity": gaussian_params["opacity"],
                "color": color, "shs": color}

    # ---- forward ---------------------------------------------------------------------------------------------
    def forward(self, triplane_features, cam_params, smpl_tokens=None, smpl_params_gt=None):
        """renderer.py:73-204.  triplane_features [B,T,C,3R^2] tokens, smpl_tokens [B,T,D,L]."""
        if smpl_tokens is None:
            raise AmavError("Renderer.forward needs smpl_tokens (the reference dereferences it too, renderer.py:84)")
        B, T = smpl_tokens.shape[:2]
        limit = int(getattr(self.cfg, "upsample_frames_per_pass", 8))
        if getattr(self.cfg, "upsample_triplane", False) and B * T > limit:
            # upsampled planes are 805 MB per frame at the reference defaults: longer calls go through in passes of
            # `limit` frames (the reference itself renders six-frame windows); frames are independent
            flat = lambda v: v.reshape(1, B * T, *v.shape[2:])
            parts = []
            for s0 in range(0, B * T, limit):
                sl = slice(s0, s0 + limit)
                parts.append(self.forward(flat(triplane_features)[:, sl], {k: flat(v)[:, sl] for k, v in cam_params.items()},
                                          flat(smpl_tokens)[:, sl], None if smpl_params_gt is None else
                                          {k: flat(v)[:, sl] for k, v in smpl_params_gt.items()}))
            images = torch.cat([o[0] for o in parts], dim=1)
            images = images.reshape(B, T, *images.shape[2:])
            gaussians = {k: torch.cat([o[1][k] for o in parts], dim=0) for k in parts[0][1]}
            if self.cfg.predict_smplx_params:
                pred = {k: torch.cat([o[2][k] for o in parts], dim=1) for k in parts[0][2]}
                return images, gaussians, {k: v.reshape(B, T, *v.shape[2:]) for k, v in pred.items()}
            return images, gaussians
        tokens = triplane_features.reshape(B * T, triplane_features.shape[2], triplane_features.shape[3]).float()

        pred_smpl_params = None
        if self.smpl_decoder is not None:
            pred_smpl_params = self.smpl_decoder(smpl_tokens.reshape(B * T, *smpl_tokens.shape[2:]))
            for key in list(pred_smpl_params.keys()):  # renderer.py:111-118
                v = pred_smpl_params[key]
                if key in ("body_pose", "left_hand_pose", "right_hand_pose"):
                    pred_smpl_params[key] = v.reshape(B, T, *v.shape[1:])
                else:
                    pred_smpl_params[key] = v.reshape(B, T, -1)
        smpl_params = smpl_params_gt if smpl_params_gt is not None else pred_smpl_params
        if smpl_params is None:
            raise AmavError("Renderer.forward: no SMPL-X parameters (predict_smplx_params is off and no smpl_params_gt)")

        chunks = int(getattr(self.cfg, "pipeline_chunks", 1)) if B * T >= 32 else 1
        grad = self._wants_grad(tokens, smpl_params["transl"], smpl_params=smpl_params)
        if grad:
            chunks = 1  # the differentiable path renders the frames as one group
        window_plan = None
        if getattr(self.cfg, "upsample_triplane", False):  # renderer.py:94-99 (library convolutions, 8(f) row 2)
            up, R = self.triplane_upsampler, self.cfg.triplane_resolution
            if up.training:
                # crops, tile mosaics (with zero filler cells) and the < 2 GiB batch chunks all change what a
                # training-mode BatchNorm2d would average over (and would overwrite its running statistics with it); the
                # point refiner folds its BatchNorms as eval too.  This package is inference-only.
                raise AmavError("Renderer.forward: the triplane upsampler is in training mode; its BatchNorm layers are "
                                "evaluated with running statistics only -- call .eval() on the module first")
            if grad and not self._differentiable_upsampler():
                raise NotImplementedError("Renderer.forward: the triplane upsampler has no backward; disable gradients "
                                          "(torch.no_grad()) or upsample_triplane=False (to train through it, set "
                                          "differentiable_upsampler=True)")
            coarse = tokens
            if getattr(self.cfg, "upsample_windows", True):
                # only the texels the body's points can sample are upsampled (TriplaneUpsampler, "windowed evaluation")
                refiner = hasattr(self, "point_encoder")
                margin = float(getattr(self.cfg, "upsample_window_margin", 0.05)) if refiner else 0.0
                with torch.no_grad():  # the plan is discrete: under grad it must not record an LBS graph of its own
                    plan = up.plan_windows(self.get_smpl_vertices(smpl_params), R, self.cfg.radius, margin)
                # under grad (cfg.differentiable_upsampler): an autograd graph on a slab of its own
                tokens = up.forward_tokens_windowed(coarse, R, plan, differentiable=grad)
                window_plan = plan if refiner else None  # refined points are checked against it
                self.last_window_plan = plan  # diagnostic only (tests / tools read it); never consumed by the path
            else:
                tokens = up.forward_tokens(coarse, R)
        try:
            rgba, packed = self.render_tokens(tokens, smpl_params, cam_params, chunks=chunks, window_plan=window_plan)
        except _WindowTooSmall:  # the refiner moved a point past the margin: full planes, once (under grad: under autograd)
            tokens = self.triplane_upsampler.forward_tokens(coarse, self.cfg.triplane_resolution)
            rgba, packed = self.render_tokens(tokens, smpl_params, cam_params, chunks=chunks)
        gaussians = self.unpack_gaussians(packed)
        rendered_images = rgba.view(B, T, *rgba.shape[1:])[..., :3]
        if self.cfg.predict_smplx_params:
            return rendered_images, gaussians, pred_smpl_params
        return rendered_images, gaussians


class ResBlock(nn.Module):
    """renderer.py:348-362 (module layout kept so `triplane_upsampler.*` checkpoint keys load)."""

    def __init__(self, in_channels, out_channels, norm_layer=nn.BatchNorm2d):
        super().__init__()
        self.block = nn.Sequential(norm_layer(in_channels), nn.ReLU(inplace=True),
                                   nn.Conv2d(in_channels, out_channels, 3, padding=1), norm_layer(out_channels),
                                   nn.ReLU(inplace=True), nn.Conv2d(out_channels, out_channels, 3, padding=1))
        self.skip = nn.Conv2d(in_channels, out_channels, 1) if in_channels != out_channels else nn.Identity()

    def forward(self, x):
        return self.skip(x) + self.block(x)


class UpsampleBlock(nn.Module):
    """renderer.py:364-375: nearest x2 -> conv3x3 -> ReLU -> ResBlock."""

    def __init__(self, in_channels, out_channels, scale_factor=2):
        super().__init__()
        self.upsample = nn.Sequential(nn.Upsample(scale_factor=scale_factor, mode="nearest"),
                                      nn.Conv2d(in_channels, out_channels, 3, padding=1), nn.ReLU(inplace=True),
                                      ResBlock(out_channels, out_channels))

    def forward(self, x):
        return self.upsample(x)


class TriplaneUpsampler(nn.Module):
    """renderer.py:377-417: `num_upsample_blocks` x (UpsampleBlock + nearest-upsampled skip) on the three planes.
    SURVEY section 8(f) row 2: library convolutions (MIOpen through torch), not a hand-written kernel; eval-mode
    BatchNorm.  At the reference defaults (4 blocks, C=256, 32^2 -> 512^2) this is ~3.7 TFLOP and 805 MB per frame."""

    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        c = cfg.triplane_feature_dim
        n = cfg.num_upsample_blocks
        self.upsample_blocks = nn.ModuleList([UpsampleBlock(c, c, 2) for _ in range(n)])
        self.skip_connections = nn.ModuleList([
            nn.Sequential(nn.Conv2d(c, c, 1) if i == 0 else nn.Identity(), nn.Upsample(scale_factor=2, mode="nearest"))
            for i in range(n)])

    def forward(self, triplanes):
        """[B,3,C,H,W] -> [B,3,C,2^n H,2^n W]"""
        B, P, C, H, W = triplanes.shape
        cur, _ = self._run(triplanes.reshape(B * P, C, H, W))
        return cur.reshape(B, P, C, cur.shape[-2], cur.shape[-1])

    def forward_tokens(self, tokens, resolution):
        """Token slab [F,C,3 R^2] -> [F,C,3 (2^n R)^2] (what the fused decode consumes)."""
        F, C, _ = tokens.shape
        planes = tokens.reshape(F, C, 3, resolution, resolution).permute(0, 2, 1, 3, 4)
        up = self.forward(planes)
        return up.permute(0, 2, 1, 3, 4).reshape(F, C, -1)

    # ---- windowed evaluation -----------------------------------------------------------------------------------------
    # The upsampled planes are only ever SAMPLED, at the body's points: a few per cent of the 512^2 texels of each plane.
    # Convolutions are translation-equivariant, so only what the sample points can reach is computed, in two stages:
    #   * blocks 1 .. n-2 (6 % of the flops) run on ONE crop per plane: the bounding box (in input cells) of the
    #     active tiles plus a 3-cell halo.  A crop border feeds zeros where the full plane has values; after k blocks
    #     of [nearest x2, three 3x3 convolutions] that error has travelled d_k = 2 d_(k-1) + 3 = 3 (2^k - 1) texels;
    #   * the last two blocks (94 % of the flops) run on the ACTIVE TILES only: output tiles of 4 x 4 input cells
    #     (64 x 64 texels for n = 4) that contain a bilinear tap of some point.  Cells of 16 + 6 texels of the
    #     level-(n-2) activation go through block n-1; the centre 32 + 4 texels of the result are the padded tiles of
    #     block n (a block's reach is 3 output texels, 4 are cut away), whose centre 64 are written into their place of
    #     the full-resolution slab.  Each stage runs as one mosaic image through the library's convolutions.
    # Texels inside active tiles are the full computation's values (identical operands, possibly another library
    # kernel: rounding-level differences); the rest of the slab keeps whatever it held and is never sampled.  Where a
    # crop coincides with the plane's own border the zero padding IS the reference's; the halo of a tile at the plane's
    # border lies outside the plane and is zeroed before every convolution, as zero padding would.  Crop sizes and tile-batch
    # sizes only grow (steps of 4 cells / 4 tiles), so the library sees few distinct convolution shapes.
    PLANE_AXES = ((0, 1), (0, 2), (1, 2))  # (width, height) coordinate of plane p (renderer.py:300-310)
    TILE_CELLS = 4

    def halo_texels(self, blocks=None):
        return 3 * (2 ** (len(self.upsample_blocks) if blocks is None else blocks) - 1)

    def _taps(self, coords, resolution, radius):
        """First / second bilinear tap index at the upsampled resolution, clamped into the plane (grid_sample,
        align_corners=False; renderer.py:298-310).  A tap outside the plane reads the zero padding: nothing to compute."""
        r_out = resolution * 2 ** len(self.upsample_blocks)
        pix = ((torch.clamp(coords / radius, -1, 1) + 1) * r_out - 1) / 2
        first = torch.floor(pix)
        return first.clamp(0, r_out - 1).long(), (first + 1).clamp(0, r_out - 1).long(), r_out

    def _active_tiles(self, points, resolution, radius, margin):
        """bool [F, 3, g, g] (frame, plane, tile row, tile column), g = resolution / TILE_CELLS: tiles holding a tap of a
        point of that frame (or of the point displaced by up to `margin` metres along every axis)."""
        g = resolution // self.TILE_CELLS
        tile = self.TILE_CELLS * 2 ** len(self.upsample_blocks)
        F, N, _ = points.shape
        flat = points.reshape(-1, 3)
        lo, _, _ = self._taps(flat - margin, resolution, radius)
        _, hi, _ = self._taps(flat + margin, resolution, radius)
        lo, hi = lo // tile, hi // tile                     # [F N, 3] tile index per coordinate
        frame = torch.arange(F, device=points.device).repeat_interleave(N)
        mask = torch.zeros(F, 3, g, g, dtype=torch.bool, device=points.device)
        span = int((hi - lo).max()) if flat.shape[0] else 0   # (host sync) usually 1: a tap pair straddles a tile edge
        for p, (aw, ah) in enumerate(self.PLANE_AXES):
            for dy in range(span + 1):
                for dx in range(span + 1):
                    mask[frame, p, torch.minimum(lo[:, ah] + dy, hi[:, ah]), torch.minimum(lo[:, aw] + dx, hi[:, aw])] = True
        return mask

    def plan_windows(self, points, resolution, radius, margin=0.0):
        """points [F,N,3] -> plan: per plane {crop (y0,y1,x0,x1) in input cells (common to the frames), tiles int64
        [K,3] (frame, tile row, tile column; None = whole planes: resolution not a multiple of TILE_CELLS, or a diverged
        pose), mask bool [F,g,g]}.  Host sync: the tile mask."""
        n = len(self.upsample_blocks)
        R = resolution
        if not hasattr(self, "_window_sizes"):
            self._window_sizes = [[0, 0] for _ in range(3)]
        if R % self.TILE_CELLS or not bool(torch.isfinite(points).all()):  # no tiling / a diverged pose: whole planes
            return [dict(crop=(0, R, 0, R), tiles=None, mask=None) for _ in range(3)]
        mask = self._active_tiles(points, R, radius, margin).cpu()
        halo_cells = 3 if n >= 2 else 2
        plan = []
        for p in range(3):
            tiles = torch.nonzero(mask[:, p])                          # [K,3]: frame, ty, tx
            if tiles.shape[0] == 0:
                plan.append(dict(crop=(0, self.TILE_CELLS, 0, self.TILE_CELLS), tiles=tiles, mask=mask[:, p]))
                continue
            spans = []
            for slot in (0, 1):
                idx = tiles[:, 1 + slot]
                c0 = max(0, int(idx.min()) * self.TILE_CELLS - halo_cells)
                c1 = min(R, (int(idx.max()) + 1) * self.TILE_CELLS + halo_cells)
                size = min(R, max(self._window_sizes[p][slot], -(-(c1 - c0) // 4) * 4))
                self._window_sizes[p][slot] = size
                start = min(max(0, c0 - (size - (c1 - c0)) // 2), R - size)
                spans.append((start, start + size))
            (y0, y1), (x0, x1) = spans
            plan.append(dict(crop=(y0, y1, x0, x1), tiles=tiles, mask=mask[:, p]))
        return plan

    def windows_contain(self, plan, points, resolution, radius):
        """True when every bilinear tap of `points` lies where the planned evaluation is exact (host sync)."""
        if all(w["mask"] is None for w in plan):
            return True
        need = self._active_tiles(points, resolution, radius, 0.0).cpu()
        return all(w["mask"] is None or not bool((need[:, p] & ~w["mask"]).any()) for p, w in enumerate(plan))

    MAX_ACTIVATION_BYTES = 2 ** 31  # the library's convolutions corrupt batch items that lie beyond a 4 GiB offset
    # (tools/upsampler_debug.py: 18 planes x 256 x 512^2 fp32 = 4.8 GB, i.e. the reference's own 6-frame window, come
    # back wrong for the last two planes); every call therefore keeps its largest activation below 2 GiB

    def _run(self, cur, first=0, last=None):
        """Blocks first .. last-1 on [B,C,h,w]; returns (activation, skip chain) at the output resolution.  The batch
        is processed in chunks small enough for MAX_ACTIVATION_BYTES."""
        blocks = list(zip(self.upsample_blocks, self.skip_connections))[first:last]
        B, C, h, w = cur.shape
        per_item = C * h * w * 4 ** len(blocks) * cur.element_size()
        step = max(1, self.MAX_ACTIVATION_BYTES // max(per_item, 1))
        outs, skips = [], []
        for s in range(0, B, step):
            x = skip = cur[s:s + step]
            for block, skip_conn in blocks:
                skip = skip_conn(skip)
                x = block(x) + skip
            outs.append(x)
            skips.append(skip)
        return (outs[0], skips[0]) if len(outs) == 1 else (torch.cat(outs), torch.cat(skips))

    @staticmethod
    def _last_block(block, image, valid=None):
        """UpsampleBlock.forward; with `valid` [1,1,2h,2w] the inputs of the 2nd and 3rd convolution are zeroed where
        the mosaic holds positions outside a plane (zero padding is what the reference's convolutions see there)."""
        if valid is None:
            return block(image)
        up, conv, relu, res = block.upsample
        x = relu(conv(up(image)))
        b = res.block
        r = b[2](b[1](b[0](x)) * valid)
        r = b[5](b[4](b[3](r)) * valid)
        return res.skip(x) + r

    def forward_tokens_windowed(self, tokens, resolution, plan, out=None, differentiable=False):
        """Token slab [F,C,3 R^2] + plan_windows()' plan -> full-resolution slab [F,C,3 (2^n R)^2] whose texels inside
        the active tiles are the upsampled planes (the rest keeps whatever the slab held: never sampled).
        differentiable: the same evaluation as an autograd graph (under grad mode): the slab is a fresh zero tensor --
        never the cached one, which earlier graphs may hold, and never `out` (refused) -- and the window cuts go through
        ops.windows_cut_differentiable (HIP cut + transpose; pad / unfold / index for CPU tensors); crops, _run, the
        mosaics, the validity masks and the placement of the tiles are torch and record their own graph.  Every
        convolution's gradient has the shape of its activation, so the MAX_ACTIVATION_BYTES chunking of _run and
        _mosaic bounds the backward's calls as it bounds the forward's."""
        F, C, _ = tokens.shape
        n = len(self.upsample_blocks)
        scale, s_in = 2 ** n, 2 ** (n - 1)
        r_out = resolution * scale
        if differentiable:
            if out is not None:
                raise ValueError("forward_tokens_windowed: differentiable=True writes a slab of its own; `out` is refused")
            out = torch.zeros(F, C, 3 * r_out * r_out, device=tokens.device, dtype=tokens.dtype)
        if out is None:
            cached = getattr(self, "_slab", None)
            if cached is None or cached.shape != (F, C, 3 * r_out * r_out) or cached.device != tokens.device:
                cached = torch.zeros(F, C, 3 * r_out * r_out, device=tokens.device)
                self._slab = cached
            out = cached
        planes = tokens.view(F, C, 3, resolution, resolution)
        ov = out.view(F, C, 3, r_out, r_out)
        hip = self._use_hip_conv(tokens, differentiable)
        hip_grad = self._use_hip_conv_grad(tokens, differentiable)
        tile_block = self._tile_block_hip_grad if hip_grad else self._tile_block_hip
        hip = hip or hip_grad
        t_in, t_out, g = self.TILE_CELLS * s_in, self.TILE_CELLS * scale, resolution // self.TILE_CELLS
        P = t_in + 4
        for p, w in enumerate(plan):
            y0, y1, x0, x1 = w["crop"]
            tiles = w["tiles"]
            if tiles is not None and tiles.shape[0] == 0:
                continue  # no point samples this plane
            crop = planes[:, :, p, y0:y1, x0:x1].contiguous()
            if tiles is None:
                up, _ = self._run(crop)
                ov[:, :, p, y0 * scale:y1 * scale, x0 * scale:x1 * scale] = up
                continue
            tiles = tiles.to(tokens.device)
            f_idx, ty, tx = tiles[:, 0], tiles[:, 1], tiles[:, 2]
            extent = resolution * scale
            if differentiable:  # the tiles as the cut's int32 arguments; tile (ty, tx) of frame f -> its index
                frame32, ty32, tx32 = f_idx.int(), ty.int(), tx.int()
                lattice = torch.full((F, g, g), -1, dtype=torch.int32, device=tokens.device)
                lattice[f_idx, ty, tx] = torch.arange(tiles.shape[0], dtype=torch.int32, device=tokens.device)

            def tile_windows(x, level_scale, pad, size):
                """[K,C,size,size]: for every active tile the window of `x` (level with `level_scale` texels per input
                cell, cropped at (y0, x0), padded by `pad`) that starts `pad` texels before the tile."""
                step = self.TILE_CELLS * level_scale
                if differentiable:  # window (ty, tx) starts at ty step - y0 level_scale - pad: a lattice over the tiles
                    off_y, off_x = -y0 * level_scale - pad, -x0 * level_scale - pad
                    return ops.windows_cut_differentiable(x, frame32, ty32 * step + off_y, tx32 * step + off_x, size,
                                                          (step, off_y, off_x, lattice))
                xp = torch.nn.functional.pad(x, (pad, pad, pad, pad)) if pad else x
                ay, ax = -(-(y0 * level_scale) // step), -(-(x0 * level_scale) // step)
                wv = xp[:, :, ay * step - y0 * level_scale:].unfold(2, size, step).permute(0, 1, 2, 4, 3)
                wv = wv[..., ax * step - x0 * level_scale:].unfold(4, size, step)       # [F,C,ky,size,kx,size]
                return wv[f_idx, :, ty - ay, :, tx - ax, :]

            def validity(step, first, length):
                """float [K,1,length,length] (or, on the library path, None when all ones): 1 where row ty step + first + j
                and the matching column lie inside the plane at that level (plane size = extent / t_out * step)."""
                size = extent // t_out * step
                pos = torch.arange(length, device=tokens.device) + first
                vy = ((ty * step)[:, None] + pos >= 0) & ((ty * step)[:, None] + pos < size)
                vx = ((tx * step)[:, None] + pos >= 0) & ((tx * step)[:, None] + pos < size)
                if not hip and bool(vy.all() and vx.all()):  # (host sync; the HIP branch multiplies unconditionally)
                    return None
                return (vy[:, :, None] & vx[:, None, :]).to(tokens.dtype)[:, None]

            def origins(step, first):
                """int32 [K,2]: the plane position (y, x) of every cell's first texel, what validity(step, first, .)
                encodes as a mask image."""
                return torch.stack((ty * step + first, tx * step + first), 1).int()

            chain = n >= 2 and bool(getattr(self.cfg, "upsample_tile_chain", True))
            if chain:
                # the LAST TWO blocks on the active tiles: cells of t2 + 6 texels at level n-2 -> block n-1 -> the centre
                # t_in + 4 texels are exactly the padded tiles of block n (reach of one block: 3 <= the 4 cut away)
                s2 = 2 ** (n - 2)
                t2 = self.TILE_CELLS * s2
                act2, skip2 = self._run(crop, 0, n - 2)
                if hip:
                    res = tile_block(self.upsample_blocks[n - 2], tile_windows(act2, s2, 3, t2 + 6),
                                     origins(t_in, -6), extent // t_out * t_in)
                else:
                    res = self._mosaic(self.upsample_blocks[n - 2], tile_windows(act2, s2, 3, t2 + 6),
                                       validity(t_in, -6, 2 * (t2 + 6)), p, 0)
                res = res[:, :, 4:-4, 4:-4]                                                             # [K,C,P,P]
                skip1 = self.skip_connections[n - 2](tile_windows(skip2, s2, 1, t2 + 2))                # [K,C,P,P]
                cells = res + skip1
                inside = validity(t_in, -2, P)   # the padded tile's positions outside the plane are zero padding
                if inside is not None:
                    cells = cells * inside
                skips = skip1[:, :, 2:-2, 2:-2]
            else:
                act, skip = self._run(crop, 0, n - 1)       # level n-1: [F,C,(y1-y0) s_in,(x1-x0) s_in]
                # the padding is only ever read where the crop ends at the plane's own border: zeros, as the reference pads
                cells = tile_windows(act, s_in, 2, P)
                skips = tile_windows(skip, s_in, 0, t_in)
            if hip:
                vals = tile_block(self.upsample_blocks[n - 1], cells, origins(t_out, -4), extent)
            else:
                vals = self._mosaic(self.upsample_blocks[n - 1], cells, validity(t_out, -4, 2 * P), p, 1)
            vals = vals[:, :, 4:4 + t_out, 4:4 + t_out] + self.skip_connections[n - 1](skips)
            ov.view(F, C, 3, g, t_out, g, t_out)[f_idx, :, p, ty, :, tx, :] = vals
        return out

    def _use_hip_conv(self, tokens, differentiable):
        """True when the tile stages run on ops.conv3x3_cells: AMAV_UPSAMPLER_CONV=hip (read per call; unset:
        cfg.upsample_conv), and nothing the kernel lacks is asked for -- no autograd, device tensors, eval-mode BatchNorm,
        channels a multiple of 32.  Otherwise the library path runs."""
        mode = os.environ.get("AMAV_UPSAMPLER_CONV") or getattr(self.cfg, "upsample_conv", "library")
        if mode not in ("library", "hip"):
            raise ValueError(f"AMAV_UPSAMPLER_CONV / cfg.upsample_conv: expected 'library' or 'hip', got {mode!r}")
        if mode != "hip" or differentiable or self.training or not tokens.is_cuda or tokens.shape[1] % 32:
            return False
        if tokens.dtype != torch.float32 or any(not q.is_cuda for q in self.parameters()):
            return False
        return not (torch.is_grad_enabled() and (tokens.requires_grad or any(q.requires_grad for q in self.parameters())))

    def _use_hip_conv_grad(self, tokens, differentiable):
        """True when a differentiable evaluation runs its tile stages on ops.conv3x3_cells_differentiable (HIP forward and
        backward, deterministic gradients): AMAV_UPSAMPLER_CONV_GRAD=hip (read per call; unset: cfg.upsample_conv_grad),
        device fp32 tensors and parameters, channels a multiple of 32, eval-mode BatchNorm.  Otherwise the library path
        runs.  AMAV_UPSAMPLER_CONV does not bear on it."""
        mode = os.environ.get("AMAV_UPSAMPLER_CONV_GRAD") or getattr(self.cfg, "upsample_conv_grad", "library")
        if mode not in ("library", "hip"):
            raise ValueError(f"AMAV_UPSAMPLER_CONV_GRAD / cfg.upsample_conv_grad: expected 'library' or 'hip', got {mode!r}")
        if mode != "hip" or not differentiable or self.training or not tokens.is_cuda or tokens.shape[1] % 32:
            return False
        return tokens.dtype == torch.float32 and all(q.is_cuda and q.dtype == torch.float32 for q in self.parameters())

    @staticmethod
    def _bn_fold(bn):
        """Eval-mode BatchNorm as (scale, shift), folded in fp64."""
        scale = torch.rsqrt(bn.running_var.double() + bn.eps)
        if bn.weight is not None:
            scale = scale * bn.weight.double()
        shift = -bn.running_mean.double() * scale
        if bn.bias is not None:
            shift = shift + bn.bias.double()
        return scale, shift

    def _prepared_block(self, block):
        """Split weights and folded vectors of one UpsampleBlock for _tile_block_hip, memoised on the version counter and
        address of every tensor they derive from (optim.Adam and load_state_dict update in place and bump the version)."""
        _, conv1, _, res = block.upsample
        bn0, _, conv_a, bn1, _, conv_b = res.block
        assert isinstance(res.skip, nn.Identity), "UpsampleBlock of the upsampler keeps its width: ResBlock.skip is Identity"
        sources = [t for m in (conv1, conv_a, conv_b) for t in (m.weight, m.bias)]
        sources += [t for bn in (bn0, bn1) for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var)]
        key = tuple((ops.tensor_version(t), t.data_ptr()) for t in sources if t is not None)
        if not hasattr(self, "_conv_memo"):
            self._conv_memo = {}
        hit = self._conv_memo.get(id(block))
        if hit is None or hit[0] != key:
            with torch.no_grad():
                s0, t0 = self._bn_fold(bn0)
                s1, t1 = self._bn_fold(bn1)
                bias_a = t1 if conv_a.bias is None else s1 * conv_a.bias.double() + t1
                prepared = dict(
                    w1=ops.conv3x3_prepare_weights(conv1.weight.detach()), b1=conv1.bias,
                    in_scale=s0.float().contiguous(), in_shift=t0.float().contiguous(),
                    wa=ops.conv3x3_prepare_weights(conv_a.weight.detach(), s1.float().contiguous()),
                    ba=bias_a.float().contiguous(),
                    wb=ops.conv3x3_prepare_weights(conv_b.weight.detach()), bb=conv_b.bias)
            hit = (key, prepared)
            self._conv_memo[id(block)] = hit
        return hit[1]

    def _tile_block_hip(self, block, cells, origin, extent):
        """One UpsampleBlock over independent cells [K,C,P,P] -> [K,C,2P,2P] (a channels-last view) in three launches of
        ops.conv3x3_cells, what _mosaic + _last_block compute on the library: every cell is zero padded on its own (the
        mosaic's neighbours only ever reach the halo the caller cuts away), and `origin` int32 [K,2] / `extent` state
        where a cell lies in its plane, so that positions outside the plane are the reference's zero padding for the
        second and third convolution (the `valid` images of _last_block).  Eval-mode BatchNorm: bn0 is the second
        launch's prologue, bn1 is folded into conv_a's prepared weights and bias."""
        w = self._prepared_block(block)
        C = cells.shape[1]
        with torch.no_grad():
            x = ops.conv3x3_cells(cells.permute(0, 2, 3, 1), w["w1"], C, w["b1"], upsample_input=True, relu_out=True)
            r = ops.conv3x3_cells(x, w["wa"], C, w["ba"], in_scale=w["in_scale"], in_shift=w["in_shift"], origin=origin,
                                  extent=extent, relu_out=True)
            out = ops.conv3x3_cells(r, w["wb"], C, w["bb"], origin=origin, extent=extent, residual=x)
        return out.permute(0, 3, 1, 2)

    def _tile_block_hip_grad(self, block, cells, origin, extent):
        """_tile_block_hip under autograd: the same three convolutions through ops.conv3x3_cells_differentiable.  The
        eval-mode BatchNorms are folded in torch (fp64, as _bn_fold, then fp32) inside the graph -- bn0 as the second
        convolution's prologue vectors, bn1 into conv_a's weight and bias -- so their affine parameters, trainable in
        eval mode, get their gradients from autograd's chain through the fold."""
        _, conv1, _, res = block.upsample
        bn0, _, conv_a, bn1, _, conv_b = res.block
        assert isinstance(res.skip, nn.Identity), "UpsampleBlock of the upsampler keeps its width: ResBlock.skip is Identity"
        s0, t0 = self._bn_fold(bn0)
        s1, t1 = self._bn_fold(bn1)
        w_a = (s1[:, None, None, None] * conv_a.weight.double()).float()
        b_a = (t1 if conv_a.bias is None else s1 * conv_a.bias.double() + t1).float()
        conv = ops.conv3x3_cells_differentiable
        x = conv(cells.permute(0, 2, 3, 1), conv1.weight, conv1.bias, upsample_input=True, relu_out=True)
        r = conv(x, w_a, b_a, in_scale=s0.float(), in_shift=t0.float(), origin=origin, extent=extent, relu_out=True)
        out = conv(r, conv_b.weight, conv_b.bias, origin=origin, extent=extent, residual=x)
        return out.permute(0, 3, 1, 2)

    def _mosaic(self, block, cells, valid, plane, stage):
        """One UpsampleBlock over cells [K,C,p,p] -> [K,C,2p,2p].  The cells are laid out as ONE mosaic image, 8 cells
        wide (the library then runs its large-image Winograd kernels whatever K is; a batch of small tiles made it pick
        an implicit-GEMM kernel at half the speed); neighbouring cells only see each other inside the halos the caller
        cuts away.  `valid` [K,1,2p,2p]: positions inside the plane (zero padding elsewhere, see _last_block).  Mosaic
        heights only grow, and an image stays below MAX_ACTIVATION_BYTES."""
        K, C, P, _ = cells.shape
        cols = 8
        if not hasattr(self, "_tile_batch"):
            self._tile_batch = {}
        rows = max(self._tile_batch.get((plane, stage), 0), -(-K // cols))
        self._tile_batch[(plane, stage)] = rows
        max_rows = max(1, self.MAX_ACTIVATION_BYTES // (C * 4 * P * P * cols * cells.element_size()))
        out = cells.new_empty(K, C, 2 * P, 2 * P)
        for r0 in range(0, rows, max_rows):
            nr = min(max_rows, rows - r0)
            k0, k1 = r0 * cols, min(K, (r0 + nr) * cols)
            if k0 >= K:
                break
            mosaic = cells.new_zeros(nr * cols, C, P, P)
            mosaic[:k1 - k0] = cells[k0:k1]
            image = mosaic.view(nr, cols, C, P, P).permute(2, 0, 3, 1, 4).reshape(1, C, nr * P, cols * P)
            m_img = None
            if valid is not None:
                m = cells.new_ones(nr * cols, 1, 2 * P, 2 * P)
                m[:k1 - k0] = valid[k0:k1]
                m_img = m.view(nr, cols, 1, 2 * P, 2 * P).permute(2, 0, 3, 1, 4).reshape(1, 1, nr * 2 * P, cols * 2 * P)
            res = self._last_block(block, image, m_img)
            res = res.view(C, nr, 2 * P, cols, 2 * P).permute(1, 3, 0, 2, 4).reshape(nr * cols, C, 2 * P, 2 * P)
            out[k0:k1] = res[:k1 - k0]
        return out


### Gaussian Splatting Renderer ###


SH_C0 = 0.28209479177387814  # 1 / (2 sqrt(pi)): the degree-0 basis function (graphic_utils.py:676)


def RGB2SH(rgb):
    """graphic_utils.py:764-765: the degree-0 coefficient whose colour is `rgb`."""
    return (rgb - 0.5) / SH_C0


def SH2RGB(sh):
    """graphic_utils.py:767-768: the colour of a degree-0 coefficient."""
    return sh * SH_C0 + 0.5


def _flat(t, width):
    return t.reshape(-1, t.shape[-2], width).float()


def _needs_grad(*tensors):
    """The differentiable rasterizer is taken only when autograd would record it; otherwise the inference path runs
    exactly as before."""
    return torch.is_grad_enabled() and any(t.requires_grad for t in tensors)


def render_multi_view(gaussians, K, E, args, bg_color=None, debug=False):
    """renderer.py:431-445: one Gaussian set per batch item, T cameras.  The views share the Gaussians through a
    zero frame stride instead of the reference's expand + reshape copy."""
    B, T = E.shape[0], E.shape[1]
    expanded = {k: v.unsqueeze(1).expand(-1, T, -1, -1) for k, v in gaussians.items()}
    if B == 1:
        expanded = {k: v[0] for k, v in expanded.items()}  # [T,N,D] with stride 0 over T: no copy
    else:
        expanded = {k: v.reshape(B * T, -1, v.shape[-1]) for k, v in expanded.items()}
    rendered = render_batch(expanded, K, E, args, bg_color, debug)
    return rendered.reshape(B, T, args.image_size[0], args.image_size[1], 3)


def render_batch(gaussians, K, E, args, bg_color=None, debug=False, return_alpha=False, workspace=None,
                 check_overflow=True, return_rgba=False, out_rgba=None, return_workspace=False, camera=None, wire=None,
                 decode=None, fuse_decode=None):
    """renderer.py:447-479: gaussians dict [(B*T),N,*], K [B,T,3,3], E [B,T,4,4] -> images [B,T,H,W,3] in [0,1].

    One camera launch + one rasterizer launch sequence for all B*T frames.  The returned image is a view of the
    kernel's RGBA output ([..., :3]); `return_alpha=True` also returns alpha [B,T,H,W] (= 1 - final transmittance);
    `return_rgba=True` returns the contiguous [B,T,H,W,4] buffer itself.
    Differentiable: when grad mode is on and a Gaussian attribute requires grad, the images (RGB and alpha) carry the
    rasterizer's backward (ops.rasterize_differentiable; bit-identical images).  `workspace`, `out_rgba`, `wire`,
    `decode` and `return_workspace` are refused then.
    `decode`, `fuse_decode`: ops.decode_source whose `out` the Gaussians view, decoded as part of the rasterizer's launch
    sequence (ops.rasterize).
    `args.rgb=False`: the reference's SH branch (renderer.py:540-545).  gaussians["color"] holds 3*K spherical-harmonic
    coefficients per Gaussian ([..., N, 3*K], coefficient-major, K >= (args.sh_degree+1)^2) and the colours are
    clamp_min(eval_sh + 0.5, 0) for each camera's centre (ops.sh_colors, not clamped at 1); the scale and opacity
    activations are then torch ops, since the rasterizer's own activation switch would clamp the colours at 1.  A
    caller's `camera=` must be the 4-tuple of ops.camera_from_intrinsics (with campos); `decode` is refused, because the
    decode writes 3 colour channels.  Under grad the colours carry ops.sh_colors_differentiable's backward.
    """
    sh_branch = not getattr(args, "rgb", True)
    B, T = E.shape[0], E.shape[1]
    H, W = int(args.image_size[0]), int(args.image_size[1])
    if sh_branch and (decode is not None or fuse_decode):
        raise AmavError("render_batch: decode= / fuse_decode= write 3 colour channels and cannot be combined with "
                        "args.rgb=False (spherical-harmonic colours)")
    campos = None
    if camera is None:
        view, proj, tanfov, campos = ops.camera_from_intrinsics(K.reshape(-1, 3, 3).float(), E.reshape(-1, 4, 4).float(),
                                                                H, W)
    elif sh_branch:
        if len(camera) != 4:
            raise AmavError("render_batch: args.rgb=False needs camera=(viewmatrix, projmatrix, tanfov, campos), the "
                            "4-tuple of ops.camera_from_intrinsics; the colours depend on the camera centre")
        view, proj, tanfov, campos = camera
    else:  # (viewmatrix, projmatrix, tanfov) already built from these K / E
        view, proj, tanfov = camera
    xyz, rot = _flat(gaussians["xyz"], 3), _flat(gaussians["rot"], 4)
    scale, opacity = _flat(gaussians["scale"], 3), _flat(gaussians["opacity"], 1)
    if xyz.shape[0] != B * T:
        raise AmavError(f"render_batch: {xyz.shape[0]} Gaussian sets for B*T = {B * T} cameras")
    bg = [1.0, 1.0, 1.0] if bg_color is None else [float(c) for c in bg_color]
    activate = True
    if debug and decode is not None:
        raise AmavError("render_batch: debug replaces the attributes; decode the Gaussians first")
    if sh_branch:
        degree, width = int(getattr(args, "sh_degree", 3)), gaussians["color"].shape[-1]
        need = (degree + 1) ** 2
        if width % 3 != 0 or width // 3 < need:
            raise AmavError(f"render_batch: args.rgb=False with sh_degree={degree} needs gaussians['color'] of 3 * K "
                            f"channels with K >= (sh_degree+1)^2 = {need} (eval_sh, graphic_utils.py:721-722); "
                            f"got {width} channels")
        sh = _flat(gaussians["color"], width)
        # renderer.py:532-537: the activations as torch ops (differentiable by autograd where a gradient is asked for)
        if debug:
            scale, opacity = torch.full_like(scale, 0.01), torch.full_like(opacity, 0.1)
        else:
            scale = torch.clamp_max(torch.exp(scale - ops.SCALE_BIAS), ops.SCALE_MAX)
            opacity = torch.sigmoid(opacity - ops.OPACITY_BIAS)
        activate = False
        if _needs_grad(xyz, rot, scale, opacity, sh):
            color = ops.sh_colors_differentiable(xyz, sh, campos, degree)
        else:
            color = ops.sh_colors(xyz, sh, campos, degree)
    else:
        color = _flat(gaussians["color"], 3)
        if debug:  # renderer.py:535-537
            scale = torch.full_like(scale, 0.01)
            opacity = torch.full_like(opacity, 0.1)
            color = color.clamp(0.0, 1.0)
            activate = False
    if _needs_grad(xyz, rot, scale, opacity, color):
        # differentiable path (ops.rasterize_differentiable): same images, owns its workspace
        refused = [n for n, v in (("workspace", workspace), ("out_rgba", out_rgba), ("wire", wire), ("decode", decode))
                   if v is not None] + (["return_workspace"] if return_workspace else [])
        if refused:
            raise NotImplementedError(f"render_batch: {', '.join(refused)} cannot be combined with gradients")
        out = ops.rasterize_differentiable(xyz, rot, scale, opacity, color, view, proj, tanfov, H, W, bg=bg,
                                           apply_activations=activate, clamp_output=True)
        rgba = out["rgba"].view(B, T, H, W, 4)
        if return_rgba:
            return rgba
        if return_alpha:
            return rgba[..., :3], rgba[..., 3]
        return rgba[..., :3]
    out = ops.rasterize(xyz, rot, scale, opacity, color, view, proj, tanfov, H, W, bg=bg, apply_activations=activate,
                        clamp_output=True, workspace=workspace, check_overflow=check_overflow, out_rgba=out_rgba, wire=wire,
                        decode=decode, fuse_decode=fuse_decode)
    rgba = out["rgba"].view(B, T, H, W, 4)
    if return_workspace:
        return rgba, out["workspace"]
    if return_rgba:
        return rgba
    if return_alpha:
        return rgba[..., :3], rgba[..., 3]
    return rgba[..., :3]


def render_one(xyzs, rots, scales, opacities, colors, K, E, args, bg_color=None, debug=False):
    """renderer.py:481-569: one frame -> [3,H,W] clamped to [0,1]."""
    g = {"xyz": xyzs[None], "rot": rots[None], "scale": scales[None], "opacity": opacities.reshape(1, -1, 1),
         "color": colors[None]}
    img = render_batch(g, K.reshape(1, 1, 3, 3), E.reshape(1, 1, 4, 4), args, bg_color, debug)
    return img[0, 0].permute(2, 0, 1)


# ---- op-level API of diff_gaussian_rasterization (renderer.py:516-566) --------------------------------------------
class GaussianRasterizationSettings:
    def __init__(self, image_height, image_width, tanfovx, tanfovy, bg, scale_modifier, viewmatrix, projmatrix,
                 sh_degree, campos, prefiltered, debug, antialiasing=False):
        self.image_height, self.image_width = int(image_height), int(image_width)
        self.tanfovx, self.tanfovy = float(tanfovx), float(tanfovy)
        self.bg, self.scale_modifier = bg, float(scale_modifier)
        self.viewmatrix, self.projmatrix = viewmatrix, projmatrix
        self.sh_degree, self.campos = sh_degree, campos
        self.prefiltered, self.debug, self.antialiasing = prefiltered, debug, antialiasing


class GaussianRasterizer(nn.Module):
    """`GaussianRasterizer(raster_settings)(means3D, means2D, shs, colors_precomp, opacities, scales, rotations,
    cov3D_precomp)` -> (color [3,H,W], radii [N] int32, inv_depth [1,H,W]); inputs already activated.

    The colours are either `colors_precomp` [N,3] or `shs` [N,K,3] (K >= (sh_degree+1)^2): spherical-harmonic
    coefficients evaluated at raster_settings.sh_degree from raster_settings.campos (ops.sh_colors); passing both or
    neither raises NotImplementedError.
    Differentiable in means3D, rotations, scales, opacities and colors_precomp / shs when grad mode is on and one of them
    requires grad (ops.rasterize_differentiable, ops.sh_colors_differentiable).  inv_depth and radii carry no gradient,
    and means2D is not used: its .grad stays None (no screen-space densification statistics)."""

    def __init__(self, raster_settings):
        super().__init__()
        self.raster_settings = raster_settings

    def forward(self, means3D, means2D=None, shs=None, colors_precomp=None, opacities=None, scales=None,
                rotations=None, cov3D_precomp=None):
        s = self.raster_settings
        if (colors_precomp is None) == (shs is None):
            raise NotImplementedError("pass either colors_precomp or shs, not both and not neither (as "
                                      "diff_gaussian_rasterization requires)")
        if cov3D_precomp is not None or scales is None or rotations is None:
            raise NotImplementedError("cov3D_precomp is not supported (the reference passes None, renderer.py:566)")
        dev = means3D.device
        if shs is not None:  # upstream's SH path: colours from shs [N,K,3] at settings.sh_degree, seen from settings.campos
            if s.campos is None:
                raise AmavError("GaussianRasterizer: shs= needs raster_settings.campos (the camera centre)")
            if shs.dim() != 3 or shs.shape[2] != 3:
                raise AmavError(f"GaussianRasterizer: shs {tuple(shs.shape)}, expected [N,K,3]")
            campos = s.campos.reshape(1, 3).float()
            if _needs_grad(means3D, shs):
                colors_precomp = ops.sh_colors_differentiable(means3D[None].float(), shs[None].float(), campos,
                                                              int(s.sh_degree))[0]
            else:
                colors_precomp = ops.sh_colors(means3D[None].float(), shs[None].float(), campos, int(s.sh_degree))[0]
        if _needs_grad(means3D, rotations, scales, opacities, colors_precomp):
            if s.antialiasing:
                raise NotImplementedError("the rasterizer has no backward for antialiasing=True")
            out = ops.rasterize_differentiable(
                means3D[None].float(), rotations[None].float(), scales[None].float(), opacities.reshape(1, -1, 1).float(),
                colors_precomp[None].float(), s.viewmatrix.reshape(1, 16).float(), s.projmatrix.reshape(1, 16).float(),
                torch.tensor([[s.tanfovx, s.tanfovy]], device=dev), s.image_height, s.image_width,
                bg=[float(b) for b in s.bg.detach().cpu().tolist()], scale_modifier=s.scale_modifier,
                want_inv_depth=True, want_radii=True)
            color = out["rgba"][0, :, :, :3].permute(2, 0, 1)
            return color, out["radii"][0], out["inv_depth"]
        out = ops.rasterize(means3D[None].float(), rotations[None].float(), scales[None].float(),
                            opacities.reshape(1, -1, 1).float(), colors_precomp[None].float(),
                            s.viewmatrix.reshape(1, 16).float(), s.projmatrix.reshape(1, 16).float(),
                            torch.tensor([[s.tanfovx, s.tanfovy]], device=dev), s.image_height, s.image_width,
                            bg=[float(b) for b in s.bg.detach().cpu().tolist()], scale_modifier=s.scale_modifier,
                            antialiasing=s.antialiasing, want_inv_depth=True, want_radii=True)
        color = out["rgba"][0, :, :, :3].permute(2, 0, 1)
        return color, out["radii"][0], out["inv_depth"]
