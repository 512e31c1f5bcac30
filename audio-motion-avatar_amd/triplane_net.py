"""Stage-1 identity encoder: reference image tokens + SMPL-X -> fused triplane / SMPL-X tokens -> rendered frame.

Mirror of `TriplaneGaussianAvatar` (src/models/lightning_model_wrapper.py:25-53) and of src/models/triplane_net.py
(`ResnetBlockFC` :16-58, `SMPLXTriplaneEncoder` :66-352, `FeatureFusionNetwork` :355-418), src/models/tokenizers.py
(`TriplaneLearnablePositionalEmbedding`) and src/models/image_feature.py:257-275 (`ImageFeature`): same classes,
constructor arguments, forward signatures, return tuples and parameter names, so the `triplane_gaussian.*` keys of a
reference checkpoint load.  SURVEY.md section 8(f) row 3 -- a "next row": it runs once per identity, so it is built for
correctness and determinism, on library kernels except where the reference's own operators are undefined on a GPU:

  * the Sapiens-1B image encoder (`sapiens_encoder`, a TorchScript file that is not available offline) is NOT part of
    this module: `forward` takes its output (`image_tokens [B,T,4096,1536]`) as an extra argument and raises when it is
    missing;
  * `torch_scatter.scatter_max / scatter_mean` (atomics: sum order undefined) -> deterministic segment reductions over
    points stably sorted by cell (csrc/splat.hip), with HIP backwards for stage-1 training (csrc/splat_backward.hip);
  * `points_projection` (pytorch3d point rasterizer + an index_put with duplicate indices: which pixel a point
    receives is undefined) -> z-buffer kernel with a fixed rule: the last pixel in (y, x) order that the point wins
    (what a sequential index_put does); with AMAV_STAGE1_SAMPLE=grid the image features are sampled from the 64 x 64
    token grid at those pixels only (ops.points_project_grid), without the [B*T,128,H,W] tensor of `ImageFeature`;
  * cross-attention to the 4096 image tokens and self-attention -> the fp16 x 2 MFMA kernels of csrc/attention.hip,
    forward and backward (transformer.py; AMAV_CROSS_ATTN=library keeps the library's fused attention for the former);
  * with cfg.upsample_triplane -- what the reference runs: renderer.yaml's `upsample_triplane: true` overrides
    triplane_net.yaml's false in the flattened config (config_loader.py:190-234) -- the encoder scatters into
    (R * upsample_factor)^2 cells and `TriplaneDownsampler` (:411-451: two ConvNeXtBlocks and a 4x4 stride-s convolution)
    brings the planes back to R^2: depthwise 7x7 + LayerNorm, bias + GELU and the convolution's patch gather are HIP
    kernels with HIP backwards (csrc/convnext.hip), its three matrix products per block go
    through transformer.linear / train_linear; AMAV_STAGE1_DOWNSAMPLER=library keeps the library's operators.

`densify_smplx_verts` here means "append the face centres" (:266-272), not the Renderer's subdivision.
"""
import math
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from ._lib import AmavError
from .body_model import BodyModel
from .renderer import Renderer
from .smplx_decoder import SMPLXDecoder
from .transformer import Transformer1D_nn, _memo, linear_presplit, split_gemm_ok, train_linear

POINT_RADIUS_NDC = 0.0075  # graphic_utils.py:280 (pytorch3d NDC: the shorter image side spans [-1, 1])


class ResnetBlockFC(nn.Module):
    """triplane_net.py:16-58."""

    def __init__(self, size_in, size_out=None, size_h=None):
        super().__init__()
        size_out = size_in if size_out is None else size_out
        size_h = min(size_in, size_out) if size_h is None else size_h
        self.size_in, self.size_h, self.size_out = size_in, size_h, size_out
        self.fc_0 = nn.Linear(size_in, size_h)
        self.fc_1 = nn.Linear(size_h, size_out)
        self.actvn = nn.ReLU()
        self.shortcut = None if size_in == size_out else nn.Linear(size_in, size_out, bias=False)
        nn.init.zeros_(self.fc_1.weight)

    def forward(self, x):
        net = self.fc_0(self.actvn(x))
        dx = self.fc_1(self.actvn(net))
        return (x if self.shortcut is None else self.shortcut(x)) + dx


class TriplaneLearnablePositionalEmbedding(nn.Module):
    """tokenizers.py: learnable [3,C,R,R] embedding added to the planes, flattened to tokens `B Ct (Np Hp Wp)`."""

    def __init__(self, num_channels=1024, plane_size=32):
        super().__init__()
        self.plane_size, self.num_channels = plane_size, num_channels
        self.embeddings = nn.Parameter(torch.randn(3, num_channels, plane_size, plane_size) / math.sqrt(num_channels))

    def forward(self, batch_size, cond_embeddings=None):
        e = self.embeddings.unsqueeze(0).expand(batch_size, -1, -1, -1, -1)
        if cond_embeddings is not None:
            e = e + cond_embeddings
        return e.permute(0, 2, 1, 3, 4).reshape(batch_size, self.num_channels, -1)

    def detokenize(self, tokens):
        B, Ct, Nt = tokens.shape
        assert Nt == self.plane_size ** 2 * 3 and Ct == self.num_channels
        return tokens.reshape(B, Ct, 3, self.plane_size, self.plane_size).permute(0, 2, 1, 3, 4)


class ImageFeature(nn.Module):
    """image_feature.py:257-275: Linear(1536 -> 125) on the 64x64 token grid, bilinear resize to the image, cat RGB."""

    def __init__(self, image_feature_dim=1536):
        super().__init__()
        self.feature_reducer = nn.Linear(image_feature_dim, 128 - 3)

    def reduce(self, feature):
        """feature [B,Nv,Nt,C] -> the reduced token grid [B*Nv, side, side, 125], channels-last as the Linear writes it
        (no permute, no resize): what ops.points_project_grid samples under the vertices (GridImageFeatures)."""
        B, Nv, Nt, C = feature.shape
        side = int(round(Nt ** 0.5))
        return self.feature_reducer(feature.reshape(B * Nv * Nt, C)).reshape(B * Nv, side, side, -1)

    def forward(self, rgb, feature):
        B, Nv, Nt, C = feature.shape
        H, W = rgb.shape[-2:]
        side = int(round(Nt ** 0.5))
        f = self.feature_reducer(feature.reshape(B * Nv * Nt, C)).reshape(B * Nv, side, side, -1).permute(0, 3, 1, 2)
        f = F.interpolate(f.contiguous(), size=(H, W), mode="bilinear", align_corners=False)
        return torch.cat([rgb.reshape(B * Nv, *rgb.shape[2:]), f], dim=1).reshape(B, Nv, -1, H, W)


class GridImageFeatures:
    """The image features of ImageFeature.forward before the resize: rgb [B,T,3,H,W] and the reduced token grid
    [B*T,Gh,Gw,125] (ImageFeature.reduce).  SMPLXTriplaneEncoder.forward takes it in place of the dense
    [B,T,128,H,W] tensor and samples the grid at the projected vertices' pixels only."""

    def __init__(self, rgb, grid):
        self.rgb, self.grid = rgb, grid


class ConvNeXtBlock(nn.Module):
    """triplane_net.py:411-429: x + pwconv2(gelu(pwconv1(LayerNorm(dwconv(x))))), the norm and the projections over the
    channels.  `forward` takes the reference's [B,C,H,W]; `forward_planes` channels-last planes [K,H,W,C], on the HIP
    kernels (hip=True) or the library's operators."""

    def __init__(self, dim):
        super().__init__()
        self.dwconv = nn.Conv2d(dim, dim, kernel_size=7, padding=3, groups=dim)
        self.norm = nn.LayerNorm(dim, eps=1e-6)
        self.pwconv1 = nn.Linear(dim, 4 * dim)
        self.act = nn.GELU()
        self.pwconv2 = nn.Linear(4 * dim, dim)

    def forward(self, x):
        return self.forward_planes(x.permute(0, 2, 3, 1), hip=False).permute(0, 3, 1, 2)

    def forward_planes(self, x, hip, grad=False):
        dw, norm, pw1, pw2 = self.dwconv, self.norm, self.pwconv1, self.pwconv2
        K, H, W, C = x.shape
        if not hip:
            y = F.conv2d(x.permute(0, 3, 1, 2), dw.weight, dw.bias, padding=3, groups=C).permute(0, 2, 3, 1)
            n = F.layer_norm(y, (C,), norm.weight, norm.bias, norm.eps)
            return F.linear(F.gelu(F.linear(n, pw1.weight, pw1.bias)), pw2.weight, pw2.bias) + x
        x = x.contiguous()
        if grad:
            n = ops.dwconv7_layernorm_differentiable(x, dw.weight, dw.bias, norm.weight, norm.bias, norm.eps)
            h = ops.gelu_bias_differentiable(train_linear(n, pw1.weight), pw1.bias)  # pwconv1's bias: added by the GELU pass
            return train_linear(h, pw2.weight, pw2.bias).view(K, H, W, C) + x
        args = (x, dw.weight, dw.bias, norm.weight, norm.bias, norm.eps)
        p = _linear_after(lambda split: ops.dwconv7_layernorm(*args, split=split), K * H * W, pw1.weight)
        return _linear_after(lambda split: ops.gelu_bias(p, pw1.bias, split=split), K * H * W, pw2.weight,
                             pw2.bias).view(K, H, W, C) + x


def _linear_after(rows_kernel, rows, weight, bias=None):
    """F.linear over the rows a HIP kernel produces, without autograd: where transformer.linear would take the bf16 x 3
    split GEMM (split_gemm_ok) the kernel writes the activation operand itself (rows_kernel(SPLIT_BF16X3)), so the rows
    never pass through HBM as fp32; elsewhere fp32 rows and the library's GEMM."""
    if split_gemm_ok(rows, weight.shape[1]):
        return linear_presplit(rows_kernel(ops.SPLIT_BF16X3), weight, bias)
    return F.linear(rows_kernel(None), weight, bias)


DOWNSAMPLER_DEFAULT = "hip"  # tools/bench_stage1_downsampler.py
DOWNSAMPLER_FRAMES_PER_PASS = 8  # frames (x 3 planes) per pass: the 4C hidden rows of a frame are 113 MB at C = 256, R = 96


class TriplaneDownsampler(nn.Module):
    """triplane_net.py:431-451: two ConvNeXtBlocks, then Conv2d(C, C, 4, stride=upsample_factor, padding=1), applied to
    every plane on its own.  Parameter names and layouts are the reference's (blocks.{0,1}.*, down.*).

    AMAV_STAGE1_DOWNSAMPLER, read per call: `hip` (the default) runs HIP fp32 planes of a width the kernels are built
    for (ops.dwconv7_channels_ok) on csrc/convnext.hip -- under autograd (grad=True) through the autograd Functions of
    ops, so every parameter and the input receive gradients; `library`, and every other input (CPU, other dtypes or
    widths), evaluates the same module with F.conv2d / F.layer_norm / F.gelu / F.linear."""

    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        self.scale = int(cfg.upsample_factor)
        if self.scale < 2:
            raise AmavError(f"TriplaneDownsampler: upsample_factor={cfg.upsample_factor} must be at least 2 (the 4x4 "
                            "padding-1 convolution returns R - 1 cells at stride 1)")
        C = cfg.triplane_feature_dim
        self.blocks = nn.ModuleList([ConvNeXtBlock(C) for _ in range(2)])
        self.down = nn.Conv2d(C, C, kernel_size=4, stride=self.scale, padding=1)

    def _hip(self, x):
        return (x.is_cuda and x.dtype == torch.float32 and self.down.weight.dtype == torch.float32
                and ops.dwconv7_channels_ok(x.shape[-1])
                and os.environ.get("AMAV_STAGE1_DOWNSAMPLER", DOWNSAMPLER_DEFAULT) != "library")

    def _down_weight(self):
        """down.weight [C_out, C_in, 4, 4] as the [C_out, 16 C_in] matrix of the tap-major patch rows, permuted once per
        version of the parameter."""
        w = self.down.weight
        return _memo("down_rows", (w,), lambda: w.detach().permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous())

    def forward_planes(self, x, grad=False):
        """x [K,H,W,C] channels-last planes -> [K,Ho,Wo,C]."""
        hip = self._hip(x)
        outs = []
        for part in x.split(3 * DOWNSAMPLER_FRAMES_PER_PASS):
            for blk in self.blocks:
                part = blk.forward_planes(part, hip, grad)
            K, H, W, C = part.shape
            if not hip:
                outs.append(F.conv2d(part.permute(0, 3, 1, 2), self.down.weight, self.down.bias, stride=self.scale,
                                     padding=1).permute(0, 2, 3, 1))
                continue
            Ho, Wo = ops.patch4_out_size(H, self.scale), ops.patch4_out_size(W, self.scale)
            if grad:
                w = self.down.weight.permute(0, 2, 3, 1).reshape(C, 16 * C)
                y = train_linear(ops.patch4_gather_differentiable(part, self.scale), w, self.down.bias,
                                 sources=(self.down.weight,))
            else:
                y = _linear_after(lambda split, part=part: ops.patch4_gather(part, self.scale, split=split), K * Ho * Wo,
                                  self._down_weight(), self.down.bias)
            outs.append(y.view(K, Ho, Wo, C))
        return outs[0] if len(outs) == 1 else torch.cat(outs)

    def forward(self, x, grad=None):
        """x [F,3,C,H,W] (the reference's layout) -> [F,3,C,H/s,W/s]; channels-last planes [K,H,W,C] -> [K,H/s,W/s,C].
        grad: whether the HIP path records an autograd graph (None: grad mode is on and the input or a parameter
        requires grad)."""
        if grad is None:
            grad = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))
        if x.dim() == 4:
            return self.forward_planes(x, grad)
        Fr, P, C, H, W = x.shape
        y = self.forward_planes(x.permute(0, 1, 3, 4, 2).reshape(Fr * P, H, W, C), grad)
        return y.view(Fr, P, *y.shape[1:]).permute(0, 1, 4, 2, 3)


class SMPLXTriplaneEncoder(nn.Module):
    """triplane_net.py:66-352: a posed SMPL-X mesh (+ per-vertex embedding, + image features under the projected
    vertices) -> PointNet with triplane-cell max pooling -> per-cell mean -> geometry triplanes [B,T,3,C,R,R].  With
    cfg.upsample_triplane the cells are those of an (R * upsample_factor)^2 grid and `triplane_downsampler` returns the
    planes to R^2 (:96-97, 176-205); self.triplane_resolution stays R (the reference multiplies and divides it on every
    call), and any number of frames B * T works (the reference's .squeeze(1) needs T = 1)."""

    def __init__(self, cfg, smpl_decoder=None):
        super().__init__()
        self.cfg = cfg
        self.triplane_resolution = cfg.triplane_resolution
        self.feature_dim = C = cfg.triplane_feature_dim
        self.smplx_model = self.init_smplx_model()
        faces = torch.as_tensor(self.smplx_model.faces.astype("int64"))
        self.register_buffer("_faces", faces, persistent=False)
        self.num_verts = self.smplx_model.num_verts + (faces.shape[0] if cfg.densify_smplx_verts else 0)
        self.fc_pos = nn.Linear(3 + C, 2 * C)
        self.blocks = nn.ModuleList([ResnetBlockFC(2 * C, C) for _ in range(3)])
        self.fc_c = nn.Linear(C, C)
        self.vertex_emb = nn.Embedding(self.num_verts, C // 2 if cfg.sample_feature else C)
        self.cell_resolution = self.triplane_resolution
        if getattr(cfg, "upsample_triplane", False):
            self.triplane_downsampler = TriplaneDownsampler(cfg)
            self.cell_resolution = self.triplane_resolution * self.triplane_downsampler.scale
        if cfg.predict_smplx_params:
            self.smpl_token_len, self.smpl_token_dim = cfg.smpl_token_len, cfg.smpl_token_dim
            self.smpl_tokens = nn.Parameter(torch.randn(self.smpl_token_dim, self.smpl_token_len))
            self.cross_attn = Transformer1D_nn(
                num_layers=cfg.smplx_transformer_layers, attention_head_dim=cfg.smplx_transformer_head_dim,
                in_channels=self.smpl_token_dim, num_attention_heads=cfg.smplx_transformer_num_heads,
                cross_attention_dim=cfg.image_feature_dim, norm_type="layer_norm", gradient_checkpointing=True)
            self.smpl_decoder = smpl_decoder
        self.actvn = nn.ReLU()

    def init_smplx_model(self):
        return BodyModel.create(getattr(self.cfg, "smplx_model_path", None), device=self.cfg.device, num_betas=10,
                                num_expression_coeffs=self.cfg.num_expression_coeffs,
                                flat_hand_mean=self.cfg.flat_hand_mean, seed=getattr(self.cfg, "body_seed", 42))

    # ---- :209-224
    def smpl_predictor(self, image_features):
        B, T, S, C = image_features.shape
        query = self.smpl_tokens.unsqueeze(0).repeat(B * T, 1, 1)
        tokens = self.cross_attn(query, image_features.reshape(B * T, S, C))
        params = self.smpl_decoder(tokens)
        for key, v in list(params.items()):
            params[key] = v.reshape(B, T, *v.shape[1:]) if key in ("body_pose", "left_hand_pose", "right_hand_pose") \
                else v.reshape(B, T, -1)
        return params, tokens

    # ---- :266-274 (LBS, then the face centres appended)
    def get_smplx_verts(self, smpl_params):
        B, T = smpl_params["global_orient"].shape[:2]
        r = lambda k: smpl_params[k].reshape(B * T, -1)
        vertices = self.smplx_model(global_orient=r("global_orient"), body_pose=r("body_pose"), betas=r("betas"),
                                    left_hand_pose=r("left_hand_pose"), right_hand_pose=r("right_hand_pose"),
                                    jaw_pose=r("jaw_pose"), leye_pose=r("leye_pose"), reye_pose=r("reye_pose"),
                                    expression=r("expression")).vertices
        if not self.cfg.densify_smplx_verts:
            return vertices
        centers = vertices[:, self._faces].mean(dim=2)
        return torch.cat([vertices, centers], dim=1)

    def cell_indices(self, verts):
        """:163-183: clamp to the cube, normalise to [0,1), cell = x + R * y for (x,y), (x,z), (y,z) -> int32 [BT,3,N]; R is
        the cell grid's resolution (triplane_resolution, times upsample_factor with upsample_triplane)."""
        R, rad = self.cell_resolution, self.cfg.radius
        pos = (torch.clamp(verts, -rad + 1e-6, rad - 1e-6) + rad) / (2 * rad)
        cells = []
        for a, b in ((0, 1), (0, 2), (1, 2)):
            x = (pos[..., [a, b]] * R).long()
            cells.append(torch.clamp(x[..., 0] + R * x[..., 1], 0, R * R - 1))
        return torch.stack(cells, dim=1).to(torch.int32)

    def _wants_grad(self, *tensors, smpl_params=None):
        """Autograd would record this call: grad mode is on and a parameter or one of the inputs requires grad."""
        if not torch.is_grad_enabled():
            return False
        tensors = tensors + tuple(v for v in (smpl_params or {}).values() if isinstance(v, torch.Tensor))
        return any(t is not None and t.requires_grad for t in tensors) or any(p.requires_grad for p in self.parameters())

    def forward(self, cam_params, img_tokens, smpl_params_gt=None, img=None):
        """Under autograd (grad mode on and a parameter or input requires grad) the three HIP reductions run as
        autograd Functions (ops.*_differentiable: the same values bit for bit, csrc/splat_backward.hip), so the point
        network, vertex_emb and the image features (with sample_feature) receive gradients; with predicted SMPL-X
        parameters the vertices carry them on to the predictor through BodyModel's LBS backward.  Neither the cell
        indices nor the projection's pixel selection carry a gradient.

        img: the dense image features [B,T,128,H,W] of ImageFeature.forward, or a GridImageFeatures (RGB + the reduced
        token grid), from which ops.points_project_grid samples the same 128 channels at the claimed pixels without the
        image-sized tensor or its gradient."""
        B, T, S, C = img_tokens.shape
        pred_smpl_params = smpl_tokens = None
        if self.cfg.predict_smplx_params:
            pred_smpl_params, smpl_tokens = self.smpl_predictor(img_tokens)
        smpl_params = smpl_params_gt if smpl_params_gt is not None else pred_smpl_params
        if smpl_params is None:
            raise AmavError("SMPLXTriplaneEncoder: no SMPL-X parameters (predict_smplx_params off, no smpl_params_gt)")
        from_grid = isinstance(img, GridImageFeatures)
        grad = self._wants_grad(img_tokens, *((img.rgb, img.grid) if from_grid else (img,)), smpl_params=smpl_params)
        project = ops.points_project_differentiable if grad else ops.points_project
        pool = ops.cell_pool_max_differentiable if grad else ops.cell_pool_max
        splat = ops.cell_splat_mean_differentiable if grad else ops.cell_splat_mean
        verts = self.get_smplx_verts(smpl_params)                                    # [BT, N, 3]
        verts_emb = self.vertex_emb.weight.unsqueeze(0).expand(verts.shape[0], -1, -1)
        if self.cfg.sample_feature:                                                  # :139-157
            rgb = img.rgb if from_grid else img
            Himg, Wimg = rgb.shape[-2:]
            pts = verts + smpl_params["transl"].reshape(B * T, 1, 3)
            camera = (pts.contiguous(), cam_params["extrinsic"].reshape(B * T, 4, 4).float(),
                      cam_params["intrinsic"].reshape(B * T, 3, 3).float())
            radius_px = POINT_RADIUS_NDC * min(Himg, Wimg) / 2.0
            if from_grid:  # channels as torch.cat([rgb, feature]): the resize is evaluated under the vertices only
                project = ops.points_project_grid_differentiable if grad else ops.points_project_grid
                sampled = project(*camera, rgb.reshape(B * T, *rgb.shape[2:]).float(), img.grid.float(), radius_px)
            else:
                sampled = project(*camera, img.reshape(B * T, *img.shape[2:]).float(), radius_px)
            verts_feat = torch.cat([verts_emb, sampled], dim=-1)
        else:
            verts_feat = verts_emb
        net = self.blocks[0](self.fc_pos(torch.cat([verts, verts_feat], dim=-1)))
        cell_of = self.cell_indices(verts)
        cells = self.cell_resolution ** 2
        segments = ops.cell_segments(cell_of, cells)
        for block in self.blocks[1:]:                                                # :185-188
            pooled = pool(net, cell_of, cells, segments)
            net = block(torch.cat([net, pooled], dim=2))
        c = self.fc_c(net)
        planes = [splat(c, cell_of[:, p].contiguous(), cells,
                        (segments[0][:, p].contiguous(), segments[1][:, p].contiguous()))
                  for p in range(3)]
        R = self.cell_resolution
        smplx_triplanes = torch.stack(planes, dim=1).view(B, T, 3, -1, R, R)
        if self.cell_resolution != self.triplane_resolution:                         # :202-205, for any B * T
            C = smplx_triplanes.shape[3]
            fine = smplx_triplanes.view(B * T * 3, C, R, R).permute(0, 2, 3, 1)      # channels-last planes [K,R,R,C]
            coarse = self.triplane_downsampler(fine, grad=grad)                      # [K,r,r,C]
            smplx_triplanes = coarse.permute(0, 3, 1, 2).reshape(B, T, 3, C, *coarse.shape[1:3])
        return smplx_triplanes, smpl_tokens, pred_smpl_params


class FeatureFusionNetwork(nn.Module):
    """triplane_net.py:355-418: geometry planes + positional embedding, SMPL-X tokens appended, 8 transformer layers
    with cross-attention to the image tokens; split back."""

    def __init__(self, cfg, feature_dim=64):
        super().__init__()
        self.cfg = cfg
        self.triplane_resolution, self.triplane_feature_dim = cfg.triplane_resolution, cfg.triplane_feature_dim
        self.triplane_tokenizer_geometry = TriplaneLearnablePositionalEmbedding(self.triplane_feature_dim,
                                                                                self.triplane_resolution)
        self.transformer_cross = Transformer1D_nn(
            num_layers=cfg.cross_transformer_layers, attention_head_dim=cfg.cross_transformer_head_dim,
            in_channels=self.triplane_feature_dim, num_attention_heads=cfg.cross_transformer_num_heads,
            cross_attention_dim=1536, norm_type="layer_norm",  # hard-coded in the reference too (:326)
            gradient_checkpointing=True)

    def forward(self, geometry_triplane, image_features, smpl_tokens):
        B, T, _, C, H, W = geometry_triplane.shape
        geo = geometry_triplane.reshape(B * T, 3, C, H, W)
        img = image_features.reshape(B * T, *image_features.shape[2:])
        geo_tokens = self.triplane_tokenizer_geometry(batch_size=B * T, cond_embeddings=geo)
        combined = torch.cat([geo_tokens, smpl_tokens], dim=2)
        out = self.transformer_cross(combined, img)
        tokens, smpl_out = torch.split(out, [geo_tokens.shape[2], smpl_tokens.shape[2]], dim=2)
        return tokens.reshape(B, T, *tokens.shape[1:]), smpl_out.reshape(B, T, *smpl_out.shape[1:])


STAGE1_SAMPLE_DEFAULT = "dense"  # `grid` becomes the default with measured numbers (tools/bench_stage1_sample.py)


class TriplaneGaussianAvatar(nn.Module):
    """lightning_model_wrapper.py:25-53.  `cfg`: the flattened model config (config.RendererConfig + the stage-1
    fields below, or any object with those attributes).  The Sapiens encoder is external: pass its tokens."""

    def __init__(self, cfg=None):
        super().__init__()
        self.cfg = cfg
        self.sapiens_encoder = None  # TorchScript Sapiens-1B in the reference (lightning_model_wrapper.py:33)
        self.image_feature = ImageFeature(getattr(cfg, "image_feature_dim", 1536))
        self.smplx_decoder = SMPLXDecoder(cfg)
        self.smplx_triplane_encoder = SMPLXTriplaneEncoder(cfg, self.smplx_decoder)
        self.fusion_network = FeatureFusionNetwork(cfg)
        self.renderer = Renderer(cfg, self.smplx_decoder)
        self.to(cfg.device)

    def forward(self, img, smpl_params_gt, cam_params, image_tokens=None):
        """img [B,T,3,H,W], smpl_params_gt dict of [B,T,...] (or None), cam_params dict -> the reference's 7-tuple
        (rendered_images, gaussians, fused_triplane_tokens, image_tokens, pred_smpl_1, pred_smpl_2, smpl_tokens).

        AMAV_STAGE1_SAMPLE, read per call: `dense` (the default) builds the reference's [B,T,128,H,W] image features
        (ImageFeature.forward) for the encoder to look up; `grid` hands it RGB and the reduced token grid
        (GridImageFeatures) and never evaluates ImageFeature.forward -- with cfg.sample_feature off it reduces and
        samples nothing at all."""
        mode = os.environ.get("AMAV_STAGE1_SAMPLE", STAGE1_SAMPLE_DEFAULT)
        if mode not in ("dense", "grid"):
            raise AmavError(f"AMAV_STAGE1_SAMPLE={mode!r}: expected `dense` or `grid`")
        B, T = img.shape[:2]
        if image_tokens is None:
            if self.sapiens_encoder is None:
                raise AmavError("TriplaneGaussianAvatar.forward: the Sapiens image encoder is not part of this build "
                                "(its TorchScript checkpoint is not available offline); pass image_tokens "
                                "[B,T,4096,image_feature_dim]")
            image_tokens = self.sapiens_encoder(img.reshape(B * T, *img.shape[2:]))
        image_tokens = image_tokens.reshape(B, T, -1, image_tokens.shape[-1])
        if mode == "dense":
            image_features = self.image_feature(img, image_tokens)
        elif self.cfg.sample_feature:
            image_features = GridImageFeatures(img, self.image_feature.reduce(image_tokens))
        else:
            image_features = None
        smplx_triplane, smpl_tokens, pred_smpl_1 = self.smplx_triplane_encoder(cam_params, image_tokens, smpl_params_gt,
                                                                              image_features)
        fused_tokens, smpl_tokens = self.fusion_network(smplx_triplane, image_tokens, smpl_tokens)
        rendered_images, gaussians, pred_smpl_2 = self.renderer(fused_tokens, cam_params, smpl_tokens, smpl_params_gt)
        return rendered_images, gaussians, fused_tokens, image_tokens, pred_smpl_1, pred_smpl_2, smpl_tokens

    def training_step(self, ref_images, smpl_params, cam_params, image_tokens, test_images=None, test_cam_params=None):
        """lightning_model_wrapper.py:82-170 (`TriplaneGaussianAvatarLightning.training_step`): renders the reference
        views, and the test views from the same Gaussians (render_multi_view), and returns (total, parts) with

            total = l1_train + 0.1 * ssim_train + (l1_test + 0.1 * ssim_test)
                    + 0.01 * (training_smplx_term(pred_smpl_1, smpl_params) + training_smplx_term(pred_smpl_2, smpl_params))

        ref_images / test_images [B,T,3,H,W] in [0,1], smpl_params the ground-truth dict of [B,T,...], cam_params /
        test_cam_params the camera dicts, image_tokens [B,T,4096,image_feature_dim] (the Sapiens output, from the
        caller as for forward).  parts: l1_train, ssim_train (= 1 - ssim), l1_test, ssim_test (0 without test images),
        loss_smplx.  Call total.backward() for the gradients.  The image terms come from the fused HIP loss
        (losses.image_losses); AMAV_IMAGE_LOSS=library, read per call, keeps the library's l1_loss and ssim.
        training_smplx_term is smplx_param_loss(...)[0], or with AMAV_SMPLX_PARAMS=hip (read per call) the fused
        losses.smplx_param_losses.

        Every stage-1 parameter receives a gradient: ImageFeature.feature_reducer, the point network (fc_pos, blocks,
        fc_c) and vertex_emb through the HIP backwards of the encoder's reductions, the SMPL-X predictor (smpl_tokens,
        cross_attn) and the shared SMPL-X decoder through the parameter loss and the SMPL-X tokens, the fusion network,
        and the renderer's decoder heads.  The reference renders with the ground-truth parameters, so LBS sits outside
        the graph here.  The step runs in the module's current mode; .eval() and .train() differ only in the
        transformers' dropout, which is 0 at the reference's settings."""
        from .losses import training_image_terms, training_smplx_term
        from .renderer import render_multi_view

        rendered, gaussians, _, _, pred_smpl_1, pred_smpl_2, _ = self(ref_images, smpl_params, cam_params, image_tokens)
        parts = dict(zip(("l1_train", "ssim_train"), training_image_terms(rendered, ref_images.permute(0, 1, 3, 4, 2))))
        if test_images is not None:
            B, T = test_images.shape[:2]
            args = type("Args", (), {"image_size": self.cfg.image_size, "rgb": True, "sh_degree": 3})()
            target = render_multi_view(gaussians, test_cam_params["intrinsic"].reshape(B, T, 3, 3),
                                       test_cam_params["extrinsic"].reshape(B, T, 4, 4), args)
            parts["l1_test"], parts["ssim_test"] = training_image_terms(target, test_images.permute(0, 1, 3, 4, 2))
        else:
            parts["l1_test"] = torch.zeros((), device=rendered.device)
            parts["ssim_test"] = torch.zeros((), device=rendered.device)
        parts["loss_smplx"] = training_smplx_term(pred_smpl_1, smpl_params) + training_smplx_term(pred_smpl_2, smpl_params)
        total = (parts["l1_train"] + 0.1 * parts["ssim_train"] + (parts["l1_test"] + 0.1 * parts["ssim_test"])
                 + 0.01 * parts["loss_smplx"])
        return total, parts

    def configure_optimizers(self, lr=1e-4, total_steps=200000, max_grad_norm=1.0, process_group=None):
        """lightning_model_wrapper.py:366-382 (`TriplaneGaussianAvatarLightning.configure_optimizers`: Adam over
        self.parameters(), LinearLR from 1.0 to 0.01 over the run's steps, stepped every step) with the Trainer's
        gradient_clip_val = 1.0 (trainer_factory.py:44-45) inside the optimizer's step: returns (optim.Adam over the
        parameters that require grad, the LinearLR scheduler); see AudioDrivenAvatar.configure_optimizers.
        process_group: a torch.distributed group for the data-parallel step of optim.Adam; None: one process."""
        from .optim import configure_optimizers

        return configure_optimizers(self, lr, total_steps, max_grad_norm, process_group)
