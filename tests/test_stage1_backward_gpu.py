"""HIP backwards of the stage-1 encoder's reductions (csrc/splat_backward.hip) on the MI355X: pool_local against fp64
with explicit arg routing (lowest point id wins a tie), the mean and projection backwards bitwise against fp32
restatements, run-to-run and frame-slicing determinism, and the encoder + ImageFeature end to end against fp64
autograd of the CPU oracle."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from helpers import ref_fixture, toy_body

pytestmark = pytest.mark.gpu


def _cells(B, N, R, seed):
    """cell_of int32 [B,3,N] from vertices with points clamped onto the cube's faces, a one-point cell and empty cells."""
    from oracle import triplane_net as o_tn

    g = torch.Generator().manual_seed(seed)
    verts = torch.randn(B, N, 3, generator=g) * 0.35
    verts[:, 0] = torch.tensor([1.4, -1.4, 1.4])        # on the faces / corners: clamped
    verts[:, 1] = torch.tensor([5.0, 0.0, -5.0])
    verts[:, 2] = torch.tensor([-1.39, 1.39, -1.39])     # alone in its corner cells
    index = o_tn.cell_indices(verts, 1.4, R)
    return torch.stack([index[k][:, 0] for k in ("xy", "xz", "yz")], dim=1).to(torch.int32)


def _pool_grad_fp64(feat, cell_of, cells, dout):
    """dfeat of pool_local in fp64 with explicit routing: per plane, the cell's summed dout goes to the lowest point id
    that holds the cell's maximum."""
    B, N, C = feat.shape
    f, g = feat.double(), dout.double()
    ids = torch.arange(N).view(1, N, 1).expand(B, N, C)
    out = torch.zeros(B, N, C, dtype=torch.float64)
    for p in range(3):
        idx = cell_of[:, p].long().unsqueeze(-1).expand(B, N, C)
        cmax = torch.full((B, cells, C), -float("inf"), dtype=torch.float64).scatter_reduce(1, idx, f, "amax")
        holds = f == cmax.gather(1, idx)
        cand = torch.where(holds, ids, torch.full_like(ids, N))
        arg = torch.full((B, cells, C), N, dtype=torch.long).scatter_reduce(1, idx, cand, "amin")
        S = torch.zeros(B, cells, C, dtype=torch.float64).scatter_add(1, idx, g)
        out += torch.where(arg.gather(1, idx) == ids, S.gather(1, idx), torch.zeros_like(f))
    return out


@pytest.mark.parametrize("C", [7, 48, 64, 260])
def test_pool_local_backward_routes_to_the_lowest_id_and_matches_fp64(C):
    from audio_motion_avatar_amd import ops

    B, N, R = 2, 700, 6
    cells = R * R
    cell_of = _cells(B, N, R, seed=C)
    g = torch.Generator().manual_seed(100 + C)
    feat = torch.randn(B, N, C, generator=g)
    feat[:, ::2] = torch.randint(-2, 3, (B, (N + 1) // 2, C), generator=g).float()  # integer values: many ties
    dout = torch.randn(B, N, C, generator=g)
    want = _pool_grad_fp64(feat, cell_of, cells, dout)
    segs = ops.cell_segments(cell_of.cuda(), cells)
    got = ops.cell_pool_max_backward(feat.cuda(), cell_of.cuda(), cells, segs, dout.cuda())
    err = float((got.cpu().double() - want).abs().max())
    scale = float(want.abs().max())
    print(f"pool_local backward C={C}: max abs err {err:.3e} of max {scale:.3g} ({err / scale:.2e})")
    assert err <= 1e-5 * scale
    # every cell's gradient lands on exactly one point per (plane, channel): no split among ties
    assert torch.equal(got, ops.cell_pool_max_backward(feat.cuda(), cell_of.cuda(), cells, segs, dout.cuda()))
    one = torch.cat([ops.cell_pool_max_backward(feat[b:b + 1].cuda(), cell_of[b:b + 1].cuda(), cells,
                                                (segs[0][b:b + 1], segs[1][b:b + 1]), dout[b:b + 1].cuda())
                     for b in range(B)])
    assert torch.equal(got, one)
    # through autograd: the forward under grad equals the no-grad forward, the gradient equals the direct call
    x = feat.cuda().requires_grad_()
    y = ops.cell_pool_max_differentiable(x, cell_of.cuda(), cells, segs)
    assert torch.equal(y.detach(), ops.cell_pool_max(feat.cuda(), cell_of.cuda(), cells, segs))
    y.backward(dout.cuda())
    assert torch.equal(x.grad, got)


def test_pool_local_backward_tie_rule_on_a_hand_built_cell():
    from audio_motion_avatar_amd import ops

    # 5 points, all in cell 0 of every plane: channel 0 ties at points 1, 3; channel 1 has one max at point 4
    feat = torch.tensor([[[0.0, 1.0], [2.0, 1.0], [1.0, 1.0], [2.0, 1.0], [-1.0, 3.0]]])
    cell_of = torch.zeros(1, 3, 5, dtype=torch.int32)
    dout = torch.tensor([[[1.0, 10.0], [2.0, 20.0], [3.0, 30.0], [4.0, 40.0], [5.0, 50.0]]])
    got = ops.cell_pool_max_backward(feat.cuda(), cell_of.cuda(), 4, ops.cell_segments(cell_of.cuda(), 4),
                                     dout.cuda()).cpu()
    want = torch.zeros(1, 5, 2)
    want[0, 1, 0] = 3 * 15.0   # three planes, each routes the whole sum 1+2+3+4+5 to point 1
    want[0, 4, 1] = 3 * 150.0
    assert torch.equal(got, want)


@pytest.mark.parametrize("C", [7, 48, 64, 260])
def test_generate_plane_features_backward_is_bitwise_the_fp32_restatement(C):
    from audio_motion_avatar_amd import ops

    B, N, R = 2, 700, 6
    cells = R * R
    cell_of = _cells(B, N, R, seed=C)[:, 1].contiguous()
    g = torch.Generator().manual_seed(200 + C)
    dplane = torch.randn(B, C, cells, generator=g)
    count = torch.stack([torch.bincount(cell_of[b].long(), minlength=cells) for b in range(B)])  # [B, cells]
    assert bool((count == 0).any()) and bool((count == 1).any())
    idx = cell_of.long()
    want = (dplane.gather(2, idx.unsqueeze(1).expand(B, C, N)) / count.gather(1, idx).float().unsqueeze(1)).permute(0, 2, 1)
    segs = ops.cell_segments(cell_of.cuda(), cells)
    got = ops.cell_splat_mean_backward(dplane.cuda(), cells, segs, N)
    assert torch.equal(got.cpu(), want)
    assert torch.equal(got, ops.cell_splat_mean_backward(dplane.cuda(), cells, segs, N))
    one = torch.cat([ops.cell_splat_mean_backward(dplane[b:b + 1].cuda(), cells, (segs[0][b:b + 1], segs[1][b:b + 1]), N)
                     for b in range(B)])
    assert torch.equal(got, one)
    feat = torch.randn(B, N, C, generator=g).cuda().requires_grad_()
    y = ops.cell_splat_mean_differentiable(feat, cell_of.cuda(), cells, segs)
    assert torch.equal(y.detach(), ops.cell_splat_mean(feat.detach(), cell_of.cuda(), cells, segs))
    y.backward(dplane.cuda())
    assert torch.equal(feat.grad, got)


def winner_map(points, w2c, intrinsics, H, W, radius_px):
    """The z-buffer of oracle.triplane_net.points_projection (the same fp32 arithmetic) -> winner ids int64 [B,H,W],
    -1 where no point covers the pixel."""
    B, N, _ = points.shape
    f32 = np.float32
    out = np.full((B, H, W), -1, dtype=np.int64)
    for b in range(B):
        zbuf = np.full((H, W), np.inf, dtype=np.float32)
        Ef, Kf, Pf = (w2c[b].numpy().astype(f32), intrinsics[b].numpy().astype(f32), points[b].numpy().astype(f32))
        for n in range(N):
            p = Pf[n]
            X = f32(f32(f32(Ef[0, 0] * p[0]) + f32(Ef[0, 1] * p[1])) + f32(Ef[0, 2] * p[2])) + Ef[0, 3]
            Y = f32(f32(f32(Ef[1, 0] * p[0]) + f32(Ef[1, 1] * p[1])) + f32(Ef[1, 2] * p[2])) + Ef[1, 3]
            Z = f32(f32(f32(Ef[2, 0] * p[0]) + f32(Ef[2, 1] * p[1])) + f32(Ef[2, 2] * p[2])) + Ef[2, 3]
            if not Z > 0:
                continue
            u, v = f32(f32(Kf[0, 0] * X) / Z) + Kf[0, 2], f32(f32(Kf[1, 1] * Y) / Z) + Kf[1, 2]
            r, half = f32(radius_px), f32(0.5)
            x0, x1 = max(0, int(np.ceil(f32(f32(u - r) - half)))), min(W - 1, int(np.floor(f32(f32(u + r) - half))))
            y0, y1 = max(0, int(np.ceil(f32(f32(v - r) - half)))), min(H - 1, int(np.floor(f32(f32(v + r) - half))))
            for y in range(y0, y1 + 1):
                for x in range(x0, x1 + 1):
                    dx, dy = f32(f32(f32(x) + half) - u), f32(f32(f32(y) + half) - v)
                    if f32(f32(dx * dx) + f32(dy * dy)) < f32(r * r) and (
                            Z < zbuf[y, x] or (Z == zbuf[y, x] and n < out[b, y, x])):
                        zbuf[y, x], out[b, y, x] = Z, n
    return torch.from_numpy(out)


def _projection_case(C, seed=1):
    g = torch.Generator().manual_seed(seed)
    B, N, H, W = 2, 300, 40, 56
    pts = torch.randn(B, N, 3, generator=g) * torch.tensor([0.5, 0.4, 0.3]) + torch.tensor([0.0, 0.0, 2.0])
    pts[:, :3, 2] = -1.0                                   # behind the camera
    pts[:, 3:6, 0] = 40.0                                  # off the image
    E = torch.eye(4).repeat(B, 1, 1)
    E[1, :3, 3] = torch.tensor([0.1, -0.05, 0.2])
    K = torch.tensor([[60.0, 0, W / 2], [0, 62.0, H / 2], [0, 0, 1]]).repeat(B, 1, 1)
    feat = torch.randn(B, C, H, W, generator=g)
    return pts, E, K, feat, 2.5


@pytest.mark.parametrize("C", [7, 48, 64, 260])
def test_points_projection_backward_is_bitwise_index_put_credit(C):
    from audio_motion_avatar_amd import ops

    pts, E, K, feat, r = _projection_case(C)
    B, N = pts.shape[:2]
    H, W = feat.shape[2:]
    win = winner_map(pts, E, K, H, W, r)
    per_point = torch.stack([torch.bincount(win[b][win[b] >= 0], minlength=N) for b in range(B)])
    assert int(per_point.max()) >= 3 and bool((per_point[:, :6] == 0).all())  # several pixels per point; culled ones
    dout = torch.randn(B, N, C, generator=torch.Generator().manual_seed(7))
    want = torch.zeros(B, C, H, W)
    for b in range(B):
        hit = win[b] >= 0
        want[b][:, hit] = dout[b][win[b][hit]].t()
    x = feat.cuda().requires_grad_()
    y = ops.points_project_differentiable(pts.cuda(), E.cuda(), K.cuda(), x, r)
    assert torch.equal(y.detach(), ops.points_project(pts.cuda(), E.cuda(), K.cuda(), feat.cuda(), r))
    y.backward(dout.cuda())
    assert torch.equal(x.grad.cpu(), want)
    x2 = feat.cuda().requires_grad_()
    ops.points_project_differentiable(pts.cuda(), E.cuda(), K.cuda(), x2, r).backward(dout.cuda())
    assert torch.equal(x2.grad, x.grad)
    for b in range(B):
        xb = feat[b:b + 1].cuda().requires_grad_()
        ops.points_project_differentiable(pts[b:b + 1].cuda(), E[b:b + 1].cuda(), K[b:b + 1].cuda(), xb, r).backward(
            dout[b:b + 1].cuda())
        assert torch.equal(xb.grad, x.grad[b:b + 1])


class _IndexPutFp64(torch.autograd.Function):
    """The reference's `proj[points_to_visible_pixels] = features[visible_pixels]` in fp64 given the winner map:
    forward keeps the last won pixel in (y, x) order, backward credits every won pixel (index_put's autograd)."""

    @staticmethod
    def forward(ctx, feat, win, N):
        B, C, H, W = feat.shape
        out = feat.new_zeros(B, N, C)
        for b in range(B):
            flat = win[b].reshape(-1)
            pix = torch.nonzero(flat >= 0)[:, 0]
            last = torch.full((N,), -1, dtype=torch.long).scatter_reduce(0, flat[pix], pix, "amax")
            got = last >= 0
            out[b][got] = feat[b].reshape(C, -1)[:, last[got]].t()
        ctx.save_for_backward(win)
        ctx.shape = feat.shape
        return out

    @staticmethod
    def backward(ctx, grad):
        (win,) = ctx.saved_tensors
        B, C, H, W = ctx.shape
        g = grad.new_zeros(B, C, H, W)
        for b in range(B):
            hit = win[b] >= 0
            g[b][:, hit] = grad[b][win[b][hit]].t()
        return g, None, None


def test_encoder_and_image_feature_gradients_match_fp64_autograd_of_the_oracle():
    """SMPLXTriplaneEncoder (sample_feature=True, C = 256 as the image features require) + ImageFeature under autograd
    against fp64 autograd of oracle.triplane_net.image_feature / encoder_forward, with the projection restated as an
    fp64 index_put (the oracle's slice assignment credits only the last pixel)."""
    from audio_motion_avatar_amd.smplx_decoder import SMPLXDecoder
    from audio_motion_avatar_amd.triplane_net import POINT_RADIUS_NDC, ImageFeature, SMPLXTriplaneEncoder
    from oracle import triplane_net as o_tn

    a, meta, _ = ref_fixture("stage1")
    body = toy_body(**meta["toy_body"]).cuda()
    cfg = SimpleNamespace(**dict(meta["cfg"], sample_feature=True, predict_smplx_params=False, triplane_feature_dim=256,
                                 triplane_resolution=4, device="cuda"))

    class Encoder(SMPLXTriplaneEncoder):
        def init_smplx_model(self):
            return body

    torch.manual_seed(3)
    enc = Encoder(cfg, SMPLXDecoder(cfg)).cuda()
    imf = ImageFeature(1536).cuda()
    with torch.no_grad():
        for blk in enc.blocks:
            blk.fc_1.weight.normal_(0, 0.05)
    smpl = {k[5:]: v.cuda() for k, v in a.items() if k.startswith("pred_")}
    B, T = 1, 2
    H, W = 96, 128
    r = POINT_RADIUS_NDC * min(H, W) / 2.0
    with torch.no_grad():
        verts = enc.get_smplx_verts(smpl)
    pts = (verts + smpl["transl"].reshape(B * T, 1, 3)).cpu()
    centre, extent = pts.mean(dim=(0, 1)), float((pts - pts.mean(dim=(0, 1))).abs().max())
    E = torch.eye(4).repeat(B * T, 1, 1)
    E[:, :3, 3] = -centre + torch.tensor([0.0, 0.0, 3.0 * extent])
    E[1, 0, 3] += 0.05 * extent
    K = torch.tensor([[1.0 * W, 0, W / 2], [0, 1.0 * W, H / 2], [0, 0, 1]]).repeat(B * T, 1, 1)
    cam = {"intrinsic": K.view(B, T, 3, 3).cuda(), "extrinsic": E.view(B, T, 4, 4).cuda()}
    g = torch.Generator().manual_seed(11)
    rgb = torch.rand(B, T, 3, H, W, generator=g)
    tokens = torch.randn(B, T, 16, 1536, generator=g)
    G = torch.randn(B, T, 3, 256, 4, 4, generator=g)

    feats = imf(rgb.cuda(), tokens.cuda())
    planes, _, _ = enc(cam, tokens.cuda(), smpl, feats)
    (planes * G.cuda()).sum().backward()

    # fp64 oracle
    p = {k: v.detach().cpu().double().requires_grad_() for k, v in
         list({"enc." + k: v for k, v in enc.named_parameters()}.items()) +
         list({"imf." + k: v for k, v in imf.named_parameters()}.items())}
    feats64 = o_tn.image_feature(p, "imf.", rgb.double(), tokens.double()).reshape(B * T, 128, H, W)
    win = winner_map(pts, E, K, H, W, r)
    assert int((win >= 0).sum()) > 20
    sampled = _IndexPutFp64.apply(feats64, win, pts.shape[1])
    assert bool((sampled != 0).any(-1).sum() > 5)
    vf = torch.cat([p["enc.vertex_emb.weight"].unsqueeze(0).expand(B * T, -1, -1), sampled], dim=-1)
    v64 = verts.cpu().double()
    index = o_tn.cell_indices(v64, cfg.radius, 4)
    assert torch.equal(torch.stack([index[k][:, 0] for k in ("xy", "xz", "yz")], 1).int(), enc.cell_indices(verts).cpu())
    planes64 = o_tn.encoder_forward(p, "enc.", v64, vf, cfg.radius, 4)
    with torch.no_grad():
        diff = (planes.cpu().double().view_as(planes64) - planes64).abs().max()
        assert float(diff) <= 1e-4 * float(planes64.abs().max())
    (planes64 * G.double().view_as(planes64)).sum().backward()

    checked = 0
    for name, mod in (("enc.", enc), ("imf.", imf)):
        for k, prm in mod.named_parameters():
            want = p[name + k].grad
            if want is None:  # the SMPL-X decoder inside the encoder is not on this path
                assert prm.grad is None or not bool(prm.grad.any()), k
                continue
            got = prm.grad.detach().cpu().double()
            scale = float(want.abs().max())
            err = float((got - want).abs().max())
            print(f"{name}{k}: max abs err {err:.3e} of max {scale:.3g}")
            assert scale > 0, k
            assert err <= 1e-4 * scale, (k, err, scale)
            checked += 1
    assert checked >= 13  # fc_pos, 3 blocks x (fc_0, fc_1 w/b, shortcut), fc_c, vertex_emb, feature_reducer
