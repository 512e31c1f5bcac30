"""amav_points_project_grid and its backward on the MI355X (csrc/splat.hip, csrc/splat_backward.hip): the image features
sampled from the token grid at the claimed pixels, and their gradient gathered straight into the grid.  Expectations
are the CPU restatements and fp64 models of tests/project_grid_cases.py (held to the oracle by
tests/test_project_grid_model.py) and the existing dense path on the GPU (F.interpolate + ops.points_project), never the
new code itself.  The bounds are derived there from u = 2**-24, not measured."""
import pytest
import torch
import torch.nn.functional as F

import project_grid_cases as pc
import stage1_splat_cases as sc

pytestmark = pytest.mark.gpu


def bitwise(a, b):
    a, b = a.cpu(), b.cpu()
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _camera(c, b=None):
    s = c["scene"]
    cut = (lambda t: t.cuda()) if b is None else (lambda t: t[b:b + 1].cuda())
    return cut(s["points"]), cut(s["w2c"]), cut(s["K"])


def _dense(c, rgb, grid):
    """the parent's path: the dense [B,3+Cg,H,W] tensor of ImageFeature.forward"""
    s = c["scene"]
    f = F.interpolate(grid.permute(0, 3, 1, 2).contiguous(), size=(s["H"], s["W"]), mode="bilinear", align_corners=False)
    return torch.cat([rgb, f], dim=1)


@pytest.mark.parametrize("key", pc.CASES, ids=pc.case_id)
def test_forward(key):
    from audio_motion_avatar_amd import ops

    c = pc.case(key)
    r = c["scene"]["radius_px"]
    rgb, grid = c["rgb"].cuda(), c["grid"].cuda()
    got = ops.points_project_grid(*_camera(c), rgb, grid, r)
    assert torch.equal((got.cpu() != 0).any(-1), c["pixel_of"] >= 0)                # zero rows exactly where -1
    assert bitwise(got[..., :3].contiguous(), sc.expected_features(c["rgb"], c["pixel_of"]))
    assert bitwise(got, pc.forward_fp32(c["rgb"], c["grid"], c["pixel_of"]))
    want, bound = pc.forward_fp64(c["rgb"], c["grid"], c["pixel_of"])
    err = (got.cpu().double() - want).abs()
    assert bool((err <= bound).all())
    dense = ops.points_project(*_camera(c), _dense(c, rgb, grid), r)
    assert bitwise(got[..., :3].contiguous(), dense[..., :3].contiguous())
    assert torch.equal((got != 0).any(-1), (dense != 0).any(-1))
    diff = (got - dense).cpu().double().abs()
    print(f"{pc.case_id(key)}: error / bound against fp64 {float((err / bound.clamp_min(1e-300)).max()):.3f}, against "
          f"the dense path {float((diff / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((diff <= bound).all())
    if (c["Gh"], c["Gw"]) == c["ids"].shape[1:]:                                     # identity scale: the node itself
        nodes = c["grid"].permute(0, 3, 1, 2).contiguous()
        assert bitwise(got[..., 3:].contiguous(), sc.expected_features(nodes, c["pixel_of"]))
    # determinism: two runs, and B frames against B calls
    assert bitwise(got, ops.points_project_grid(*_camera(c), rgb, grid, r))
    one = torch.cat([ops.points_project_grid(*_camera(c, b), rgb[b:b + 1], grid[b:b + 1], r) for b in range(rgb.shape[0])])
    assert bitwise(got, one)
    # under autograd: the same bits
    leaf = grid.clone().requires_grad_()
    with_grad = ops.points_project_grid_differentiable(*_camera(c), rgb, leaf, r)
    assert with_grad.requires_grad and bitwise(with_grad.detach(), got)


@pytest.mark.parametrize("key", pc.CASES, ids=pc.case_id)
def test_backward(key):
    from audio_motion_avatar_amd import ops

    c = pc.case(key)
    s = c["scene"]
    r, H, W = s["radius_px"], s["H"], s["W"]
    B = c["rgb"].shape[0]
    rgb, dout = c["rgb"].cuda(), c["dout"].cuda()
    grid = c["grid"].cuda().requires_grad_()
    out, ws = ops._points_project_grid(*_camera(c), rgb, grid.detach(), r)
    got, got_rgb = ops.points_project_grid_backward(dout, ws, grid.shape, H, W, want_rgb=True)
    want, bound = pc.backward_fp64(c["dout"], c["ids"], c["Gh"], c["Gw"])
    err = (got.cpu().double() - want).abs()
    assert bool((err <= bound).all())
    # the parent's path on the GPU: F.interpolate under autograd + ops.points_project_differentiable
    rgb_leaf = rgb.clone().requires_grad_()
    ops.points_project_differentiable(*_camera(c), _dense(c, rgb_leaf, grid), r).backward(dout)
    diff = (got - grid.grad).cpu().double().abs()
    print(f"{pc.case_id(key)}: error / bound against fp64 {float((err / bound.clamp_min(1e-300)).max()):.3f}, against "
          f"the dense path {float((diff / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((diff <= bound).all())
    assert bitwise(got_rgb, rgb_leaf.grad)
    assert bitwise(got_rgb, ops.points_project_backward(dout[..., :3].contiguous(), ws, H, W))
    assert bool((got.cpu()[~c["reached"]] == 0).all())                               # nodes out of reach: exactly 0
    restated, restated_rgb, _ = pc.backward_fp32(c["dout"], c["ids"], c["Gh"], c["Gw"])
    assert bitwise(got, restated) and bitwise(got_rgb, restated_rgb)                 # the stated order of the sums
    # want_rgb=False keeps the grid gradient's bits; two runs; B frames against B calls
    alone, none = ops.points_project_grid_backward(dout, ws, grid.shape, H, W)
    assert none is None and bitwise(alone, got)
    again = ops.points_project_grid_backward(dout, ws, grid.shape, H, W, want_rgb=True)
    assert bitwise(again[0], got) and bitwise(again[1], got_rgb)
    ones = []
    for b in range(B):
        _, ws_b = ops._points_project_grid(*_camera(c, b), rgb[b:b + 1], grid.detach()[b:b + 1], r)
        ones.append(ops.points_project_grid_backward(dout[b:b + 1], ws_b, grid.shape[1:], H, W, want_rgb=True))
    assert bitwise(got, torch.cat([g for g, _ in ones])) and bitwise(got_rgb, torch.cat([g for _, g in ones]))
    # through autograd: grid always, rgb when it requires grad; points and cameras never
    leaf, rgb_leaf2 = grid.detach().clone().requires_grad_(), rgb.clone().requires_grad_()
    pts, E, K = (t.requires_grad_() for t in _camera(c))
    ops.points_project_grid_differentiable(pts, E, K, rgb_leaf2, leaf, r).backward(dout)
    assert bitwise(leaf.grad, got) and bitwise(rgb_leaf2.grad, got_rgb)
    assert pts.grad is None and E.grad is None and K.grad is None
    leaf2 = grid.detach().clone().requires_grad_()
    ops.points_project_grid_differentiable(*_camera(c), rgb, leaf2, r).backward(dout)
    assert bitwise(leaf2.grad, got)


def test_peak_memory_stays_far_below_the_dense_tensor():
    """A condition, not a measurement: the op allocates out [B,N,128], the workspace (8 H W + 4 N bytes per frame) and
    the grid gradient, a few MiB, against the 64 MiB of the dense [B,128,H,W] tensor."""
    from audio_motion_avatar_amd import ops

    B, N, H, W, Cg, G = 2, 1029, 256, 256, 125, 64
    g = torch.Generator().manual_seed(3)
    pts = torch.randn(B, N, 3, generator=g) * torch.tensor([0.55, 0.55, 0.3]) + torch.tensor([0.0, 0.0, 2.0])
    E = torch.eye(4).repeat(B, 1, 1)
    K = torch.tensor([[0.9 * W, 0, 0.45 * W], [0, 1.1 * H, 0.55 * H], [0, 0, 1]]).repeat(B, 1, 1)
    pts, E, K = pts.cuda(), E.cuda(), K.cuda()
    rgb = torch.rand(B, 3, H, W, generator=g).cuda()
    grid = torch.randn(B, G, G, Cg, generator=g).cuda().requires_grad_()
    dout = torch.randn(B, N, 3 + Cg, generator=g).cuda()
    r = 0.0075 * min(H, W) / 2.0
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = ops.points_project_grid_differentiable(pts, E, K, rgb, grid, r)
    (grad,) = torch.autograd.grad(out, grid, dout)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"peak allocated over forward + backward: {peak / 2 ** 20:.2f} MiB; dense tensor {B * 128 * H * W * 4 / 2 ** 20:.0f} MiB")
    assert bool((out != 0).any()) and bool((grad != 0).any())
    assert peak < B * 128 * H * W * 4 / 8
