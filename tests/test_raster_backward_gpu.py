"""GPU: the rasterizer's backward (amav_rasterize_backward, ops.rasterize_differentiable) against torch autograd of the
brute-force restatement oracle.rasterizer.rasterize_torch in float64 on the CPU.

Decision flips between fp32 and fp64 are removed without widening a tolerance: the output gradient dL/d rgba is drawn
at random and zeroed on the pixels the fp32 C oracle flags `unstable` (a blend decision within rounding of a threshold).
Every gradient term is proportional to its pixel's incoming gradient, so flagged pixels contribute nothing.  Opacities
stay <= 0.95, so the 0.99 clamp (passed through upstream, zeroed by torch) never engages, and the GPU forward's radii
must equal the reference's, which (with unflagged pixels) makes both sides blend the same Gaussians per tile.

Tolerance.  The backward recovers the colour behind Gaussian j front to back, as (C_total - C_through_j) + T_final bg
with the replay's own FMAs, instead of dividing T by (1 - alpha) once per Gaussian (upstream), whose error compounds
with the list length.  What is left are fp32 roundings of single terms -- the subtraction above, at most ~n ulp of the
pixel's colour for a list of n, divided by 1 - alpha >= 0.05 -- that enter each gradient with their pixel's random sign
and are summed over many pixels, so against the largest gradient of an attribute they stay well below 1e-3 (measured
values are printed).  TOL = 1e-3 is the issue's bound, applied as max|g - g_ref| <= TOL * max|g_ref| per attribute.
"""
import types

import numpy as np
import pytest
import torch

from helpers import oracle_frames, random_scene

pytestmark = pytest.mark.gpu
TOL = 1e-3
NAMES = ("xyz", "rot", "scale", "opacity", "color")
OPS_NAMES = ("means3d", "rotations", "scales", "opacities", "colors")


def scene_of(seed, N, H, W, F=1, **kw):
    s = random_scene(seed, N, H, W, F, **kw)
    s["opacity"] = s["opacity"].clamp(max=0.95)
    return s


def grad_out(scene, seed, bg=(1.0, 1.0, 1.0)):
    """Random dL/d rgba [F,H,W,4], zero on the pixels the fp32 oracle flags."""
    g = torch.Generator().manual_seed(seed)
    F, H, W = scene["xyz"].shape[0], scene["H"], scene["W"]
    go = torch.randn(F, H, W, 4, generator=g)
    for f, r in enumerate(oracle_frames(scene, np.float32, bg=bg)):
        go[f][torch.from_numpy(r["unstable"] != 0)] = 0.0
    return go


def reference(scene, go, bg=(1.0, 1.0, 1.0), activations=False, clamp=False, raw=None):
    """fp64 CPU autograd of rasterize_torch (with torch's activations and output clamp when asked) -> gradients of
    the five attributes [F,N,*] and the radii [F,N]."""
    from oracle import camera
    from oracle.rasterizer import rasterize_torch

    F = scene["xyz"].shape[0]
    src = raw if raw is not None else scene
    grads = {k: torch.zeros(src[k].shape, dtype=torch.float64) for k in NAMES}
    radii = []
    for f in range(F):
        p = {k: src[k][f].double().clone().requires_grad_() for k in NAMES}
        s, o, c = p["scale"], p["opacity"], p["color"]
        if activations:
            s = torch.min(torch.exp(s - 3.9), torch.tensor(0.1, dtype=torch.float64))
            o = torch.sigmoid(o)
            c = torch.clamp(c, 0.0, 1.0)
        view, proj, tx, ty, _ = camera.camera_setup(scene["K"][f].double(), scene["E"][f].double(), scene["H"],
                                                    scene["W"])
        out = rasterize_torch(p["xyz"], p["rot"], s, o, c, view, proj, tx, ty, bg, scene["H"], scene["W"])
        rgb = out["color"].permute(1, 2, 0)
        if clamp:
            rgb = rgb.clamp(0.0, 1.0)
        loss = (rgb * go[f, ..., :3].double()).sum() + (out["alpha"] * go[f, ..., 3].double()).sum()
        gs = torch.autograd.grad(loss, [p[k] for k in NAMES])
        for k, g in zip(NAMES, gs):
            grads[k][f] = g
        radii.append(out["radii"])
    return grads, torch.stack(radii)


def camera(scene):
    from audio_motion_avatar_amd import ops

    return ops.camera_from_intrinsics(scene["K"].cuda(), scene["E"].cuda(), scene["H"], scene["W"])[:3]


def hip_grads(scene, go, bg=(1.0, 1.0, 1.0), **kw):
    """Forward + backward through ops.rasterize_differentiable (autograd)."""
    from audio_motion_avatar_amd import ops

    p = {k: scene[k].cuda().requires_grad_() for k in NAMES}
    view, proj, tanfov = camera(scene)
    out = ops.rasterize_differentiable(*[p[k] for k in NAMES], view, proj, tanfov, scene["H"], scene["W"], bg=bg,
                                       want_radii=True, **kw)
    (out["rgba"] * go.cuda()).sum().backward()
    return {k: p[k].grad.cpu() for k in NAMES}, out


def check_grads(name, got, ref, tol=TOL):
    errs = {}
    for k in NAMES:
        g, r = got[k].double(), ref[k]
        scale = r.abs().max().item()
        assert scale > 0, f"{name}: reference gradient of {k} is zero"
        errs[k] = (g - r).abs().max().item() / scale
    print(f"raster backward {name}: max|g - g_ref| / max|g_ref| =", {k: f"{v:.2e}" for k, v in errs.items()})
    for k, e in errs.items():
        assert e <= tol, f"{name}: gradient of {k} off by {e:.3e} of its largest value"
    return errs


@pytest.mark.parametrize("seed,N,H,W,F", [(401, 300, 50, 70, 3), (402, 2000, 128, 128, 1)])
def test_gradients_match_fp64_autograd(seed, N, H, W, F):
    scene = scene_of(seed, N, H, W, F)
    go = grad_out(scene, seed + 1)
    got, out = hip_grads(scene, go)
    ref, ref_radii = reference(scene, go)
    assert torch.equal(out["radii"].cpu().long(), ref_radii.long())
    check_grads(f"{F}x{N} {H}x{W}", got, ref)


def test_render_batch_with_activations_and_clamp():
    """render_batch(apply activations, clamp output) against torch activations + rasterize_torch + clamp(0, 1)."""
    from audio_motion_avatar_amd import renderer

    g = torch.Generator().manual_seed(411)
    N, H, W = 800, 80, 96
    raw = dict(xyz=torch.randn(1, N, 3, generator=g) * 0.3 + torch.tensor([0, 0, 2.4]),
               rot=torch.nn.functional.normalize(torch.randn(1, N, 4, generator=g), dim=-1),
               scale=torch.randn(1, N, 3, generator=g) * 0.5,
               opacity=(torch.randn(1, N, 1, generator=g)).clamp(max=2.9),  # sigmoid <= 0.948
               color=torch.rand(1, N, 3, generator=g) * 1.4 - 0.2)         # exercises clamp(c, 0, 1)
    K = torch.tensor([[[96.0, 0, 48], [0, 96.0, 40], [0, 0, 1]]])
    E = torch.eye(4)[None]
    bg = (0.5, 0.5, 0.5)  # colours in [0, 1] over a mid-grey background never reach the output clamp's thresholds
    act = dict(xyz=raw["xyz"], rot=raw["rot"], scale=torch.min(torch.exp(raw["scale"] - 3.9), torch.tensor(0.1)),
               opacity=torch.sigmoid(raw["opacity"]), color=raw["color"].clamp(0, 1), K=K, E=E, H=H, W=W)
    go = grad_out(act, 412, bg=bg)
    ref, ref_radii = reference(act, go, bg=bg, activations=True, clamp=True, raw=raw)
    p = {k: raw[k].cuda().requires_grad_() for k in NAMES}
    args = types.SimpleNamespace(image_size=(H, W), rgb=True)
    rgb, alpha = renderer.render_batch(p, K[None].cuda(), E[None].cuda(), args, bg_color=bg, return_alpha=True)
    (torch.cat([rgb, alpha[..., None]], -1)[0] * go.cuda()).sum().backward()
    check_grads("render_batch activations", {k: p[k].grad.cpu() for k in NAMES}, ref)
    from audio_motion_avatar_amd import ops

    radii = ops.rasterize(*[raw[k].cuda() for k in NAMES], *ops.camera_from_intrinsics(K.cuda(), E.cuda(), H, W)[:3], H, W,
                          apply_activations=True, want_radii=True)["radii"].cpu()
    assert torch.equal(radii.long(), ref_radii.long())


@pytest.mark.parametrize("N", [1500, 3000])
def test_long_lists_and_terminated_pixels(N):
    """Clustered Gaussians on a 32x32 image: lists longer than 512 (sort_big's bucket sort) and longer than 2048 (its
    bitonic network in place), and pixels whose transmittance ends below 1e-4."""
    from audio_motion_avatar_amd import ops

    scene = scene_of(99 + N, N, 32, 32, 1, spread=0.05, log_scale=-2.5, scale_jitter=0.2)
    go = grad_out(scene, N)
    got, out = hip_grads(scene, go)
    view, proj, tanfov = camera(scene)
    fwd = ops.rasterize(*[scene[k].cuda() for k in NAMES], view, proj, tanfov, 32, 32)
    lengths = fwd["workspace"].tile_counts().cpu()
    assert lengths.max().item() > (2048 if N == 3000 else 512)
    assert (fwd["rgba"][..., 3] > 0.998).any()  # transmittance ended near 1e-4: the pixel finished early
    ref, ref_radii = reference(scene, go)
    assert torch.equal(out["radii"].cpu().long(), ref_radii.long())
    check_grads(f"long lists N={N}", got, ref)


def _replay_alpha(scene, F=None, grad_seed=0):
    from audio_motion_avatar_amd import ops

    view, proj, tanfov = camera(scene)
    attrs = [scene[k].cuda() for k in NAMES]
    fwd = ops.rasterize(*attrs, view, proj, tanfov, scene["H"], scene["W"], check_overflow=True)
    go = torch.randn(fwd["rgba"].shape, generator=torch.Generator().manual_seed(grad_seed)).cuda()
    g = ops.rasterize_backward(*attrs, view, proj, tanfov, scene["H"], scene["W"], go, fwd["workspace"],
                               fwd["max_frame"], want_alpha=True)
    return fwd, g


@pytest.mark.parametrize("case", ["small", "long", "longest"])
def test_replay_alpha_is_the_forward_alpha_bit_for_bit(case):
    scene = {"small": lambda: scene_of(401, 300, 50, 70, 3),
             "long": lambda: scene_of(1599, 1500, 32, 32, 1, spread=0.05, log_scale=-2.5, scale_jitter=0.2),
             "longest": lambda: scene_of(3099, 3000, 32, 32, 1, spread=0.05, log_scale=-2.5, scale_jitter=0.2)}[case]()
    fwd, g = _replay_alpha(scene)
    a, r = fwd["rgba"][..., 3].contiguous(), g["alpha"]
    assert torch.equal(a.view(torch.int32), r.view(torch.int32)), f"{(a != r).sum().item()} pixels differ"
    if case != "small":  # some pixels finished (the next Gaussian would have taken T below 1e-4)
        assert (a > 0.998).any()


def _shard(F=250, seed=7):
    return scene_of(seed, 10000, 512, 512, F, spread=0.3, log_scale=-4.9, scale_jitter=0.55)


def test_shard_replay_alpha_and_frame_independence():
    """250 x 10 k x 512^2 (the fused-binning shard): the replay's alpha is the forward's bit for bit; two backward calls
    agree bit for bit; and the gradients of the 250-frame call equal those of ten 25-frame calls (the few-frame
    binning path) bit for bit."""
    from audio_motion_avatar_amd import ops

    scene = _shard()
    view, proj, tanfov = camera(scene)
    attrs = [scene[k].cuda() for k in NAMES]
    fwd = ops.rasterize(*attrs, view, proj, tanfov, 512, 512, check_overflow=True)
    go = torch.randn(250, 512, 512, 4, generator=torch.Generator().manual_seed(5)).cuda()
    g1 = ops.rasterize_backward(*attrs, view, proj, tanfov, 512, 512, go, fwd["workspace"], fwd["max_frame"],
                                want_alpha=True)
    assert torch.equal(fwd["rgba"][..., 3].contiguous().view(torch.int32), g1["alpha"].view(torch.int32))
    g2 = ops.rasterize_backward(*attrs, view, proj, tanfov, 512, 512, go, fwd["workspace"], fwd["max_frame"])
    for k in OPS_NAMES:
        assert torch.equal(g1[k].view(torch.int32), g2[k].view(torch.int32)), f"{k}: two calls differ"
        assert g1[k].abs().max().item() > 0
    del fwd
    for c in range(10):
        sl = slice(25 * c, 25 * (c + 1))
        part = [a[sl] for a in attrs]
        fp = ops.rasterize(*part, view[sl], proj[sl], tanfov[sl], 512, 512, check_overflow=True)
        gp = ops.rasterize_backward(*part, view[sl], proj[sl], tanfov[sl], 512, 512, go[sl].contiguous(),
                                    fp["workspace"], fp["max_frame"])
        for k in OPS_NAMES:
            assert torch.equal(g1[k][sl].view(torch.int32), gp[k].view(torch.int32)), f"frames {sl}: {k} differs"


def test_images_with_grad_equal_no_grad():
    from audio_motion_avatar_amd import renderer

    g = torch.Generator().manual_seed(421)
    N, H, W = 1200, 72, 88
    gauss = dict(xyz=torch.randn(2, N, 3, generator=g) * 0.3 + torch.tensor([0, 0, 2.4]),
                 rot=torch.nn.functional.normalize(torch.randn(2, N, 4, generator=g), dim=-1),
                 scale=torch.randn(2, N, 3, generator=g) * 0.5, opacity=torch.randn(2, N, 1, generator=g),
                 color=torch.rand(2, N, 3, generator=g) * 1.4 - 0.2)
    K = torch.tensor([[72.0, 0, 44], [0, 72.0, 36], [0, 0, 1]]).repeat(1, 2, 1, 1).cuda()
    E = torch.eye(4).repeat(1, 2, 1, 1).cuda()
    E[0, 1, 0, 3] = 0.05
    args = types.SimpleNamespace(image_size=(H, W), rgb=True)
    with torch.no_grad():
        ref = renderer.render_batch({k: v.cuda() for k, v in gauss.items()}, K, E, args, return_rgba=True).clone()
    p = {k: v.cuda().requires_grad_() for k, v in gauss.items()}
    got = renderer.render_batch(p, K, E, args, return_rgba=True)
    assert got.requires_grad
    assert torch.equal(got.detach().view(torch.int32), ref.view(torch.int32))

    # GaussianRasterizer (op-level API, activated inputs, inv_depth and radii too)
    from oracle import camera as ocam

    scene = scene_of(422, 900, 64, 80, 1)
    view, proj, tx, ty, campos = ocam.camera_setup(scene["K"][0], scene["E"][0], 64, 80)
    settings = renderer.GaussianRasterizationSettings(64, 80, tx, ty, torch.tensor([1.0, 1.0, 1.0]).cuda(), 1.0,
                                                      view.float().cuda(), proj.float().cuda(), 3, campos, False, False)
    rast = renderer.GaussianRasterizer(settings)
    inputs = dict(means3D=scene["xyz"][0], opacities=scene["opacity"][0], scales=scene["scale"][0],
                  rotations=scene["rot"][0], colors_precomp=scene["color"][0])
    with torch.no_grad():
        c0, r0, d0 = rast(**{k: v.cuda() for k, v in inputs.items()})
    leaf = {k: v.cuda().requires_grad_() for k, v in inputs.items()}
    means2D = torch.zeros_like(leaf["means3D"], requires_grad=True)
    c1, r1, d1 = rast(means2D=means2D, **leaf)
    assert torch.equal(c1.detach().view(torch.int32), c0.view(torch.int32))
    assert torch.equal(r1, r0) and torch.equal(d1.view(torch.int32), d0.view(torch.int32))
    assert not d1.requires_grad and not r1.requires_grad
    c1.sum().backward()
    assert all(v.grad is not None and v.grad.abs().max() > 0 for v in leaf.values())
    assert means2D.grad is None


def test_render_multi_view_gradient_is_the_sum_over_views():
    from audio_motion_avatar_amd import renderer

    g = torch.Generator().manual_seed(431)
    N, H, W, V = 700, 64, 64, 3
    gauss = dict(xyz=torch.randn(1, N, 3, generator=g) * 0.3 + torch.tensor([0, 0, 2.4]),
                 rot=torch.nn.functional.normalize(torch.randn(1, N, 4, generator=g), dim=-1),
                 scale=torch.randn(1, N, 3, generator=g) * 0.5, opacity=torch.randn(1, N, 1, generator=g),
                 color=torch.rand(1, N, 3, generator=g))
    K = torch.tensor([[64.0, 0, 32], [0, 64.0, 32], [0, 0, 1]]).repeat(1, V, 1, 1).cuda()
    E = torch.eye(4).repeat(1, V, 1, 1)
    for v in range(V):
        a = 0.15 * (v - 1)
        E[0, v, 0, 0], E[0, v, 0, 2], E[0, v, 2, 0], E[0, v, 2, 2] = np.cos(a), np.sin(a), -np.sin(a), np.cos(a)
    E = E.cuda()
    args = types.SimpleNamespace(image_size=(H, W), rgb=True)
    go = torch.randn(1, V, H, W, 3, generator=g).cuda()
    p = {k: v.cuda().requires_grad_() for k, v in gauss.items()}
    (renderer.render_multi_view(p, K, E, args) * go).sum().backward()
    total = {k: torch.zeros_like(v) for k, v in p.items()}
    for v in range(V):
        q = {k: t.detach().clone().requires_grad_() for k, t in p.items()}
        img = renderer.render_batch(q, K[:, v:v + 1], E[:, v:v + 1], args)
        (img * go[:, v:v + 1]).sum().backward()
        for k in total:
            total[k] += q[k].grad
    for k in p:
        assert p[k].grad.abs().max() > 0
        torch.testing.assert_close(p[k].grad, total[k], rtol=1e-5, atol=1e-6 * total[k].abs().max().item())


def test_fit_colours_opacities_and_means_with_adam():
    """End to end: recover perturbed colours, opacities and means from a rendered target with Adam on
    l1 + 0.1 * (1 - ssim) through render_batch."""
    from audio_motion_avatar_amd import losses, renderer

    g = torch.Generator().manual_seed(441)
    N, H, W = 60, 64, 64  # separated blobs, so that every colour is determined by the images
    gt = dict(xyz=torch.randn(1, N, 3, generator=g) * 0.5 + torch.tensor([0, 0, 2.4]),
              rot=torch.nn.functional.normalize(torch.randn(1, N, 4, generator=g), dim=-1),
              scale=torch.randn(1, N, 3, generator=g) * 0.3 + 1.2, opacity=torch.randn(1, N, 1, generator=g) + 1.0,
              color=torch.rand(1, N, 3, generator=g))
    gt = {k: v.cuda() for k, v in gt.items()}
    K = torch.tensor([[64.0, 0, 32], [0, 64.0, 32], [0, 0, 1]]).repeat(1, 2, 1, 1).cuda()
    E = torch.eye(4).repeat(1, 2, 1, 1)
    E[0, 1, 0, 0], E[0, 1, 0, 2], E[0, 1, 2, 0], E[0, 1, 2, 2] = np.cos(0.2), np.sin(0.2), -np.sin(0.2), np.cos(0.2)
    E = E.cuda()
    args = types.SimpleNamespace(image_size=(H, W), rgb=True)
    with torch.no_grad():
        target = renderer.render_multi_view(gt, K, E, args).clone()
    p = {k: v.clone() for k, v in gt.items()}
    p["color"] = (torch.rand(1, N, 3, generator=g).cuda())
    p["opacity"] = gt["opacity"] + torch.randn(1, N, 1, generator=g).cuda() * 0.5
    p["xyz"] = gt["xyz"] + torch.randn(1, N, 3, generator=g).cuda() * 0.01
    for k in ("color", "opacity", "xyz"):
        p[k].requires_grad_()
    opt = torch.optim.Adam([{"params": [p["color"]], "lr": 0.02}, {"params": [p["opacity"]], "lr": 0.02},
                            {"params": [p["xyz"]], "lr": 2e-4}])

    def loss_of():
        img = renderer.render_multi_view(p, K, E, args)
        return losses.l1_loss(img, target) + 0.1 * (1.0 - losses.ssim(img, target))

    colour_err = lambda: (p["color"].detach().clamp(0, 1) - gt["color"]).abs().mean().item()  # noqa: E731
    err0 = colour_err()
    first = None
    for _ in range(300):
        opt.zero_grad()
        loss = loss_of()
        first = loss.item() if first is None else first
        loss.backward()
        opt.step()
    with torch.no_grad():
        last = loss_of().item()
    err = colour_err()
    print(f"raster backward fit: loss {first:.4e} -> {last:.4e}, mean |colour - gt| {err0:.3f} -> {err:.3f}")
    assert last * 5 <= first, f"loss {first} -> {last}"
    assert err < 0.1 and err < 0.5 * err0


def test_refusals():
    from audio_motion_avatar_amd import ops, renderer

    scene = scene_of(451, 50, 32, 32, 1)
    view, proj, tanfov = camera(scene)
    p = [scene[k].cuda().requires_grad_() for k in NAMES]
    with pytest.raises(NotImplementedError):
        ops.rasterize_differentiable(*p, view, proj, tanfov, 32, 32, antialiasing=True)
    ws = ops.RasterWorkspace(1, 50, 32, 32, 1000, "cuda")
    with pytest.raises(NotImplementedError):
        ops.rasterize_differentiable(*p, view, proj, tanfov, 32, 32, workspace=ws)
    with pytest.raises(NotImplementedError):
        ops.rasterize_differentiable(*p, view, proj, tanfov, 32, 32, wire=(torch.empty(16, dtype=torch.uint8), 1))
    args = types.SimpleNamespace(image_size=(32, 32), rgb=True)
    gd = dict(zip(NAMES, p))
    K, E = scene["K"][None].cuda(), scene["E"][None].cuda()
    for kw in (dict(workspace=ws), dict(wire=(torch.empty(16, dtype=torch.uint8).cuda(), 1)), dict(decode={"out": None})):
        with pytest.raises(NotImplementedError):
            renderer.render_batch(gd, K, E, args, **kw)
    vm, pm, tx, ty = view[0].reshape(4, 4), proj[0].reshape(4, 4), tanfov[0, 0].item(), tanfov[0, 1].item()
    bgt = torch.ones(3).cuda()
    aa = renderer.GaussianRasterizer(renderer.GaussianRasterizationSettings(32, 32, tx, ty, bgt, 1.0, vm, pm, 3, None,
                                                                             False, False, antialiasing=True))
    leaf = dict(means3D=p[0][0], rotations=p[1][0], scales=p[2][0], opacities=p[3][0], colors_precomp=p[4][0])
    with pytest.raises(NotImplementedError):
        aa(**leaf)
    plain = renderer.GaussianRasterizer(renderer.GaussianRasterizationSettings(32, 32, tx, ty, bgt, 1.0, vm, pm, 3, None,
                                                                                False, False))
    with pytest.raises(NotImplementedError):
        plain(shs=torch.zeros(50, 16, 3).cuda(), **leaf)
    with pytest.raises(NotImplementedError):
        plain(cov3D_precomp=torch.zeros(50, 6).cuda(), **leaf)
    # without gradients the inference paths are untouched: antialiasing still renders
    with torch.no_grad():
        aa(**{k: v.detach() for k, v in leaf.items()})
