"""GPU: spherical-harmonic colours behind the drop-in surface -- render_batch / render_one / render_multi_view with
args.rgb=False and GaussianRasterizer(shs=...) -- against the ops they are made of (bit for bit), against the RGB
branch at degree 0, their refusals, and a fit of the coefficients through render_multi_view."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
SIZES = [(32, 32, 50), (48, 64, 300)]


def orbit(T, H, W, distance=2.4, device="cuda"):
    """T cameras on a circle around the origin, looking at it: K [1,T,3,3], E [1,T,4,4] (x_view = R x + t)."""
    K = torch.tensor([[float(W), 0, W / 2], [0, float(W), H / 2], [0, 0, 1.0]]).repeat(1, T, 1, 1)
    E = torch.eye(4).repeat(1, T, 1, 1)
    for v in range(T):
        a = 2.0 * np.pi * v / T + 0.3
        E[0, v, 0, 0], E[0, v, 0, 2], E[0, v, 2, 0], E[0, v, 2, 2] = np.cos(a), np.sin(a), -np.sin(a), np.cos(a)
        E[0, v, 2, 3] = distance
    return K.to(device), E.to(device)


def raw_gaussians(seed, N, K, spread=0.3, device="cuda"):
    """Raw (not activated) Gaussians around the origin, [1,N,*], with 3*K colour channels ~ N(0, 0.5^2)."""
    g = torch.Generator().manual_seed(seed)
    out = dict(xyz=torch.randn(1, N, 3, generator=g) * spread,
               rot=torch.nn.functional.normalize(torch.randn(1, N, 4, generator=g), dim=-1),
               scale=torch.randn(1, N, 3, generator=g) * 0.3 + 1.4, opacity=torch.randn(1, N, 1, generator=g) + 1.0,
               color=torch.randn(1, N, 3 * K, generator=g) * 0.5)
    return {k: v.to(device) for k, v in out.items()}


def activated(g):
    """renderer.py:532-533 as torch ops."""
    scale = torch.min(torch.exp(g["scale"] - 3.9), torch.tensor(0.1, device=g["scale"].device))
    return scale, torch.sigmoid(g["opacity"])


def sh_args(H, W, degree):
    return types.SimpleNamespace(image_size=(H, W), rgb=False, sh_degree=degree)


@pytest.mark.parametrize("H,W,N", SIZES)
@pytest.mark.parametrize("degree", [1, 3])
def test_render_batch_is_sh_colors_plus_rasterize(H, W, N, degree):
    from audio_motion_avatar_amd import ops, renderer

    T, Kc = 2, (degree + 1) ** 2
    K, E = orbit(T, H, W)
    g = {k: v.expand(T, -1, -1).contiguous() for k, v in raw_gaussians(810 + degree, N, Kc).items()}
    g["xyz"] = g["xyz"] + torch.randn(T, N, 3, generator=torch.Generator().manual_seed(3)).cuda() * 0.02
    img = renderer.render_batch(g, K, E, sh_args(H, W, degree))
    assert img.shape == (1, T, H, W, 3)
    view, proj, tanfov, campos = ops.camera_from_intrinsics(K, E, H, W)
    scale, opacity = activated(g)
    colors = ops.sh_colors(g["xyz"], g["color"], campos, degree)
    assert colors.max() > 1.0 and (colors == 0).any()          # above 1 is kept, below 0 is clamped
    ref = ops.rasterize(g["xyz"], g["rot"], scale, opacity, colors, view, proj, tanfov, H, W, apply_activations=False,
                        clamp_output=True)["rgba"]
    assert torch.equal(img[0], ref[..., :3])
    assert img.min() >= 0 and img.max() <= 1 and (img < 1).any()
    # the other outputs and arguments work as in the RGB branch
    rgb, alpha = renderer.render_batch(g, K, E, sh_args(H, W, degree), return_alpha=True)
    assert torch.equal(rgb[0], ref[..., :3]) and torch.equal(alpha[0], ref[..., 3])
    out = torch.empty(T, H, W, 4, device="cuda")
    rgba = renderer.render_batch(g, K, E, sh_args(H, W, degree), return_rgba=True, out_rgba=out,
                                 camera=(view, proj, tanfov, campos))
    assert rgba.data_ptr() == out.data_ptr() and torch.equal(out, ref)
    # debug (renderer.py:535-537) replaces scales and opacities ahead of the colour branch
    dbg = renderer.render_batch(g, K, E, sh_args(H, W, degree), debug=True)
    ref_dbg = ops.rasterize(g["xyz"], g["rot"], torch.full_like(scale, 0.01), torch.full_like(opacity, 0.1), colors, view,
                            proj, tanfov, H, W, apply_activations=False, clamp_output=True)["rgba"]
    assert torch.equal(dbg[0], ref_dbg[..., :3])
    # with a gradient asked for, the same image
    q = dict(g, color=g["color"].clone().requires_grad_())
    assert torch.equal(renderer.render_batch(q, K, E, sh_args(H, W, degree)).detach(), img)


@pytest.mark.parametrize("H,W,N", SIZES)
def test_degree_zero_equals_the_rgb_branch(H, W, N):
    """render_batch(rgb=False, degree 0, color=RGB2SH(c)) against render_batch(rgb=True, color=c), c in (0, 1): the
    colours differ by one fp32 rounding of c through the two maps, 2^-22 at the most, and so does a pixel, because the
    blend weights (and the background's) sum to at most 1."""
    from audio_motion_avatar_amd import renderer

    T = 2
    K, E = orbit(T, H, W)
    g = {k: v.expand(T, -1, -1).contiguous() for k, v in raw_gaussians(820, N, 1).items()}
    c = torch.rand(T, N, 3, generator=torch.Generator().manual_seed(821)).cuda() * 0.98 + 0.01
    rgb = renderer.render_batch(dict(g, color=c), K, E, types.SimpleNamespace(image_size=(H, W), rgb=True))
    sh = renderer.render_batch(dict(g, color=renderer.RGB2SH(c)), K, E, sh_args(H, W, 0))
    err = (rgb - sh).abs().max().item()
    print(f"sh render degree 0 vs rgb {H}x{W} N {N}: max |difference| {err:.3e} (bound {2.0 ** -22:.3e})")
    assert (rgb < 1).any() and err <= 2.0 ** -22


def test_multi_view_equals_render_one_and_depends_on_the_view():
    from audio_motion_avatar_amd import renderer

    H, W, N, T, degree = 48, 64, 300, 3, 2
    K, E = orbit(T, H, W)
    g = raw_gaussians(830, N, 9)
    views = renderer.render_multi_view(g, K, E, sh_args(H, W, degree))
    assert views.shape == (1, T, H, W, 3)
    dc = renderer.render_multi_view(dict(g, color=g["color"][..., :3].contiguous()), K, E, sh_args(H, W, 0))
    for v in range(T):
        one = renderer.render_one(g["xyz"][0], g["rot"][0], g["scale"][0], g["opacity"][0], g["color"][0], K[0, v], E[0, v],
                                  sh_args(H, W, degree))
        assert one.shape == (3, H, W)
        assert torch.equal(views[0, v], one.permute(1, 2, 0)), f"view {v}"
        assert (views[0, v] - dc[0, v]).abs().max() > 0.05, f"view {v} does not differ from its DC render"


@pytest.mark.parametrize("H,W,N", SIZES)
def test_gaussian_rasterizer_with_shs(H, W, N):
    """GaussianRasterizer(shs=[N,K,3]) on activated inputs against render_one(rgb=False) on the raw ones, bit for bit
    (render_one clamps its image to [0,1], the op-level rasterizer does not: the clamp is applied here)."""
    from audio_motion_avatar_amd import ops, renderer

    degree = 3
    K, E = orbit(1, H, W)
    g = raw_gaussians(840, N, 16)
    one = renderer.render_one(g["xyz"][0], g["rot"][0], g["scale"][0], g["opacity"][0], g["color"][0], K[0, 0], E[0, 0],
                              sh_args(H, W, degree))
    view, proj, tanfov, campos = ops.camera_from_intrinsics(K, E, H, W)
    settings = renderer.GaussianRasterizationSettings(H, W, tanfov[0, 0].item(), tanfov[0, 1].item(), torch.ones(3).cuda(),
                                                      1.0, view[0].reshape(4, 4), proj[0].reshape(4, 4), degree, campos[0],
                                                      False, False)
    scale, opacity = activated(g)
    kw = dict(means3D=g["xyz"][0], means2D=None, opacities=opacity[0], scales=scale[0], rotations=g["rot"][0])
    shs = g["color"][0].reshape(N, 16, 3)
    color, radii, inv_depth = renderer.GaussianRasterizer(settings)(shs=shs, **kw)
    assert color.shape == (3, H, W) and radii.shape == (N,) and (radii > 0).any()
    assert torch.equal(color.clamp(0.0, 1.0), one)
    # differentiable like the colors_precomp path
    leaf = shs.clone().requires_grad_()
    out, _, _ = renderer.GaussianRasterizer(settings)(shs=leaf, **kw)
    assert torch.equal(out.detach(), color)
    out.sum().backward()
    assert leaf.grad.shape == (N, 16, 3) and leaf.grad.abs().max() > 0


def test_refusals():
    from audio_motion_avatar_amd import ops, renderer

    H = W = 32
    K, E = orbit(1, H, W)
    g = raw_gaussians(850, 50, 9)
    with pytest.raises(ops.AmavError, match=r"\(sh_degree\+1\)\^2 = 16"):            # too few coefficients
        renderer.render_batch(g, K, E, sh_args(H, W, 3))
    with pytest.raises(ops.AmavError, match=r"\(sh_degree\+1\)\^2"):
        renderer.render_batch(dict(g, color=g["color"][..., :3].contiguous()), K, E, sh_args(H, W, 1))
    camera = ops.camera_from_intrinsics(K, E, H, W)
    with pytest.raises(ops.AmavError, match="campos"):                               # a 3-tuple camera=
        renderer.render_batch(g, K, E, sh_args(H, W, 2), camera=camera[:3])
    for kw in (dict(decode={"out": None}), dict(fuse_decode=True)):
        with pytest.raises(ops.AmavError, match="decode"):
            renderer.render_batch(g, K, E, sh_args(H, W, 2), **kw)
    renderer.render_batch(g, K, E, sh_args(H, W, 2), camera=camera)                  # the 4-tuple renders
    renderer.render_batch(dict(g, color=g["color"][..., :3].contiguous()), K, E, sh_args(H, W, 0))  # 3 channels, degree 0
    view, proj, tanfov, campos = camera
    scale, opacity = torch.full((50, 3), 0.02).cuda(), torch.full((50, 1), 0.5).cuda()
    kw = dict(means3D=g["xyz"][0], opacities=opacity, scales=scale, rotations=g["rot"][0])
    shs = g["color"][0].reshape(50, 9, 3)

    def rasterizer(campos_):
        return renderer.GaussianRasterizer(renderer.GaussianRasterizationSettings(
            H, W, tanfov[0, 0].item(), tanfov[0, 1].item(), torch.ones(3).cuda(), 1.0, view[0].reshape(4, 4),
            proj[0].reshape(4, 4), 2, campos_, False, False))

    with pytest.raises(ops.AmavError, match="campos"):                               # missing campos
        rasterizer(None)(shs=shs, **kw)
    with pytest.raises(NotImplementedError):                                         # both
        rasterizer(campos[0])(shs=shs, colors_precomp=torch.zeros(50, 3).cuda(), **kw)
    with pytest.raises(NotImplementedError):                                         # neither
        rasterizer(campos[0])(**kw)
    rasterizer(campos[0])(shs=shs, **kw)


def fit_scene(device="cuda"):
    """4 cameras around 200 Gaussians whose target colours come from degree-2 coefficients (fixed seeds, 32 x 32)."""
    H = W = 32
    K, E = orbit(4, H, W)
    g = raw_gaussians(860, 200, 9, spread=0.35)
    return H, W, K.to(device), E.to(device), {k: v.to(device) for k, v in g.items()}


def fit(render, g, K, E, H, W, degree, target, steps=100, lr=0.05):
    """Adam on the coefficients alone, from zero, on the L1 loss -> (first loss, last loss)."""
    Kc = (degree + 1) ** 2
    sh = torch.zeros(1, g["xyz"].shape[1], 3 * Kc, device=g["xyz"].device, dtype=g["xyz"].dtype).requires_grad_()
    opt = torch.optim.Adam([sh], lr=lr)
    first = None
    for _ in range(steps):
        opt.zero_grad()
        loss = (render(dict(g, color=sh), K, E, sh_args(H, W, degree)) - target).abs().mean()
        first = loss.item() if first is None else first
        loss.backward()
        opt.step()
    with torch.no_grad():
        last = (render(dict(g, color=sh), K, E, sh_args(H, W, degree)) - target).abs().mean().item()
    return first, last


def test_fit_the_coefficients_through_render_multi_view():
    """From zero coefficients, 100 Adam steps on sh alone through render_multi_view(rgb=False) cut the L1 loss at least
    5-fold (the bar of the rasterizer's fit test), and the same fit restricted to degree 0 ends higher: one colour per
    Gaussian cannot follow four cameras."""
    from audio_motion_avatar_amd import renderer

    H, W, K, E, g = fit_scene()
    with torch.no_grad():
        target = renderer.render_multi_view(g, K, E, sh_args(H, W, 2)).clone()
    first2, last2 = fit(renderer.render_multi_view, g, K, E, H, W, 2, target)
    first0, last0 = fit(renderer.render_multi_view, g, K, E, H, W, 0, target)
    print(f"sh fit: degree 2 loss {first2:.4e} -> {last2:.4e} ({first2 / last2:.1f}x), degree 0 {first0:.4e} -> {last0:.4e}")
    assert first0 == first2
    assert last2 * 5 <= first2, f"loss {first2} -> {last2}"
    assert last0 > last2, f"degree 0 ends at {last0}, degree 2 at {last2}"
