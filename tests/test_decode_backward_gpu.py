"""GPU: the triplane decode's backward (amav_triplane_decode_backward, ops.triplane_decode_differentiable) and training
through Renderer.

Accuracy is checked against torch autograd, in float64 on the CPU, of the oracle's restatement of the reference
(oracle.triplane: tokens_to_planes -> sample_from_triplane -> gaussian_heads -> construct_gaussians).  The derivative
of bilinear sampling jumps where a point crosses a texel centre and where p / radius crosses the clamp at +-1, so the
random points are kept 1e-3 texel away from both (fp32 and fp64 then take the same branch); test_gradients_at_kinks
puts points exactly on them, at dyadic coordinates that both precisions compute exactly.  Bound, chosen and not measured:
max|g - g_ref| <= 1e-4 max|g_ref| per tensor; the measured ratios are printed.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
TOL = 1e-4
LAYERS = {"xyz_layer": 3, "rotation_layer": 4, "scaling_layer": 3, "opacity_layer": 1, "shs_layer": 3}
PAD = (11, 15)


def _points(g, F, N, R, radius, spread=1.15):
    """Uniform in +-spread * radius (some beyond the clamp, some with taps off the plane edge), nudged 1e-3 texel away
    from texel centres and from the clamp boundary."""
    p = ((torch.rand(F, N, 3, generator=g, dtype=torch.float64) * 2 - 1) * spread * radius)
    u = p / radius
    for _ in range(3):
        pix = ((u.clamp(-1, 1) + 1) * R - 1) / 2
        frac = pix - pix.round()
        near = (frac.abs() < 1e-3) | ((u.abs() - 1).abs() < 1e-3 * 2 / R)
        u = torch.where(near, u + 3e-3 * 2 / R, u)
    return (u * radius).float()


def make_case(F, N, C, R, seed, radius=1.4, spread=1.15, exact=None):
    """`exact` [F, M, 3]: points placed first as given (not nudged); the other N - M are drawn by _points."""
    g = torch.Generator().manual_seed(seed)
    tokens = torch.randn(F, C, 3 * R * R, generator=g)
    # raw head outputs of order one whatever C; the rotation's norm stays away from 0, where F.normalize's backward
    # would amplify the fp32 rounding of its input (the forward's own) beyond the bound
    std = 0.5 / math.sqrt(3 * C + 3)
    heads = {k: (torch.randn(n, 3 * C + 3, generator=g) * std, torch.randn(n, generator=g) * 0.3)
             for k, n in LAYERS.items()}
    heads["rotation_layer"][1][0] += 2.0
    points = _points(g, F, N - (0 if exact is None else exact.shape[1]), R, radius, spread)
    if exact is not None:
        points = torch.cat([exact.float(), points], 1)
    transl = torch.randn(F, 3, generator=g) * 0.1
    grec = torch.randn(F, N, 16, generator=g)
    grec[..., PAD] = 0.0
    return dict(tokens=tokens, heads=heads, points=points, transl=transl, grec=grec, R=R, radius=radius)


def reference_grads(case):
    from oracle import triplane as orc

    d = lambda t: t.double().clone().requires_grad_()
    tok, pts, tr = d(case["tokens"]), d(case["points"]), d(case["transl"])
    heads = {k: (d(w), d(b)) for k, (w, b) in case["heads"].items()}
    params = {}
    for k, (w, b) in heads.items():
        params[f"gaussian_decoder.{k}.weight"], params[f"gaussian_decoder.{k}.bias"] = w, b
    planes = orc.tokens_to_planes(tok[None], case["R"])
    feats = orc.sample_from_triplane(planes, pts, case["radius"])
    out = orc.construct_gaussians(orc.gaussian_heads(params, torch.cat([pts, feats], -1)), pts, tr)
    z = torch.zeros_like(out["opacity"])
    rec = torch.cat([out["xyz"], out["opacity"], out["rot"], out["scale"], z, out["color"], z], -1)
    (rec * case["grec"].double()).sum().backward()
    g = dict(tokens=tok.grad, points=pts.grad, transl=tr.grad)
    for k, (w, b) in heads.items():
        g[k + ".weight"], g[k + ".bias"] = w.grad, b.grad
    return g, rec


def gpu_grads(case, region=True, tokens=None):
    from audio_motion_avatar_amd import ops

    c = lambda t: t.cuda().clone().requires_grad_()
    tok = c(case["tokens"] if tokens is None else tokens)
    pts, tr = c(case["points"]), c(case["transl"])
    heads = {k: (c(w), c(b)) for k, (w, b) in case["heads"].items()}
    C = tok.shape[1]
    wpl, wpt = ops.pack_head_weights(heads, C, "cuda", differentiable=True)
    rec = ops.triplane_decode_differentiable(tok, wpl, wpt, pts, tr, case["R"], case["radius"], region=region)
    (rec * case["grec"].cuda()).sum().backward()
    g = dict(tokens=tok.grad, points=pts.grad, transl=tr.grad)
    for k, (w, b) in heads.items():
        g[k + ".weight"], g[k + ".bias"] = w.grad, b.grad
    return {k: v.cpu() for k, v in g.items()}, rec.detach().cpu()


@pytest.mark.parametrize("F,N,C,R", [(3, 300, 8, 8), (4, 2000, 32, 32), (2, 3000, 512, 128)])
def test_gradients_match_fp64_autograd(F, N, C, R):
    case = make_case(F, N, C, R, seed=F * 1000 + C)
    ref, ref_rec = reference_grads(case)
    got, rec = gpu_grads(case)
    assert (rec - ref_rec.float()).abs().max() < 1e-3
    ratios = {}
    for k, r in ref.items():
        scale = float(r.abs().max())
        ratios[k] = float((got[k].double() - r).abs().max()) / max(scale, 1e-30)
    print(f"\nF={F} N={N} C={C} R={R} max|g - g_ref| / max|g_ref|: " +
          ", ".join(f"{k} {v:.1e}" for k, v in ratios.items()))
    bad = {k: v for k, v in ratios.items() if not v <= TOL}
    assert not bad, bad


def _texel_rects(points, R, radius):
    """Per frame and plane, the projected rectangle grown by one texel (and to whole quads in x): a superset of what
    amav_triplane_project_region projects, computed in float64."""
    lo, hi = points.double().amin(1), points.double().amax(1)
    tap = lambda v: math.floor((((max(-1.0, min(1.0, v / radius))) + 1) * R - 1) / 2)
    rects = []
    for f in range(points.shape[0]):
        per = []
        for ax, ay in ((0, 1), (0, 2), (1, 2)):
            x0 = max(tap(float(lo[f, ax])) - 1, 0) & ~3
            x1 = min(tap(float(hi[f, ax])) + 2, R - 1) | 3
            y0 = max(tap(float(lo[f, ay])) - 1, 0)
            y1 = min(tap(float(hi[f, ay])) + 2, R - 1)
            per.append((x0, x1, y0, y1))
        rects.append(per)
    return rects


def test_region_poisoned_slab_is_never_read():
    F, N, C, R = 3, 2000, 32, 32
    case = make_case(F, N, C, R, seed=5, spread=0.45)
    clean, rec = gpu_grads(case)
    inside = torch.zeros(F, 3, R, R, dtype=torch.bool)
    for f, per in enumerate(_texel_rects(case["points"], R, case["radius"])):
        for p, (x0, x1, y0, y1) in enumerate(per):
            inside[f, p, y0:y1 + 1, x0:x1 + 1] = True
    assert (~inside).sum() > 0.3 * inside.numel()  # the test means something: most of each plane is poisoned
    poisoned = case["tokens"].clone().view(F, C, 3, R, R)
    poisoned.masked_fill_(~inside[:, None].expand(F, C, 3, R, R), float("nan"))
    poisoned = poisoned.view(F, C, 3 * R * R)
    dirty, rec2 = gpu_grads(case, tokens=poisoned)
    assert torch.equal(rec, rec2)
    for k, v in dirty.items():
        assert torch.isfinite(v).all(), k
        assert torch.equal(v, clean[k]), k
    outside = dirty["tokens"].view(F, C, 3, R, R).permute(0, 2, 3, 4, 1)[~inside]  # [texels, C]
    assert (outside == 0).all() and not torch.signbit(outside).any()


def _backward_once(case, F0, F1, proj, boxes, wpl, wpt):
    from audio_motion_avatar_amd import ops

    s = slice(F0, F1)
    return ops.triplane_decode_backward(case["tokens"][s].cuda(), wpl, wpt, case["points"][s].cuda(), proj[s], case["grec"][s].cuda(),
                                        case["radius"], boxes=boxes[s])


def test_deterministic_and_independent_of_frame_slicing():
    from audio_motion_avatar_amd import ops

    F, N, C, R = 250, 2000, 16, 32
    case = make_case(F, N, C, R, seed=11, spread=0.6)
    heads = {k: (w.cuda(), b.cuda()) for k, (w, b) in case["heads"].items()}
    wpl, wpt = ops.pack_head_weights(heads, C, "cuda")
    pts = case["points"].cuda()
    boxes = ops.points_bbox(pts)
    proj = ops.triplane_project(case["tokens"].cuda(), wpl, R, region=(boxes, case["radius"]))
    a = _backward_once(case, 0, F, proj, boxes, wpl, wpt)
    b = _backward_once(case, 0, F, proj, boxes, wpl, wpt)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    for s in range(0, F, 25):
        part = _backward_once(case, s, s + 25, proj, boxes, wpl, wpt)
        for k in ("tokens", "points", "transl"):
            assert torch.equal(part[k], a[k][s:s + 25]), (k, s)


def _compare(label, got, ref):
    """max|g - g_ref| / max|g_ref| per tensor, printed, each within TOL."""
    ratios = {}
    for k, r in ref.items():
        scale = float(r.abs().max())
        assert torch.isfinite(got[k]).all(), f"{label}: {k} not finite"
        ratios[k] = float((got[k].double() - r).abs().max()) / max(scale, 1e-30)
    print(f"\n{label} max|g - g_ref| / max|g_ref|: " + ", ".join(f"{k} {v:.1e}" for k, v in ratios.items()))
    bad = {k: v for k, v in ratios.items() if not v <= TOL}
    assert not bad, bad
    return ratios


# Shapes the default cases do not reach: R % 4 != 0 (no region; R = 5, 7: R^2 % 4 != 0, dtokens_kernel's scalar form;
# R = 6: its vector form with quads that straddle rows), C % 64 != 0 above 64 (dwplane_kernel's partial last block),
# C % 4 != 0, C = 1, C = 1024 (the ABI's largest), N = 1, N just past a 256-point block, N not a multiple of 64.
EDGE_SHAPES = [(2, 300, 16, 5), (2, 300, 16, 6), (2, 300, 16, 7), (2, 400, 1, 16), (2, 400, 3, 8), (2, 500, 100, 16),
               (2, 500, 200, 32), (2, 300, 1024, 16), (3, 1, 8, 8), (2, 257, 32, 16), (2, 321, 40, 12)]


@pytest.mark.parametrize("F,N,C,R", EDGE_SHAPES)
def test_gradients_at_edge_shapes(F, N, C, R):
    assert R % 4 != 0 or C % 64 != 0 or C % 4 != 0 or C == 1024 or N % 64 != 0
    case = make_case(F, N, C, R, seed=F * 7919 + N * 31 + C * 7 + R)
    ref, ref_rec = reference_grads(case)
    got, rec = gpu_grads(case, region=True)
    assert (rec - ref_rec.float()).abs().max() < 1e-3
    _compare(f"F={F} N={N} C={C} R={R}", got, ref)
    flat, rec_flat = gpu_grads(case, region=False)
    if R % 4 != 0:  # amav_triplane_project_region ignores boxes there: the same launches, the same bits
        assert torch.equal(rec_flat, rec)
        for k in got:
            assert torch.equal(flat[k], got[k]), k
    else:
        _compare(f"F={F} N={N} C={C} R={R} no region", flat, ref)


def _kink_points(F, R, g):
    """Points on the derivative's kinks, exactly: p / radius (radius 2) on texel centres ((2k + 1) / R - 1), on +-1 and
    beyond +-1 (+-1.25), each coordinate drawn from those values (dyadic: fp32 and fp64 take the same branch)."""
    centres = [(2 * k + 1) / R - 1 for k in range(R)]
    values = torch.tensor(centres + [-1.0, 1.0, -1.0, 1.0, -1.25, 1.25], dtype=torch.float64)
    idx = torch.randint(0, len(values), (F, 6 * R, 3), generator=g)
    return values[idx] * 2.0


def test_gradients_at_kinks():
    F, N, C, R, radius = 2, 400, 16, 16, 2.0
    g = torch.Generator().manual_seed(551)
    exact = _kink_points(F, R, g)
    case = make_case(F, N, C, R, seed=552, radius=radius, exact=exact)
    u = case["points"][:, :exact.shape[1]].double() / radius
    assert torch.equal(case["points"][:, :exact.shape[1]].double(), exact)
    pix = ((u.clamp(-1, 1) + 1) * R - 1) / 2
    assert (pix == pix.round()).sum() > 200 and (u.abs() == 1).sum() > 50 and (u.abs() > 1).sum() > 20
    ref, ref_rec = reference_grads(case)
    got, rec = gpu_grads(case)
    assert (rec - ref_rec.float()).abs().max() < 1e-3
    _compare("kinks", got, ref)


def test_zero_rotation_head():
    """The reference's zero-initialised gaussian_decoder: the raw quaternion is exactly 0 and F.normalize takes its
    eps branch (dv = g / 1e-12); every gradient, the amplified ones included, against fp64 autograd."""
    F, N, C, R = 2, 600, 32, 16
    case = make_case(F, N, C, R, seed=561)
    w, b = case["heads"]["rotation_layer"]
    case["heads"]["rotation_layer"] = (torch.zeros_like(w), torch.zeros_like(b))
    ref, ref_rec = reference_grads(case)
    assert (ref_rec[..., 4:8] == 0).all()
    assert ref["rotation_layer.bias"].abs().max() > 1e9  # the eps branch really ran
    got, rec = gpu_grads(case)
    assert (rec[..., 4:8] == 0).all()
    _compare("zero rotation head", got, ref)


def test_token_frame_stride_is_passed_through(monkeypatch):
    """tokens as a view whose frame stride exceeds C 3R^2: ops hands the view's pointer and stride to the library (no
    copy), and the gradients equal those of a contiguous copy bit for bit."""
    from audio_motion_avatar_amd import _lib, ops

    F, N, C, R = 3, 500, 24, 16
    S = 3 * R * R
    case = make_case(F, N, C, R, seed=571)
    lib = _lib.lib()
    seen = []
    for name in ("amav_triplane_project_region", "amav_triplane_decode_backward"):
        orig = getattr(lib, name)

        def spy(*args, _orig=orig, _name=name):
            if _name == "amav_triplane_project_region":
                seen.append((_name, args[3], args[4]))
            else:
                a = args[0]._obj
                seen.append((_name, a.tokens, a.tokens_frame_stride))
            return _orig(*args)

        monkeypatch.setattr(lib, name, spy)
    for pad in (4, 1):  # 16-B aligned frames, and not (the forward's scalar path)
        slab = torch.zeros(F, C * S + pad)
        slab[:, :C * S] = case["tokens"].reshape(F, C * S)
        slab = slab.cuda().requires_grad_()
        tokens = slab[:, :C * S].view(F, C, S)
        assert tokens.stride(0) == C * S + pad
        c = lambda t: t.cuda().clone().requires_grad_()  # noqa: E731
        pts, tr = c(case["points"]), c(case["transl"])
        heads = {k: (c(w), c(b)) for k, (w, b) in case["heads"].items()}
        wpl, wpt = ops.pack_head_weights(heads, C, "cuda", differentiable=True)
        seen.clear()
        rec = ops.triplane_decode_differentiable(tokens, wpl, wpt, pts, tr, R, case["radius"])
        (rec * case["grec"].cuda()).sum().backward()
        assert [s[0] for s in seen] == ["amav_triplane_project_region", "amav_triplane_decode_backward"]
        for name, ptr, stride in seen:
            assert ptr == tokens.data_ptr() and stride == C * S + pad, name
        want, want_rec = gpu_grads(case)
        assert torch.equal(rec.detach().cpu(), want_rec)
        assert torch.equal(slab.grad[:, :C * S].reshape(F, C, S).cpu(), want["tokens"])
        assert (slab.grad[:, C * S:] == 0).all()
        got = dict(points=pts.grad, transl=tr.grad)
        for k, (w, b) in heads.items():
            got[k + ".weight"], got[k + ".bias"] = w.grad, b.grad
        for k, v in got.items():
            assert torch.equal(v.cpu(), want[k]), (pad, k)


# ---- Renderer ------------------------------------------------------------------------------------------------------
def _renderer(F=4, size=96, seed=3, C=32, **cfg_kw):
    from audio_motion_avatar_amd.config import RendererConfig
    from audio_motion_avatar_amd.renderer import Renderer
    from audio_motion_avatar_amd.synthetic import init_random_heads, make_render_inputs

    cfg = RendererConfig(image_size=(size, size), subdivide_steps=0, predict_smplx_params=False, device="cuda",
                         triplane_feature_dim=C, **cfg_kw)
    r = init_random_heads(Renderer(cfg).eval())
    tokens, smpl, cam = make_render_inputs(F, cfg, seed=seed)
    return r, cfg, tokens, smpl, cam


def test_renderer_images_and_records_unchanged_with_grad():
    r, cfg, tokens, smpl, cam = _renderer()
    F = tokens.shape[1]
    st = torch.zeros(1, F, 1, 1, device="cuda")
    with torch.no_grad():
        ref_rgba, ref_packed = [t.clone() for t in r.render_tokens(tokens[0], smpl, cam)]
        ref_img, ref_g = r(tokens, cam, st, smpl)
    tok = tokens.clone().requires_grad_()
    rgba, packed = r.render_tokens(tok[0], smpl, cam)
    assert rgba.grad_fn is not None and packed.grad_fn is not None
    assert torch.equal(rgba, ref_rgba) and torch.equal(packed, ref_packed)
    img, g = r(tok, cam, st, smpl)
    assert img.grad_fn is not None
    assert torch.equal(img, ref_img)
    for k in ref_g:
        assert torch.equal(g[k], ref_g[k]), k


def test_renderer_gradient_chain_is_the_decode_backward(monkeypatch):
    from audio_motion_avatar_amd import losses, ops

    r, cfg, tokens, smpl, cam = _renderer(seed=8)
    F = tokens.shape[1]
    with torch.no_grad():
        target = r(tokens * 0.9, cam, torch.zeros(1, F, 1, 1, device="cuda"), smpl)[0]
    seen = {}
    orig = ops.triplane_decode_differentiable

    def spy(*args, **kw):
        out = orig(*args, **kw)
        seen["args"] = (args, kw)
        out.register_hook(lambda g: seen.__setitem__("grad", g.clone()))
        return out

    monkeypatch.setattr(ops, "triplane_decode_differentiable", spy)
    tok = tokens.clone().requires_grad_()
    img, _ = r(tok, cam, torch.zeros(1, F, 1, 1, device="cuda"), smpl)
    loss = losses.l1_loss(img, target) + 0.1 * (1.0 - losses.ssim(img, target))  # [B,T,H,W,3]
    loss.backward()
    assert float(seen["grad"].abs().max()) > 0
    with torch.no_grad():
        pts = r.get_smpl_vertices(smpl)
        wpl, wpt = r._head_weights()
        boxes = ops.points_bbox(pts)
        R = cfg.triplane_resolution
        proj = ops.triplane_project(tokens[0], wpl, R, region=(boxes, cfg.radius))
        want = ops.triplane_decode_backward(tokens[0], wpl, wpt, pts, proj, seen["grad"], cfg.radius, boxes=boxes)
    assert torch.equal(tok.grad[0], want["tokens"])
    C = cfg.triplane_feature_dim
    rows = {"xyz_layer": (0, 3), "opacity_layer": (3, 1), "rotation_layer": (4, 4), "scaling_layer": (8, 3),
            "shs_layer": (12, 3)}
    gd = r.gaussian_decoder
    for name, (o, n) in rows.items():
        layer = getattr(gd, name)
        wg = torch.cat([want["head_w_point"][o:o + n, :3],
                        want["head_w_plane"][:, :, o:o + n].permute(2, 0, 1).reshape(n, 3 * C)], dim=1)
        assert torch.equal(layer.weight.grad, wg), name
        assert torch.equal(layer.bias.grad, want["head_w_point"][o:o + n, 3]), name


def test_fit_from_reference_initialisation():
    from audio_motion_avatar_amd import losses
    from audio_motion_avatar_amd.renderer import Renderer

    r_true, cfg, tokens, smpl, cam = _renderer(F=2, size=64, seed=21)
    F = tokens.shape[1]
    st = torch.zeros(1, F, 1, 1, device="cuda")
    with torch.no_grad():
        target = r_true(tokens, cam, st, smpl)[0]
    r = Renderer(cfg).eval()  # the reference's zero-initialised heads
    opt = torch.optim.Adam(r.gaussian_decoder.parameters(), lr=3e-3)

    def loss_of():
        img = r(tokens, cam, st, smpl)[0]
        return losses.l1_loss(img, target) + 0.1 * (1.0 - losses.ssim(img, target))

    first = None
    for _ in range(300):
        opt.zero_grad()
        loss = loss_of()
        first = float(loss.detach()) if first is None else first
        loss.backward()
        opt.step()
    with torch.no_grad():
        last = float(loss_of())
    print(f"\nfit: loss {first:.4e} -> {last:.4e} (factor {last / first:.3f})")
    assert last < 0.5 * first


def test_refusals_under_grad():
    from audio_motion_avatar_amd.config import RendererConfig
    from audio_motion_avatar_amd.renderer import Renderer
    from audio_motion_avatar_amd.smplx_decoder import SMPLXDecoder
    from audio_motion_avatar_amd.synthetic import make_render_inputs

    r, cfg, tokens, smpl, cam = _renderer(F=2, size=64)
    tok = tokens[0].clone().requires_grad_()
    with pytest.raises(NotImplementedError, match="chunks"):
        r.render_tokens(tok, smpl, cam, chunks=2)
    with pytest.raises(NotImplementedError, match="wire"):
        r.render_tokens(tok, smpl, cam, wire=(torch.zeros(16, dtype=torch.uint8, device="cuda"), 4))
    with pytest.raises(NotImplementedError, match="fuse_decode"):
        r.render_tokens(tok, smpl, cam, fuse_decode=True)
    posed = dict(smpl, body_pose=smpl["body_pose"].clone().requires_grad_())
    with pytest.raises(NotImplementedError, match="body_pose"):
        r.render_tokens(tok, posed, cam)
    # the point refiner: the refusal is keyed on its encoder module being present
    r.point_encoder = torch.nn.Identity()
    with pytest.raises(NotImplementedError, match="point refiner"):
        r.render_tokens(tok, smpl, cam)
    del r.point_encoder
    # upsampler
    up_cfg = RendererConfig(image_size=(64, 64), subdivide_steps=0, predict_smplx_params=False, device="cuda",
                            triplane_feature_dim=8, triplane_resolution=8, upsample_triplane=True, num_upsample_blocks=1)
    up = Renderer(up_cfg).eval()
    t8, s8, c8 = make_render_inputs(2, up_cfg, seed=1)
    with pytest.raises(NotImplementedError, match="upsampler"):
        up(t8.requires_grad_(), c8, torch.zeros(1, 2, 1, 1, device="cuda"), s8)
    # SMPL-X parameters predicted by a decoder that requires grad (LBS has no backward)
    dcfg = RendererConfig(image_size=(64, 64), subdivide_steps=0, predict_smplx_params=True, device="cuda",
                          triplane_feature_dim=32)
    dr = Renderer(dcfg, smpl_decoder=SMPLXDecoder(dcfg).cuda()).eval()
    t2, _, c2 = make_render_inputs(2, dcfg, seed=2)
    st = torch.randn(1, 2, dcfg.smpl_token_len, dcfg.smpl_token_dim, device="cuda")
    with pytest.raises(NotImplementedError, match="LBS"):
        dr(t2, c2, st)
    with torch.no_grad():  # the same calls without gradients still run
        r.render_tokens(tokens[0], smpl, cam, chunks=2)
        dr(t2, c2, st)
