"""Training through the triplane upsampler on the device (cfg.differentiable_upsampler): the
windowed evaluation as an autograd graph -- library convolution backwards, HIP window cuts -- against fp64 CPU
gradients of the full planes, and Renderer.forward end to end, with the point refiner, in passes, and its refusals."""
import pytest
import torch

import upsampler_cases as uc

pytestmark = pytest.mark.gpu

# the small PTv3 of tests/test_point_refiner_gpu.py::test_windowed_upsampler_with_refiner_and_fallback (copied)
PCFG = dict(stride=(2,), enc_depths=(1, 1), enc_channels=(32, 64), enc_num_head=(2, 4), enc_patch_size=(256, 256),
            dec_depths=(1,), dec_channels=(32,), dec_num_head=(2,), dec_patch_size=(256,))


@pytest.mark.parametrize("box", sorted(uc.BOXES))
@pytest.mark.parametrize("n_blocks,R", uc.CASES)
def test_windowed_chain_gradients_stay_within_the_librarys_own_error(n_blocks, R, box):
    """Loss = weighted sum of ops.triplane_sample_features_differentiable on the windowed slab; every gradient against
    the fp64 CPU gradients of the full planes (upsampler_cases.reference_gradients), relative to max |grad| per tensor.

    The yardstick is the library: e_lib is the same error of plain fp32 full-plane forward_tokens + torch autograd
    (grid_sample) on the device.  The windowed path must stay within 4 e_lib: its mosaic images make the library pick
    other convolution kernels than whole planes do, and its sums run in another order, but it is the same arithmetic
    at the same precision.  Both values are printed per tensor."""
    from audio_motion_avatar_amd import ops

    want = uc.reference_gradients(n_blocks, R, box)
    r_out = R * 2 ** n_blocks
    tokens, points, weights = (t.cuda() for t in uc.make_inputs(n_blocks, R, box))

    up = uc.make_upsampler(n_blocks).cuda()
    tok = tokens.clone().requires_grad_()
    uc.oracle_loss(up.forward_tokens(tok, R), points, weights, r_out).backward()
    lib = uc.gradients(up, tok)

    up = uc.make_upsampler(n_blocks).cuda()
    plan = uc.fresh_plan(up, points, R)
    assert all(w["tiles"] is not None and len(w["tiles"]) > 0 and bool((~w["mask"]).any()) for w in plan)
    tok = tokens.clone().requires_grad_()
    slab = up.forward_tokens_windowed(tok, R, plan, differentiable=True)
    planes = slab.view(uc.F, uc.C, 3, r_out, r_out).permute(0, 2, 1, 3, 4)
    (ops.triplane_sample_features_differentiable(planes, points, uc.RADIUS) * weights).sum().backward()
    got = uc.gradients(up, tok)

    assert set(got) == set(want) == set(lib)
    failed = []
    for name in sorted(want):
        e_win, e_lib = uc.relative_error(got[name], want[name]), uc.relative_error(lib[name], want[name])
        print(f"blocks {n_blocks} {box} {name}: windowed {e_win:.3e}  library full planes {e_lib:.3e}  "
              f"ratio {e_win / max(e_lib, 1e-300):.2f}")
        assert torch.isfinite(got[name]).all(), name
        if not e_win <= 4 * e_lib:
            failed.append((name, e_win, e_lib))
    assert not failed, failed


def _config(**over):
    from audio_motion_avatar_amd.config import RendererConfig

    kw = dict(image_size=(64, 64), subdivide_steps=0, triplane_feature_dim=8, triplane_resolution=16,
              predict_smplx_params=False, num_gaussians=1500, upsample_triplane=True, num_upsample_blocks=2,
              differentiable_upsampler=True)
    kw.update(over)
    return RendererConfig(**kw)


def _renderer(cfg, std=0.05):
    from audio_motion_avatar_amd.renderer import Renderer
    from audio_motion_avatar_amd.synthetic import init_random_heads

    torch.manual_seed(0)
    return init_random_heads(Renderer(cfg).eval(), std=std)


def _upsampler_parameters(r):
    return {k: p for k, p in r.named_parameters() if k.startswith("triplane_upsampler.")}


def _assert_gradients(named, what):
    for k, g in named.items():
        assert g is not None and torch.isfinite(g).all() and bool((g != 0).any()), (what, k)


def test_an_image_loss_trains_the_upsampler():
    """Renderer end to end at its smallest: only the upsampler's parameters and the coarse tokens require grad (the
    heads are frozen, so the graph is recorded because of THEM).  Every one of them gets a finite, non-zero gradient,
    and 12 Adam steps of l1 + 0.1 (1 - ssim) towards frames rendered from perturbed upsampler weights lower the loss."""
    from audio_motion_avatar_amd import losses
    from audio_motion_avatar_amd.synthetic import make_render_inputs

    r = _renderer(_config())
    tokens, smpl, cam = make_render_inputs(2, r.cfg, seed=4)
    zeros = torch.zeros(1, 2, 1, 1, device="cuda")
    trainable = _upsampler_parameters(r)
    assert len(trainable) == len(list(r.triplane_upsampler.parameters())) > 20
    for k, p in r.named_parameters():
        p.requires_grad_(k in trainable)
    saved = {k: p.detach().clone() for k, p in trainable.items()}
    g = torch.Generator().manual_seed(31)
    with torch.no_grad():
        for p in trainable.values():
            p.add_((torch.randn(p.shape, generator=g) * 0.05).cuda())
        target, _ = r(tokens, cam, zeros, smpl)
        for k, p in trainable.items():
            p.copy_(saved[k])
    tok = tokens.clone().requires_grad_()
    opt = torch.optim.Adam(trainable.values(), lr=1e-3)
    history = []
    for step in range(12):
        opt.zero_grad(set_to_none=True)
        images, _ = r(tok, cam, zeros, smpl)
        assert images.requires_grad
        loss = losses.l1_loss(images, target) + 0.1 * (1.0 - losses.ssim(images, target))
        loss.backward()
        if step == 0:
            _assert_gradients({k: p.grad for k, p in trainable.items()}, "upsampler")
            _assert_gradients({"tokens": tok.grad}, "tokens")
            assert all(w["tiles"] is not None for w in r.last_window_plan)  # the windowed path ran
        opt.step()
        history.append(float(loss.detach()))
    print("losses:", " ".join(f"{v:.6f}" for v in history))
    assert all(v == v for v in history) and history[-1] < history[0], history
    # whole planes under autograd (upsample_windows=False) deliver gradients too
    r.cfg.upsample_windows = False
    r.zero_grad(set_to_none=True)
    tok.grad = None
    images, _ = r(tok, cam, zeros, smpl)
    (images - target).abs().mean().backward()
    _assert_gradients({k: p.grad for k, p in trainable.items()}, "upsampler, whole planes")
    _assert_gradients({"tokens": tok.grad}, "tokens, whole planes")


def test_refined_points_that_leave_the_plan_fall_back_under_grad():
    """With the refiner's flags on as well: a uniform shift of every refined point (zero last-layer weight, constant
    bias, as test_windowed_upsampler_with_refiner_and_fallback forces it) past the planned margin must take the
    full-plane fallback -- forward_tokens, called under grad mode -- and still deliver the gradients."""
    from audio_motion_avatar_amd.synthetic import make_render_inputs

    r = _renderer(_config(triplane_feature_dim=16, triplane_resolution=32, num_gaussians=1200, radius=2.8,
                          no_point_refiner=False, differentiable_refiner=True, differentiable_refine_points=True, **PCFG))
    tokens, smpl, cam = make_render_inputs(2, r.cfg, seed=9)
    zeros = torch.zeros(1, 2, 1, 1, device="cuda")
    up = r.triplane_upsampler
    orig = up.forward_tokens
    for shift, expect_fallback in ((0.02, False), (1.5, True)):  # metres; the planned margin is 0.05 m + tile rounding
        with torch.no_grad():
            r.point_refiner[-1].weight.zero_()
            r.point_refiner[-1].bias.fill_(shift)
        calls = []
        up.forward_tokens = lambda *a, **k: (calls.append(torch.is_grad_enabled()), orig(*a, **k))[1]
        try:
            r.zero_grad(set_to_none=True)
            tok = tokens.clone().requires_grad_()
            images, _ = r(tok, cam, zeros, smpl)
        finally:
            up.forward_tokens = orig
        assert calls == ([True] if expect_fallback else []), (shift, calls)
        assert images.requires_grad
        (1.0 - images).abs().mean().backward()
        _assert_gradients({k: p.grad for k, p in _upsampler_parameters(r).items()}, f"upsampler, shift {shift}")
        _assert_gradients({"tokens": tok.grad, "refiner bias": r.point_refiner[-1].bias.grad}, f"shift {shift}")


def test_refusals_stay_and_inference_is_unchanged():
    from audio_motion_avatar_amd.synthetic import make_render_inputs

    on, off = _renderer(_config()), _renderer(_config(differentiable_upsampler=False))
    off.load_state_dict(on.state_dict())
    tokens, smpl, cam = make_render_inputs(3, on.cfg, seed=4)
    zeros = torch.zeros(1, 3, 1, 1, device="cuda")
    # flag off: refused under grad, as before
    with pytest.raises(NotImplementedError, match="the triplane upsampler has no backward"):
        off(tokens.clone().requires_grad_(), cam, zeros, smpl)
    with torch.no_grad():
        plan = off.triplane_upsampler.plan_windows(off.get_smpl_vertices(smpl), 16, off.cfg.radius)
        fine = off.triplane_upsampler.forward_tokens_windowed(tokens[0], 16, plan).clone()
    for fn in (off.gaussians_from_tokens, lambda *a, **k: off.render_tokens(*a[:2], cam, **k)):
        with pytest.raises(NotImplementedError, match="window_plan"):
            fn(fine.requires_grad_(), smpl, window_plan=plan)
    # training mode stays refused, flag or not
    on.triplane_upsampler.train()
    with pytest.raises(Exception, match="training mode"):
        on(tokens.clone().requires_grad_(), cam, zeros, smpl)
    on.triplane_upsampler.eval()
    # flag on, no grad: the inference path, bit for bit (cached slab and all)
    with torch.no_grad():
        img_on, g_on = on(tokens, cam, zeros, smpl)
        img_off, g_off = off(tokens, cam, zeros, smpl)
    assert img_on.grad_fn is None and torch.equal(img_on, img_off)
    for k in g_off:
        assert torch.equal(g_on[k], g_off[k]), k
    assert getattr(on.triplane_upsampler, "_slab", None) is not None
    # ... and with grad mode on but nothing that requires grad
    for p in on.parameters():
        p.requires_grad_(False)
    img, _ = on(tokens, cam, zeros, smpl)
    assert img.grad_fn is None and torch.equal(img, img_off)


def test_passes_of_a_long_call_give_the_same_gradients():
    """upsample_frames_per_pass = 2 on four frames (P = 2 passes) against one pass.  Frames are independent, so both
    compute the same sums; the passes only change the images the library's convolutions see (another kernel, another
    summation order) and add each parameter's P partial gradients in P - 1 further fp32 additions.
    Bound per tensor: (P + 1) * 2e-5 * max |grad| -- 2e-5 of the largest entry is the floor this suite allows ONE fp32
    evaluation of a rendering chain against exact arithmetic (tests/test_refiner_renderer_training_gpu.py); the single
    pass is one such evaluation and each of the P passes another, and the P - 1 additions (2^-24 each) vanish in it."""
    from audio_motion_avatar_amd.synthetic import make_render_inputs

    P = 2
    one, split = _renderer(_config()), _renderer(_config(upsample_frames_per_pass=2))
    split.load_state_dict(one.state_dict())
    tokens, smpl, cam = make_render_inputs(2 * P, one.cfg, seed=4)
    zeros = torch.zeros(1, 2 * P, 1, 1, device="cuda")
    g = torch.Generator().manual_seed(5)
    cot = torch.randn(1, 2 * P, 64, 64, 3, generator=g).cuda()
    grads = []
    for r in (one, split):
        tok = tokens.clone().requires_grad_()
        images, _ = r(tok, cam, zeros, smpl)
        (images * cot).sum().backward()
        named = {k: p.grad for k, p in r.named_parameters() if p.grad is not None}
        named["tokens"] = tok.grad
        grads.append(named)
    assert set(grads[0]) == set(grads[1]) and set(_upsampler_parameters(one)) <= set(grads[0])
    worst = 0.0
    for k in sorted(grads[0]):
        a, b = grads[0][k].double(), grads[1][k].double()
        rel = float((a - b).abs().max()) / max(float(a.abs().max()), 1e-300)
        worst = max(worst, rel)
        assert rel <= (P + 1) * 2e-5, (k, rel)
    print(f"split in {P} passes vs one pass: worst relative difference {worst:.3e} (bound {(P + 1) * 2e-5:.1e})")
