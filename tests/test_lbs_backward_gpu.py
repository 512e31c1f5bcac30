"""GPU checks of the SMPL-X LBS backward (amav_lbs_backward), the gather backward (amav_points_gather_backward), their
autograd Functions, BodyModel under grad and Renderer(differentiable_smplx=True).  Gradients are compared with fp64
autograd of oracle.lbs.lbs (bound: max |g - g_ref| / max |g_ref| <= 1e-4 per tensor, ratios printed)."""
import functools

import numpy as np
import pytest
import torch

from helpers import random_pose

pytestmark = pytest.mark.gpu
BOUND = 1e-4
NAMES = ("global_orient", "body_pose", "jaw_pose", "leye_pose", "reye_pose", "left_hand_pose", "right_hand_pose")
WIDTHS = (3, 63, 3, 3, 3, 45, 45)


@functools.lru_cache(maxsize=1)
def body():
    from audio_motion_avatar_amd.body_model import BodyModel

    return BodyModel.synthetic_model(seed=42, device="cuda")


def _split(full):
    out, c = [], 0
    for w in WIDTHS:
        out.append(full[:, c:c + w])
        c += w
    return out


def _pose(seed, F, scale):
    pose, coeffs = random_pose(seed, F, scale=scale)
    pose[:, 66:75] = 0.0  # jaw and both eyes exactly zero: Rodrigues at r = 0
    return pose, coeffs


def reference_grads(b, pose, coeffs, G):
    from oracle import lbs

    m = b.oracle_arrays(torch.float64)
    p = pose.double().requires_grad_()
    c = coeffs.double().requires_grad_()
    v, _, _ = lbs.lbs(c, p + m["pose_mean"], m)
    (v * G.double()).sum().backward()
    return p.grad, c.grad


def _ratio(got, ref):
    return float((got.detach().cpu().double() - ref).abs().max() / ref.abs().max())


def _gpu_grads_through_function(b, pose, coeffs, G):
    from audio_motion_avatar_amd import ops

    parts = [p.clone().requires_grad_() for p in _split(pose.cuda())]
    coef = [coeffs[:, :10].cuda().requires_grad_(), coeffs[:, 10:].cuda().requires_grad_()]
    verts = ops.lbs_differentiable(b.device_tables(), parts, coef, pose_mean=b.pose_mean)
    with torch.no_grad():
        plain = ops.lbs_forward_parts(b.device_tables(), parts, coef, pose_mean=b.pose_mean)
    assert torch.equal(verts.detach(), plain)  # the forward is lbs_forward_parts, bit for bit
    verts.backward(G.cuda())
    return torch.cat([p.grad for p in parts], 1), torch.cat([c.grad for c in coef], 1)


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("F", [1, 6, 16, 17, 40])  # FMA forwards (<= 16), MFMA forwards (fp32 or split table)
def test_gradients_match_fp64_autograd(F, split):
    from audio_motion_avatar_amd import ops

    b = body()
    pose, coeffs = _pose(500 + F, F, 0.3)
    G = torch.randn(F, b.num_verts, 3, generator=torch.Generator().manual_seed(F))
    ops.set_option("lbs", "split" if split else "f32")
    try:
        gp, gc = _gpu_grads_through_function(b, pose, coeffs, G)
    finally:
        ops.set_option("lbs", "default")
    rp, rc = reference_grads(b, pose, coeffs, G)
    ratios = _ratio(gp, rp), _ratio(gc, rc)
    print(f"\nF={F} split={split}: pose {ratios[0]:.2e}, coeffs {ratios[1]:.2e}")
    assert torch.isfinite(gp).all() and torch.isfinite(gc).all()
    assert max(ratios) <= BOUND


@pytest.mark.parametrize("scale", [1e-3, 0.3, 1.5])
def test_gradients_across_pose_scales(scale):
    b = body()
    F = 17
    pose, coeffs = _pose(700, F, scale)
    G = torch.randn(F, b.num_verts, 3, generator=torch.Generator().manual_seed(3))
    gp, gc = _gpu_grads_through_function(b, pose, coeffs, G)
    rp, rc = reference_grads(b, pose, coeffs, G)
    ratios = _ratio(gp, rp), _ratio(gc, rc)
    zero = _ratio(gp[:, 66:75], rp[:, 66:75]) * float(rp.abs().max() / rp[:, 66:75].abs().max())
    print(f"\nscale {scale}: pose {ratios[0]:.2e}, coeffs {ratios[1]:.2e}, zero joints (own scale) {zero:.2e}")
    assert max(ratios) <= BOUND
    # the exactly-zero joints (Rodrigues' eps branch) against their own largest gradient: their dA terms cancel more
    # (vertices close to the joint), so the bar is 1e-3 there; a wrong eps branch would be off by O(1) or non-finite
    assert torch.isfinite(gp[:, 66:75]).all() and zero <= 1e-3


@pytest.mark.parametrize("F", [3, 40])
def test_dense_skin_weights_and_a_non_zero_hand_mean(F):
    from audio_motion_avatar_amd.body_model import BodyModel, _synthetic_arrays

    arrays = dict(_synthetic_arrays(42))
    rng = np.random.default_rng(7)
    V, J = arrays["lbs_weights"].shape
    W = np.zeros((V, J))
    for v in range(V):
        k = int(rng.integers(8, 13))
        js = rng.choice(J, size=k, replace=False)
        w = rng.random(k) ** 3 + 1e-3
        W[v, js] = w / w.sum()
    arrays["lbs_weights"] = W
    mean = np.zeros(J * 3)
    mean[75:165] = rng.normal(0.0, 0.25, 90)
    arrays["pose_mean"] = mean
    b = BodyModel(arrays, "cuda", True)
    pose, coeffs = _pose(300 + F, F, 0.3)
    G = torch.randn(F, V, 3, generator=torch.Generator().manual_seed(11))
    gp, gc = _gpu_grads_through_function(b, pose, coeffs, G)
    rp, rc = reference_grads(b, pose, coeffs, G)
    ratios = _ratio(gp, rp), _ratio(gc, rc)
    print(f"\ndense weights F={F}: pose {ratios[0]:.2e}, coeffs {ratios[1]:.2e}")
    assert max(ratios) <= BOUND


def _gather_table(levels, N, seed):
    from audio_motion_avatar_amd.body_model import build_subdivision_table

    b = body()
    g = torch.Generator().manual_seed(seed)
    if levels == 0:
        ids = torch.randperm(b.num_verts, generator=g)[:N].to(torch.int32)
        return ids[:, None].repeat(1, 4).contiguous()
    table = torch.as_tensor(build_subdivision_table(b.faces, b.num_verts, levels))
    return table[torch.randperm(table.shape[0], generator=g)[:N]].contiguous()


@pytest.mark.parametrize("levels", [0, 1, 2])
def test_gather_backward_matches_fp64_autograd(levels):
    from audio_motion_avatar_amd import ops

    V, F, N = body().num_verts, 3, 10000
    idx = _gather_table(levels, N, levels)
    verts = torch.randn(F, V, 3, generator=torch.Generator().manual_seed(1))
    G = torch.randn(F, N, 3, generator=torch.Generator().manual_seed(2))
    vg = verts.cuda().requires_grad_()
    pts = ops.points_gather_differentiable(vg, idx.cuda())
    assert torch.equal(pts.detach(), ops.points_gather(verts.cuda(), idx.cuda()))
    pts.backward(G.cuda())
    v64 = verts.double().requires_grad_()
    i = idx.long()
    p = ((v64[:, i[:, 0]] + v64[:, i[:, 1]]) * 0.5 + (v64[:, i[:, 2]] + v64[:, i[:, 3]]) * 0.5) * 0.5
    (p * G.double()).sum().backward()
    ratio = _ratio(vg.grad, v64.grad)
    unref = torch.ones(V, dtype=torch.bool)
    unref[i.reshape(-1)] = False
    got = vg.grad.cpu()
    print(f"\ngather levels {levels}: {ratio:.2e}, {int(unref.sum())} unreferenced vertices")
    assert ratio <= 1e-6
    assert int(unref.sum()) > 0
    assert (got[:, unref] == 0).all() and not torch.signbit(got[:, unref]).any()  # exactly +0


def test_part_gradients_strided_broadcast_and_contiguous_agree():
    from audio_motion_avatar_amd import ops

    b = body()
    F = 20
    pose, coeffs = _pose(41, F, 0.3)
    G = torch.randn(F, b.num_verts, 3, generator=torch.Generator().manual_seed(4)).cuda()
    # strided: every part a column slice of one wider leaf; betas broadcast from one row
    wide = torch.zeros(F, 200, device="cuda")
    cols, c0 = [], 0
    for w in WIDTHS:
        cols.append((c0 + 7, c0 + 7 + w))
        c0 += w + 3
    with torch.no_grad():
        for (a, e), part in zip(cols, _split(pose.cuda())):
            wide[:, a:e] = part
    wide.requires_grad_()
    betas_row = coeffs[:1, :10].cuda().requires_grad_()
    expr = coeffs[:, 10:].cuda().requires_grad_()
    verts = ops.lbs_differentiable(b.device_tables(), [wide[:, a:e] for a, e in cols],
                                   [betas_row.expand(F, 10), expr], pose_mean=b.pose_mean)
    verts.backward(G)
    # contiguous copies
    parts = [wide.detach()[:, a:e].clone().requires_grad_() for a, e in cols]
    betas = betas_row.detach().expand(F, 10).clone().requires_grad_()
    expr2 = expr.detach().clone().requires_grad_()
    verts2 = ops.lbs_differentiable(b.device_tables(), parts, [betas, expr2], pose_mean=b.pose_mean)
    assert torch.equal(verts.detach(), verts2.detach())
    verts2.backward(G)
    for (a, e), p in zip(cols, parts):
        assert torch.equal(wide.grad[:, a:e], p.grad)
    assert (wide.grad[:, :7] == 0).all()
    assert torch.equal(betas_row.grad, betas.grad.sum(0, keepdim=True))
    assert torch.equal(expr.grad, expr2.grad)


def test_body_model_call_under_grad_reaches_all_nine_arguments():
    from audio_motion_avatar_amd import ops

    b = body()
    F = 5
    pose, coeffs = _pose(9, F, 0.3)
    G = torch.randn(F, b.num_verts, 3, generator=torch.Generator().manual_seed(5)).cuda()
    kw = {n: p.cuda().reshape(F, -1, 3).squeeze(1).clone().requires_grad_() for n, p in zip(NAMES, _split(pose))}
    kw["betas"] = coeffs[:, :10].cuda().requires_grad_()
    kw["expression"] = coeffs[:, 10:].cuda().requires_grad_()
    with torch.no_grad():
        plain = b(**kw).vertices
    out = b(**kw).vertices
    assert out.grad_fn is not None and torch.equal(out.detach(), plain)
    out.backward(G)
    gp, gc = ops.lbs_backward(b.device_tables(), _split(pose.cuda()), [coeffs[:, :10].cuda(), coeffs[:, 10:].cuda()], G,
                              pose_mean=b.pose_mean)
    for n, w in zip(NAMES, _split(gp)):
        assert kw[n].grad is not None and torch.equal(kw[n].grad.reshape(F, -1), w), n
    assert torch.equal(kw["betas"].grad, gc[:, :10]) and torch.equal(kw["expression"].grad, gc[:, 10:])
    # float64 arguments: assembled in float64 with torch, then the full-pose Function
    kw64 = {k: v.detach().double().requires_grad_() for k, v in kw.items()}
    with torch.no_grad():
        plain64 = b(**kw64).vertices
    out64 = b(**kw64).vertices
    assert torch.equal(out64.detach(), plain64)
    out64.backward(G)
    rp, rc = reference_grads(b, pose, coeffs, G.cpu())
    got = torch.cat([kw64[n].grad.reshape(F, -1) for n in NAMES], 1)
    assert kw64["betas"].grad.dtype == torch.float64
    assert _ratio(got, rp) <= BOUND
    assert _ratio(torch.cat([kw64["betas"].grad, kw64["expression"].grad], 1), rc) <= BOUND


def test_deterministic_and_independent_of_frame_slicing():
    from audio_motion_avatar_amd import ops

    b = body()
    F = 250
    pose, coeffs = _pose(13, F, 0.5)
    pose, coeffs = pose.cuda(), coeffs.cuda()
    G = torch.randn(F, b.num_verts, 3, generator=torch.Generator().manual_seed(6)).cuda()
    run = lambda s, e: ops.lbs_backward(b.device_tables(), _split(pose[s:e]), [coeffs[s:e, :10], coeffs[s:e, 10:]],  # noqa: E731
                                        G[s:e], pose_mean=b.pose_mean)
    a = run(0, F)
    a2 = run(0, F)
    assert torch.equal(a[0], a2[0]) and torch.equal(a[1], a2[1])
    parts = [run(s, s + 25) for s in range(0, F, 25)]
    assert torch.equal(a[0], torch.cat([p[0] for p in parts])) and torch.equal(a[1], torch.cat([p[1] for p in parts]))
    idx = _gather_table(1, 10000, 0).cuda()
    csr = ops.points_gather_csr(idx, b.num_verts)
    gpts = torch.randn(F, 10000, 3, generator=torch.Generator().manual_seed(7)).cuda()
    g1 = ops.points_gather_backward(gpts, csr, b.num_verts)
    assert torch.equal(g1, ops.points_gather_backward(gpts, csr, b.num_verts))
    assert torch.equal(g1, torch.cat([ops.points_gather_backward(gpts[s:s + 25], csr, b.num_verts)
                                      for s in range(0, F, 25)]))


# ---- Renderer ------------------------------------------------------------------------------------------------------
def _renderer(F=4, size=96, seed=3, C=32, **cfg_kw):
    from audio_motion_avatar_amd.config import RendererConfig
    from audio_motion_avatar_amd.renderer import Renderer
    from audio_motion_avatar_amd.synthetic import init_random_heads, make_render_inputs

    cfg = RendererConfig(image_size=(size, size), subdivide_steps=0, predict_smplx_params=False, device="cuda",
                         triplane_feature_dim=C, differentiable_smplx=True, **cfg_kw)
    r = init_random_heads(Renderer(cfg).eval())
    tokens, smpl, cam = make_render_inputs(F, cfg, seed=seed)
    return r, cfg, tokens, smpl, cam


def _with_grad(smpl, keys=("global_orient", "body_pose", "betas", "jaw_pose")):
    return {k: (v.clone().requires_grad_() if k in keys else v) for k, v in smpl.items()}


def test_renderer_images_and_records_unchanged_with_grad():
    r, cfg, tokens, smpl, cam = _renderer()
    F = tokens.shape[1]
    st = torch.zeros(1, F, 1, 1, device="cuda")
    with torch.no_grad():
        ref_rgba, ref_packed = [t.clone() for t in r.render_tokens(tokens[0], smpl, cam)]
        ref_img, ref_g = r(tokens, cam, st, smpl)
    r.gaussian_decoder.requires_grad_(False)  # only the SMPL-X parameters require grad
    sg = _with_grad(smpl)
    rgba, packed = r.render_tokens(tokens[0], sg, cam)
    assert rgba.grad_fn is not None and packed.grad_fn is not None
    assert torch.equal(rgba, ref_rgba) and torch.equal(packed, ref_packed)
    img, g = r(tokens, cam, st, sg)
    assert img.grad_fn is not None and torch.equal(img, ref_img)
    for k in ref_g:
        assert torch.equal(g[k], ref_g[k]), k


def test_renderer_smplx_gradients_are_the_gather_and_lbs_backwards(monkeypatch):
    from audio_motion_avatar_amd import losses, ops

    r, cfg, tokens, smpl, cam = _renderer(seed=8)
    F = tokens.shape[1]
    st = torch.zeros(1, F, 1, 1, device="cuda")
    with torch.no_grad():
        target = r(tokens * 0.9, cam, st, smpl)[0]
    seen = {}
    orig = ops.triplane_decode_differentiable

    def spy(*args, **kw):
        args[3].register_hook(lambda g: seen.__setitem__("points", g.clone()))
        return orig(*args, **kw)

    monkeypatch.setattr(ops, "triplane_decode_differentiable", spy)
    sg = _with_grad(smpl, keys=("global_orient", "body_pose", "betas", "jaw_pose", "left_hand_pose", "expression"))
    img, _ = r(tokens, cam, st, sg)
    loss = losses.l1_loss(img, target) + 0.1 * (1.0 - losses.ssim(img, target))
    loss.backward()
    assert float(seen["points"].abs().max()) > 0
    b = r.smplx_model
    with torch.no_grad():
        gv = ops.points_gather_backward(seen["points"], (r._gather_csr_offsets, r._gather_csr_entries), b.num_verts)
        flat = {k: v.reshape(F, -1) for k, v in smpl.items()}
        gp, gc = ops.lbs_backward(b.device_tables(), [flat[n] for n in NAMES], [flat["betas"], flat["expression"]], gv,
                                  pose_mean=b.pose_mean)
    want = dict(zip(NAMES, _split(gp)), betas=gc[:, :10], expression=gc[:, 10:])
    for k, v in sg.items():
        if k in want and v.requires_grad:
            assert torch.equal(v.grad.reshape(F, -1), want[k]), k
            assert float(v.grad.abs().max()) > 0, k
    assert sg["reye_pose"].grad is None


def test_stage2_call_trains_the_smplx_decoder():
    from audio_motion_avatar_amd import losses
    from audio_motion_avatar_amd.config import RendererConfig
    from audio_motion_avatar_amd.renderer import Renderer
    from audio_motion_avatar_amd.smplx_decoder import SMPLXDecoder
    from audio_motion_avatar_amd.synthetic import init_random_heads, make_render_inputs

    cfg = RendererConfig(image_size=(64, 64), subdivide_steps=0, predict_smplx_params=True, device="cuda",
                         triplane_feature_dim=32, differentiable_smplx=True)
    dec = SMPLXDecoder(cfg).cuda()
    with torch.no_grad():  # put the predicted body in front of the camera
        dec.dec_transl.weight.mul_(0.01)
        dec.dec_transl.bias.copy_(torch.tensor([0.0, -0.15, 2.4]))
    r = init_random_heads(Renderer(cfg, smpl_decoder=dec).eval())
    tokens, _, cam = make_render_inputs(2, cfg, seed=2)
    st = torch.randn(1, 2, cfg.smpl_token_len, cfg.smpl_token_dim, device="cuda", requires_grad=True)
    img, _, pred = r(tokens, cam, st)
    target = torch.full_like(img, 0.5)
    loss = losses.l1_loss(img, target) + 0.1 * (1.0 - losses.ssim(img, target))
    loss.backward()
    for name in ("dec_body_pose", "dec_body_root_pose", "dec_body_shape", "dec_hand_pose", "dec_transl"):
        g = getattr(dec, name).weight.grad
        assert g is not None and torch.isfinite(g).all() and float(g.abs().max()) > 0, name
    assert dec.mlp[0].weight.grad is not None and float(dec.mlp[0].weight.grad.abs().max()) > 0
    assert torch.isfinite(st.grad).all() and float(st.grad.abs().max()) > 0


def test_pose_fit_from_a_perturbed_pose():
    from audio_motion_avatar_amd import losses

    r, cfg, tokens, smpl, cam = _renderer(F=2, size=96, seed=21)
    F = tokens.shape[1]
    st = torch.zeros(1, F, 1, 1, device="cuda")
    r.gaussian_decoder.requires_grad_(False)
    with torch.no_grad():
        target = r(tokens, cam, st, smpl)[0]
        target_verts = r._posed_vertices(smpl)
    g = torch.Generator().manual_seed(5)
    noise = lambda t: (torch.randn(t.shape, generator=g) * (0.15 / 3 ** 0.5)).cuda()  # noqa: E731  ~0.15 rad per joint
    params = {k: (smpl[k] + noise(smpl[k])).requires_grad_() for k in ("global_orient", "body_pose")}
    params["betas"] = smpl["betas"].clone().requires_grad_()
    opt = torch.optim.Adam([{"params": [params["global_orient"], params["body_pose"]], "lr": 1e-2},
                            {"params": [params["betas"]], "lr": 1e-3}])
    steps = 300
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda i: 1.0 - 0.9 * i / steps)

    def current():
        return dict(smpl, **params)

    def loss_of():
        img = r(tokens, cam, st, current())[0]
        return losses.l1_loss(img, target) + 0.1 * (1.0 - losses.ssim(img, target))

    with torch.no_grad():
        dist0 = float((r._posed_vertices(current()) - target_verts).norm(dim=-1).mean())
    first = None
    for _ in range(steps):
        opt.zero_grad()
        loss = loss_of()
        first = float(loss.detach()) if first is None else first
        loss.backward()
        opt.step()
        sched.step()
    with torch.no_grad():
        last = float(loss_of())
        dist1 = float((r._posed_vertices(current()) - target_verts).norm(dim=-1).mean())
    print(f"\npose fit: loss {first:.4e} -> {last:.4e} (factor {last / first:.3f}); mean vertex distance "
          f"{dist0 * 1e3:.2f} -> {dist1 * 1e3:.2f} mm")
    assert last < 0.5 * first
    assert dist1 < dist0
