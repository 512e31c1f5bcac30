"""Stage-1 training (TriplaneGaussianAvatar.training_step, lightning_model_wrapper.py:82-170) on the MI355X: every
stage-1 parameter receives a gradient (the point network, vertex_emb and ImageFeature through the HIP backwards of the
encoder's reductions), the loss is the reference's formula, a short Adam fit lowers it, and one step runs at the
reference's widths."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu


def _model(cfg, seed=0):
    from audio_motion_avatar_amd.synthetic import init_random_heads
    from audio_motion_avatar_amd.triplane_net import TriplaneGaussianAvatar

    torch.manual_seed(seed)
    model = TriplaneGaussianAvatar(cfg).eval()
    init_random_heads(model.renderer)
    with torch.no_grad():  # the reference zero-initialises them: every gradient upstream would be 0 at step 0
        for blk in model.smplx_triplane_encoder.blocks:
            blk.fc_1.weight.normal_(0, 0.02)
    return model


def _small_cfg():
    from audio_motion_avatar_amd.config import Stage1Config

    return Stage1Config(image_size=(64, 48), subdivide_steps=0, smplx_transformer_layers=1, cross_transformer_layers=1,
                        device="cuda")


def _inputs(cfg, B, T, seed):
    from audio_motion_avatar_amd.synthetic import make_render_inputs

    H, W = cfg.image_size
    _, smpl, cam = make_render_inputs(T, cfg, seed=seed, batch=B)
    _, _, test_cam = make_render_inputs(T, cfg, seed=seed + 1, batch=B)
    test_cam["extrinsic"] = test_cam["extrinsic"].clone()
    test_cam["extrinsic"][..., 0, 3] += 0.05  # a second viewpoint
    g = torch.Generator().manual_seed(seed)
    ref = torch.rand(B, T, 3, H, W, generator=g).cuda()
    test = torch.rand(B, T, 3, H, W, generator=g).cuda()
    tokens = (torch.randn(B, T, 4096, cfg.image_feature_dim, generator=g) * 0.5).cuda()
    return ref, smpl, cam, tokens, test, test_cam


def _formula(parts):
    return (parts["l1_train"] + 0.1 * parts["ssim_train"] + (parts["l1_test"] + 0.1 * parts["ssim_test"])
            + 0.01 * parts["loss_smplx"])


def test_training_step_gives_every_stage1_parameter_a_gradient():
    cfg = _small_cfg()
    model = _model(cfg)
    ref, smpl, cam, tokens, test, test_cam = _inputs(cfg, 1, 2, seed=4)
    total, parts = model.training_step(ref, smpl, cam, tokens, test, test_cam)
    assert set(parts) == {"l1_train", "ssim_train", "l1_test", "ssim_test", "loss_smplx"}
    assert torch.equal(total, _formula(parts))
    assert float(parts["l1_test"].detach()) > 0 and float(parts["ssim_test"].detach()) > 0
    total.backward()
    names = [n for n, _ in model.named_parameters()]
    bad = [n for n, p in model.named_parameters() if p.grad is None or not bool(torch.isfinite(p.grad).all())
           or not bool(p.grad.any())]
    assert not bad, f"{len(bad)} of {len(names)} parameters get no finite non-zero gradient: {bad}"
    for n in ("smplx_triplane_encoder.fc_pos.weight", "smplx_triplane_encoder.blocks.2.fc_0.weight",
              "smplx_triplane_encoder.fc_c.weight", "smplx_triplane_encoder.vertex_emb.weight",
              "image_feature.feature_reducer.weight"):
        assert n in names

    # the encoder's geometry planes under autograd equal the inference path's, bit for bit
    enc = model.smplx_triplane_encoder
    with torch.no_grad():
        planes0 = enc(cam, tokens, smpl, model.image_feature(ref, tokens))[0]
    planes1 = enc(cam, tokens, smpl, model.image_feature(ref, tokens))[0]
    assert planes1.requires_grad and torch.equal(planes0, planes1.detach())

    # without test views the test terms are 0
    total0, parts0 = model.training_step(ref, smpl, cam, tokens)
    assert float(parts0["l1_test"]) == 0.0 and float(parts0["ssim_test"]) == 0.0
    assert torch.equal(total0, _formula(parts0))
    assert torch.equal(parts0["l1_train"], parts["l1_train"])


def test_adam_fit_lowers_the_stage1_loss():
    """Targets rendered by a copy whose point network is perturbed; Adam on the point network, vertex_emb and the
    image-feature reducer (the parameters only the new backwards reach) brings the image loss down."""
    from audio_motion_avatar_amd.renderer import render_multi_view

    cfg = _small_cfg()
    model = _model(cfg)
    ref, smpl, cam, tokens, _, test_cam = _inputs(cfg, 1, 2, seed=8)
    enc = model.smplx_triplane_encoder
    teacher = copy.deepcopy(model)
    g = torch.Generator().manual_seed(1)
    tenc = teacher.smplx_triplane_encoder
    trained = [enc.fc_pos, *enc.blocks, enc.fc_c, enc.vertex_emb, model.image_feature.feature_reducer]
    with torch.no_grad():
        for mod in [tenc.fc_pos, *tenc.blocks, tenc.fc_c, tenc.vertex_emb]:
            for p in mod.parameters():
                p.add_(torch.randn(p.shape, generator=g).cuda() * 0.5 * float(p.std()))
        img, gaussians = teacher(ref, smpl, cam, image_tokens=tokens)[:2]
        args = type("Args", (), {"image_size": cfg.image_size, "rgb": True, "sh_degree": 3})()
        tgt_test = render_multi_view(gaussians, test_cam["intrinsic"], test_cam["extrinsic"], args)
    target = img.permute(0, 1, 4, 2, 3).contiguous()
    target_test = tgt_test.permute(0, 1, 4, 2, 3).contiguous()
    params = [p for m in trained for p in m.parameters()]
    opt = torch.optim.Adam(params, lr=3e-5)
    losses = []
    for _ in range(25):
        opt.zero_grad(set_to_none=True)
        total, parts = model.training_step(target, smpl, cam, tokens, target_test, test_cam)
        image_loss = total - 0.01 * parts["loss_smplx"]
        total.backward()
        opt.step()
        losses.append(float(image_loss.detach()))
    print("stage-1 image loss:", " ".join(f"{x:.5f}" for x in losses))
    assert all(x == x for x in losses)
    # measured on the MI355X: 0.0452 -> 0.0052 (last five steps' minimum, 0.12x); threshold with 3x headroom
    assert min(losses[-5:]) < 0.4 * losses[0], losses


def test_one_training_step_at_the_reference_widths():
    """C = 256, R = 32, 4096 x 1536 image tokens, 8 fusion + 4 SMPL-X transformer layers, 512^2 views."""
    from audio_motion_avatar_amd.config import Stage1Config

    cfg = Stage1Config(subdivide_steps=0, device="cuda")
    assert (cfg.triplane_feature_dim, cfg.triplane_resolution, cfg.cross_transformer_layers,
            cfg.smplx_transformer_layers, cfg.image_feature_dim) == (256, 32, 8, 4, 1536)
    model = _model(cfg)
    ref, smpl, cam, tokens, test, test_cam = _inputs(cfg, 1, 1, seed=12)
    total, parts = model.training_step(ref, smpl, cam, tokens, test, test_cam)
    total.backward()
    assert bool(torch.isfinite(total))
    for name in ("fc_pos", "fc_c", "vertex_emb"):
        grad = getattr(model.smplx_triplane_encoder, name).weight.grad
        assert grad is not None and bool(torch.isfinite(grad).all()) and bool(grad.any()), name
    grad = model.image_feature.feature_reducer.weight.grad
    assert grad is not None and bool(torch.isfinite(grad).all()) and bool(grad.any())
