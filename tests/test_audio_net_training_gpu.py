"""The audio net under autograd: Attention, one BasicTransformerBlock and the token generator on the HIP self-attention
backward against fp64 autograd of the functional oracle (oracle.transformer, same state_dict, evaluated with torch on
the GPU), and AudioDrivenAvatar.training_step -- the reference's stage-2 loss -- end to end.  Bound style: max |error|
<= tol * max |grad| per parameter / input."""
import re

import pytest
import torch

pytestmark = pytest.mark.gpu


def randomize(module, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in module.named_parameters():
            if "conv_time" in name:
                p.copy_(torch.rand(p.shape, generator=g))
            elif p.dim() > 1:
                p.copy_(torch.randn(p.shape, generator=g) * (0.5 / p.shape[-1] ** 0.5))
            else:
                p.copy_(torch.randn(p.shape, generator=g) * 0.1 + (1.0 if "norm" in name and "weight" in name else 0.0))


def small_cfg(differentiable_smplx=False):
    from audio_motion_avatar_amd.config import AudioNetConfig, ModelConfig, RendererConfig

    a = AudioNetConfig(triplane_feature_dim=32, triplane_resolution=8, smpl_token_len=10, smpl_token_dim=32,
                       transformer_layers=2, transformer_head_dim=64, transformer_num_heads=2, audio_feature_dim=48,
                       triplane_output_frames=3)
    r = RendererConfig(triplane_feature_dim=32, triplane_resolution=8, smpl_token_len=10, smpl_token_dim=32,
                       image_size=(64, 64), subdivide_steps=0, differentiable_smplx=differentiable_smplx)
    return ModelConfig(triplane_audio_net=a, renderer=r)


def oracle_grads(fn, params, inputs, upstream):
    """fp64 autograd of fn(params, *inputs) on the GPU -> (grads of params by name, grads of inputs)."""
    p64 = {k: v.detach().double().cuda().requires_grad_(v.is_floating_point()) for k, v in params.items()}
    x64 = [x.detach().double().cuda().requires_grad_() for x in inputs]
    out = fn(p64, *x64)
    out = out if isinstance(out, (tuple, list)) else (out,)
    torch.autograd.backward(list(out), [u.double() for u in upstream])
    return {k: v.grad for k, v in p64.items() if v.grad is not None}, [x.grad for x in x64]


# The cross-attention (attn2) has ONE key: softmax over it is exactly 1, so its output to_out(to_v(context)) does not
# depend on its queries -- norm2 and attn2.to_q / to_k are outside the differentiable graph (in the reference their
# gradient is rounding noise of P (dP - delta) = 1 (dP - dP)).
DISCONNECTED = re.compile(r"(^|transformer_blocks\.\d+\.)(norm2|attn2\.to_q|attn2\.to_k)\.")


def connected(name):
    return DISCONNECTED.search(name) is None


def check(name, got, ref, tol, report):
    err = float((got.double() - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)
    report[name] = err
    assert err <= tol, (name, err)


def _compare_module(module, prefix, fn, inputs, upstream, tol):
    report = {}
    outs = module(*inputs)
    outs = outs if isinstance(outs, (tuple, list)) else (outs,)
    torch.autograd.backward(list(outs), upstream)
    params = {prefix + k: v for k, v in module.state_dict().items()}
    ref_p, ref_x = oracle_grads(fn, params, inputs, upstream)
    for k, p in module.named_parameters():
        if not connected(k):
            assert p.grad is None, k
            continue
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
        check(k, p.grad, ref_p[prefix + k], tol, report)
    for i, (x, r) in enumerate(zip(inputs, ref_x)):
        if x.requires_grad:
            check(f"input{i}", x.grad, r, tol, report)
    worst = max(report, key=report.get)
    print(f"\n{type(module).__name__}: largest gradient error / max {report[worst]:.2e} ({worst}), "
          f"{len(report)} tensors")
    return report


def test_attention_alone():
    from audio_motion_avatar_amd.transformer import Attention
    from oracle import transformer as o_tr

    attn = Attention(128, None, heads=2, dim_head=64).cuda()
    randomize(attn, 1)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 300, 128, generator=g).cuda().requires_grad_()
    up = torch.randn(2, 300, 128, generator=g).cuda()
    _compare_module(attn, "a.", lambda p, h: o_tr.attention(p, "a.", h, None, 2), [x], [up], 1e-5)


def test_one_transformer_block():
    from audio_motion_avatar_amd.transformer import BasicTransformerBlock
    from oracle import transformer as o_tr

    blk = BasicTransformerBlock(128, 2, 64, cross_attention_dim=48).cuda()
    randomize(blk, 3)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 257, 128, generator=g).cuda().requires_grad_()
    enc = torch.randn(2, 1, 48, generator=g).cuda().requires_grad_()
    up = torch.randn(2, 257, 128, generator=g).cuda()
    _compare_module(blk, "b.", lambda p, h, e: o_tr.transformer_block(p, "b.", h, e, 2), [x, enc], [up], 1e-5)


def test_token_generator_gradients_match_fp64_oracle():
    from audio_motion_avatar_amd.triplane_audio_net import AudioTriplaneNet
    from oracle import transformer as o_tr

    net = AudioTriplaneNet(small_cfg(), renderer=None).eval()
    randomize(net, 0)
    net = net.cuda()
    g = torch.Generator().manual_seed(1)
    B = 2
    audio = torch.randn(B, 4, 48, generator=g).cuda().requires_grad_()
    tri = torch.randn(B, 2, 32, 3 * 64, generator=g).cuda().requires_grad_()
    smpl = torch.randn(B, 2, 32, 10, generator=g).cuda().requires_grad_()
    up = [torch.randn(B, 3, 32, 192, generator=g).cuda(), torch.randn(B, 3, 32, 10, generator=g).cuda()]
    fn = lambda p, a, t, s: o_tr.audio_triplane_tokens(p, a, t, s, resolution=8, smpl_len=10, t_output=3,  # noqa: E731
                                                       num_layers=2, heads=2)
    outs = net.generate_tokens(audio, tri, smpl)
    torch.autograd.backward(list(outs), up)
    ref_p, ref_x = oracle_grads(fn, dict(net.state_dict()), [audio, tri, smpl], up)
    report = {}
    for k, p in net.named_parameters():
        if not connected(k):
            assert p.grad is None, k
            continue
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
        check(k, p.grad, ref_p[k], 1e-4, report)
    for name, x, r in zip(("audio", "tri", "smpl"), (audio, tri, smpl), ref_x):
        check(name, x.grad, r, 1e-4, report)
    worst = max(report, key=report.get)
    print(f"\ntoken generator: largest gradient error / max {report[worst]:.2e} ({worst}), {len(report)} tensors")


def test_full_size_token_gradients_two_steps():
    """The reference width (8 layers, 512 wide, 8 x 64 heads, S = 6304), two autoregressive steps, B = 1: gradients of
    the input tokens against the fp64 oracle."""
    from audio_motion_avatar_amd.config import ModelConfig
    from audio_motion_avatar_amd.triplane_audio_net import AudioTriplaneNet
    from oracle import transformer as o_tr

    net = AudioTriplaneNet(ModelConfig(), renderer=None).eval()
    randomize(net, 11)
    net = net.cuda()
    g = torch.Generator().manual_seed(12)
    audio = torch.randn(1, 2, 768, generator=g).cuda()
    tri = torch.randn(1, 2, 256, 3 * 32 * 32, generator=g).cuda().requires_grad_()
    smpl = torch.randn(1, 2, 256, 80, generator=g).cuda().requires_grad_()
    up = [torch.randn(1, 2, 256, 3072, generator=g).cuda(), torch.randn(1, 2, 256, 80, generator=g).cuda()]
    outs = net.generate_tokens(audio, tri, smpl, num_steps=2)
    torch.autograd.backward(list(outs), up)
    fn = lambda p, a, t, s: o_tr.audio_triplane_tokens(p, a, t, s, t_output=2)  # noqa: E731
    ref_p, ref_x = oracle_grads(fn, dict(net.state_dict()), [audio, tri, smpl], up)
    report = {}
    check("tri", tri.grad, ref_x[1], 1e-4, report)
    check("smpl", smpl.grad, ref_x[2], 1e-4, report)
    w = "transformer.transformer_blocks.0.attn1.to_q.weight"
    check(w, dict(net.named_parameters())[w].grad, ref_p[w], 1e-4, report)
    print(f"\nfull-size token gradients: {report}")


def _stage2_model(seed=0):
    from audio_motion_avatar_amd.harness import AudioDrivenAvatar
    from audio_motion_avatar_amd.synthetic import init_random_heads

    model = AudioDrivenAvatar(small_cfg(differentiable_smplx=True))
    randomize(model.audio_triplane.transformer, seed)
    init_random_heads(model.renderer)
    dec = model.smpl_decoder
    with torch.no_grad():  # put the predicted body in front of the camera
        dec.dec_transl.weight.mul_(0.01)
        dec.dec_transl.bias.copy_(torch.tensor([0.0, -0.15, 2.4], device=dec.dec_transl.bias.device))
    return model.cuda().eval()


def _stage2_batch(model, seed):
    from audio_motion_avatar_amd.synthetic import make_render_inputs

    T = model.audio_triplane.T_output
    _, smpl, cam = make_render_inputs(T, model.cfg.renderer, seed=seed)
    g = torch.Generator().manual_seed(seed)
    audio = torch.randn(1, T, 48, generator=g).cuda()
    tri = torch.randn(1, 2, 32, 192, generator=g).cuda()
    st = (torch.randn(1, 2, 32, 10, generator=g) * 0.2).cuda()
    return tri, st, audio, cam, smpl


def test_training_step_reaches_every_trained_module():
    model = _stage2_model()
    tri, st, audio, cam, smpl = _stage2_batch(model, 5)
    target = torch.full((1, 3, 3, 64, 64), 0.5, device="cuda")
    total, parts = model.training_step(tri, st, audio, cam, target, smpl)
    assert set(parts) == {"l1_target", "ssim_target", "loss_target", "smpl_loss_future"}
    want = 10 * (parts["l1_target"] + 0.1 * parts["ssim_target"]) + 0.05 * parts["smpl_loss_future"]
    assert torch.allclose(total, want)
    total.backward()
    net = model.audio_triplane
    for owner, mod in (("transformer", net.transformer), ("triplane_motion_encoder", net.triplane_motion_encoder),
                       ("smplx_motion_encoder", net.smplx_motion_encoder), ("decoder heads", model.renderer.gaussian_decoder),
                       ("smpl_decoder", model.smpl_decoder)):
        for k, p in mod.named_parameters():
            if not connected(k):
                continue
            assert p.grad is not None, (owner, k)
            assert torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0, (owner, k)


def test_adam_fit_lowers_the_stage2_loss():
    """Targets rendered from perturbed transformer weights (each tensor + 0.2 x its mean magnitude of noise); 50 Adam
    steps on the transformer from the unperturbed ones lower the stage-2 loss at least 3x (measured: ~7x)."""
    model = _stage2_model(seed=1)
    tri, st, audio, cam, smpl = _stage2_batch(model, 9)
    tf = model.audio_triplane.transformer
    start = {k: v.detach().clone() for k, v in tf.state_dict().items()}
    with torch.no_grad():
        g = torch.Generator().manual_seed(3)
        for p in tf.parameters():
            p.add_(torch.randn(p.shape, generator=g).cuda() * 0.2 * (p.abs().mean() + 1e-3))
        images, _, pred, _, _ = model.audio_triplane(audio, tri, None, cam, st)
        target_video = images.permute(0, 1, 4, 2, 3).contiguous()
        target_smpl = {k: v.detach().clone() for k, v in pred.items()}
        tf.load_state_dict(start)
    model.renderer.requires_grad_(False)
    model.smpl_decoder.requires_grad_(False)
    opt = torch.optim.Adam(model.audio_triplane.transformer.parameters(), lr=3e-5)
    trace = []
    for _ in range(50):
        opt.zero_grad()
        loss, _ = model.training_step(tri, st, audio, cam, target_video, target_smpl)
        trace.append(float(loss.detach()))
        loss.backward()
        opt.step()
    last = float(model.training_step(tri, st, audio, cam, target_video, target_smpl)[0].detach())
    first = trace[0]
    print(f"\nstage-2 fit: loss {first:.4e} -> {last:.4e} (factor {last / first:.3f}); every 10th step "
          f"{['%.3e' % x for x in trace[::10]]}")
    assert last < first / 3
