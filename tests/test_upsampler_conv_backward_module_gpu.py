"""Training the windowed triplane upsampler's tile stages on the HIP convolution (AMAV_UPSAMPLER_CONV_GRAD=hip,
TriplaneUpsampler._tile_block_hip_grad): slab, token gradient and every parameter gradient of
forward_tokens_windowed(differentiable=True) against fp64 full planes under autograd, with the library path of the same
call as the yardstick; determinism; the silent fall-backs; Renderer end to end.

Bound per tensor (tests/test_split_gemm_gpu.py's rule): err = max |got - ref|, e_lib the same for the library's windowed
path with deterministic convolutions; err <= max(1.5 e_lib, 2e-6 max |ref|)."""
import copy
import functools

import pytest
import torch

import upsampler_cases as uc8
import upsampler_conv_cases as cc

pytestmark = pytest.mark.gpu
VAR = "AMAV_UPSAMPLER_CONV_GRAD"


def spy(monkeypatch):
    """Count the calls of the tile-stage implementations."""
    from audio_motion_avatar_amd.renderer import TriplaneUpsampler

    calls = {"hip_grad": 0, "hip": 0, "library": 0}

    def counted(key, fn):
        def call(self, *a, **k):
            calls[key] += 1
            return fn(self, *a, **k)
        return call

    for key, name in (("hip_grad", "_tile_block_hip_grad"), ("hip", "_tile_block_hip"), ("library", "_mosaic")):
        monkeypatch.setattr(TriplaneUpsampler, name, counted(key, getattr(TriplaneUpsampler, name)))
    return calls


def loss_weights(n_blocks, R, box):
    g = torch.Generator().manual_seed(7000 + 10 * n_blocks + len(box))
    return torch.randn(cc.F, cc.N, 3 * cc.C, generator=g)


@functools.lru_cache(maxsize=None)
def reference(n_blocks, R, box):
    """fp64 CPU: slab-independent reference -- the gradients of the random-weighted sum of the features sampled from
    full-plane forward_tokens, for the tokens and every parameter.  Shared: do not modify."""
    up = copy.deepcopy(cc.make_upsampler(n_blocks)).double()
    tokens, points = (t.double() for t in cc.make_inputs(n_blocks, R, box))
    tok = tokens.clone().requires_grad_()
    uc8.oracle_loss(up.forward_tokens(tok, R), points, loss_weights(n_blocks, R, box).double(), R * 2 ** n_blocks).backward()
    return uc8.gradients(up, tok)


def windowed_gradients(up, tokens, points, weights, R, n_blocks):
    """{name: tensor}: the slab and the gradients of the sampled, weighted features through the windowed autograd graph."""
    from audio_motion_avatar_amd import ops

    plan = cc.fresh_plan(up, points, R)
    assert all(w["tiles"] is not None and len(w["tiles"]) > 0 for w in plan)
    r_out = R * 2 ** n_blocks
    tok = tokens.clone().requires_grad_()
    slab = up.forward_tokens_windowed(tok, R, plan, differentiable=True)
    planes = slab.view(tokens.shape[0], tokens.shape[1], 3, r_out, r_out).permute(0, 2, 1, 3, 4)
    (ops.triplane_sample_features_differentiable(planes, points, uc8.RADIUS) * weights).sum().backward()
    named = uc8.gradients(up, tok)
    named["slab"] = slab.detach()
    return named


@pytest.mark.parametrize("box", sorted(cc.BOXES))
@pytest.mark.parametrize("n_blocks,R", cc.CASES)
def test_gradients_are_fp32_equivalent(n_blocks, R, box, monkeypatch):
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    calls = spy(monkeypatch)
    want = reference(n_blocks, R, box)
    tokens, points = (t.cuda() for t in cc.make_inputs(n_blocks, R, box))
    weights = loss_weights(n_blocks, R, box).cuda()
    monkeypatch.setenv(VAR, "library")
    lib = windowed_gradients(cc.make_upsampler(n_blocks).cuda(), tokens, points, weights, R, n_blocks)
    assert calls["hip_grad"] == 0 and calls["library"] > 0
    calls["library"] = 0
    monkeypatch.setenv(VAR, "hip")
    up = cc.make_upsampler(n_blocks).cuda()
    got = windowed_gradients(up, tokens, points, weights, R, n_blocks)
    assert calls["hip_grad"] == 3 * min(n_blocks, 2) and calls["library"] == 0 and calls["hip"] == 0
    assert set(got) == set(lib) == set(want) | {"slab"} and len(want) == len(list(up.parameters())) + 1
    assert any("upsample.3.block.0.weight" in k for k in want)   # BatchNorm's affine terms are among them
    failed = []
    for name in sorted(want):
        ref = want[name]
        err = float((got[name].cpu().double() - ref).abs().max())
        e_lib = float((lib[name].cpu().double() - ref).abs().max())
        top = float(ref.abs().max())
        print(f"blocks {n_blocks} {box} {name}: err {err:.3e}  e_lib {e_lib:.3e}  max|ref| {top:.3e}")
        assert torch.isfinite(got[name]).all() and top > 0, name
        if not err <= max(1.5 * e_lib, 2e-6 * top):
            failed.append((name, err, e_lib, top))
    assert not failed, failed
    # the slab, where it is sampled: the features against those of the fp64 full planes, under the same rule
    ref, r_out = cc.reference_features(n_blocks, R, box), R * 2 ** n_blocks
    err = float((cc.sampled(got["slab"], points, r_out) - ref).abs().max())
    e_lib = float((cc.sampled(lib["slab"], points, r_out) - ref).abs().max())
    print(f"blocks {n_blocks} {box} sampled slab: err {err:.3e}  e_lib {e_lib:.3e}  max|ref| {float(ref.abs().max()):.3e}")
    assert err <= max(1.5 * e_lib, 2e-6 * float(ref.abs().max()))


def test_two_runs_are_bit_equal(monkeypatch):
    """What the library's atomically accumulated weight gradients cannot promise."""
    monkeypatch.setenv(VAR, "hip")
    tokens, points = (t.cuda() for t in cc.make_inputs(2, 16, "border"))
    weights = loss_weights(2, 16, "border").cuda()
    runs = [windowed_gradients(cc.make_upsampler(2).cuda(), tokens, points, weights, 16, 2) for _ in range(2)]
    assert set(runs[0]) == set(runs[1])
    differ = [k for k in runs[0] if not torch.equal(runs[0][k], runs[1][k])]
    assert not differ, differ


def _library_run(monkeypatch, run):
    """`run` with both switches unset and deterministic convolutions, where library against library is bit-stable."""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    monkeypatch.delenv(VAR, raising=False)
    monkeypatch.delenv("AMAV_UPSAMPLER_CONV", raising=False)
    return run()


def _assert_same(want, got):
    assert set(want) == set(got)
    differ = [k for k in want if not torch.equal(want[k], got[k])]
    assert not differ, differ


def test_fallback_switch_unset(monkeypatch):
    """AMAV_UPSAMPLER_CONV=hip alone does not bear on a differentiable evaluation."""
    calls = spy(monkeypatch)
    tokens, points = (t.cuda() for t in cc.make_inputs(1, 16, "border"))
    weights = loss_weights(1, 16, "border").cuda()
    run = lambda: windowed_gradients(cc.make_upsampler(1).cuda(), tokens, points, weights, 16, 1)  # noqa: E731
    want = _library_run(monkeypatch, run)
    monkeypatch.setenv("AMAV_UPSAMPLER_CONV", "hip")
    _assert_same(want, run())
    assert calls["hip_grad"] == 0 and calls["hip"] == 0 and calls["library"] == 6


def test_fallback_narrow_channels(monkeypatch):
    calls = spy(monkeypatch)
    tokens, points, weights = (t.cuda() for t in uc8.make_inputs(2, 16, "border"))
    run = lambda: windowed_gradients(uc8.make_upsampler(2).cuda(), tokens, points, weights, 16, 2)  # noqa: E731
    want = _library_run(monkeypatch, run)
    monkeypatch.setenv(VAR, "hip")
    _assert_same(want, run())
    assert calls["hip_grad"] == 0 and calls["library"] > 0


def test_fallback_train_mode(monkeypatch):
    calls = spy(monkeypatch)
    tokens, points = (t.cuda() for t in cc.make_inputs(1, 16, "off_centre"))
    weights = loss_weights(1, 16, "off_centre").cuda()
    run = lambda: windowed_gradients(cc.make_upsampler(1).cuda().train(), tokens, points, weights, 16, 1)  # noqa: E731
    want = _library_run(monkeypatch, run)
    monkeypatch.setenv(VAR, "hip")
    _assert_same(want, run())
    assert calls["hip_grad"] == 0 and calls["library"] > 0


def test_fallback_cpu_module(monkeypatch):
    calls = spy(monkeypatch)
    tokens, points = cc.make_inputs(1, 16, "off_centre")

    def run():
        up = cc.make_upsampler(1)
        tok = tokens.clone().requires_grad_()
        slab = up.forward_tokens_windowed(tok, 16, cc.fresh_plan(up, points, 16), differentiable=True)
        slab.square().sum().backward()
        return dict(uc8.gradients(up, tok), slab=slab.detach())

    want = _library_run(monkeypatch, run)
    monkeypatch.setenv(VAR, "hip")
    _assert_same(want, run())
    assert calls["hip_grad"] == 0 and calls["library"] > 0


def test_unknown_switch_value(monkeypatch):
    tokens, points = (t.cuda() for t in cc.make_inputs(1, 16, "off_centre"))
    up = cc.make_upsampler(1).cuda()
    monkeypatch.setenv(VAR, "fast")
    with pytest.raises(ValueError, match="AMAV_UPSAMPLER_CONV_GRAD"):
        up.forward_tokens_windowed(tokens, 16, cc.fresh_plan(up, points, 16), differentiable=True)
    monkeypatch.delenv(VAR)
    up.cfg.upsample_conv_grad = "quick"
    with pytest.raises(ValueError, match="upsample_conv_grad"):
        up.forward_tokens_windowed(tokens, 16, cc.fresh_plan(up, points, 16), differentiable=True)


def test_an_image_loss_trains_the_upsampler_on_hip(monkeypatch):
    """The Renderer of tests/test_upsampler_backward_gpu.py::test_an_image_loss_trains_the_upsampler at C = 32, where the
    HIP path is eligible, switched on by the configuration: the path is taken, every upsampler tensor gets a finite
    gradient, two identical steps give bit-equal gradients, and 6 Adam steps lower the loss.

    Deterministic convolutions are selected for what stays on the library: the 1 x 1 skip convolution's weight gradient
    is accumulated atomically by the library's default kernel at this shape (it alone differed between two steps, the
    tile stages' gradients never did); the HIP backward does not read the flag."""
    from audio_motion_avatar_amd import losses
    from audio_motion_avatar_amd.config import RendererConfig
    from audio_motion_avatar_amd.renderer import Renderer
    from audio_motion_avatar_amd.synthetic import init_random_heads, make_render_inputs

    calls = spy(monkeypatch)
    monkeypatch.delenv(VAR, raising=False)
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    cfg = RendererConfig(image_size=(64, 64), subdivide_steps=0, triplane_feature_dim=32, triplane_resolution=16,
                         predict_smplx_params=False, num_gaussians=1500, upsample_triplane=True, num_upsample_blocks=2,
                         differentiable_upsampler=True)
    assert cfg.upsample_conv_grad == "library"
    cfg.upsample_conv_grad = "hip"
    torch.manual_seed(0)
    r = init_random_heads(Renderer(cfg).eval(), std=0.05)
    tokens, smpl, cam = make_render_inputs(2, cfg, seed=4)
    zeros = torch.zeros(1, 2, 1, 1, device="cuda")
    trainable = {k: p for k, p in r.named_parameters() if k.startswith("triplane_upsampler.")}
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
    assert calls["hip_grad"] == 0          # no_grad: nothing differentiable was asked for
    calls.update(hip=0, library=0)
    tok = tokens.clone().requires_grad_()

    def step_gradients():
        r.zero_grad(set_to_none=True)
        tok.grad = None
        images, _ = r(tok, cam, zeros, smpl)
        loss = losses.l1_loss(images, target) + 0.1 * (1.0 - losses.ssim(images, target))
        loss.backward()
        return loss.detach(), dict({k: p.grad.clone() for k, p in trainable.items()}, tokens=tok.grad.clone())

    _, first = step_gradients()
    assert calls["hip_grad"] == 6 and calls["library"] == 0
    for k, v in first.items():
        assert torch.isfinite(v).all() and bool((v != 0).any()), k
    _, second = step_gradients()
    differ = [k for k in first if not torch.equal(first[k], second[k])]
    assert not differ, differ
    opt = torch.optim.Adam(trainable.values(), lr=1e-3)
    history = []
    for _ in range(6):
        loss, _ = step_gradients()
        opt.step()
        history.append(float(loss))
    print("losses:", " ".join(f"{v:.6f}" for v in history))
    assert all(v == v for v in history) and history[-1] < history[0], history
