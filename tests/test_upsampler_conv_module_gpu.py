"""The windowed triplane upsampler on the HIP tile convolution (AMAV_UPSAMPLER_CONV=hip, TriplaneUpsampler._tile_block_hip,
DESIGN.md section 4.6): sampled features against the fp64 full planes with the library path of the same call as the
yardstick, the silent fall-backs, the memo of prepared weights, Renderer.forward end to end, and the default.

Bound (tests/test_split_gemm_gpu.py's rule): err = max |got - ref| over the sampled features, err32 the same for
AMAV_UPSAMPLER_CONV=library; err <= max(1.5 err32, 2e-6 max |ref|)."""
import copy

import pytest
import torch

import upsampler_cases as uc8
import upsampler_conv_cases as cc

pytestmark = pytest.mark.gpu
VAR = "AMAV_UPSAMPLER_CONV"


def spy(monkeypatch):
    """Count the calls of the two tile-stage implementations."""
    from audio_motion_avatar_amd.renderer import TriplaneUpsampler

    calls = {"hip": 0, "library": 0}
    hip, library = TriplaneUpsampler._tile_block_hip, TriplaneUpsampler._mosaic

    def count_hip(self, *a, **k):
        calls["hip"] += 1
        return hip(self, *a, **k)

    def count_library(self, *a, **k):
        calls["library"] += 1
        return library(self, *a, **k)

    monkeypatch.setattr(TriplaneUpsampler, "_tile_block_hip", count_hip)
    monkeypatch.setattr(TriplaneUpsampler, "_mosaic", count_library)
    return calls


def windowed(up, tokens, points, R, **kw):
    """forward_tokens_windowed into a slab of its own, from a clean plan history."""
    plan = cc.fresh_plan(up, points, R)
    assert all(w["tiles"] is not None and len(w["tiles"]) > 0 for w in plan)
    if kw.get("differentiable"):
        return up.forward_tokens_windowed(tokens, R, plan, **kw)
    with torch.no_grad():
        return up.forward_tokens_windowed(tokens, R, plan, **kw).clone()


@pytest.mark.parametrize("box", sorted(cc.BOXES))
@pytest.mark.parametrize("n_blocks,R", cc.CASES)
def test_sampled_features_are_fp32_equivalent(n_blocks, R, box, monkeypatch):
    calls = spy(monkeypatch)
    ref = cc.reference_features(n_blocks, R, box)
    tokens, points = (t.cuda() for t in cc.make_inputs(n_blocks, R, box))
    up = cc.make_upsampler(n_blocks).cuda()
    r_out = R * 2 ** n_blocks
    monkeypatch.setenv(VAR, "library")
    lib = cc.sampled(windowed(up, tokens, points, R), points, r_out)
    assert calls["hip"] == 0 and calls["library"] > 0
    monkeypatch.setenv(VAR, "hip")
    got = cc.sampled(windowed(up, tokens, points, R), points, r_out)
    assert calls["hip"] == 3 * min(n_blocks, 2)   # every plane has tiles; one or two tile stages
    err, err32, top = float((got - ref).abs().max()), float((lib - ref).abs().max()), float(ref.abs().max())
    print(f"blocks {n_blocks} {box}: err {err:.3e}  err32 {err32:.3e}  max|ref| {top:.3e}")
    assert torch.isfinite(got).all()
    assert err <= max(1.5 * err32, 2e-6 * top), (err, err32, top)


def _both(monkeypatch, run):
    monkeypatch.setenv(VAR, "library")
    want = run()
    monkeypatch.setenv(VAR, "hip")
    return want, run()


def test_fallback_narrow_channels(monkeypatch):
    calls = spy(monkeypatch)
    tokens, points, _ = (t.cuda() for t in uc8.make_inputs(2, 16, "border"))
    want, got = _both(monkeypatch, lambda: windowed(uc8.make_upsampler(2).cuda(), tokens, points, 16))
    assert calls["hip"] == 0 and torch.equal(want, got)


def test_fallback_differentiable(monkeypatch):
    """Slab, token gradient and every parameter gradient.  The library's default weight-gradient kernels of a 3x3
    convolution accumulate with atomics and differ from run to run under EITHER setting (1e-5 absolute here), so the
    comparison runs with deterministic convolutions selected, where library against library is bit-stable."""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    calls = spy(monkeypatch)
    tokens, points = (t.cuda() for t in cc.make_inputs(1, 16, "border"))
    weights = torch.randn(cc.F, cc.C, 3 * 32 * 32, generator=torch.Generator().manual_seed(1)).cuda()

    def run():
        up = cc.make_upsampler(1).cuda()
        tok = tokens.clone().requires_grad_()
        slab = windowed(up, tok, points, 16, differentiable=True)
        (slab * weights).sum().backward()
        named = {"slab": slab.detach(), "tokens": tok.grad}
        named.update({k: p.grad for k, p in up.named_parameters() if p.grad is not None})
        return named

    want, got = _both(monkeypatch, run)
    assert calls["hip"] == 0 and set(want) == set(got) and len(want) > 5
    differ = [k for k in want if not torch.equal(want[k], got[k])]
    assert not differ, differ


def test_fallback_train_mode(monkeypatch):
    calls = spy(monkeypatch)
    tokens, points = (t.cuda() for t in cc.make_inputs(1, 16, "off_centre"))
    want, got = _both(monkeypatch, lambda: windowed(cc.make_upsampler(1).cuda().train(), tokens, points, 16))
    assert calls["hip"] == 0 and torch.equal(want, got)


def test_fallback_cpu_module(monkeypatch):
    calls = spy(monkeypatch)
    tokens, points = cc.make_inputs(1, 16, "off_centre")
    want, got = _both(monkeypatch, lambda: windowed(cc.make_upsampler(1), tokens, points, 16))
    assert calls["hip"] == 0 and torch.equal(want, got)


def test_fallback_under_grad_mode(monkeypatch):
    """Parameters that require grad under grad mode: autograd would have to record the call, so the library runs."""
    calls = spy(monkeypatch)
    tokens, points = (t.cuda() for t in cc.make_inputs(1, 16, "off_centre"))
    up = cc.make_upsampler(1).cuda()
    monkeypatch.setenv(VAR, "hip")
    up.forward_tokens_windowed(tokens, 16, cc.fresh_plan(up, points, 16))
    assert calls["hip"] == 0 and calls["library"] == 3


def test_memo_follows_its_sources(monkeypatch):
    monkeypatch.setenv(VAR, "hip")
    tokens, points = (t.cuda() for t in cc.make_inputs(2, 16, "border"))
    up = cc.make_upsampler(2).cuda()
    stale = windowed(up, tokens, points, 16)
    assert torch.equal(stale, windowed(up, tokens, points, 16))       # served from the memo
    res = up.upsample_blocks[1].upsample[3].block
    with torch.no_grad():
        res[2].weight.mul_(1.5)                                        # conv_a of the last block
        up.upsample_blocks[0].upsample[1].weight.add_(0.01)            # conv1 of the first tile stage
        res[3].running_var.add_(0.3)                                   # bn1, folded into conv_a's prepared weights
        res[0].running_mean.sub_(0.1)                                  # bn0, the prologue
    got = windowed(up, tokens, points, 16)
    fresh = copy.deepcopy(up)
    fresh._conv_memo = {}
    want = windowed(fresh, tokens, points, 16)
    assert torch.equal(got, want) and not torch.equal(got, stale)


def test_renderer_end_to_end(monkeypatch):
    from audio_motion_avatar_amd.config import RendererConfig
    from audio_motion_avatar_amd.renderer import Renderer
    from audio_motion_avatar_amd.synthetic import init_random_heads, make_render_inputs

    calls = spy(monkeypatch)
    cfg = RendererConfig(image_size=(64, 64), subdivide_steps=0, triplane_feature_dim=32, triplane_resolution=16,
                         predict_smplx_params=False, num_gaussians=1500, upsample_triplane=True, num_upsample_blocks=2)
    assert cfg.upsample_conv == "library"
    torch.manual_seed(0)
    r = init_random_heads(Renderer(cfg).eval(), std=0.05)
    tokens, smpl, cam = make_render_inputs(2, cfg, seed=4)
    zeros = torch.zeros(1, 2, 1, 1, device="cuda")

    def run():
        with torch.no_grad():
            return r(tokens, cam, zeros, smpl)[0].clone()

    want, got = _both(monkeypatch, run)
    assert calls["hip"] > 0
    diff = float((want - got).abs().max())
    print(f"hip against library frames: max-abs {diff:.3e}")
    assert diff <= 1e-3 and not torch.equal(want, got)
    # the configuration supplies the value when the variable is unset
    monkeypatch.delenv(VAR)
    before = calls["hip"]
    r.cfg.upsample_conv = "hip"
    assert torch.equal(run(), got) and calls["hip"] > before


def test_default_is_the_library(monkeypatch):
    calls = spy(monkeypatch)
    monkeypatch.delenv(VAR, raising=False)
    tokens, points = (t.cuda() for t in cc.make_inputs(2, 16, "off_centre"))
    up = cc.make_upsampler(2).cuda()
    default = windowed(up, tokens, points, 16)
    assert calls["hip"] == 0 and calls["library"] == 6
    monkeypatch.setenv(VAR, "library")
    assert torch.equal(default, windowed(up, tokens, points, 16))
    monkeypatch.setenv(VAR, "fast")
    with pytest.raises(ValueError, match="AMAV_UPSAMPLER_CONV"):
        windowed(up, tokens, points, 16)
