"""The two training steps on the fused image loss against the same steps on the library's (AMAV_IMAGE_LOSS=library): the
small configurations of tests/test_stage1_training_gpu.py and tests/test_audio_net_training_gpu.py, one seeded batch, in
.eval().  The parts have the same keys; every image part is within the value bound of tests/test_image_loss_gpu.py of
the float64 oracle on the very frames the step rendered; the gradient that reaches the renderer's decoder heads agrees
in the err sense, within twice the run-to-run difference of the library side with itself, or 16 * 2^-24 if that is 0."""
import pytest
import torch

pytestmark = pytest.mark.gpu

GRAD_FLOOR = 16 * 2.0 ** -24


def _stage1():
    from test_stage1_training_gpu import _inputs, _model, _small_cfg

    cfg = _small_cfg()
    model = _model(cfg)
    ref, smpl, cam, tokens, test, test_cam = _inputs(cfg, 1, 2, seed=4)
    return model, lambda: model.training_step(ref, smpl, cam, tokens, test, test_cam), ("train", "test")


def _stage2():
    from test_audio_net_training_gpu import _stage2_batch, _stage2_model

    model = _stage2_model()
    tri, st, audio, cam, smpl = _stage2_batch(model, 5)
    target = torch.rand(1, 3, 3, 64, 64, generator=torch.Generator().manual_seed(6)).cuda()
    return model, lambda: model.training_step(tri, st, audio, cam, target, smpl), ("target",)


def _run(model, step, monkeypatch, setting):
    """One step and its backward under AMAV_IMAGE_LOSS=setting (None: the default) -> (parts, decoder-head gradients,
    the (rendered, target) pairs the step handed to the loss)."""
    from audio_motion_avatar_amd import losses

    seen = []
    terms = losses.training_image_terms

    def recording(rendered, target):
        seen.append((rendered.detach().clone(), target.detach().clone()))
        return terms(rendered, target)

    if setting is None:
        monkeypatch.delenv("AMAV_IMAGE_LOSS", raising=False)
    else:
        monkeypatch.setenv("AMAV_IMAGE_LOSS", setting)
    with monkeypatch.context() as m:
        m.setattr(losses, "training_image_terms", recording)
        model.zero_grad(set_to_none=True)
        total, parts = step()
        total.backward()
    grads = {k: p.grad.clone() for k, p in model.renderer.gaussian_decoder.named_parameters()}
    return {k: v.detach() for k, v in parts.items()}, grads, seen


def _diff(a, b):
    return max(float((a[k] - b[k]).abs().max()) / float(b[k].abs().max()) for k in b)


@pytest.mark.parametrize("stage", (_stage1, _stage2), ids=("stage1", "stage2"))
def test_training_step_on_the_fused_loss_matches_the_library_path(stage, monkeypatch):
    from audio_motion_avatar_amd import losses

    assert losses.IMAGE_LOSS_DEFAULT == "hip"
    model, step, suffixes = stage()
    fused_parts, fused_grads, fused_seen = _run(model, step, monkeypatch, None)
    lib_parts, lib_grads, lib_seen = _run(model, step, monkeypatch, "library")
    _, lib_grads_again, _ = _run(model, step, monkeypatch, "library")

    assert list(fused_parts) == list(lib_parts)
    assert len(fused_seen) == len(lib_seen) == len(suffixes)
    for suffix, (rendered, target), (rendered_lib, _) in zip(suffixes, fused_seen, lib_seen):
        assert torch.equal(rendered, rendered_lib)      # both sides scored the same frames
        x, y = rendered.double().cpu(), target.double().cpu()
        oracle = {"l1_" + suffix: losses.l1_loss(x, y), "ssim_" + suffix: 1 - losses.ssim(x, y)}
        for key, want in oracle.items():
            lib_err = abs(float(lib_parts[key]) - float(want))
            our_err = abs(float(fused_parts[key]) - float(want))
            print(f"\n{key}: |library - oracle| = {lib_err:.2e}, |fused - oracle| = {our_err:.2e}")
            assert our_err <= max(1e-6, 2 * lib_err), key
    for key in fused_parts:   # what does not come from the image loss is untouched
        if not key.startswith(("l1_", "ssim_", "loss_target")):
            assert torch.equal(fused_parts[key], lib_parts[key]), key

    run_to_run = _diff(lib_grads_again, lib_grads)
    between = _diff(fused_grads, lib_grads)
    bound = 2 * run_to_run if run_to_run > 0 else GRAD_FLOOR
    print(f"\ndecoder heads: library run to run {run_to_run:.2e}, fused against library {between:.2e}, bound {bound:.2e}")
    assert between <= bound
