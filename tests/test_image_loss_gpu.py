"""The fused image loss (csrc/image_loss.hip through losses.image_losses) on the MI355X against the float64 oracle of
tests/image_loss_cases.py, with the library path -- losses.l1_loss / losses.ssim in fp32 on the GPU -- as the yardstick:

    values      |fused - oracle| <= max(1e-6, 2 |library - oracle|)
    gradients   err(fused) <= max(2 err(library), 16 * 2^-24),  err(a) = max |a - oracle| / max |oracle|

Both sides evaluate one formula in fp32 and differ in summation order (11 + 11 separable taps against 121), and a
maximum over thousands of elements is a stable statistic: hence the factor 2.  Every test prints its figures."""
import functools

import pytest
import torch

from helpers import ref_fixture
from image_loss_cases import EQUAL_BLOCK, NAMES, case, err, evaluate, oracle

pytestmark = pytest.mark.gpu

GRAD_FLOOR = 16 * 2.0 ** -24


class _Fused:
    """The interface of `losses` that image_loss_cases.evaluate uses, served by the fused kernels."""

    @staticmethod
    def l1_loss(x, y):
        from audio_motion_avatar_amd import losses

        return losses.image_losses(x, y)[0]

    @staticmethod
    def ssim(x, y, size_average=True):
        from audio_motion_avatar_amd import losses

        return losses.image_losses(x, y, size_average)[1]


@functools.lru_cache(maxsize=None)
def results(name):
    """(oracle, library, fused) of one case, each computed once."""
    from audio_motion_avatar_amd import losses

    x, y = (t.float().cuda() for t in case(name))
    return oracle(name), evaluate(x, y, losses), evaluate(x, y, _Fused)


def test_values_on_the_reference_run_fixture():
    from audio_motion_avatar_amd import losses

    a, _, tier = ref_fixture("losses")
    assert tier == 1 and tuple(a["img1"].shape) == (2, 3, 24, 20, 3)
    x, y = a["img1"].float().cuda(), a["img2"].float().cuda()
    l1, s = losses.image_losses(x, y)
    _, per_image = losses.image_losses(x, y, size_average=False)
    for name, got, want in (("l1", l1, a["l1"]), ("ssim", s, a["ssim"]), ("ssim_per_image", per_image, a["ssim_per_image"])):
        diff = float((got.cpu().double() - want.double()).abs().max())
        print(f"\nfixture {name}: |fused - reference run| = {diff:.2e}")
        assert diff <= 1e-6, name


@pytest.mark.parametrize("name", NAMES)
def test_values(name):
    ref, library, fused = results(name)
    for key in ("l1", "ssim", "ssim_per_image"):
        lib_err = float((library[key].double().cpu() - ref[key]).abs().max())
        our_err = float((fused[key].double().cpu() - ref[key]).abs().max())
        print(f"\n{name} {key}: |library - oracle| = {lib_err:.2e}, |fused - oracle| = {our_err:.2e}")
        assert our_err <= max(1e-6, 2 * lib_err), key


@pytest.mark.parametrize("name", NAMES)
def test_gradients(name):
    ref, library, fused = results(name)
    for key in ("grad_total", "grad_ssim"):
        lib_err, our_err = err(library[key], ref[key]), err(fused[key], ref[key])
        print(f"\n{name} {key}: err(library) = {lib_err:.2e}, err(fused) = {our_err:.2e}, "
              f"ratio {our_err / max(lib_err, 1e-30):.2f}")
        assert our_err <= max(2 * lib_err, GRAD_FLOOR), key


def test_l1_gradient_is_zero_where_the_images_are_equal():
    """sign(0) = 0, as torch.abs's backward has it."""
    from audio_motion_avatar_amd import losses

    x, y = (t.float().cuda() for t in case("equal_block"))
    x.requires_grad_()
    losses.image_losses(x, y)[0].backward()
    assert float(x.grad[EQUAL_BLOCK].abs().max()) == 0.0
    outside = x.grad.clone()                                    # and nowhere else: the inputs are continuous draws
    outside[EQUAL_BLOCK] = 1.0
    assert bool((outside != 0).all())


def _in_place_pair(name):
    """(x, y): x a [..., :3] view of an RGBA buffer whose alpha is NaN, y a permuted planar tensor."""
    x64, y64 = case(name)
    buf = torch.full((*x64.shape[:-1], 4), float("nan"), device="cuda")
    buf[..., :3] = x64.float().cuda()
    planar = y64.float().cuda().permute(0, 1, 4, 2, 3).contiguous()
    return buf[..., :3], planar.permute(0, 1, 3, 4, 2)


@pytest.mark.parametrize("name", ("tiles_37x41", "white_background"))
def test_strided_inputs_are_read_in_place(name):
    from audio_motion_avatar_amd import losses

    xv, yv = _in_place_pair(name)
    assert not xv.is_contiguous() and not yv.is_contiguous()
    out = []
    for x, y in ((xv, yv), (xv.contiguous(), yv.contiguous())):
        x = x.detach().requires_grad_()      # detach keeps the view's strides and storage
        l1, s = losses.image_losses(x, y, size_average=False)
        (l1 + 0.1 * (1 - s).sum()).backward()
        out.append((l1.detach(), s.detach(), x.grad))
    assert out[0][2].shape == xv.shape
    assert all(bool(torch.isfinite(t).all()) for t in out[0])       # the NaN alpha was never read
    for a, b in zip(*out):
        assert torch.equal(a, b)


def test_one_backward_serves_any_weights():
    """10 (l1 + 0.1 (1 - ssim)) backpropagates as 10 dl1 - dssim, to 4 ulp of the largest entry."""
    from audio_motion_avatar_amd import losses

    x, y = (t.float().cuda() for t in case("tiles_37x41"))
    grads = []
    for weigh in (lambda l1, s: 10 * (l1 + 0.1 * (1 - s)), lambda l1, s: l1, lambda l1, s: s):
        xg = x.clone().requires_grad_()
        weigh(*losses.image_losses(xg, y)).backward()
        grads.append(xg.grad.double())
    both, d_l1, d_ssim = grads
    want = 10 * d_l1 - d_ssim
    largest = float(want.abs().max())
    ulp = 2.0 ** (torch.tensor(largest).log2().floor().item() - 23)
    diff = float((both - want).abs().max())
    print(f"\nweights: |one backward - assembled| = {diff:.2e} = {diff / ulp:.2f} ulp of the largest entry {largest:.2e}")
    assert diff <= 4 * ulp


def test_per_image_weights_reach_their_images():
    from audio_motion_avatar_amd import losses

    x64, y64 = case("mono_24x20")
    weights = torch.tensor([0.0, 1.5, -2.0], dtype=torch.float64)

    def grad(x, y, lib, w):
        x = x.clone().requires_grad_()
        (lib.ssim(x, y, size_average=False) * w).sum().backward()
        return x.grad

    ref = grad(x64, y64, losses, weights)
    x, y = x64.float().cuda(), y64.float().cuda()
    library, fused = grad(x, y, losses, weights.float().cuda()), grad(x, y, _Fused, weights.float().cuda())
    assert float(fused[0, 0].abs().max()) == 0.0                 # weight 0: exactly nothing
    for n in (1, 2):
        lib_err, our_err = err(library[0, n], ref[0, n]), err(fused[0, n], ref[0, n])
        print(f"\nimage {n} (weight {float(weights[n])}): err(library) = {lib_err:.2e}, err(fused) = {our_err:.2e}")
        assert our_err <= max(2 * lib_err, GRAD_FLOOR), n


def test_two_runs_are_bit_identical():
    from audio_motion_avatar_amd import ops

    x, y = (t.float().cuda()[0] for t in case("tiles_70x67"))
    runs = []
    for _ in range(2):
        xg = x.clone().requires_grad_()
        l1, s = ops.image_loss_differentiable(xg, y)
        (l1.sum() + 0.1 * s.sum()).backward()
        runs.append((l1.detach(), s.detach(), xg.grad))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_no_grad_forward_allocates_no_derivative_maps():
    from audio_motion_avatar_amd import _lib, ops

    x, y = (t.float().cuda()[0] for t in case("tiles_70x67"))
    N, H, W, C = x.shape
    workspace = _lib.lib().amav_image_loss_workspace_bytes(N, H, W)
    assert workspace == N * 25 * 8
    xg = x.clone().requires_grad_()
    with_grad = ops.image_loss_differentiable(xg, y)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    with torch.no_grad():
        without = ops.image_loss_differentiable(xg, y)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    # the workspace and the [2, N] sums, each rounded up to the allocator's 512-byte block
    allowed = (workspace + 511) // 512 * 512 + 512
    one_map = N * H * W * C * 4
    print(f"\nno-grad forward: peak {peak} B over the inputs; workspace {workspace} B, one derivative map {one_map} B")
    assert peak <= allowed < one_map
    assert without[0].grad_fn is None and with_grad[0].grad_fn is not None
    for a, b in zip(with_grad, without):
        assert torch.equal(a.detach(), b)


def test_refusals():
    from audio_motion_avatar_amd import losses, ops

    x, y = (t.float().cuda() for t in case("below_window_8x8"))
    with pytest.raises(ops.AmavError, match="requires a gradient"):
        losses.image_losses(x, y.clone().requires_grad_())
    five = torch.rand(1, 1, 8, 8, 5, device="cuda")
    with pytest.raises(ops.AmavError, match="channels"):
        losses.image_losses(five, five.clone())
    with pytest.raises(ops.AmavError, match="only runs on an MI355X"):
        losses.image_losses(x.cpu(), y.cpu())
    with pytest.raises(ops.AmavError, match="only runs on an MI355X"):
        losses.image_losses(x, y.cpu())
    with pytest.raises(ops.AmavError, match="dtype"):
        losses.image_losses(x.double(), y.double())
