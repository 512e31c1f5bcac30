"""GPU: ops.sh_colors / sh_colors_backward / sh_colors_differentiable (amav_sh_colors*) against the float64 torch model of
tests/sh_model.py, with that file's tolerances (2 x the fp32 model's own error; the measured ratios are printed).

Every (degree, F, N) is run in each memory layout on the same values: dense (the LDS tile with 16-byte copies), a base
address 4 bytes off (the tile with dword copies), an element stride of 3K + 5 (lane by lane) and the 4-d [F,N,K,3]
form; all must give the same bits, twice.  N covers a partial wave, one wave, a wave + 1 and several blocks."""
import os

import numpy as np
import pytest
import torch

import sh_model as sm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 63, 64, 65, 257, 1000)
FRAMES = (1, 3)


def _wider(t, extra):
    """The same values as a view of a buffer whose last axis is `extra` floats wider (NaN in the padding)."""
    buf = torch.full((*t.shape[:-1], t.shape[-1] + extra), float("nan"), device=t.device)
    buf[..., :t.shape[-1]] = t
    return buf[..., :t.shape[-1]]


def _shifted(t):
    """The same values, contiguous, starting 4 bytes behind a 16-byte boundary."""
    buf = torch.full((t.numel() + 1,), float("nan"), device=t.device)
    assert buf.data_ptr() % 16 == 0
    buf[1:] = t.reshape(-1)
    return buf[1:].view(t.shape)


def layouts(means3d, sh):
    """means3d [F,N,3], sh [F,N,K,3] dense on the device -> {name: (means3d, sh)} of equal values."""
    F, N, K, _ = sh.shape
    flat = sh.reshape(F, N, 3 * K)
    return {"dense": (means3d, flat), "4d": (means3d, sh), "shifted": (means3d, _shifted(flat)),
            "padded": (_wider(means3d, 2), _wider(flat, 5))}


def run(means3d, sh, campos, degree, grad_colors):
    """One forward and one backward -> (colors [F,N,3], grad_sh [F,N,K,3] from a NaN-filled buffer, grad_means3d)."""
    from audio_motion_avatar_amd import ops

    F, N = means3d.shape[0], means3d.shape[1]
    K = sh.shape[2] if sh.dim() == 4 else sh.shape[2] // 3
    colors = ops.sh_colors(means3d, sh, campos, degree)
    buf = torch.full((F, N, 3 * K), float("nan"), device=means3d.device)
    grad_sh, grad_means3d = ops.sh_colors_backward(means3d, sh, campos, degree, grad_colors, grad_sh=buf)
    assert grad_sh.data_ptr() == buf.data_ptr()
    return colors, grad_sh.view(F, N, K, 3), grad_means3d


def check_case(name, c):
    """All layouts of one case: the tolerances against the model on the dense layout, equal bits on the others."""
    truth, fp32 = sm.yardstick(c)
    means3d, sh = (t.contiguous().cuda() for t in sm.expanded(c))
    campos, go, degree = c["campos"].cuda(), c["grad_colors"].cuda(), c["degree"]
    first = None
    for layout, (p, s) in layouts(means3d, sh).items():
        got = run(p, s, campos, degree, go)
        again = run(p, s, campos, degree, go)
        for a, b in zip(got, again):
            assert torch.equal(a, b), f"{name} {layout}: two runs differ"
        if first is None:
            first = got
            colors, grad_sh, grad_means3d = (t.cpu() for t in got)
            assert not torch.isnan(grad_sh).any()
            used = sm.num_coeffs(degree)
            assert torch.equal(grad_sh[:, :, used:], torch.zeros_like(grad_sh[:, :, used:])), f"{name}: unused coefficients"
            sm.check_forward(name, colors, truth["colors"], fp32["colors"].float())
            sm.check_gradients(name, grad_sh, grad_means3d, truth, fp32)
        else:
            for what, a, b in zip(("colors", "grad_sh", "grad_means3d"), first, got):
                assert torch.equal(a, b), f"{name}: {what} of layout {layout} differs from dense"
    return first


@pytest.mark.parametrize("degree", [0, 1, 2, 3, 4])
def test_forward_and_backward_match_the_model_in_every_layout(degree):
    for F in FRAMES:
        for N in SIZES:
            check_case(f"deg {degree} F {F} N {N}", sm.case(1000 * degree + 10 * N + F, degree, F, N))


@pytest.mark.parametrize("N", SIZES)
def test_sixteen_stored_coefficients_at_degree_one(N):
    for F in FRAMES:
        check_case(f"deg 1 K 16 F {F} N {N}", sm.case(5000 + 10 * N + F, 1, F, N, K=16))


@pytest.mark.parametrize("degree", [0, 1, 2, 3, 4])
def test_shared_gaussians_frame_stride_zero(degree):
    """sh and means3d with frame stride 0: the bits of the expanded dense copy, one gradient row per frame, and through
    autograd .grad = the ascending sum of those rows."""
    from audio_motion_avatar_amd import ops

    for N in (65, 257):
        c = sm.case(6000 + 10 * degree + N, degree, 3, N, shared=True)
        truth, fp32 = sm.yardstick(c)
        p1, s1 = c["means3d"].cuda(), c["sh"].cuda()
        campos, go = c["campos"].cuda(), c["grad_colors"].cuda()
        pe, se = p1.expand(3, -1, -1), s1.expand(3, -1, -1, -1)
        assert pe.stride(0) == 0 and se.stride(0) == 0
        shared = run(pe, se, campos, degree, go)
        dense = run(pe.contiguous(), se.contiguous(), campos, degree, go)
        for what, a, b in zip(("colors", "grad_sh", "grad_means3d"), shared, dense):
            assert torch.equal(a, b), f"deg {degree} N {N}: {what} with stride 0 differs from the dense copy"
        sm.check_forward(f"shared deg {degree} N {N}", shared[0].cpu(), truth["colors"], fp32["colors"].float())
        sm.check_gradients(f"shared deg {degree} N {N}", shared[1].cpu(), shared[2].cpu(), truth, fp32)
        # autograd: expanded views go in as they are, expand's backward sums the rows
        p, s = p1.clone().requires_grad_(), s1.clone().requires_grad_()
        out = ops.sh_colors_differentiable(p.expand(3, -1, -1), s.expand(3, -1, -1, -1), campos, degree)
        assert torch.equal(out, shared[0])
        (out * go).sum().backward()
        rows_sh, rows_p = shared[1], shared[2]
        assert torch.equal(s.grad[0], (rows_sh[0] + rows_sh[1]) + rows_sh[2])
        if degree > 0:
            assert torch.equal(p.grad[0], (rows_p[0] + rows_p[1]) + rows_p[2])
        else:
            assert p.grad is None or not p.grad.any()


def test_autograd_dense_and_needs_input_grad():
    from audio_motion_avatar_amd import ops

    c = sm.case(6500, 2, 2, 130)
    truth, fp32 = sm.yardstick(c)
    campos, go = c["campos"].cuda(), c["grad_colors"].cuda()
    p, s = c["means3d"].cuda().requires_grad_(), c["sh"].cuda().requires_grad_()
    (ops.sh_colors_differentiable(p, s, campos, 2) * go).sum().backward()
    assert s.grad.shape == s.shape and p.grad.shape == p.shape
    sm.check_gradients("autograd deg 2", s.grad.cpu(), p.grad.cpu(), truth, fp32)
    q = c["sh"].cuda().requires_grad_()
    (ops.sh_colors_differentiable(c["means3d"].cuda(), q.reshape(2, 130, 27), campos, 2) * go).sum().backward()
    assert torch.equal(q.grad, s.grad)
    with torch.no_grad():
        assert not ops.sh_colors_differentiable(p, s, campos, 2).requires_grad


def test_fixture_on_the_device():
    """tests/golden/ref_sh.npz (the reference's own eval_sh, fp32 on the CPU): the device's colours against the float64
    model, with e32 = the error of the reference's stored result."""
    from audio_motion_avatar_amd import ops

    data = np.load(os.path.join(ROOT, "tests", "golden", "ref_sh.npz"))
    for name in ("deg0", "deg1", "deg2", "deg3", "deg4", "deg1_k16"):
        c = {k: torch.from_numpy(data[f"{name}/{k}"]) for k in ("means3d", "sh", "campos", "colors")}
        degree = int(data[f"{name}/degree"])
        means3d, sh = c["means3d"].cuda().expand(3, -1, -1), c["sh"].cuda().expand(3, -1, -1, -1)
        got = ops.sh_colors(means3d, sh, c["campos"].cuda(), degree).cpu()
        f64 = sm.colors(c["means3d"].double().expand(3, -1, -1), c["sh"].double().expand(3, -1, -1, -1),
                        c["campos"].double(), degree)
        sm.check_forward("fixture " + name, got, f64, c["colors"])


def test_refusals_on_the_device():
    from audio_motion_avatar_amd import ops

    p, sh, cam = torch.zeros(2, 8, 3).cuda(), torch.zeros(2, 8, 9, 3).cuda(), torch.zeros(2, 3).cuda()
    with pytest.raises(ops.AmavError, match=r"needs \(degree\+1\)\^2 = 16"):
        ops.sh_colors(p, sh, cam, 3)
    with pytest.raises(ops.AmavError, match="does not match means3d"):
        ops.sh_colors(p[:, :4], sh, cam, 2)
    with pytest.raises(ops.AmavError, match="campos"):
        ops.sh_colors(p, sh, cam[:1], 2)
    with pytest.raises(ops.AmavError, match="grad_colors"):
        ops.sh_colors_backward(p, sh, cam, 2, torch.zeros(2, 8, 4).cuda())
    assert ops.sh_colors(p[:, :0], sh[:, :0], cam, 2).shape == (2, 0, 3)
