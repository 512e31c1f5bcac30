"""Backward of the triplane feature sampling (csrc/triplane_sample_backward.hip) against fp64
torch autograd of oracle.triplane.sample_from_triplane on the CPU.

Bound per gradient tensor, the convention of tests/test_point_refiner_backward_gpu.py:
    max|g - g64| <= max(4 * err32, 2e-5 * max|g64|),   err32 = max|g32 - g64| of the same restatement run in fp32.
Every comparison prints err, err32 and max|g64| before it asserts."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

RADIUS = 1.4

# (F, N, C, R): the issue's five -- tiled forward with a ragged last 64-point block; general forward; general forward
# above one wave of channels; two channel chunks per plane; the refiner's own widths -- and three of this file's: R = 6
# (tiles ragged in both directions, R^2 % 4 != 0) with a single point, R = 48 (the point ordering keeps its histograms
# in the workspace above R = 41, in LDS below), and N = 1200 at R = 8 (waves of the ordering with several chunks each).
SHAPES = [(2, 130, 64, 8), (3, 300, 8, 8), (2, 257, 48, 16), (2, 1000, 128, 32), (1, 3000, 256, 32),
          (2, 1, 5, 6), (2, 200, 8, 48), (1, 1200, 3, 8)]
# every shape with contiguous planes and with the renderer's view of a token slab; one with a frame stride beyond the frame
CASES = [(*s, layout) for s in SHAPES for layout in ("contiguous", "slab")] + [(2, 257, 48, 16, "gapped")]


def _ops():
    from audio_motion_avatar_amd import ops

    return ops


def _points(g, F, N, R, radius, spread=1.15):
    """Uniform in +-spread * radius (some beyond the clamp, some with taps off the plane edge), nudged 1e-3 texel away
    from texel centres and from the clamp boundary (tests/test_decode_backward_gpu.py::_points)."""
    p = ((torch.rand(F, N, 3, generator=g, dtype=torch.float64) * 2 - 1) * spread * radius)
    u = p / radius
    for _ in range(3):
        pix = ((u.clamp(-1, 1) + 1) * R - 1) / 2
        frac = pix - pix.round()
        near = (frac.abs() < 1e-3) | ((u.abs() - 1).abs() < 1e-3 * 2 / R)
        u = torch.where(near, u + 3e-3 * 2 / R, u)
    return (u * radius).float()


def _oracle(planes, points, gout, radius, dtype):
    from oracle import triplane as orc

    pl = planes.to(dtype).clone().requires_grad_()
    pt = points.to(dtype).clone().requires_grad_()
    out = orc.sample_from_triplane(pl, pt, radius)
    out.backward(gout.to(dtype))
    return out.detach(), pl.grad, pt.grad


@functools.lru_cache(maxsize=None)
def _case(F, N, C, R):
    """Inputs and the fp64 / fp32 CPU references of one shape, computed once for the module and never modified."""
    g = torch.Generator().manual_seed(F * 7919 + N * 31 + C * 7 + R)
    planes = torch.randn(F, 3, C, R, R, generator=g)
    points = _points(g, F, N, R, RADIUS)
    gout = torch.randn(F, N, 3 * C, generator=g)
    return dict(planes=planes, points=points, gout=gout, ref64=_oracle(planes, points, gout, RADIUS, torch.float64),
                ref32=_oracle(planes, points, gout, RADIUS, torch.float32))


def _check(name, got, g64, g32):
    """The module's bound; returns err / bound."""
    g64 = g64.double()
    err = float((got.detach().cpu().double() - g64).abs().max())
    err32 = float((g32.double() - g64).abs().max())
    big = float(g64.abs().max())
    bound = max(4 * err32, 2e-5 * big)
    print(f"{name}: err {err:.3e}  err32 {err32:.3e}  max|g64| {big:.3e}  err/bound {err / max(bound, 1e-300):.3f}")
    assert torch.isfinite(got).all(), name
    assert err <= bound, (name, err, err32, big)
    return err / max(bound, 1e-300)


def _to_slab(planes):
    """[F,3,C,R,R] -> the token slab [F,C,3R^2] whose permuted view it is."""
    F, _, C, R, _ = planes.shape
    return planes.permute(0, 2, 1, 3, 4).reshape(F, C, 3 * R * R).contiguous()


def _gpu_grads(planes, points, gout, layout="contiguous", radius=RADIUS, want=(True, True)):
    """-> (features, gradient at the leaf in the layout of [F,3,C,R,R], d points, the leaf)."""
    ops = _ops()
    F, _, C, R, _ = planes.shape
    if layout == "contiguous":
        leaf = planes.cuda().requires_grad_(want[0])
        view = leaf
    else:
        slab = _to_slab(planes).cuda()
        if layout == "gapped":  # frame stride larger than the frame: five more channel rows per frame
            slab = torch.cat([slab, torch.full((F, 5, 3 * R * R), 7.0, device="cuda")], 1)
        leaf = slab.requires_grad_(want[0])
        view = leaf[:, :C].view(F, C, 3, R, R).permute(0, 2, 1, 3, 4)
        assert view.stride(0) == leaf.shape[1] * 3 * R * R and view.stride(1) == R * R and view.stride(2) == 3 * R * R
    pts = points.cuda().requires_grad_(want[1])
    out = ops.triplane_sample_features_differentiable(view, pts, radius)
    out.backward(gout.cuda())
    gl = leaf.grad
    if gl is not None and layout != "contiguous":
        if layout == "gapped":
            assert (gl[:, C:] == 0).all()
        gl = gl[:, :C].reshape(F, C, 3, R, R).permute(0, 2, 1, 3, 4)
    return out.detach(), gl, pts.grad, leaf


# ------------------------------------------------------------------------------------------------------- accuracy
@pytest.mark.parametrize("F,N,C,R,layout", CASES)
def test_gradients_match_fp64_autograd(F, N, C, R, layout):
    case = _case(F, N, C, R)
    (o64, pl64, pt64), (o32, pl32, pt32) = case["ref64"], case["ref32"]
    out, gpl, gpt, _ = _gpu_grads(case["planes"], case["points"], case["gout"], layout)
    assert (out.cpu().double() - o64).abs().max() <= max(4 * float((o32.double() - o64).abs().max()), 2e-5 * float(o64.abs().max()))
    label = f"F={F} N={N} C={C} R={R} {layout}"
    _check(f"{label} d planes", gpl, pl64, pl32)
    _check(f"{label} d points", gpt, pt64, pt32)
    if layout != "contiguous":  # the strides only say where a sum is stored
        _, gpl0, gpt0, _ = _gpu_grads(case["planes"], case["points"], case["gout"], "contiguous")
        assert torch.equal(gpl, gpl0) and torch.equal(gpt, gpt0)


def _kink_points(F, R, g):
    """Points on the derivative's kinks, exactly: p / radius (radius 2) on texel centres ((2k + 1) / R - 1), on +-1 and
    beyond +-1 (+-1.25), each coordinate drawn from those values (dyadic: fp32 and fp64 take the same branch)."""
    centres = [(2 * k + 1) / R - 1 for k in range(R)]
    values = torch.tensor(centres + [-1.0, 1.0, -1.0, 1.0, -1.25, 1.25], dtype=torch.float64)
    idx = torch.randint(0, len(values), (F, 6 * R, 3), generator=g)
    return values[idx] * 2.0


def test_gradients_at_kinks():
    """Texel centres (weights exactly 0 and 1), plane edges (taps at -1 and R) and |p / radius| = 1: the conventions of
    torch's grid_sampler and clamp backwards, through fp64 autograd of the oracle."""
    F, C, R, radius = 2, 16, 16, 2.0
    g = torch.Generator().manual_seed(551)
    exact = _kink_points(F, R, g)
    points = torch.cat([exact.float(), _points(g, F, 400 - exact.shape[1], R, radius)], 1)
    assert torch.equal(points[:, :exact.shape[1]].double(), exact)
    u = exact / radius
    pix = ((u.clamp(-1, 1) + 1) * R - 1) / 2
    assert (pix == pix.round()).sum() > 200 and (u.abs() == 1).sum() > 50 and (u.abs() > 1).sum() > 20
    assert (pix.floor() == -1).any() and (pix.floor() + 1 == R).any()  # taps at -1 and at R
    planes = torch.randn(F, 3, C, R, R, generator=g)
    gout = torch.randn(F, 400, 3 * C, generator=g)
    _, pl64, pt64 = _oracle(planes, points, gout, radius, torch.float64)
    _, pl32, pt32 = _oracle(planes, points, gout, radius, torch.float32)
    M = exact.shape[1]
    assert (pt64[:, :M][u.abs() > 1] == 0).all() and (pt64[:, :M][u.abs() == 1] != 0).any()
    _, gpl, gpt, _ = _gpu_grads(planes, points, gout, "slab", radius=radius)
    _check("kinks d planes", gpl, pl64, pl32)
    _check("kinks d points", gpt, pt64, pt32)
    assert (gpt.cpu()[:, :M][u.abs() > 1] == 0).all()


def _raw_backward(planes, points, gout, grad_planes, radius=RADIUS):
    """The C entry point on the caller's output buffer (contiguous [F,3,C,R,R])."""
    from audio_motion_avatar_amd import _lib

    F, _, C, R, _ = planes.shape
    N = points.shape[1]
    lib = _lib.lib()
    nbytes = lib.amav_triplane_sample_features_backward_bytes(F, N, C, R)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    gpts = torch.full((F, N, 3), float("nan"), device="cuda")
    a = _lib.TriplaneSampleBackwardArgs()
    a.num_frames, a.num_points, a.channels, a.resolution, a.radius = F, N, C, R, radius
    a.planes, a.points, a.grad_out = planes.data_ptr(), points.data_ptr(), gout.data_ptr()
    a.planes_frame_stride, a.planes_plane_stride, a.planes_chan_stride = planes.stride(0), planes.stride(1), planes.stride(2)
    a.grad_planes, a.grad_points = grad_planes.data_ptr(), gpts.data_ptr()
    a.grad_frame_stride, a.grad_plane_stride, a.grad_chan_stride = (grad_planes.stride(0), grad_planes.stride(1),
                                                                    grad_planes.stride(2))
    a.scratch, a.scratch_bytes = scratch.data_ptr(), nbytes
    _lib.check(lib.amav_triplane_sample_features_backward(ctypes.byref(a), None))
    torch.cuda.synchronize()
    return gpts


def test_clustered_points_and_untouched_texels():
    """500 points inside one texel cell of every plane (long ordered sums on four texels per plane), nothing anywhere
    else: those texels against fp64, exact zeros everywhere else, and every element of a canary-filled buffer written."""
    F, N, C, R = 2, 500, 70, 16
    g = torch.Generator().manual_seed(77)
    # pixel coordinates in (5.1, 5.9) x (9.1, 9.9) x (2.1, 2.9): the taps are texels 5, 6 / 9, 10 / 2, 3
    lo = torch.tensor([5.1, 9.1, 2.1], dtype=torch.float64)
    pix = lo + 0.8 * torch.rand(F, N, 3, generator=g, dtype=torch.float64)
    points = (((2 * pix + 1) / R - 1) * RADIUS).float()
    planes = torch.randn(F, 3, C, R, R, generator=g)
    gout = torch.randn(F, N, 3 * C, generator=g)
    _, pl64, pt64 = _oracle(planes, points, gout, RADIUS, torch.float64)
    _, pl32, pt32 = _oracle(planes, points, gout, RADIUS, torch.float32)
    touched = torch.zeros(3, R, R, dtype=torch.bool)
    touched[0, 9:11, 5:7] = touched[1, 2:4, 5:7] = touched[2, 2:4, 9:11] = True  # plane 0 (x, y), 1 (x, z), 2 (y, z)
    assert (pl64[:, ~touched.unsqueeze(1).expand(3, C, R, R)] == 0).all() and (pl64[:, touched.unsqueeze(1).expand(3, C, R, R)] != 0).all()
    buf = torch.full((F, 3, C, R, R), float("nan"), device="cuda")
    gpts = _raw_backward(planes.cuda(), points.cuda(), gout.cuda(), buf)
    assert not torch.isnan(buf).any() and not torch.isnan(gpts).any()  # every element written
    mask = touched.unsqueeze(1).expand(3, C, R, R)
    outside = buf.cpu()[:, ~mask]
    assert (outside == 0).all() and not torch.signbit(outside).any()  # exactly +0.0 where no tap lands
    _check("clustered d planes", buf, pl64, pl32)
    _check("clustered d points", gpts, pt64, pt32)


# ---------------------------------------------------------------------------------------------------- determinism
def test_gradients_are_bitwise_reproducible_and_frame_independent():
    F, N, C, R = 3, 700, 64, 16
    g = torch.Generator().manual_seed(5)
    planes, gout = torch.randn(F, 3, C, R, R, generator=g), torch.randn(F, N, 3 * C, generator=g)
    points = _points(g, F, N, R, RADIUS)
    points[:, 100:400] = points[:, :1] + 0.01 * torch.randn(F, 300, 3, generator=g)  # long sums on few texels
    _, gpl, gpt, _ = _gpu_grads(planes, points, gout, "slab")
    _, gpl2, gpt2, _ = _gpu_grads(planes, points, gout, "slab")
    assert torch.equal(gpl, gpl2) and torch.equal(gpt, gpt2)
    for f in range(F):  # a frame of the batch = that frame alone
        _, g1, p1, _ = _gpu_grads(planes[f:f + 1], points[f:f + 1], gout[f:f + 1], "slab")
        assert torch.equal(g1[0], gpl[f]) and torch.equal(p1[0], gpt[f]), f
    perm = [2, 0, 1]  # permuting the frames permutes the result
    _, gp, pp, _ = _gpu_grads(planes[perm], points[perm], gout[perm], "slab")
    assert torch.equal(gp, gpl[perm]) and torch.equal(pp, gpt[perm])


# ------------------------------------------------------------------------------------------------- the Function
@pytest.mark.parametrize("C", [64, 24])  # the tiled and the general forward kernel
def test_forward_is_unchanged_and_gradients_follow_needs_input_grad(C):
    ops = _ops()
    F, N, R = 2, 150, 8
    g = torch.Generator().manual_seed(C)
    planes, gout = torch.randn(F, 3, C, R, R, generator=g), torch.randn(F, N, 3 * C, generator=g)
    points = _points(g, F, N, R, RADIUS)
    plain = ops.triplane_sample_features(planes.cuda(), points.cuda(), RADIUS)
    assert plain.grad_fn is None
    out, gpl, gpt, leaf = _gpu_grads(planes, points, gout, "contiguous")
    assert torch.equal(out, plain)
    assert leaf.grad.stride() == leaf.stride()
    slab_out, _, _, slab = _gpu_grads(planes, points, gout, "slab")
    assert torch.equal(slab_out, plain) and slab.grad.is_contiguous()
    # only one input requires grad: the other's .grad stays None, the wanted one keeps its bits
    out_p, gpl_only, none_pts, _ = _gpu_grads(planes, points, gout, "contiguous", want=(True, False))
    assert none_pts is None and torch.equal(gpl_only, gpl) and torch.equal(out_p, plain)
    out_q, none_planes, gpt_only, _ = _gpu_grads(planes, points, gout, "contiguous", want=(False, True))
    assert none_planes is None and torch.equal(gpt_only, gpt) and torch.equal(out_q, plain)
    # nothing requires grad: no graph
    assert ops.triplane_sample_features_differentiable(planes.cuda(), points.cuda(), RADIUS).grad_fn is None
