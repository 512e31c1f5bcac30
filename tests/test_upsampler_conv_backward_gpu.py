"""GPU tests of the 3x3 cell convolution's backward (csrc/upsample_conv.hip, amav_conv3x3_cells_backward) through
ops.conv3x3_cells_differentiable with a random grad_out: every gradient against torch's autograd in fp64 on the CPU of
the forward restated on F.conv2d (tests/conv_backward_cases.py).

Bound for every gradient tensor (the rule of tests/test_split_gemm_gpu.py and tests/test_upsampler_conv_gpu.py): with
err = max |got - ref| and err32 the same for the library's fp32 autograd on the device with deterministic convolutions,
err <= max(1.5 err32, 2e-6 max |ref|).  All three numbers are printed."""
import pytest
import torch

from conv_backward_cases import GRADS, PLANE_ORIGINS, autograd_gradients, draw, library_gradients, within_bound

pytestmark = pytest.mark.gpu


def hip_gradients(tensors, grad_out, options, require=GRADS):
    """{name: gradient or None} through ops.conv3x3_cells_differentiable for the tensors of `require` that are there."""
    from audio_motion_avatar_amd import ops

    leaves = {k: v.cuda().requires_grad_(k in require) for k, v in tensors.items() if v is not None}
    opts = {k: v.cuda() if isinstance(v, torch.Tensor) else v for k, v in options.items()}
    out = ops.conv3x3_cells_differentiable(leaves["x"], leaves["weight"], leaves.get("bias"), in_scale=leaves.get("in_scale"),
                                           in_shift=leaves.get("in_shift"), residual=leaves.get("residual"), **opts)
    out.backward(grad_out.cuda())
    return {k: v.grad for k, v in leaves.items()}, out.detach()


def check(tensors, grad_out, **options):
    ref, _ = autograd_gradients(tensors, grad_out, options, torch.float64, "cpu")
    lib32 = library_gradients(tensors, grad_out, options)
    got, _ = hip_gradients(tensors, grad_out, options)
    assert set(got) == set(ref)
    for name in ref:
        within_bound(name, got[name], ref[name], lib32[name])
    return got


def test_plain_partial_tile():
    """75 rows: one partial tile in both directions, one slice, one 32 x 32 block."""
    check(*draw(3, 5, 5, 32, 32, 101))


def test_plain_several_tiles():
    """Several tiles per cell with tails, two chunks, three column blocks; Cin != Cout, so a transposed preparation
    that mixes the two widths up cannot pass."""
    check(*draw(5, 12, 12, 64, 96, 102))


@pytest.mark.parametrize("cout", [64, 128])
def test_every_column_width(cout):
    """The data gradient runs the 32-column kernel here and the forward the 64- / 128-column ones; the reversed widths
    send the data gradient through the wide kernels."""
    check(*draw(2, 9, 20, 32, cout, 103 + cout))
    check(*draw(2, 9, 20, cout, 32, 104 + cout))


def test_upsample_input_small():
    check(*draw(4, 3, 3, 32, 64, 105, upsample_input=True), upsample_input=True)


def test_upsample_input_pool_crosses_tiles():
    """22 x 18 fine texels: the 2 x 2 pool of grad_x reads across tile borders in both directions."""
    check(*draw(2, 11, 9, 32, 32, 106, upsample_input=True), upsample_input=True, relu_out=True)


def test_prologue_and_plane_rule():
    """relu(in_shift) > 0 at every zero of the operand: a backward that masks before the prologue, or forgets the plane
    rule in grad_x / grad_in_scale / grad_weight, is wrong at every one of them.  Then each half alone."""
    origin = torch.tensor(PLANE_ORIGINS, dtype=torch.int32)
    tensors, grad_out = draw(5, 12, 12, 64, 96, 107, prologue=True)
    check(tensors, grad_out, origin=origin, extent=20, relu_out=True)
    check(tensors, grad_out)                                   # the prologue without the plane rule
    plain, grad_out = draw(5, 12, 12, 64, 96, 108)
    check(plain, grad_out, origin=origin, extent=20)           # the plane rule without the prologue


def test_prologue_with_upsample_input():
    """All of the operand's steps at once, as no block needs them; the pooled gradient passes the prologue's gate."""
    tensors, grad_out = draw(3, 5, 7, 32, 64, 109, prologue=True, upsample_input=True)
    origin = torch.tensor([[-3, -2], [5, 9], [2, 2]], dtype=torch.int32)
    check(tensors, grad_out, upsample_input=True, origin=origin, extent=16)


def test_epilogues():
    check(*draw(3, 7, 18, 32, 64, 110, bias=False))
    check(*draw(3, 7, 18, 32, 64, 111), relu_out=True)
    got = check(*draw(3, 7, 18, 32, 64, 112, residual=True))
    assert got["residual"] is not None
    check(*draw(3, 7, 18, 32, 64, 113, bias=False, residual=True))


def test_grad_residual_is_grad_out_exactly():
    tensors, grad_out = draw(3, 7, 18, 32, 64, 114, residual=True)
    got, _ = hip_gradients(tensors, grad_out, {})
    assert torch.equal(got["residual"].cpu(), grad_out)


def test_relu_out_with_residual_is_refused():
    from audio_motion_avatar_amd import ops
    from audio_motion_avatar_amd._lib import AmavError

    tensors, _ = draw(2, 6, 6, 32, 32, 115, residual=True)
    with pytest.raises(AmavError, match="relu_out"):
        ops.conv3x3_cells_differentiable(tensors["x"].cuda().requires_grad_(), tensors["weight"].cuda(), tensors["bias"].cuda(),
                                         relu_out=True, residual=tensors["residual"].cuda())


@pytest.mark.parametrize("magnitude", [1e-4, 1.0, 3e3])
def test_grad_out_magnitudes(magnitude):
    tensors, grad_out = draw(3, 10, 10, 64, 32, 116, prologue=True)
    check(tensors, grad_out * magnitude, relu_out=True)


def test_zero_grad_out_gives_exact_zeros():
    tensors, grad_out = draw(5, 12, 12, 64, 96, 117, prologue=True)
    origin = torch.tensor(PLANE_ORIGINS, dtype=torch.int32)
    got, _ = hip_gradients(tensors, torch.zeros_like(grad_out), dict(origin=origin, extent=20, relu_out=True))
    for name, g in got.items():
        assert g is not None and not g.any(), name


def test_two_runs_are_bit_equal():
    tensors, grad_out = draw(5, 12, 12, 64, 96, 118, prologue=True)
    options = dict(origin=torch.tensor(PLANE_ORIGINS, dtype=torch.int32), extent=20, relu_out=True)
    a, out_a = hip_gradients(tensors, grad_out, options)
    b, out_b = hip_gradients(tensors, grad_out, options)
    assert torch.equal(out_a, out_b)
    for name in a:
        assert torch.equal(a[name], b[name]), name


@pytest.mark.parametrize("slices", [1, 3, 40])
def test_split_k_slices(slices):
    """The weight gradient's split-K on the multi-tile shape (5 cells x 2 tiles = 10 (cell, tile) pairs): one slice, three
    uneven ones, and more slices than pairs (empty ranges write zeros).  Each is within the bound and repeats itself bit
    for bit."""
    from audio_motion_avatar_amd import ops

    tensors, grad_out = draw(5, 12, 12, 64, 96, 119, prologue=True)
    options = dict(origin=torch.tensor(PLANE_ORIGINS, dtype=torch.int32), extent=20, relu_out=True)
    ref, _ = autograd_gradients(tensors, grad_out, options, torch.float64, "cpu")
    lib32 = library_gradients(tensors, grad_out, options)
    dev = {k: v.cuda() for k, v in tensors.items() if v is not None}
    with torch.no_grad():
        out = ops.conv3x3_cells(dev["x"], ops.conv3x3_prepare_weights(dev["weight"]), 96, dev["bias"], in_scale=dev["in_scale"],
                                in_shift=dev["in_shift"], origin=options["origin"].cuda(), extent=20, relu_out=True)
        runs = [ops.conv3x3_cells_backward(grad_out.cuda(), dev["x"], ops.conv3x3_prepare_weights_transposed(dev["weight"]),
                                           out=out, in_scale=dev["in_scale"], in_shift=dev["in_shift"],
                                           origin=options["origin"].cuda(), extent=20, relu_out=True, wgrad_slices=slices)
                for _ in range(2)]
    for name, got in zip(("x", "weight", "bias", "in_scale", "in_shift"), runs[0]):
        within_bound(name, got, ref[name], lib32[name])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_no_cells_returns_zeros():
    from audio_motion_avatar_amd import ops

    tensors, _ = draw(1, 6, 6, 32, 64, 120, prologue=True)
    leaves = {k: v.cuda().requires_grad_() for k, v in tensors.items() if v is not None}
    out = ops.conv3x3_cells_differentiable(leaves["x"][:0], leaves["weight"], leaves["bias"], in_scale=leaves["in_scale"],
                                           in_shift=leaves["in_shift"], relu_out=True)
    assert out.shape == (0, 6, 6, 64)
    out.sum().backward()
    for name, t in leaves.items():
        assert t.grad is not None and t.grad.shape == t.shape and not t.grad.any(), name


def test_only_some_inputs_require_grad():
    tensors, grad_out = draw(5, 12, 12, 64, 96, 121, prologue=True)
    options = dict(origin=torch.tensor(PLANE_ORIGINS, dtype=torch.int32), extent=20, relu_out=True)
    ref, _ = autograd_gradients(tensors, grad_out, options, torch.float64, "cpu")
    lib32 = library_gradients(tensors, grad_out, options)
    for require in (("weight",), ("x",), ("bias", "in_shift"), ("in_scale",)):
        got, _ = hip_gradients(tensors, grad_out, options, require)
        for name, g in got.items():
            if name in require:
                within_bound(name, g, ref[name], lib32[name])
            else:
                assert g is None, (require, name)


def test_refusals():
    from audio_motion_avatar_amd import ops
    from audio_motion_avatar_amd._lib import AmavError

    tensors, _ = draw(2, 6, 6, 32, 32, 122)
    x, w, b = tensors["x"], tensors["weight"], tensors["bias"]
    with pytest.raises(AmavError):
        ops.conv3x3_cells_differentiable(x.clone().requires_grad_(), w, b)                           # CPU tensors
    with pytest.raises(AmavError):
        ops.conv3x3_cells_differentiable(x.cuda(), w.cuda()[:, :, :2], b.cuda())            # not 3 x 3
    with pytest.raises(AmavError):
        ops.conv3x3_cells_differentiable(x.cuda(), torch.zeros(32, 64, 3, 3).cuda(), b.cuda())  # C_in does not match x
    with pytest.raises(AmavError, match="multiples of 32"):
        ops.conv3x3_cells_differentiable(x.cuda(), torch.zeros(40, 32, 3, 3).cuda())
    with pytest.raises(AmavError, match="multiples of 32"):
        ops.conv3x3_cells_differentiable(x[..., :24].cuda(), torch.zeros(32, 24, 3, 3).cuda())
    # what the new code must not change: the plain wrappers still carry no autograd
    prepared = ops.conv3x3_prepare_weights(w.cuda())
    with pytest.raises(AmavError, match="autograd"):
        ops.conv3x3_cells(x.cuda().requires_grad_(), prepared, 32)
    with pytest.raises(AmavError, match="autograd"):
        ops.conv3x3_prepare_weights(w.cuda().requires_grad_())
