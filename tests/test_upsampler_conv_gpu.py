"""GPU tests of ops.conv3x3_cells / ops.conv3x3_prepare_weights (csrc/upsample_conv.hip): the 3x3 convolution over
independent channels-last cells on fp16 x 2 split products, against F.conv2d in fp64 on the CPU from the same
fp32-drawn inputs.

Bound (the rule of tests/test_split_gemm_gpu.py): with err = max |got - ref| and err32 the same for the library's fp32
convolution on the device, err <= max(1.5 err32, 2e-6 max |ref|): fp32-equivalent, with a floor of a few fp32 ulps of
the largest output for the cases where the library happens to be nearly exact."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def reference(x, w, bias=None, *, upsample_input=False, in_scale=None, in_shift=None, origin=None, extent=0,
              relu_out=False, residual=None, dtype=torch.float64, device="cpu"):
    """conv3x3_cells restated on F.conv2d: x [K,h,w,Cin] channels-last -> [K,H,W,Cout] in `dtype` on `device`.  The
    operand is masked AFTER BatchNorm + ReLU and zero padded by the convolution."""
    def cast(t):
        return None if t is None else t.to(device=device, dtype=dtype)

    v = cast(x).permute(0, 3, 1, 2)
    if upsample_input:
        v = F.interpolate(v, scale_factor=2, mode="nearest")
    if in_scale is not None:
        v = torch.relu(v * cast(in_scale)[None, :, None, None] + cast(in_shift)[None, :, None, None])
    if origin is not None:
        K, _, H, W = v.shape
        o = origin.to(device).long()
        py = o[:, 0, None] + torch.arange(H, device=device)
        px = o[:, 1, None] + torch.arange(W, device=device)
        inside = ((py >= 0) & (py < extent))[:, :, None] & ((px >= 0) & (px < extent))[:, None, :]
        v = v * inside[:, None].to(dtype)
    y = F.conv2d(v, cast(w), cast(bias), padding=1)
    if relu_out:
        y = torch.relu(y)
    y = y.permute(0, 2, 3, 1)
    if residual is not None:
        y = y + cast(residual)
    return y


def check(x, w, bias=None, *, prepared=None, w_ref=None, **options):
    """Run the kernel and both references; print and bound the errors.  w_ref: the weight the references use when the
    prepared buffer was made from something else (an output scale).  -> the kernel's result."""
    from audio_motion_avatar_amd import ops

    def dev(t):
        return None if t is None else t.cuda()

    options_dev = {k: dev(v) if isinstance(v, torch.Tensor) else v for k, v in options.items()}
    if prepared is None:
        prepared = ops.conv3x3_prepare_weights(w.cuda())
    w_ref = w if w_ref is None else w_ref
    with torch.no_grad():
        got = ops.conv3x3_cells(x.cuda(), prepared, w.shape[0], dev(bias), **options_dev)
        ref = reference(x, w_ref, bias, **options)
        lib32 = reference(x, w_ref.float(), bias, dtype=torch.float32, device="cuda", **options)
    assert got.dtype == torch.float32 and got.shape == ref.shape
    err = float((got.cpu().double() - ref).abs().max())
    err32 = float((lib32.cpu().double() - ref).abs().max())
    top = float(ref.abs().max())
    print(f"err {err:.3e}  err32 {err32:.3e}  max|ref| {top:.3e}")
    assert torch.isfinite(got).all()
    assert err <= max(1.5 * err32, 2e-6 * top), (err, err32, top)
    return got


def draw(K, h, w, cin, cout, seed, bias=True):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(K, h, w, cin, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) * (9 * cin) ** -0.5
    b = torch.randn(cout, generator=g) if bias else None
    return g, x, wt, b


def test_plain_small():
    """75 rows: less than one tile, odd sizes, a partial tile in both directions."""
    _, x, w, b = draw(3, 5, 5, 32, 32, 1)
    check(x, w, b)


def test_plain_several_tiles():
    """720 rows: several tiles per cell with a tail, three column blocks, two K chunks per tap."""
    _, x, w, b = draw(5, 12, 12, 64, 96, 2)
    check(x, w, b)


@pytest.mark.parametrize("cout", [64, 128])
def test_every_column_width(cout):
    """The 64- and 128-column kernels (the two above run the 32-column one), two tiles along x."""
    _, x, w, b = draw(2, 9, 20, 32, cout, 3 + cout)
    check(x, w, b)


def test_upsample_input_pads_at_the_fine_level():
    _, x, w, b = draw(4, 3, 3, 32, 64, 4)
    check(x, w, b, upsample_input=True)


def test_upsample_input_larger_than_a_tile():
    _, x, w, b = draw(2, 11, 9, 32, 32, 5)
    check(x, w, b, upsample_input=True, relu_out=True)


def test_prologue_and_plane_rule():
    """Cells over the low corner (negative origin), over the high corner, inside, mixed, and touching the far border:
    relu(in_shift) > 0, so a kernel that pads or masks before the prologue is wrong at every zero."""
    g, x, w, b = draw(5, 12, 12, 64, 96, 6)
    in_scale = torch.rand(64, generator=g) + 0.5
    in_shift = torch.rand(64, generator=g) + 0.25
    origin = torch.tensor([[-3, -2], [14, 13], [4, 4], [-3, 13], [0, 8]], dtype=torch.int32)
    got = check(x, w, b, in_scale=in_scale, in_shift=in_shift, origin=origin, extent=20, relu_out=True)
    wrong = reference(x, w, b, in_scale=in_scale, in_shift=in_shift, relu_out=True)  # no plane rule
    assert float((got.cpu().double() - wrong).abs().max()) > 1e-2
    # the prologue without the plane rule: the cell's own padding must still be zero, not relu(in_shift)
    check(x, w, b, in_scale=in_scale, in_shift=in_shift)
    # the plane rule without the prologue (the third convolution of a block)
    check(x, w, b, origin=origin, extent=20)


def test_epilogues():
    g, x, w, b = draw(3, 7, 18, 32, 64, 7)
    res = torch.randn(3, 7, 18, 64, generator=g)
    check(x, w, None)                       # bias absent
    check(x, w, b, relu_out=True)
    check(x, w, b, residual=res)
    check(x, w, None, residual=res)


@pytest.mark.parametrize("magnitude", [1e-4, 1.0, 3e3])
def test_activation_magnitudes(magnitude):
    _, x, w, b = draw(3, 10, 10, 64, 32, 8)
    check(x * magnitude, w, b * magnitude)


def test_zero_input_returns_the_bias_exactly():
    from audio_motion_avatar_amd import ops

    _, x, w, b = draw(2, 6, 6, 32, 32, 9)
    got = ops.conv3x3_cells(torch.zeros_like(x).cuda(), ops.conv3x3_prepare_weights(w.cuda()), 32, b.cuda())
    assert torch.equal(got.cpu(), b.expand(2, 6, 6, 32))


def test_tiny_weights():
    _, x, w, b = draw(3, 10, 10, 64, 32, 10)
    check(x, w * 2.0 ** -20, b * 2.0 ** -20)


def test_repeatable():
    from audio_motion_avatar_amd import ops

    g, x, w, b = draw(5, 12, 12, 64, 96, 11)
    x, b, prepared = x.cuda(), b.cuda(), ops.conv3x3_prepare_weights(w.cuda())
    origin = torch.tensor([[-3, -2], [14, 13], [4, 4], [-3, 13], [0, 8]], dtype=torch.int32).cuda()
    scale, shift = torch.rand(64, generator=g).cuda(), torch.rand(64, generator=g).cuda()
    runs = [ops.conv3x3_cells(x, prepared, 96, b, in_scale=scale, in_shift=shift, origin=origin, extent=20) for _ in range(2)]
    assert torch.equal(runs[0], runs[1])
    assert torch.equal(prepared, ops.conv3x3_prepare_weights(w.cuda()))


def test_prepared_output_scale():
    from audio_motion_avatar_amd import ops

    g, x, w, b = draw(3, 10, 10, 64, 96, 12)
    scale = torch.randn(96, generator=g) * 2.0
    prepared = ops.conv3x3_prepare_weights(w.cuda(), scale.cuda())
    check(x, w, b, prepared=prepared, w_ref=w.double() * scale.double()[:, None, None, None])


def test_wrappers_refuse_what_they_cannot_do():
    from audio_motion_avatar_amd import ops
    from audio_motion_avatar_amd._lib import AmavError

    _, x, w, b = draw(2, 6, 6, 32, 32, 13)
    prepared = ops.conv3x3_prepare_weights(w.cuda())
    with pytest.raises(AmavError):
        ops.conv3x3_cells(x, prepared, 32)                                # not on the device
    with pytest.raises(AmavError):
        ops.conv3x3_cells(x.cuda().requires_grad_(), prepared, 32)        # no autograd
    with pytest.raises(AmavError):
        ops.conv3x3_prepare_weights(w.cuda().requires_grad_())
    with pytest.raises(AmavError):
        ops.conv3x3_cells(x.cuda(), prepared, 64)                         # prepared for other widths
    with pytest.raises(AmavError):
        ops.conv3x3_cells(x[:, :5].cuda(), prepared, 32, upsample_input=False, in_scale=torch.ones(32).cuda())
    with pytest.raises(AmavError):
        ops.conv3x3_prepare_weights(torch.zeros(40, 32, 3, 3).cuda())     # channels
    with torch.no_grad():                                                  # grad mode off: parameters are fine
        ops.conv3x3_cells(x.cuda().requires_grad_(), prepared, 32)
