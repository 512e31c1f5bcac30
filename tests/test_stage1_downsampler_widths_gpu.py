"""The TriplaneDownsampler kernels (csrc/convnext.hip) on the MI355X at every built width, on
off-square tile grids and at small, large and offset magnitudes, against the fp64 restatement of
tests/downsampler_cases.py.  tests/test_stage1_downsampler_gpu.py runs V = C / 64 = 1 and 4 on square grids of at most
2 x 2 tiles with var(y) ~ 1; here (downsampler_cases.WIDE_CASES, whose conditions tests/test_stage1_downsampler_cases.py
asserts on the CPU):

    widths   V = 1..8 on 19 x 27 (3 x 4 tiles, ragged, two tiles with their halo inside the plane; 12 tiles), 27 x 19,
             17 x 17 (9 tiles; 289 rows: a last LayerNorm chunk of one row) and K = 3 of them (27 tiles)
    eps      var(y) ~ eps = 1e-6: a kernel that drops eps, or adds it outside the root, is off by half the output
    large    inputs x 1e3
    offset   row mean 8 at a row deviation of 1

Bounds (downsampler_cases.bound_wide): LIBRARY_ERR_WIDE[group, kind] x 4 -- the library's own fp32 error against the
same restatement over the group's cases (measure_library_wide; the larger of CPU and MI355X, rounded up to one digit),
times 4 for the different summation order.  Measured (every test prints its own figure):

    group    kind     library fp32, CPU   library fp32, MI355X   HIP kernels, MI355X   bound
    widths   conv         2.8e-7              3.1e-7                 2.8e-7                1.6e-06
    widths   norm         4.6e-7              3.2e-7                 3.2e-7                2.0e-06
    widths   dx           3.3e-7              3.1e-7                 3.2e-7                1.6e-06
    widths   dparam       9.0e-7              9.8e-7                 2.6e-7                4.0e-06
    eps      conv         2.3e-7              2.4e-7                 2.3e-7                1.2e-06
    eps      norm         2.8e-7              2.7e-7                 3.2e-7                1.2e-06
    eps      dx           2.1e-7              2.5e-7                 2.3e-7                1.2e-06
    eps      dparam       2.8e-7              5.2e-7                 2.0e-7                2.4e-06
    large    conv         2.6e-7              2.1e-7                 2.6e-7                1.2e-06
    large    norm         2.8e-7              2.7e-7                 2.8e-7                1.2e-06
    large    dx           2.6e-7              2.3e-7                 2.5e-7                1.2e-06
    large    dparam       3.2e-7              5.2e-7                 1.5e-7                2.4e-06
    offset   conv         9.1e-8              9.9e-8                 9.1e-8                4.0e-07
    offset   norm         6.6e-7              2.6e-6                 6.8e-7                1.2e-05
    offset   dx           3.2e-7              6.4e-7                 2.5e-7                2.8e-06
    offset   dparam       7.3e-7              5.1e-6                 6.3e-7                2.4e-05

bias + GELU at inner = 1024 (the product's 4 C) and inner = 12 keeps LIBRARY_ERR's gelu / dgelu / dparam entries: the
library measures 8.8e-8 / 1.5e-7 / 1.3e-7 (value, d proj, d bias) on the CPU and 6.6e-8 / 8.6e-8 / 1.4e-7 on the MI355X
there, the HIP kernels 6.6e-8 / 8.6e-8 / 1.5e-7.  The patch gather is a copy and its transpose adds at most four
terms: exact / three roundings, as in tests/test_stage1_downsampler_gpu.py."""
import pytest
import torch

import downsampler_cases as dc

pytestmark = pytest.mark.gpu

GRADS = ("dx", "d dw_weight", "d dw_bias", "d ln_weight", "d ln_bias")


def check(bound, got, want, what):
    err = dc.rel_err(got, want)
    print(f"{what}: error {err:.3e} (bound {bound:.1e})")
    assert err <= bound, f"{what}: {err:.3e} > {bound:.1e}"


def cuda(ts):
    return [t.cuda() for t in ts]


# ------------------------------------------------------------------------------------------ depthwise 7x7 + LayerNorm
@pytest.mark.parametrize("case", dc.WIDE_CASES, ids=dc.case_id)
def test_dwconv7_layernorm_forward(case):
    from audio_motion_avatar_amd import ops

    group, name = case[0], dc.case_id(case)
    args, eps, (y, n), _, _ = dc.wide_case(case)
    dev = cuda(args)
    rows, got_y = ops.dwconv7_layernorm(*dev, eps=eps, want_y=True)
    check(dc.bound_wide(group, "conv"), got_y, y, f"{name} conv")
    check(dc.bound_wide(group, "norm"), rows, n, f"{name} norm")
    assert torch.equal(ops.dwconv7_layernorm(*dev, eps=eps), rows)      # with and without the stored y
    again, y_again = ops.dwconv7_layernorm(*dev, eps=eps, want_y=True)
    assert torch.equal(again, rows) and torch.equal(y_again, got_y)     # two calls bit-equal
    # the split outputs are amav_split_operand's operands of the fp32 rows, part for part
    bf = ops.dwconv7_layernorm(*dev, eps=eps, split=ops.SPLIT_BF16X3)
    assert torch.equal(bf.float(), ops.split_operand(rows).float())
    fp = ops.dwconv7_layernorm(*dev, eps=eps, split=ops.SPLIT_FP16X2, split_exp=9)
    assert torch.equal(fp.float(), ops.split_operand(rows, fmt=ops.SPLIT_FP16X2, scale_exp=9).float())


@pytest.mark.parametrize("case", dc.WIDE_CASES, ids=dc.case_id)
def test_dwconv7_layernorm_backward(case):
    from audio_motion_avatar_amd import ops

    group, name = case[0], dc.case_id(case)
    args, eps, _, g, want = dc.wide_case(case)
    x, dw_w, dw_b, ln_w, ln_b = cuda(args)
    g = g.cuda()
    rows, y = ops.dwconv7_layernorm(x, dw_w, dw_b, ln_w, ln_b, eps=eps, want_y=True)
    got = ops.dwconv7_layernorm_backward(x, y, dw_w, ln_w, eps, g)
    failed = []
    for what, a, b in zip(GRADS, got, want):
        kind = "dx" if what == "dx" else "dparam"
        err, limit = dc.rel_err(a, b), dc.bound_wide(group, kind)
        print(f"{name} {what}: {kind} error {err:.3e} (bound {limit:.1e})")
        if not err <= limit:
            failed.append(f"{what}: {err:.3e} > {limit:.1e}")
    assert not failed, f"{name}: {failed}"
    again = ops.dwconv7_layernorm_backward(x, y, dw_w, ln_w, eps, g)
    assert all(torch.equal(a, b) for a, b in zip(got, again))           # two calls bit-equal
    # under autograd: the forward is the plain call bit for bit and backward() returns the same gradients
    leaves = [t.clone().requires_grad_(True) for t in (x, dw_w, dw_b, ln_w, ln_b)]
    out = ops.dwconv7_layernorm_differentiable(*leaves, eps=eps)
    assert torch.equal(out.detach(), rows)
    out.backward(g)
    assert all(torch.equal(t.grad, a) for t, a in zip(leaves, got))


@pytest.mark.parametrize("C", (192, 512))
def test_impulses_land_where_the_tile_grid_says(C):
    """19 x 27 is 3 x 4 tiles.  One impulse in the interior tile (1, 2), one in the corner of the last, partial tile (2, 3);
    zero bias, unit norm weight: y is the flipped kernel about each impulse (cut at the border) and +0 elsewhere, exactly
    -- every other term is 0 * w.  A tile index decoded with the counts of the two axes swapped moves both."""
    from audio_motion_avatar_amd import ops

    H, W = 19, 27
    w = dc.randn(7, C, 1, 7, 7).cuda()
    zeros, ones = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    x = torch.zeros(1, H, W, C, device="cuda")
    x[0, 12, 19] = 1.0
    x[0, 18, 26] = 1.0
    rows, y = ops.dwconv7_layernorm(x, w, zeros, ones, zeros, want_y=True)
    flipped = w[:, 0].flip(1, 2).permute(1, 2, 0)                       # [7, 7, C]: y[p + dy, q + dx] = w[3 - dy, 3 - dx]
    want = torch.zeros_like(y)
    want[0, 9:16, 16:23] = flipped
    want[0, 15:19, 23:27] = flipped[:4, :4]
    assert torch.equal(y, want)
    assert not bool(torch.signbit(y[want == 0]).any())                  # +0, not -0
    # the rows are the LayerNorm of that y: zero (variance 0) away from the impulses
    quiet = (want == 0).all(-1).reshape(-1)
    assert int(quiet.sum()) == H * W - 49 - 16 and bool((rows[quiet] == 0).all())
    # dwconv7_backward_kernel decodes the same grid: an upstream gradient at those two pixels alone gives a dy that is
    # zero in every other row (LayerNorm's backward is row-wise), so dx is non-zero on the two footprints and exactly zero
    # elsewhere; its values are test_dwconv7_layernorm_backward's business
    g = torch.zeros(H * W, C, device="cuda")
    g[12 * W + 19] = dc.randn(11, C).cuda()
    g[18 * W + 26] = dc.randn(12, C).cuda()
    xr = dc.randn(13, 1, H, W, C).cuda()
    _, yr = ops.dwconv7_layernorm(xr, w, zeros, ones, zeros, want_y=True)
    dx = ops.dwconv7_layernorm_backward(xr, yr, w, ones, 1e-6, g)[0]
    touched = torch.zeros(H, W, dtype=torch.bool, device="cuda")
    touched[9:16, 16:23] = True
    touched[15:19, 23:27] = True
    assert bool(torch.isfinite(dx).all()) and bool((dx[0][~touched] == 0).all()) and bool((dx[0][touched] != 0).any(-1).all())


@pytest.mark.parametrize("C", (128, 512))
def test_planes_do_not_bleed_at_the_new_widths(C):
    """K = 2 on 19 x 27 with a NaN-poisoned neighbour plane: the clean plane is finite and, as plane 0, equals the call
    on plane 0 alone bit for bit -- the forward's y and rows, and the backward's dx."""
    from audio_motion_avatar_amd import ops

    H, W = 19, 27
    args, eps, _, g, _ = dc.wide_tensors(2, H, W, C)
    x, params = args[0].cuda(), cuda(args[1:])
    g = g.cuda().view(2, H * W, C)
    alone, y_alone = ops.dwconv7_layernorm(x[:1].contiguous(), *params, want_y=True)
    dx_alone = ops.dwconv7_layernorm_backward(x[:1].contiguous(), y_alone, params[0], params[2], eps, g[0].contiguous())[0]
    _, y_clean = ops.dwconv7_layernorm(x, *params, want_y=True)
    for poisoned in (1, 0):
        clean = 1 - poisoned
        xp = x.clone()
        xp[poisoned] = float("nan")
        rows, y = ops.dwconv7_layernorm(xp, *params, want_y=True)
        rows = rows.view(2, H * W, C)
        assert bool(torch.isfinite(rows[clean]).all()) and bool(torch.isfinite(y[clean]).all())
        assert bool(torch.isnan(rows[poisoned]).all())
        # the backward: x, y and the upstream gradient of the neighbour are all NaN
        gp = g.clone()
        gp[poisoned] = float("nan")
        dx = ops.dwconv7_layernorm_backward(xp, y, params[0], params[2], eps, gp.view(-1, C))[0]
        assert bool(torch.isfinite(dx[clean]).all()) and bool(torch.isnan(dx[poisoned]).all())
        if clean == 0:
            assert torch.equal(rows[0], alone) and torch.equal(y[0], y_alone[0]) and torch.equal(dx[0], dx_alone[0])
        else:
            assert torch.equal(y[1], y_clean[1])


# ------------------------------------------------------------------------------------------------------ bias + GELU
@pytest.mark.parametrize("rows,inner", dc.GELU_WIDE)
def test_gelu_bias_at_the_product_width_and_off_the_octet(rows, inner):
    from audio_motion_avatar_amd import ops

    (proj, bias, g), (out, d_proj, d_bias) = dc.gelu_case(rows, inner)
    proj, bias, g = cuda((proj, bias, g))
    got = ops.gelu_bias(proj, bias)
    check(dc.bound("gelu"), got, out, f"({rows}, {inner}) gelu")
    check(dc.bound("gelu"), ops.gelu_bias(proj + bias), out, f"({rows}, {inner}) gelu without a bias")
    if inner % 8:
        for split in (ops.SPLIT_BF16X3, ops.SPLIT_FP16X2):
            with pytest.raises(ops.AmavError):
                ops.gelu_bias(proj, bias, split=split)
    else:
        bf = ops.gelu_bias(proj, bias, split=ops.SPLIT_BF16X3)
        assert torch.equal(bf.float(), ops.split_operand(got).float())
        fp = ops.gelu_bias(proj, bias, split=ops.SPLIT_FP16X2, split_exp=10)
        assert torch.equal(fp.float(), ops.split_operand(got, fmt=ops.SPLIT_FP16X2, scale_exp=10).float())
    grad = ops.gelu_bias_backward(proj, bias, g)
    check(dc.bound("dgelu"), grad, d_proj, f"({rows}, {inner}) d proj")
    assert torch.equal(grad, ops.gelu_bias_backward(proj, bias, g))
    # without a bias: the kernel's g = proj + bias is the same fp32 addition
    assert torch.equal(ops.gelu_bias_backward(proj + bias, None, g), grad)
    leaves = [proj.clone().requires_grad_(True), bias.clone().requires_grad_(True)]
    y = ops.gelu_bias_differentiable(*leaves)
    assert torch.equal(y.detach(), got)
    y.backward(g)
    assert torch.equal(leaves[0].grad, grad)
    check(dc.bound("dparam"), leaves[1].grad, d_bias, f"({rows}, {inner}) d bias")
    leaf = (proj + bias).requires_grad_(True)
    ops.gelu_bias_differentiable(leaf).backward(g)
    assert torch.equal(leaf.grad, grad)


@pytest.mark.parametrize("rows,inner", dc.GELU_WIDE)
def test_gelu_bias_reads_and_writes_row_strides(rows, inner):
    """amav_gelu_bias / amav_gelu_bias_backward on buffers of row stride inner + 8 (which ops.gelu_bias does not offer): proj
    read inside a wider buffer, dproj written into one; bit-equal to the dense calls, the padding as it was."""
    from audio_motion_avatar_amd import ops

    (proj, bias, g), _ = dc.gelu_case(rows, inner)
    stride = inner + 8
    buf = torch.full((rows, stride), -7.25)
    buf[:, :inner] = proj
    buf_dev, proj, bias, g = cuda((buf, proj, bias, g))
    dense, dense_grad = ops.gelu_bias(proj, bias), ops.gelu_bias_backward(proj, bias, g)
    out = torch.full((rows, inner), -1.0, device="cuda")
    ops._call("amav_gelu_bias", rows, inner, buf_dev.data_ptr(), stride, bias.data_ptr(), out.data_ptr(), None, 0, 0)
    assert torch.equal(out, dense)
    out.fill_(-1.0)
    ops._call("amav_gelu_bias", rows, inner, buf_dev.data_ptr(), stride, None, out.data_ptr(), None, 0, 0)
    assert torch.equal(out, ops.gelu_bias(proj))
    if inner % 8 == 0:
        for fmt, e, dtype, parts in ((ops.SPLIT_BF16X3, 0, torch.bfloat16, 6), (ops.SPLIT_FP16X2, 10, torch.float16, 3)):
            out_split = torch.full((rows, parts * inner), -1.0, dtype=dtype, device="cuda")
            ops._call("amav_gelu_bias", rows, inner, buf_dev.data_ptr(), stride, bias.data_ptr(), None,
                      out_split.data_ptr(), fmt, e)
            assert torch.equal(out_split.float(), ops.gelu_bias(proj, bias, split=fmt, split_exp=e).float())
    sentinel = 1234.5
    dbuf = torch.full((rows, stride), sentinel, device="cuda")
    ops._call("amav_gelu_bias_backward", rows, inner, buf_dev.data_ptr(), stride, bias.data_ptr(), g.data_ptr(),
              dbuf.data_ptr(), stride)
    assert torch.equal(dbuf[:, :inner], dense_grad)
    assert bool((dbuf[:, inner:] == sentinel).all())
    # a dense proj into a strided dproj, and a strided proj into a dense dproj
    dbuf.fill_(sentinel)
    ops._call("amav_gelu_bias_backward", rows, inner, proj.data_ptr(), inner, bias.data_ptr(), g.data_ptr(),
              dbuf.data_ptr(), stride)
    assert torch.equal(dbuf[:, :inner], dense_grad) and bool((dbuf[:, inner:] == sentinel).all())
    dgrad = torch.full((rows, inner), sentinel, device="cuda")
    ops._call("amav_gelu_bias_backward", rows, inner, buf_dev.data_ptr(), stride, None, g.data_ptr(), dgrad.data_ptr(), inner)
    assert torch.equal(dgrad, ops.gelu_bias_backward(proj, None, g))
    assert torch.equal(buf_dev.cpu(), buf)                              # the inputs' padding too
    for bad in (inner - 4, inner + 2):                                  # below inner; no multiple of 4
        with pytest.raises(ops.AmavError):
            ops._call("amav_gelu_bias", rows, inner, buf_dev.data_ptr(), bad, None, out.data_ptr(), None, 0, 0)
        with pytest.raises(ops.AmavError):
            ops._call("amav_gelu_bias_backward", rows, inner, buf_dev.data_ptr(), stride, None, g.data_ptr(),
                      dbuf.data_ptr(), bad)


# ------------------------------------------------------------------------------- 4x4 stride-s patch gather / transpose
# (K, H, W, C, stride): the minimal plane at C4 = 1; a stride larger than the plane (one window); C = 12 (no multiple of
# 8: fp32 only) with three planes; the product's plane size
@pytest.mark.parametrize("K,H,W,C,stride", [(1, 2, 2, 4, 2), (1, 5, 6, 4, 7), (3, 9, 12, 12, 3), (2, 96, 96, 64, 3)])
def test_patch4_gather_at_the_edges_of_its_sizes(K, H, W, C, stride):
    from audio_motion_avatar_amd import ops

    x = dc.randn(90 + C + H, K, H, W, C)
    want = dc.patch4_gather(x, stride)
    Ho, Wo = ops.patch4_out_size(H, stride), ops.patch4_out_size(W, stride)
    assert want.shape == (K * Ho * Wo, 16 * C) and Ho >= 1 and Wo >= 1
    got = ops.patch4_gather(x.cuda(), stride)
    assert torch.equal(got.cpu(), want)
    assert torch.equal(got, ops.patch4_gather(x.cuda(), stride))
    if C % 8:
        for split in (ops.SPLIT_BF16X3, ops.SPLIT_FP16X2):
            with pytest.raises(ops.AmavError):
                ops.patch4_gather(x.cuda(), stride, split=split)
    else:
        assert torch.equal(ops.patch4_gather(x.cuda(), stride, split=ops.SPLIT_BF16X3).float(),
                           ops.split_operand(got).float())
        assert torch.equal(ops.patch4_gather(x.cuda(), stride, split=ops.SPLIT_FP16X2, split_exp=11).float(),
                           ops.split_operand(got, fmt=ops.SPLIT_FP16X2, scale_exp=11).float())
    # transpose: fp64 autograd of the restatement; at most four terms per pixel, added in the same (window) order
    g = dc.randn(91 + C + H, *want.shape)
    leaf = x.double().requires_grad_(True)
    (dx,) = torch.autograd.grad(dc.patch4_gather(leaf, stride), leaf, g.double())
    got_dx = ops.patch4_gather_backward(g.cuda(), x.shape, stride)
    # <= 4 fp32 terms: three additions, each rounding a partial sum of magnitude <= 4 max |g| to 2^-24 of itself
    limit = 3 * 2.0 ** -24 * 4 * float(g.abs().max()) / float(dx.abs().max())
    err = dc.rel_err(got_dx, dx)
    print(f"{(K, H, W, C, stride)}: transpose error {err:.3e} (bound {limit:.1e})")
    assert err <= limit
    if stride >= 4:                                                     # windows do not overlap: a copy
        assert torch.equal(got_dx.cpu().double(), dx)
    assert torch.equal((got_dx == 0).cpu(), dx == 0)                    # exactly 0 where no window reads
    assert torch.equal(got_dx, ops.patch4_gather_backward(g.cuda(), x.shape, stride))
    leaf = x.cuda().requires_grad_(True)
    cols = ops.patch4_gather_differentiable(leaf, stride)
    assert torch.equal(cols.detach(), got)
    cols.backward(g.cuda())
    assert torch.equal(leaf.grad, got_dx)
