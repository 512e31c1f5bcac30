"""The row kernels of the transformer step (csrc/attention_rows.hip: add_layernorm_kernel at its 4 widths x 3 output
formats, geglu_kernel, the split_operand kernels) one by one through their ops wrappers, against the CPU statements of
tests/split_model.py: fp64 for the arithmetic, bit for bit for the operand formats.  Shapes are the edges of each
kernel's launch geometry (fewer rows than a block holds, dead rows and idle lanes in the last block, a batch boundary
inside a block) at every built width.  Every comparison with a yardstick prints `rows| ...` with both figures."""
import pytest
import torch
import torch.nn.functional as F

import split_model as sm

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23  # fp32 spacing at 1.0
DIMS = [256, 512, 768, 1024]
SHAPES = [(1, 1), (1, 3), (3, 5), (2, 501)]  # rows < the 4 of a block; dead rows; batch boundaries inside a block
COMBOS = {"plain": (False, False, False), "add": (True, False, False), "add+bias": (True, True, False),
          "add+row": (True, False, True), "all": (True, True, True)}  # add, add_bias, batch_row present


def _ops():
    from audio_motion_avatar_amd import ops

    return ops


def _affine(dim, gen):
    return 1.0 + 0.5 * torch.randn(dim, generator=gen), 0.3 * torch.randn(dim, generator=gen)


def _operands(B, S, dim, gen, combo="all"):
    """(hidden, add, add_bias, batch_row) on the CPU, None where `combo` leaves one out."""
    has_add, has_bias, has_row = COMBOS[combo]
    h = torch.randn(B, S, dim, generator=gen)
    a = torch.randn(B, S, dim, generator=gen) if has_add else None
    ab = torch.randn(dim, generator=gen) if has_bias else None
    row = torch.randn(B, 1, dim, generator=gen) if has_row else None
    return h, a, ab, row


def _sum32(h, a, ab, row):
    """The kernel's association in fp32: row + ((a + a_bias) + h), a term left out where its operand is absent."""
    t = h
    if a is not None:
        t = (a + ab if ab is not None else a) + t
    if row is not None:
        t = row + t
    return t


def _dev(*ts):
    return [None if t is None else t.cuda() for t in ts]


def _run(h, a, ab, row, w, b, **kw):
    h, a, ab, row, w, b = _dev(h, a, ab, row, w, b)
    h_out, n = _ops().add_layernorm(h, a, row, w, b, add_bias=ab, **kw)
    return h_out.cpu(), n.cpu()


def _torch_ln(h_out, w, b, eps):
    return F.layer_norm(h_out.cuda(), h_out.shape[-1:], w.cuda(), b.cuda(), eps).cpu()


def _same_bits(got, want):
    return got.shape == want.shape and got.dtype == want.dtype and torch.equal(sm.bits(got), sm.bits(want))


# --------------------------------------------------------------------------------------------------- add_layernorm
@pytest.mark.parametrize("combo", list(COMBOS))
@pytest.mark.parametrize("dim", DIMS)
def test_add_layernorm_matches_fp64(dim, combo):
    """Every operand combination at every width and row geometry.  hidden_out is the fp32 sum in the kernel's
    association, bit for bit; the fp32 normalised rows are within 2e-6 of the largest |value| of fp64 LayerNorm of
    that sum (the bound rows_norm is held to: a few fp32 ulps of the normalised values from two-pass statistics)."""
    gen = torch.Generator().manual_seed(dim + len(combo))
    w, b = _affine(dim, gen)
    worst = worst_torch = 0.0
    for B, S in SHAPES:
        h, a, ab, row = _operands(B, S, dim, gen, combo)
        h_out, n = _run(h, a, ab, row, w, b)
        assert torch.equal(h_out, _sum32(h, a, ab, row)), (B, S)
        want = sm.layer_norm64(h_out, w, b, 1e-5)
        scale = float(want.abs().max())
        err = float((n.double() - want).abs().max())
        worst, worst_torch = max(worst, err / scale), max(worst_torch, float((_torch_ln(h_out, w, b, 1e-5).double() - want).abs().max()) / scale)
        assert err <= 2e-6 * scale, (B, S, err, scale)
    print(f"rows| add_layernorm fp64 dim={dim} {combo}: kernel {worst:.3e} of max|want| (bound 2e-6: {worst / 2e-6:.3f}), "
          f"torch fp32 {worst_torch:.3e} (kernel / torch {worst / worst_torch:.2f})")


@pytest.mark.parametrize("dim", DIMS)
def test_add_layernorm_large_mean_rows_against_torch(dim):
    """Rows whose mean is hundreds of standard deviations (10 + 0.03 randn, plus an `add` of 0.02 randn): cancellation
    in the variance.  The kernel's error against fp64 is at most 4x that of torch's fp32 F.layer_norm on the device,
    plus 1e-6 of the largest output; a one-pass E[x^2] - mean^2 variance exceeds that 140-fold."""
    gen = torch.Generator().manual_seed(100 + dim)
    w, b = _affine(dim, gen)
    B, S = 2, 501
    h = 10.0 + 0.03 * torch.randn(B, S, dim, generator=gen)
    a = 0.02 * torch.randn(B, S, dim, generator=gen)
    h_out, n = _run(h, a, None, None, w, b)
    assert torch.equal(h_out, a + h)
    want = sm.layer_norm64(h_out, w, b, 1e-5)
    err = float((n.double() - want).abs().max())
    err_torch = float((_torch_ln(h_out, w, b, 1e-5).double() - want).abs().max())
    bound = 4 * err_torch + 1e-6 * float(want.abs().max())
    print(f"rows| add_layernorm large mean dim={dim}: kernel {err:.3e}, torch fp32 {err_torch:.3e} "
          f"(kernel / torch {err / err_torch:.2f}, of the bound {err / bound:.3f})")
    assert err <= bound, (err, err_torch)


@pytest.mark.parametrize("fmt", ["fp32", "bf16x3", "fp16x2"])
@pytest.mark.parametrize("dim", DIMS)
def test_add_layernorm_constant_rows_equal_the_bias(dim, fmt):
    """Constant rows whose sums are exact in fp32 (sum * fl(1 / dim) returns the value at all four widths): the
    deviations are exactly 0, so the normalised row is `bias` bit for bit -- in all three output formats."""
    ops = _ops()
    gen = torch.Generator().manual_seed(200 + dim)
    w, b = _affine(dim, gen)
    values = torch.tensor([0.75, -3.0, 5.5, 0.0, 1024.0, -0.125])
    B, S = 2, 501
    h = values[torch.arange(B * S) % len(values)].view(B, S, 1).expand(B, S, dim).contiguous()
    assert all(float(torch.tensor(v * dim, dtype=torch.float32) * torch.tensor(1.0 / dim, dtype=torch.float32)) == v
               for v in values.tolist())
    kw = {"fp32": {}, "bf16x3": {"split": ops.SPLIT_BF16X3}, "fp16x2": {"split": ops.SPLIT_FP16X2, "split_exp": 7}}[fmt]
    h_out, n = _run(h, None, None, None, w, b, **kw)
    assert torch.equal(h_out, h)
    rows = b.expand(B * S, dim)
    if fmt == "fp32":
        assert torch.equal(n, rows.view(B, S, dim))
    else:
        assert _same_bits(n, sm.operand(rows, sm.BF16X3 if fmt == "bf16x3" else sm.FP16X2, e=7))


@pytest.mark.parametrize("eps", [1e-6, 1e-5, 1e-3])
@pytest.mark.parametrize("dim", DIMS)
def test_add_layernorm_spike_rows_and_eps(dim, eps):
    """One channel of 300 among zeros: the normalised row reaches the |z| = sqrt(dim - 1) that the fp16 pre-scales are
    derived from.  Rows of scale 1e-4: the variance (1e-8) is below every eps, which then sets the result.  Both within
    2e-6 of the largest |value| of fp64, as unit rows."""
    gen = torch.Generator().manual_seed(300 + dim)
    w, b = _affine(dim, gen)
    B, S = 3, 5
    spike = torch.zeros(B, S, dim)
    at = torch.randint(0, dim, (B * S,), generator=gen)
    at[0], at[1] = 0, dim - 1
    spike.view(-1, dim)[torch.arange(B * S), at] = 300.0
    small = 1e-4 * torch.randn(B, S, dim, generator=gen)
    for name, h in (("spike", spike), ("1e-4", small)):
        h_out, n = _run(h, None, None, None, w, b, eps=eps)
        assert torch.equal(h_out, h)
        want = sm.layer_norm64(h, w, b, eps)
        scale, err = float(want.abs().max()), float((n.double() - want).abs().max())
        err_torch = float((_torch_ln(h, w, b, eps).double() - want).abs().max())
        print(f"rows| add_layernorm {name} dim={dim} eps={eps:g}: kernel {err / scale:.3e} of max|want| {scale:.1f} "
              f"(bound 2e-6: {err / scale / 2e-6:.3f}), torch fp32 {err_torch / scale:.3e}")
        assert err <= 2e-6 * scale, (name, err, scale)
    z = (sm.layer_norm64(spike, torch.ones(dim), torch.zeros(dim), 1e-6)).abs().max()
    assert abs(float(z) - (dim - 1) ** 0.5) < 1e-3


@pytest.mark.parametrize("dim", DIMS)
def test_add_layernorm_split_outputs_are_the_model_of_the_fp32_rows(dim):
    """The 8 split instantiations: with split = bf16 x 3, and fp16 x 2 at pre-scales 2^-3, 2^0, 2^7, the operand is bit
    for bit split_model's activation layout of the fp32 rows the same call writes without `split` (those rows are held
    to fp64 above).  All three addends present; every row geometry."""
    ops = _ops()
    gen = torch.Generator().manual_seed(400 + dim)
    w, b = _affine(dim, gen)
    for B, S in SHAPES:
        h, a, ab, row = _operands(B, S, dim, gen)
        h_out, n = _run(h, a, ab, row, w, b)
        rows = n.view(B * S, dim)
        for kw, want in (({"split": ops.SPLIT_BF16X3}, sm.operand(rows, sm.BF16X3)),
                         *(({"split": ops.SPLIT_FP16X2, "split_exp": e}, sm.operand(rows, sm.FP16X2, e=e)) for e in (-3, 0, 7))):
            h_split, got = _run(h, a, ab, row, w, b, **kw)
            assert torch.equal(h_split, h_out), (B, S, kw)
            assert torch.isfinite(want.float()).all()
            assert _same_bits(got, want), (B, S, kw, int((sm.bits(got) != sm.bits(want)).sum()))


# ----------------------------------------------------------------------------------------------------------- geglu
def _geglu_inputs(rows, inner, gen):
    """proj [rows, 2 * inner]: hidden N(0, 3) with every seventh value x 100 and every eleventh exactly 0; gates: two in
    three from a shuffled list of a linspace over [-12, 12] (erf saturates at both ends), +-0 and +-1e-40 (an fp32
    subnormal), the rest N(0, 2)."""
    n = rows * inner
    i = torch.arange(n)
    hidden = 3.0 * torch.randn(n, generator=gen)
    hidden[i % 7 == 3] *= 100.0
    hidden[i % 11 == 5] = 0.0
    special = torch.cat([torch.linspace(-12, 12, 251), torch.tensor([0.0, -0.0, 1e-40, -1e-40])])
    special = special[torch.randperm(len(special), generator=gen)]
    gate = torch.where(i % 3 != 0, special[i % len(special)], 2.0 * torch.randn(n, generator=gen))
    return torch.cat([hidden.view(rows, inner), gate.view(rows, inner)], dim=1)


def _geglu_bound(h, g, biased):
    """Per element 4 ulps of |h| (|g| + 1): the roundings of erff and of gelu's and the gate's products, each a fraction
    of an ulp of that magnitude (|gelu(g)| <= |g|).  With a bias, one rounding of h + b_h and one of g + b_g on top:
    2^-24 |h| |gelu(g)| + |h| sup|gelu'| 2^-24 |g| <= 1.07 ulp |h| |g|  (sup|gelu'| = 1.13)."""
    return 4 * ULP * h.abs() * (g.abs() + 1.0) + (1.07 * ULP * h.abs() * g.abs() if biased else 0.0)


@pytest.mark.parametrize("rows", [1, 37, 257])
@pytest.mark.parametrize("inner", [4, 12, 2048, 4096])
def test_geglu_matches_fp64(inner, rows):
    """h * gelu(g), exact-erf, without and with the projection's bias, against fp64 of the same (biased) operands; quad
    counts from 1 to 263 168, most of which leave the last block partly idle.  Finite everywhere: a saturated gate
    gives -x * 0, not NaN.  torch's fp32 F.gelu uses 0.60 of the bound, the tanh approximation 270x it."""
    ops = _ops()
    gen = torch.Generator().manual_seed(inner + rows)
    proj = _geglu_inputs(rows, inner, gen)
    bias = torch.randn(2 * inner, generator=gen)
    for b in (None, bias):
        got = ops.geglu(proj.cuda(), bias=None if b is None else b.cuda()).cpu()
        assert got.shape == (rows, inner) and torch.isfinite(got).all()
        want, h, g = sm.geglu64(proj, b)
        tol = _geglu_bound(h, g, b is not None)
        used = float(((got.double() - want).abs() / tol.clamp_min(1e-300)).max())
        p32 = (proj if b is None else proj + b).cuda()
        t32 = (p32[:, :inner] * F.gelu(p32[:, inner:])).cpu()
        used_torch = float(((t32.double() - want).abs() / tol.clamp_min(1e-300)).max())
        print(f"rows| geglu inner={inner} rows={rows} bias={b is not None}: kernel {used:.3f} of the bound, "
              f"torch fp32 {used_torch:.3f}")
        assert ((got.double() - want).abs() <= tol).all(), used
    zero = proj[:, :inner] == 0   # exact zeros of the hidden half stay zeros, whatever the gate
    assert zero.any() == (rows * inner >= 6) and (ops.geglu(proj.cuda()).cpu()[zero] == 0).all()


def _fit_fp16(proj, bias, inner, e):
    """proj and bias with the hidden half scaled by a power of two (exact) so that |h gelu(g)| 2^e <= 32768."""
    top = float(sm.geglu64(proj, bias)[0].abs().max()) * 2.0 ** e * 1.001
    s = 2.0 ** min(0, int(torch.floor(torch.log2(torch.tensor(sm.FP16_TARGET / top)))))
    proj, bias = proj.clone(), bias.clone()
    proj[:, :inner] *= s
    bias[:inner] *= s
    return proj, bias


@pytest.mark.parametrize("e", [-2, 0, 9])
@pytest.mark.parametrize("inner", [4, 12, 2048])
def test_geglu_split_output_is_the_model_of_the_fp32_result(inner, e):
    """split_exp: the operand is bit for bit split_model's fp16 x 2 activation layout of the fp32 result of the same
    call, without and with the bias -- at inner 4 and 12, where a row of the operand is shorter than a wave, too.  The gates
    saturate, so many results are -0: their zero residual is +0, as x - x is (geglu_kernel once wrote -0 there for two
    elements of each quad)."""
    ops = _ops()
    gen = torch.Generator().manual_seed(10 * inner + e)
    rows = 37
    proj, bias = _fit_fp16(_geglu_inputs(rows, inner, gen), torch.randn(2 * inner, generator=gen), inner, e)
    for b in (None, bias):
        bd = None if b is None else b.cuda()
        y = ops.geglu(proj.cuda(), bias=bd).cpu()
        want = sm.operand(y, sm.FP16X2, e=e)
        assert torch.isfinite(want.float()).all() and float(y.abs().max()) * 2.0 ** e > 64.0
        got = ops.geglu(proj.cuda(), bias=bd, split_exp=e).cpu()
        assert _same_bits(got, want), int((sm.bits(got) != sm.bits(want)).sum())


def test_geglu_reads_a_row_stride():
    """amav_geglu on a padded buffer (row stride 2 * inner + 8, which ops.geglu does not offer) equals the contiguous
    call bit for bit, fp32 and split, and leaves the padding as it was."""
    ops = _ops()
    gen = torch.Generator().manual_seed(21)
    rows, inner, e = 37, 12, 3
    proj, bias = _fit_fp16(_geglu_inputs(rows, inner, gen), torch.randn(2 * inner, generator=gen), inner, e)
    stride = 2 * inner + 8
    buf = torch.full((rows, stride), -7.25)
    buf[:, :2 * inner] = proj
    buf_dev, bias_dev = buf.cuda(), bias.cuda()
    out = torch.full((rows, inner), -1.0).cuda()
    out_split = torch.full((rows, 3 * inner), -1.0, dtype=torch.float16).cuda()
    ops._call("amav_geglu", rows, inner, buf_dev.data_ptr(), stride, bias_dev.data_ptr(), out.data_ptr(), None, 0)
    ops._call("amav_geglu", rows, inner, buf_dev.data_ptr(), stride, bias_dev.data_ptr(), None, out_split.data_ptr(), e)
    assert torch.equal(out, ops.geglu(proj.cuda(), bias=bias_dev))
    assert _same_bits(out_split.cpu(), ops.geglu(proj.cuda(), bias=bias_dev, split_exp=e).cpu())
    assert torch.equal(buf_dev.cpu(), buf)
    with pytest.raises(ops.AmavError):
        ops._call("amav_geglu", rows, inner, buf_dev.data_ptr(), 2 * inner - 4, None, out.data_ptr(), None, 0)


# --------------------------------------------------------------------------------------------------- split_operand
def _strided(x):
    """x on the device as a view of a wider buffer (row stride k + 24, first column 8: still 16-byte aligned)."""
    rows, k = x.shape
    buf = torch.full((rows, k + 24), float("nan")).cuda()
    buf[:, 8:8 + k] = x.cuda()
    return buf[:, 8:8 + k]


def _subnormal_report(got, want):
    """Where the device's operand differs from the model's, and whether only at parts that are fp16 / bf16 subnormals."""
    diff = sm.bits(got) != sm.bits(want)
    tiny = torch.finfo(want.dtype).tiny
    sub = (want != 0) & (want.float().abs() < tiny)
    return f"{int(diff.sum())} differ, {int((diff & sub).sum())} of them where the model's part is subnormal"


@pytest.mark.parametrize("rows,k", [(1, 8), (3, 24), (37, 520)])
@pytest.mark.parametrize("fmt,e", [("bf16x3", 0)] + [("fp16x2", e) for e in (-126, -3, 0, 10, 126)])
def test_split_operand_is_the_cpu_model_on_edge_values(fmt, e, rows, k):
    """Both formats, both roles, contiguous and strided, over split_model.edge_values(): signed zeros, parts and
    residuals that are fp16 subnormals, rounding ties of both formats, the fp16 target bound, an fp32 subnormal, 13
    decades of magnitudes -- bit for bit what IEEE conversions on the CPU make (round to nearest even, subnormals
    kept).  k = 520 is 65 octets a row: a block's 256 octets straddle rows."""
    ops = _ops()
    x = sm.edge_matrix(rows, k, e)
    f_model, f_ops = (sm.BF16X3, ops.SPLIT_BF16X3) if fmt == "bf16x3" else (sm.FP16X2, ops.SPLIT_FP16X2)
    for weights in (False, True):
        want = sm.operand(x, f_model, weights=weights, e=e)
        assert torch.isfinite(want.float()).all()
        for src in (x.cuda(), _strided(x)):
            got = ops.split_operand(src, weights=weights, fmt=f_ops, scale_exp=e).cpu()
            assert _same_bits(got, want), (weights, src.stride(), _subnormal_report(got, want))
    # -0 keeps its sign in the leading part (column 1 of the edge list; the activations' leading part is the last block)
    lead = ops.split_operand(x.cuda(), fmt=f_ops, scale_exp=e).cpu()[:, -k:]
    assert sm.bits(lead)[0, 1].item() == -32768 and sm.bits(lead)[0, 0].item() == 0
