"""The backwards of the transformer step's row kernels (csrc/attention_rows_backward.hip) through
their ops wrappers: amav_rows_colsum, amav_geglu_backward, amav_add_layernorm_backward and the two autograd Functions
built on them.

The reference is fp64 autograd on the CPU of the reference's formulas (F.layer_norm, h * F.gelu(g)); the yardstick
e_torch is torch's fp32 autograd of the same formulas on the device against that fp64 (never the code under test).  Every
gradient element is held to 4 e_torch + 2^-22 max|ref|, the form of tests/attention_cases.py; a gradient that is a sum over
n rows additionally gets the derivable (n - 1) 2^-24 sum|terms| of its column.  Each family prints `rowsbwd| ...` with its
worst error / bound and error / e_torch."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DIMS = [256, 512, 768, 1024]
COMBOS = {"plain": (False, False, False), "add": (True, False, False), "add+bias": (True, True, False),
          "add+row": (True, False, True), "all": (True, True, True)}  # add, add_bias, batch_row present
SHAPES = [(1, 1), (1, 37), (3, 37), (2, 257)]
UPSTREAMS = {"both": (True, True), "norm": (False, True), "h": (True, False)}  # upstream on (h, norm)
FLOOR = 2.0 ** -22
EPS24 = 2.0 ** -24


def _ops():
    from audio_motion_avatar_amd import ops

    return ops


class Worst:
    """Largest error / bound and error / e_torch of a family, printed once."""

    def __init__(self, family):
        self.family, self.of_bound, self.of_torch = family, 0.0, 0.0

    def check(self, name, got, ref64, torch32, colsum_bound=None):
        got, torch32 = got.detach().cpu().double(), torch32.detach().cpu().double()
        assert got.shape == ref64.shape, (name, got.shape, ref64.shape)
        assert bool(torch.isfinite(got).all()), f"{name}: non-finite"
        e_torch = float((torch32 - ref64).abs().max())
        bound = 4.0 * e_torch + FLOOR * float(ref64.abs().max())
        bound = bound + colsum_bound if colsum_bound is not None else torch.full_like(ref64, bound)
        err = (got - ref64).abs()
        self.of_bound = max(self.of_bound, float((err / bound.clamp_min(1e-300)).max()))
        if e_torch > 0:
            self.of_torch = max(self.of_torch, float(err.max()) / e_torch)
        assert bool((err <= bound).all()), (f"{self.family} {name}: error {float(err.max()):.3e}, e_torch {e_torch:.3e}, "
                                            f"worst error / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")

    def report(self):
        print(f"rowsbwd| {self.family}: worst error / bound {self.of_bound:.3f}, worst error / e_torch {self.of_torch:.3f}")


# ------------------------------------------------------------------------------------------------------ column sum
ROWS_PER_GROUP = [1, 15, 16, 17, 63, 64, 65, 1000]  # below, at and above the chunk of 16 rows and its multiples


def test_chunk_size_is_the_documented_one():
    assert _ops().ROWS_CHUNK == 16


@pytest.mark.parametrize("cols", [8, 256, 4096])
@pytest.mark.parametrize("groups", [1, 3])
def test_colsum_is_exact_on_integers_and_bounded_on_random_rows(groups, cols):
    ops = _ops()
    worst = 0.0
    for per_group in ROWS_PER_GROUP:
        gen = torch.Generator().manual_seed(1000 * groups + cols + per_group)
        rows = groups * per_group
        ints = torch.randint(-8, 9, (rows, cols), generator=gen).float()
        got = ops.rows_colsum(ints.cuda(), per_group).cpu()
        assert got.shape == (groups, cols)
        assert torch.equal(got, ints.view(groups, per_group, cols).sum(1)), (per_group, "integer sums must be exact")
        x = torch.randn(rows, cols, generator=gen) * torch.exp(2.0 * torch.randn(rows, 1, generator=gen))
        xd = x.cuda()
        got = ops.rows_colsum(xd, per_group)
        assert torch.equal(got, ops.rows_colsum(xd, per_group)), "two calls differ"
        for g in range(groups):  # a batch of groups equals the groups one by one, bit for bit
            assert torch.equal(got[g], ops.rows_colsum(xd[g * per_group:(g + 1) * per_group])[0]), (per_group, g)
        x64 = x.double().view(groups, per_group, cols)
        bound = (per_group - 1) * EPS24 * x64.abs().sum(1)
        err = (got.cpu().double() - x64.sum(1)).abs()
        assert bool((err <= bound).all()), (per_group, float((err / bound.clamp_min(1e-300)).max()))
        if per_group > 1:
            worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
    print(f"rowsbwd| colsum groups={groups} cols={cols}: worst error / ((n - 1) 2^-24 sum|x|) {worst:.3f}")


def test_colsum_reads_a_row_stride_and_refuses_bad_shapes():
    ops = _ops()
    gen = torch.Generator().manual_seed(5)
    wide = torch.randint(-8, 9, (130, 72), generator=gen).float().cuda()
    view = wide[:, 8:40]  # row stride 72, 32 columns, 16-byte aligned start
    assert torch.equal(ops.rows_colsum(view, 65), view.contiguous().view(2, 65, 32).sum(1))
    assert torch.equal(ops.rows_colsum(view, 65), ops.rows_colsum(view.contiguous(), 65))
    with pytest.raises(ops.AmavError):
        ops.rows_colsum(wide, 7)            # rows_per_group must divide the rows
    with pytest.raises(ops.AmavError):
        ops.rows_colsum(wide[:, :6])        # cols % 4
    with pytest.raises(ops.AmavError):
        ops.rows_colsum(wide.cpu())
    with pytest.raises(ops.AmavError):
        ops.rows_colsum(wide.double())


# ---------------------------------------------------------------------------------------------------- GEGLU backward
def _geglu_inputs(rows, inner, gen):
    """proj [rows, 2 * inner]: hidden N(0, 3) with every seventh value x 100 and every eleventh exactly 0; gates: two in
    three from a shuffled list holding 0, +-0.0, +-1e-4, the saturated +-40 and a linspace over [-12, 12], the rest
    N(0, 2)."""
    n = rows * inner
    i = torch.arange(n)
    hidden = 3.0 * torch.randn(n, generator=gen)
    hidden[i % 7 == 3] *= 100.0
    hidden[i % 11 == 5] = 0.0
    special = torch.cat([torch.linspace(-12, 12, 61), torch.tensor([0.0, -0.0, 1e-4, -1e-4, 40.0, -40.0])])
    special = special[torch.randperm(len(special), generator=gen)]
    gate = torch.where(i % 3 != 0, special[i % len(special)], 2.0 * torch.randn(n, generator=gen))
    return torch.cat([hidden.view(rows, inner), gate.view(rows, inner)], dim=1)


def _geglu_grads(proj, bias, dout, dtype, device):
    p = proj.to(device=device, dtype=dtype).requires_grad_()
    b = None if bias is None else bias.to(device=device, dtype=dtype).requires_grad_()
    x = p if b is None else p + b
    inner = p.shape[-1] // 2
    (x[:, :inner] * F.gelu(x[:, inner:])).backward(dout.to(device=device, dtype=dtype))
    return p.grad.cpu(), None if b is None else b.grad.cpu()


@pytest.mark.parametrize("rows", [1, 37, 257])
@pytest.mark.parametrize("inner", [4, 12, 2048])
def test_geglu_backward_matches_fp64(inner, rows):
    ops = _ops()
    gen = torch.Generator().manual_seed(7 * inner + rows)
    proj = _geglu_inputs(rows, inner, gen)
    gates = proj[:, inner:]
    if rows * inner >= 200:
        assert all(bool((gates == v).any()) for v in (0.0, 1e-4, -1e-4, 40.0, -40.0)) and bool(torch.signbit(gates[gates == 0]).any())
    bias_cpu = 0.5 * torch.randn(2 * inner, generator=gen)
    dout = torch.randn(rows, inner, generator=gen)
    worst = Worst(f"geglu backward inner={inner} rows={rows}")
    for bias in (None, bias_cpu):
        ref_p, ref_b = _geglu_grads(proj, bias, dout, torch.float64, "cpu")
        t32_p, t32_b = _geglu_grads(proj, bias, dout, torch.float32, "cuda")
        p = proj.cuda().requires_grad_()
        b = None if bias is None else bias.cuda().requires_grad_()
        out = ops.geglu_differentiable(p, b)
        assert torch.equal(out, ops.geglu(proj.cuda(), bias=None if bias is None else bias.cuda()))  # the forward, bit for bit
        out.backward(dout.cuda())
        worst.check("dproj", p.grad, ref_p, t32_p)
        direct = ops.geglu_backward(proj.cuda(), None if bias is None else bias.cuda(), dout.cuda())
        assert torch.equal(direct, p.grad) and torch.equal(direct, ops.geglu_backward(
            proj.cuda(), None if bias is None else bias.cuda(), dout.cuda()))
        if bias is not None:
            worst.check("dbias", b.grad, ref_b, t32_b, colsum_bound=(rows - 1) * EPS24 * ref_p.abs().sum(0))
        else:  # saturated gates: exp(-800) = 0 and Phi = 0 or 1 exactly
            got, h = direct.cpu(), proj[:, :inner]
            assert bool((got[:, inner:][gates == -40.0] == 0).all()) and bool((got[:, :inner][gates == -40.0] == 0).all())
            assert torch.equal(got[:, inner:][gates == 40.0], (dout * h)[gates == 40.0])
            assert torch.equal(got[:, :inner][gates == 40.0], (dout * 40.0)[gates == 40.0])
        zeros = ops.geglu_backward(proj.cuda(), None if bias is None else bias.cuda(), torch.zeros_like(dout).cuda())
        assert bool((zeros == 0).all())
    worst.report()


def test_geglu_differentiable_gives_gradients_only_where_needed_and_refuses_other_tensors():
    ops = _ops()
    proj = torch.randn(5, 16).cuda()
    bias = torch.randn(16).cuda().requires_grad_()
    ops.geglu_differentiable(proj, bias).sum().backward()  # proj needs none
    assert proj.grad is None and bias.grad is not None
    with pytest.raises(ops.AmavError):
        ops.geglu_differentiable(torch.randn(5, 16))
    with pytest.raises(ops.AmavError):
        ops.geglu_differentiable(proj.double())


# --------------------------------------------------------------------------------------------- add + LayerNorm backward
NAMES = ("hidden", "add", "add_bias", "batch_row", "weight", "bias")


def _operands(B, S, dim, gen, combo, rows=None):
    has_add, has_bias, has_row = COMBOS[combo]
    h = torch.randn(B, S, dim, generator=gen) if rows is None else rows
    a = 0.5 * torch.randn(B, S, dim, generator=gen) * float(h.std()) if has_add else None
    ab = 0.5 * torch.randn(dim, generator=gen) * float(h.std()) if has_bias else None
    row = 0.5 * torch.randn(B, 1, dim, generator=gen) * float(h.std()) if has_row else None
    w = 1.0 + 0.5 * torch.randn(dim, generator=gen)
    b = 0.3 * torch.randn(dim, generator=gen)
    return dict(hidden=h, add=a, add_bias=ab, batch_row=row, weight=w, bias=b)


def _leaves(operands, dtype, device):
    return {k: None if v is None else v.to(device=device, dtype=dtype).requires_grad_() for k, v in operands.items()}


def _backward(outs, ups, leaves):
    pairs = [(o, u.to(device=o.device, dtype=o.dtype)) for o, u in zip(outs, ups) if u is not None]
    torch.autograd.backward([o for o, _ in pairs], [u for _, u in pairs])
    return {k: (None if v is None else (torch.zeros_like(v) if v.grad is None else v.grad).cpu()) for k, v in leaves.items()}


def _formula_grads(operands, eps, ups, dtype, device):
    """Autograd of the reference's formulas: the two adds, then F.layer_norm.  -> (grads by name, the summed rows)."""
    x = _leaves(operands, dtype, device)
    t = x["hidden"]
    if x["add"] is not None:
        t = (x["add"] + x["add_bias"] if x["add_bias"] is not None else x["add"]) + t
    if x["batch_row"] is not None:
        t = x["batch_row"] + t
    t = t + 0.0  # a non-leaf even with no operand to add
    n = F.layer_norm(t, t.shape[-1:], x["weight"], x["bias"], eps)
    return _backward((t, n), ups, x), t.detach().cpu()


def _kernel_grads(operands, eps, ups):
    x = _leaves(operands, torch.float32, "cuda")
    outs = _ops().add_layernorm_differentiable(x["hidden"], x["add"], x["batch_row"], x["weight"], x["bias"], eps,
                                               add_bias=x["add_bias"])
    values = tuple(o.detach().clone() for o in outs)
    return _backward(outs, ups, x), values


def _colsum_bounds(operands, eps, ups, ref, t64):
    """(n - 1) 2^-24 sum|terms| per column for the four gradients that are sums over rows."""
    B, S, dim = t64.shape
    xhat = (t64 - t64.mean(-1, keepdim=True)) / torch.sqrt(t64.var(-1, unbiased=False, keepdim=True) + eps)
    up_n = torch.zeros_like(t64) if ups[1] is None else ups[1].double()
    dh = ref["hidden"].double().abs()
    return {"weight": (B * S - 1) * EPS24 * (up_n * xhat).abs().sum((0, 1)),
            "bias": (B * S - 1) * EPS24 * up_n.abs().sum((0, 1)),
            "batch_row": (S - 1) * EPS24 * dh.sum(1, keepdim=True),
            "add_bias": (B * S - 1) * EPS24 * dh.sum((0, 1))}


def _check_case(worst, operands, eps, ups, label):
    ref, t64 = _formula_grads(operands, eps, ups, torch.float64, "cpu")
    t32, _ = _formula_grads(operands, eps, ups, torch.float32, "cuda")
    got, values = _kernel_grads(operands, eps, ups)
    again, _ = _kernel_grads(operands, eps, ups)
    sums = _colsum_bounds(operands, eps, ups, ref, t64)
    for name in NAMES:
        if operands[name] is None:
            continue
        worst.check(f"{label} d {name}", got[name], ref[name], t32[name], colsum_bound=sums.get(name))
        assert torch.equal(got[name], again[name]), f"{label} d {name}: two calls differ"
    if ups[1] is None:  # no upstream on norm: dweight and dbias are +0
        for name in ("weight", "bias"):
            assert bool((got[name] == 0).all()) and not bool(torch.signbit(got[name]).any())
    return got, values


@pytest.mark.parametrize("combo", list(COMBOS))
@pytest.mark.parametrize("dim", DIMS)
def test_add_layernorm_backward_matches_fp64(dim, combo):
    ops = _ops()
    worst = Worst(f"add_layernorm backward dim={dim} {combo}")
    for B, S in SHAPES:
        gen = torch.Generator().manual_seed(dim + 31 * B + S)
        operands = _operands(B, S, dim, gen, combo)
        up_h, up_n = torch.randn(B, S, dim, generator=gen), torch.randn(B, S, dim, generator=gen)
        for mode, (on_h, on_n) in UPSTREAMS.items():
            ups = (up_h if on_h else None, up_n if on_n else None)
            got, values = _check_case(worst, operands, 1e-5, ups, f"B={B} S={S} upstream={mode}")
            if mode != "both":
                continue
            dev = {k: None if v is None else v.cuda() for k, v in operands.items()}
            h_plain, n_plain = ops.add_layernorm(dev["hidden"], dev["add"], dev["batch_row"], dev["weight"], dev["bias"],
                                                 1e-5, add_bias=dev["add_bias"])
            assert torch.equal(values[0], h_plain) and torch.equal(values[1], n_plain)  # the forward, bit for bit
            if B == 2:  # a batch of two equals two single calls, for everything but the sums over the batch
                for i in range(2):
                    one = {k: (v[i:i + 1] if v is not None and v.dim() == 3 else v) for k, v in operands.items()}
                    single, _ = _kernel_grads(one, 1e-5, (up_h[i:i + 1], up_n[i:i + 1]))
                    for name in ("hidden", "add", "batch_row"):
                        if operands[name] is not None:
                            assert torch.equal(single[name][0], got[name][i]), (name, i)
    worst.report()


@pytest.mark.parametrize("dim", DIMS)
def test_add_layernorm_backward_on_large_mean_and_small_rows(dim):
    worst = Worst(f"add_layernorm backward dim={dim} row families")
    B, S = 3, 37
    gen = torch.Generator().manual_seed(dim)
    up = (torch.randn(B, S, dim, generator=gen), torch.randn(B, S, dim, generator=gen))
    families = [("unit", torch.randn(B, S, dim, generator=gen), 1e-5),
                ("mean 10", 10.0 + 0.03 * torch.randn(B, S, dim, generator=gen), 1e-5)]
    families += [(f"scale 1e-4 eps={eps:g}", 1e-4 * torch.randn(B, S, dim, generator=gen), eps) for eps in (1e-6, 1e-5, 1e-3)]
    for name, rows, eps in families:
        _check_case(worst, _operands(B, S, dim, gen, "all", rows=rows), eps, up, name)
        _check_case(worst, _operands(B, S, dim, gen, "plain", rows=rows), eps, up, name + " plain")
    worst.report()


@pytest.mark.parametrize("dim", DIMS)
def test_add_layernorm_backward_closed_forms(dim):
    """fp32-sense spot checks against hand-derived gradients.
    One-hot row x = e_k, weight 1, upstream e_k on norm: with r = rstd = (var + eps)^-1/2, var = (N - 1) / N^2,
    xhat_k = (1 - 1/N) r and xhat_j = -r / N:  dh_k = r (1 - 1/N - xhat_k^2 / N),  dh_j = r (-1/N - xhat_j xhat_k / N).
    Every term is at most r in magnitude and the kernel rounds a dozen times on the way: 2^-20 r.
    Constant rows with dnorm = 1 / weight (weights powers of two, so t = dnorm * weight = 1 exactly): xhat = 0 and
    t - mean(t) = 0, the LayerNorm part vanishes and d hidden = d hidden_out exactly, whatever rstd = eps^-1/2 is."""
    ops = _ops()
    N, k, eps = dim, 5, 1e-3
    x = torch.zeros(1, 2, N)
    x[0, :, k] = 1.0
    up_n = torch.zeros(1, 2, N)
    up_n[0, :, k] = 1.0
    ones = torch.ones(N).cuda()
    dh, dw, db = ops.add_layernorm_backward(x.cuda(), ones, eps, up_n.cuda(), None)
    r = (float(N - 1) / N ** 2 + eps) ** -0.5
    xk, xj = (1 - 1 / N) * r, -r / N
    want = torch.full((N,), r * (-1 / N - xj * xk / N), dtype=torch.float64)
    want[k] = r * (1 - 1 / N - xk * xk / N)
    assert float((dh.cpu().double()[0] - want).abs().max()) <= 2.0 ** -20 * r
    want_w = torch.zeros(N, dtype=torch.float64)
    want_w[k] = 2 * xk
    assert float((dw.cpu().double() - want_w).abs().max()) <= 2.0 ** -20 * r and torch.equal(db.cpu(), 2 * up_n[0, 0])

    gen = torch.Generator().manual_seed(dim)
    w = 2.0 ** torch.randint(-2, 3, (N,), generator=gen).float()
    const = torch.tensor([2.5, -0.75, 40.0]).view(1, 3, 1).expand(1, 3, N).contiguous()
    up_h = torch.randn(1, 3, N, generator=gen)
    dh, _, _ = ops.add_layernorm_backward(const.cuda(), w.cuda(), 1e-5, (1.0 / w).expand(1, 3, N).contiguous().cuda(),
                                          up_h.cuda())
    assert torch.equal(dh.cpu(), up_h)


def test_add_layernorm_differentiable_refuses_other_tensors():
    ops = _ops()
    w = torch.ones(256)
    with pytest.raises(ops.AmavError):
        ops.add_layernorm_differentiable(torch.randn(1, 2, 256), None, None, w, w)
    with pytest.raises(ops.AmavError):
        ops.add_layernorm_differentiable(torch.randn(1, 2, 256).cuda().double(), None, None, w.cuda(), w.cuda())
    with pytest.raises(ops.AmavError):
        ops.add_layernorm_differentiable(torch.randn(1, 2, 128).cuda(), None, None, torch.ones(128).cuda(),
                                         torch.ones(128).cuda())  # width 128 is not built
