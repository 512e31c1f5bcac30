"""Train-mode BatchNorm of the point refiner (csrc/cloud_norm.hip): batch statistics, the
backward through them, and the pooling composition, against the same torch formula in fp64 on the CPU.

Bound per tensor, the project's yardstick (tests/test_point_refiner_backward_gpu.py):
    max|got - ref64| <= max(4 * err32, 2e-5 * max|ref64|),   err32 = max|ref32 - ref64| of the formula run in fp32.
Every comparison prints err, err32 and max|ref64| before it asserts."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

EPS = 1e-3
ROWS = (2, 15, 16, 17, 1000, 4099)   # one chunk of 64 rows, ragged chunks, 65 chunks (stage 2 wraps past its 64 lanes)
WIDTHS = (32, 260, 512)


def _ops():
    from audio_motion_avatar_amd import ops

    return ops


def _check(name, got, r64, r32):
    r64 = r64.double()
    err = float((got.detach().cpu().double() - r64).abs().max())
    err32 = float((r32.double() - r64).abs().max())
    big = float(r64.abs().max())
    bound = max(4 * err32, 2e-5 * big)
    print(f"{name}: err {err:.3e}  err32 {err32:.3e}  max|ref64| {big:.3e}  err/bound {err / max(bound, 1e-300):.3f}")
    assert err <= bound, (name, err, err32, big)


def _stats_case(name, x):
    ops = _ops()
    mean, var = ops.bn_batch_stats(x.cuda())
    v64, m64 = torch.var_mean(x.double(), 0, unbiased=False)
    v32, m32 = torch.var_mean(x, 0, unbiased=False)
    _check(name + " mean", mean, m64, m32)
    _check(name + " var", var, v64, v32)
    assert bool((var >= 0).all())
    again = ops.bn_batch_stats(x.cuda())
    assert torch.equal(again[0], mean) and torch.equal(again[1], var)


@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("rows", ROWS)
def test_batch_stats_match_fp64(rows, C):
    gen = torch.Generator().manual_seed(rows * 1000 + C)
    x = torch.randn(rows, C, generator=gen) * (torch.rand(C, generator=gen) * 3 + 0.1) + torch.randn(C, generator=gen)
    _stats_case(f"stats rows={rows} C={C}", x)


@pytest.mark.parametrize("C", WIDTHS)
def test_batch_stats_survive_a_large_common_offset(C):
    """Columns with mean 50 and standard deviation 0.05: E[x^2] - E[x]^2 in fp32 keeps no digit of this variance."""
    gen = torch.Generator().manual_seed(7 + C)
    _stats_case(f"offset C={C}", 50.0 + 0.05 * torch.randn(4099, C, generator=gen))


def test_batch_stats_of_one_row_are_refused():
    from audio_motion_avatar_amd._lib import AmavError

    ops = _ops()
    with pytest.raises(AmavError):
        ops.bn_batch_stats(torch.randn(1, 32).cuda())
    with pytest.raises(AmavError):
        ops.bn_gelu_train_differentiable(torch.randn(1, 32).cuda(), torch.ones(32).cuda(), torch.zeros(32).cuda(), EPS)


@pytest.mark.parametrize("rows", (2, 17, 4099))
def test_constant_columns_have_exactly_zero_variance(rows):
    ops = _ops()
    row = torch.randn(260, generator=torch.Generator().manual_seed(3)) * 37.0
    x = row.expand(rows, 260).contiguous().cuda()
    mean, var = ops.bn_batch_stats(x)
    assert torch.equal(var, torch.zeros_like(var)) and torch.equal(mean.cpu(), row)
    w, b = torch.randn(260).cuda(), torch.randn(260).cuda()
    out, _, _ = ops.bn_gelu_train_differentiable(x, w, b, EPS)
    assert bool(torch.isfinite(out).all())


def _affine(C, gen):
    w = torch.rand(C, generator=gen) + 0.5
    w[1], w[2] = 0.0, -0.8  # a dead channel and a negative scale
    return w, torch.randn(C, generator=gen) * 0.3


def _bn_reference(x, w, b, dout, dtype):
    x, w, b = (t.detach().clone().to(dtype).requires_grad_() for t in (x, w, b))
    out = F.gelu(F.batch_norm(x, None, None, w, b, True, 0.0, EPS))
    out.backward(dout.to(dtype))
    return out.detach(), x.grad, w.grad, b.grad


def _bn_hip(x, w, b, dout):
    ops = _ops()
    xg, wg, bg = (t.cuda().requires_grad_() for t in (x, w, b))
    out, mean, var = ops.bn_gelu_train_differentiable(xg, wg, bg, EPS)
    assert not mean.requires_grad and not var.requires_grad
    out.backward(dout.cuda())
    return out.detach(), xg.grad, wg.grad, bg.grad, mean, var


@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("rows", ROWS)
def test_bn_gelu_train_forward_and_backward_match_fp64(rows, C):
    gen = torch.Generator().manual_seed(rows * 77 + C)
    x = torch.randn(rows, C, generator=gen) * 1.5 + 0.5
    w, b = _affine(C, gen)
    dout = torch.randn(rows, C, generator=gen)
    r64, r32 = _bn_reference(x, w, b, dout, torch.float64), _bn_reference(x, w, b, dout, torch.float32)
    got = _bn_hip(x, w, b, dout)
    for name, g, a, c in zip(("out", "grad_x", "grad_weight", "grad_bias"), got, r64, r32):
        _check(f"bn_gelu_train rows={rows} C={C} {name}", g, a, c)
    again = _bn_hip(x, w, b, dout)
    for a, c in zip(got, again):
        assert torch.equal(a, c)
    v64, m64 = torch.var_mean(x.double(), 0, unbiased=False)
    v32, m32 = torch.var_mean(x, 0, unbiased=False)
    _check("mean output", got[4], m64, m32)
    _check("var output", got[5], v64, v32)


@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("rows", ROWS)
def test_grad_x_column_sums_vanish(rows, C):
    """The two mean-subtraction terms of a batch-normalised layer: |sum_r grad_x| <= 1e-4 * sum_r |grad_x| per column.

    rows = 2 is the hard case: there xhat = +-(1 - d) with d ~ eps / (2 var), so grad_x is itself only 2 d ~ 5e-4 of g
    and one fp32 rounding of g, of a column sum or of the mean is 1e-4 of it (torch's own fp32 backward on the CPU gives
    1.9e-4 to 7.4e-4 on these inputs).  The kernel keeps its column sums in fp64 and centres both terms (DESIGN.md
    section 4.18), which holds the ratio at fp32 rounding (<= 6e-8) for every row count."""
    gen = torch.Generator().manual_seed(rows * 77 + C)
    x = torch.randn(rows, C, generator=gen) * 1.5 + 0.5
    w, b = _affine(C, gen)
    gx = _bn_hip(x, w, b, torch.randn(rows, C, generator=gen))[1].double()
    total, mass = gx.sum(0).abs(), gx.abs().sum(0)
    print(f"grad_x column sums rows={rows} C={C}: worst |sum| / sum|.| {float((total / mass.clamp_min(1e-300)).max()):.3e}")
    assert bool((total <= 1e-4 * mass).all())


def _segments(gen):
    sizes = [1, 2, 3, 4, 5, 6, 7, 8, 1, 8, 2, 5] + [40]  # singletons, ties inside the 8, a long segment
    n = sum(sizes)
    members = torch.randperm(n, generator=gen)
    seg = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64)
    return sizes, n, members, seg


def _pool_reference(x, members, seg, w, b, dout, dtype):
    x, w, b = (t.detach().clone().to(dtype).requires_grad_() for t in (x, w, b))
    rows = []
    for j in range(seg.shape[0] - 1):
        m = x[members[seg[j]:seg[j + 1]]]
        first = torch.from_numpy(np.argmax(m.detach().numpy(), axis=0))  # numpy: the first occurrence
        rows.append(m.gather(0, first[None])[0])
    out = F.gelu(F.batch_norm(torch.stack(rows), None, None, w, b, True, 0.0, EPS))
    out.backward(dout.to(dtype))
    return out.detach(), x.grad, w.grad, b.grad


@functools.lru_cache(maxsize=None)
def _pool_case(C):
    gen = torch.Generator().manual_seed(51 + C)
    sizes, n, members, seg = _segments(gen)
    x = torch.randn(n, C, generator=gen)
    tie_first, tie_second = int(members[seg[9]]), int(members[seg[9] + 3])
    x[tie_first] = x[tie_second] = 6.0
    w, b = _affine(C, gen)
    dout = torch.randn(len(sizes), C, generator=gen)
    refs = tuple(_pool_reference(x, members, seg, w, b, dout, t) for t in (torch.float64, torch.float32))
    landed = torch.zeros(n, C, dtype=torch.bool)  # (first attaining member in segment order, channel) of every segment
    for j in range(len(sizes)):
        rows = members[seg[j]:seg[j + 1]]
        landed[rows[torch.from_numpy(np.argmax(x[rows].numpy(), axis=0))], torch.arange(C)] = True
    return x, members, seg, w, b, dout, tie_first, tie_second, refs, landed


def _pool_hip(C):
    ops = _ops()
    x, members, seg, w, b, dout = _pool_case(C)[:6]
    xg, wg, bg = (t.cuda().requires_grad_() for t in (x, w, b))
    out, mean, var = ops.cluster_max_bn_train_differentiable(xg, members.cuda(), seg.cuda(), wg, bg, EPS)
    out.backward(dout.cuda())
    return out.detach(), xg.grad, wg.grad, bg.grad


@pytest.mark.parametrize("C", WIDTHS)
def test_cluster_max_bn_train_matches_fp64(C):
    ops = _ops()
    x, members, seg, w, b, dout, tie_first, tie_second, (r64, r32), landed = _pool_case(C)
    got = _pool_hip(C)
    for name, g, a, c in zip(("out", "grad_x", "grad_weight", "grad_bias"), got, r64, r32):
        _check(f"cluster_max_bn_train C={C} {name}", g, a, c)
    gx = got[1].cpu()
    # the gradient lands on the first attaining member only: every other entry is exactly +0
    assert int(landed.sum()) == (seg.shape[0] - 1) * C and not bool((r64[1] != 0)[~landed].any())
    rest = gx[~landed]
    assert torch.equal(rest, torch.zeros_like(rest)) and not bool(torch.signbit(rest).any())
    assert float(gx[tie_second].abs().max()) == 0.0 and float(gx[tie_first].abs().max()) > 0
    raw = ops.cluster_max_raw(x.cuda(), members.cuda(), seg.cuda()).cpu()
    want = torch.stack([x[members[seg[j]:seg[j + 1]]].max(0).values for j in range(seg.shape[0] - 1)])
    assert torch.equal(raw, want)
    for a, c in zip(got, _pool_hip(C)):
        assert torch.equal(a, c)


def test_entries_are_bitwise_reproducible():
    ops = _ops()
    gen = torch.Generator().manual_seed(5)
    x, dout = torch.randn(4099, 260, generator=gen).cuda(), torch.randn(4099, 260, generator=gen).cuda()
    w, b = (t.cuda() for t in _affine(260, gen))
    mean, var = ops.bn_batch_stats(x)
    rstd = torch.rsqrt(var + EPS)
    first = ops.bn_gelu_train_backward(x, mean, rstd, w, b, dout)
    second = ops.bn_gelu_train_backward(x, mean, rstd, w, b, dout)
    assert all(torch.equal(a, c) for a, c in zip(first, second))
    sizes, n, members, seg = _segments(gen)
    xs, g = torch.randn(n, 260, generator=gen).cuda(), torch.randn(len(sizes), 260, generator=gen).cuda()
    members, seg = members.cuda(), seg.cuda()
    assert torch.equal(ops.cluster_max_raw(xs, members, seg), ops.cluster_max_raw(xs, members, seg))
    assert torch.equal(ops.cluster_max_route(xs, members, seg, g), ops.cluster_max_route(xs, members, seg, g))


@pytest.mark.parametrize("C", WIDTHS)
def test_library_switch_gives_the_same_values(C, monkeypatch):
    monkeypatch.setenv("AMAV_REFINER_BN", "library")
    gen = torch.Generator().manual_seed(900 + C)
    x = torch.randn(1000, C, generator=gen) * 1.5 + 0.5
    w, b = _affine(C, gen)
    dout = torch.randn(1000, C, generator=gen)
    r64, r32 = _bn_reference(x, w, b, dout, torch.float64), _bn_reference(x, w, b, dout, torch.float32)
    for name, g, a, c in zip(("out", "grad_x", "grad_weight", "grad_bias"), _bn_hip(x, w, b, dout), r64, r32):
        _check(f"library bn_gelu_train C={C} {name}", g, a, c)
    r64, r32 = _pool_case(C)[8]
    for name, g, a, c in zip(("out", "grad_x", "grad_weight", "grad_bias"), _pool_hip(C), r64, r32):
        _check(f"library cluster_max_bn_train C={C} {name}", g, a, c)
