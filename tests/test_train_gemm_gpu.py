"""GPU tests of the training GEMMs: the transposing operand split is bit-exact against a torch
restatement (the split3 of test_split_gemm_gpu.py applied to x^T), and ops.linear_split_differentiable -- forward, dgrad,
wgrad and bias gradient -- is as close to the fp64 products as F.linear with its autograd on the same fp32 inputs."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ACT, WTS = (2, 1, 0, 1, 0, 0), (0, 1, 2, 0, 1, 0)  # part order [x3 x2 x1 x2 x1 x1] / [x1 x2 x3 x1 x2 x1]


def split3(x):
    a = x.to(torch.bfloat16)
    r = x - a.float()
    b = r.to(torch.bfloat16)
    c = (r - b.float()).to(torch.bfloat16)
    return a, b, c


def bits(t):
    return t.view(torch.int16)


def transposed_reference(x, order):
    """[k, 6 Rp]: per part the split of x^T with Rp - rows zeros after it."""
    rows = x.shape[0]
    parts = [F.pad(p.t(), (0, (rows + 7) // 8 * 8 - rows)) for p in split3(x)]
    return torch.cat([parts[i] for i in order], dim=1).contiguous()


def _input(rows, k):
    g = torch.Generator().manual_seed(rows + k)
    x = (torch.randn(rows, k, generator=g) * torch.logspace(-6, 6, k)[None]).cuda()  # 12 decades of magnitudes
    x[0, 0] = 0.0
    return x


@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("rows,k", [(1, 8), (7, 8), (37, 72), (64, 64), (65, 136), (300, 512), (1029, 40)])
def test_transposed_layout_is_bit_exact(rows, k, weights):
    """A single row, a tail shorter than 8, exact and off-by-one tiles in both directions, many row tiles under one column
    tile.  The entry point writes into buffers pre-filled with NaN bit patterns: an unwritten element (a tail entry, a
    partial tile's edge) cannot pass for a zero."""
    from audio_motion_avatar_amd import _lib, ops

    x = _input(rows, k)
    padded = _lib.lib().amav_split_transposed_rows(rows)
    assert padded == (rows + 7) // 8 * 8
    out_t = torch.full((k, 6 * padded), float("nan"), dtype=torch.bfloat16, device="cuda")
    out_rows = torch.full((rows, 6 * k), float("nan"), dtype=torch.bfloat16, device="cuda")
    ops._call("amav_split_operand_transposed", rows, k, x.data_ptr(), x.stride(0), int(weights), out_rows.data_ptr(),
              out_t.data_ptr())
    want = transposed_reference(x, WTS if weights else ACT)
    assert out_t.shape == want.shape and torch.equal(bits(out_t), bits(want))
    if padded > rows:
        assert not bits(out_t).view(k, 6, padded)[:, :, rows:].any()  # the tails are +0
    assert torch.equal(bits(out_rows), bits(ops.split_operand(x)))  # the activation operand whatever `weights` is
    # the wrapper returns the same bits
    assert torch.equal(bits(ops.split_operand_transposed(x, weights=weights)), bits(want))
    # every part equals split_operand's, bit for bit
    row_major = ops.split_operand(x, weights=weights).view(rows, 6, k)
    assert torch.equal(bits(out_t.view(k, 6, padded)[:, :, :rows]), bits(row_major.permute(2, 1, 0).contiguous()))


@pytest.mark.parametrize("rows,k", [(7, 8), (65, 136), (300, 512)])
def test_also_rows_is_split_operand_and_leaves_the_transposed_operand_alone(rows, k):
    from audio_motion_avatar_amd import ops

    x = _input(rows, k)
    for weights in (False, True):
        out_rows, out_t = ops.split_operand_transposed(x, weights=weights, also_rows=True)
        assert torch.equal(out_rows, ops.split_operand(x)) and torch.equal(bits(out_rows), bits(ops.split_operand(x)))
        assert torch.equal(bits(out_t), bits(ops.split_operand_transposed(x, weights=weights)))


def test_strided_view_and_refused_inputs():
    from audio_motion_avatar_amd import ops
    from audio_motion_avatar_amd._lib import AmavError

    g = torch.Generator().manual_seed(5)
    buf = torch.randn(100, 3 * 64, generator=g).cuda()
    view = buf[:, 64:128]
    for a, b in zip(ops.split_operand_transposed(view, also_rows=True),
                    ops.split_operand_transposed(view.contiguous(), also_rows=True)):
        assert torch.equal(bits(a), bits(b))
    with pytest.raises(AmavError):
        ops.split_operand_transposed(torch.zeros(4, 12).cuda())      # k not a multiple of 8
    with pytest.raises(AmavError):
        ops.split_operand_transposed(torch.zeros(4, 16))             # not on the device
    with pytest.raises(AmavError):
        ops.split_operand_transposed(torch.zeros(4, 16, dtype=torch.float64).cuda())


CASES = [(300, 64, 40, True), (257, 72, 136, False), (1029, 520, 264, True), (6304, 512, 1536, False)]


@functools.lru_cache(maxsize=None)
def _case(M, K, N, bias):
    """Inputs N(0, 1), weights N(0, 1/K), upstream gradient N(0, 1); the fp64 products on the device and the errors of
    F.linear with its autograd on the same fp32 inputs."""
    g = torch.Generator().manual_seed(M + N)
    x = torch.randn(M, K, generator=g).cuda()
    w = (torch.randn(N, K, generator=g) * K ** -0.5).cuda()
    b = torch.randn(N, generator=g).cuda() if bias else None
    up = torch.randn(M, N, generator=g).cuda()
    ref = {"y": x.double() @ w.double().t() + (b.double() if bias else 0.0), "dx": up.double() @ w.double(),
           "dW": up.double().t() @ x.double()}
    if bias:
        ref["db"] = up.double().sum(0)
    got32 = _run(F.linear, x, w, b, up)
    err32 = {k: (got32[k].double() - ref[k]).abs().max().item() for k in ref}
    return x, w, b, up, ref, err32


def _run(fn, x, w, b, up, x_grad=True, w_grad=True):
    xs, ws = x.clone().requires_grad_(x_grad), w.clone().requires_grad_(w_grad)
    bs = None if b is None else b.clone().requires_grad_()
    y = fn(xs, ws, bs)
    y.backward(up)
    out = {"y": y.detach(), "dx": xs.grad, "dW": ws.grad}
    if b is not None:
        out["db"] = bs.grad
    return out


@pytest.mark.parametrize("M,K,N,bias", CASES)
def test_linear_split_differentiable_is_fp32_equivalent(M, K, N, bias):
    """err <= max(1.5 err32, 2e-6 max|ref|) for each of y, dx, dW, db: the bar of test_linear_is_fp32_equivalent, relative
    to the result's scale.  For K <= 1024 the forward also equals transformer.linear under no_grad bit for bit."""
    from audio_motion_avatar_amd import ops, transformer

    x, w, b, up, ref, err32 = _case(M, K, N, bias)
    got = _run(ops.linear_split_differentiable, x, w, b, up)
    failures = []
    for name, r in ref.items():
        assert got[name].dtype == torch.float32 and got[name].shape == r.shape
        err = (got[name].double() - r).abs().max().item()
        bound = max(1.5 * err32[name], 2e-6 * r.abs().max().item())
        print(f"traingemm| M={M} K={K} N={N} {name}: err {err:.3e}, err32 {err32[name]:.3e}, err / err32 "
              f"{err / max(err32[name], 1e-300):.3f}, bound {bound:.3e}")
        if not err <= bound:
            failures.append((name, err, bound))
    assert not failures, failures
    with torch.no_grad():
        assert torch.equal(got["y"], transformer.linear(x, w, b))


def test_needs_input_grad_is_honoured():
    """No dx for a leaf input without grad, no dW for a frozen weight, and the gradient that IS produced is unchanged: the
    one-sided backward hands the same operand bits (the transposed operand does not depend on also_rows, split_operand's
    row-major one is the also_rows one) to the same library product."""
    from audio_motion_avatar_amd import ops

    x, w, b, up, _, _ = _case(300, 64, 40, True)
    both = _run(ops.linear_split_differentiable, x, w, b, up)
    only_w = _run(ops.linear_split_differentiable, x, w, b, up, x_grad=False)
    only_x = _run(ops.linear_split_differentiable, x, w, b, up, w_grad=False)
    assert only_w["dx"] is None and only_x["dW"] is None
    assert torch.equal(only_w["dW"], both["dW"])
    assert torch.equal(only_x["dx"], both["dx"])
    for one in (only_w, only_x):
        assert torch.equal(one["db"], both["db"]) and torch.equal(one["y"], both["y"])


def test_expanded_gradient_and_batched_input():
    """The gradient of .sum() is an expanded scalar (every stride 0); x is [B, S, K] and a strided view."""
    from audio_motion_avatar_amd import ops

    g = torch.Generator().manual_seed(9)
    buf = torch.randn(2, 150, 96, generator=g).cuda()
    w = (torch.randn(24, 64, generator=g) / 8).cuda().requires_grad_()
    b = torch.randn(24, generator=g).cuda().requires_grad_()
    x = buf[..., 16:80].detach().requires_grad_()
    y = ops.linear_split_differentiable(x, w, b)
    assert y.shape == (2, 150, 24)
    y.sum().backward()
    x64, w64 = x.detach().double(), w.detach().double()
    ones = torch.ones(300, 24, dtype=torch.float64, device="cuda")
    for got, want in ((x.grad, (ones @ w64).view(2, 150, 64)), (w.grad, ones.t() @ x64.view(300, 64)), (b.grad, ones.sum(0))):
        assert got.shape == want.shape and (got.double() - want).abs().max().item() <= 2e-6 * want.abs().max().item()


def test_sizes_off_the_split_path_raise():
    from audio_motion_avatar_amd import ops
    from audio_motion_avatar_amd._lib import AmavError

    x = torch.zeros(300, 64).cuda()
    with pytest.raises(AmavError):
        ops.linear_split_differentiable(x, torch.zeros(36, 64).cuda())      # N % 8
    with pytest.raises(AmavError):
        ops.linear_split_differentiable(x[:, :60], torch.zeros(40, 60).cuda())  # K % 8
    with pytest.raises(AmavError):
        ops.linear_split_differentiable(x.cpu(), torch.zeros(40, 64))


def test_train_linear_follows_weight_updates(monkeypatch):
    """Both memoised weight operands are rebuilt after an in-place update: y (the forward operand) and dx (the transposed
    one) follow weight.mul_(2)."""
    from audio_motion_avatar_amd import transformer

    monkeypatch.setenv("AMAV_TRAIN_GEMM", "split")
    g = torch.Generator().manual_seed(3)
    x = torch.randn(512, 64, generator=g).cuda().requires_grad_()
    up = torch.randn(512, 32, generator=g).cuda()
    lin = torch.nn.Linear(64, 32).cuda()

    def step():
        x.grad = lin.weight.grad = None
        y = transformer.train_linear(x, lin.weight, lin.bias)
        assert type(y.grad_fn).__name__.startswith("_LinearSplit")
        y.backward(up)
        return y.detach(), x.grad.clone(), lin.weight.grad.clone()

    y0, dx0, dw0 = step()
    y0b, dx0b, _ = step()  # served from the memo
    assert torch.equal(y0, y0b) and torch.equal(dx0, dx0b)
    with torch.no_grad():
        lin.weight.mul_(2.0)
    y1, dx1, dw1 = step()
    bias = lin.bias.detach()
    assert torch.allclose(y1 - bias, 2.0 * (y0 - bias), atol=1e-5)
    assert torch.allclose(dx1, 2.0 * dx0, atol=1e-5)
    assert torch.allclose(dw1, dw0, atol=1e-5)


def test_default_train_linear_is_f_linear_on_the_device(monkeypatch):
    """Unset and `f32`: values and all three gradients are those of F.linear itself, bit for bit, at a shape the split
    setting would take."""
    from audio_motion_avatar_amd import transformer

    x, w, b, up, _, _ = _case(300, 64, 40, True)
    want = _run(F.linear, x, w, b, up)
    for value in (None, "f32"):
        if value is None:
            monkeypatch.delenv("AMAV_TRAIN_GEMM", raising=False)
        else:
            monkeypatch.setenv("AMAV_TRAIN_GEMM", value)
        got = _run(transformer.train_linear, x, w, b, up)
        for name in want:
            assert torch.equal(got[name], want[name]), (value, name)


def test_products_left_to_the_library():
    """`library` moves single products to the library's fp32 GEMM inside the same Function: every result still meets the
    bound of the accuracy test, and the products that stay split keep their bits."""
    from audio_motion_avatar_amd import ops

    x, w, b, up, ref, err32 = _case(300, 64, 40, True)
    split = _run(ops.linear_split_differentiable, x, w, b, up)
    for library, same in ((("wgrad",), ("y", "dx")), (("forward", "dgrad"), ("dW",)), (ops.LINEAR_PRODUCTS, ())):
        got = _run(lambda *a: ops.linear_split_differentiable(*a, library=library), x, w, b, up)
        for name, r in ref.items():
            err = (got[name].double() - r).abs().max().item()
            assert err <= max(1.5 * err32[name], 2e-6 * r.abs().max().item()), (library, name)
        for name in same:
            assert torch.equal(got[name], split[name]), (library, name)
    with pytest.raises(ops.AmavError):
        ops.linear_split_differentiable(x, w, b, library=("backward",))


def test_train_linear_keeps_the_losing_products_on_the_library(monkeypatch):
    """train_linear's per-product gates (transformer.SPLIT_GEMM_MAX_K, TRAIN_SPLIT_DGRAD_MAX_N, TRAIN_SPLIT_WGRAD): which
    products of a shape reach the split path, and F.linear itself when none does or the rows are too few."""
    from audio_motion_avatar_amd import ops, transformer

    seen = []
    real = ops.linear_split_differentiable

    def spy(x, weight, bias=None, **kw):
        seen.append(tuple(sorted(kw.get("library", ()))))
        return real(x, weight, bias, **kw)

    monkeypatch.setattr(ops, "linear_split_differentiable", spy)
    monkeypatch.setenv("AMAV_TRAIN_GEMM", "split")
    lost_wgrad = () if transformer.TRAIN_SPLIT_WGRAD else ("wgrad",)
    big_k, big_n = transformer.SPLIT_GEMM_MAX_K + 8, transformer.TRAIN_SPLIT_DGRAD_MAX_N + 8
    for rows, K, N, want in ((256, 64, 32, [lost_wgrad]), (256, big_k, 32, [tuple(sorted(("forward",) + lost_wgrad))]),
                             (256, 64, big_n, [tuple(sorted(("dgrad",) + lost_wgrad))]),
                             (256, big_k, big_n, [] if lost_wgrad else [("dgrad", "forward")]), (255, 64, 32, []),
                             (256, 60, 32, []), (256, 64, 36, [])):
        seen.clear()
        x = torch.randn(rows, K, device="cuda").requires_grad_()
        w = (torch.randn(N, K, device="cuda") * K ** -0.5).requires_grad_()
        y = transformer.train_linear(x, w)
        y.sum().backward()
        assert seen == want, (rows, K, N, seen)
        ref = x.detach().double() @ w.detach().double().t()
        assert (y.detach().double() - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()
        assert x.grad is not None and w.grad is not None
