"""Shared by the TriplaneDownsampler tests: an fp64 torch restatement of ConvNeXtBlock and of the
4x4 strided convolution (src/models/triplane_net.py:411-451) on channels-last planes [K,H,W,C], the same expressions in the
library's fp32 (the yardstick the HIP bounds are derived from), seeded inputs, and the error measure.

Bounds.  Every HIP result is compared with the fp64 restatement, relative to max |reference| of the tensor (`rel_err`; the
measure of close() in tests/test_stage1_gpu.py without its floor of 1).  The bound of a tensor is LIBRARY_ERR[kind] *
ORDER_FACTOR: the error of the library's own fp32 evaluation (F.conv2d, F.layer_norm, F.gelu, F.linear and their
autograd) against the same restatement, measured over every case of the tests on the CPU and on the MI355X by
measure_library() (the larger of the two, rounded up to one digit; the figures stand beside the table), times 4 for a
summation order that differs from the library's over 49 taps and up to 256 channels.  Neither number comes from the HIP
kernels; their measured errors are listed for comparison only."""
import functools

import torch
import torch.nn.functional as F

ORDER_FACTOR = 4.0
# kind -> the library's fp32 error against the fp64 restatement (relative to max |reference|), measured as described above
LIBRARY_ERR = {         # library fp32: CPU / MI355X      HIP kernels on the MI355X
    "conv": 3e-7,       # 2.8e-7 / 2.7e-7                 2.8e-7   depthwise 7x7 + bias
    "norm": 4e-7,       # 2.4e-7 / 3.5e-7                 2.7e-7   ... + LayerNorm
    "gelu": 2e-7,       # 1.0e-7 / 6.2e-8                 6.2e-8   gelu(proj + bias)
    "block": 3e-6,      # 2.5e-6 / 8.6e-7                 8.6e-7   the downsampler after one / two blocks and after the
    #                                                              strided convolution, fp32 GEMMs (C = 64 fixture, C = 256)
    "dx": 3e-7,         # 2.1e-7 / 2.6e-7                 2.1e-7   d input of dwconv + LayerNorm
    "dparam": 5e-7,     # 4.9e-7 / 3.7e-7                 2.2e-7   d dwconv weight / bias, d LayerNorm weight / bias, d GELU bias
    "dgelu": 2e-7,      # 1.4e-7 / 7.3e-8                 7.3e-8   d proj of the GELU
    "dmodule": 2e-6,    # 1.7e-6 / 1.8e-6                 1.9e-6   d input and d parameters of the whole downsampler (C = 256,
    #                                                              24 x 24 planes; the largest are the library GEMMs' own wgrads)
}


def bound(kind):
    return LIBRARY_ERR[kind] * ORDER_FACTOR


def rel_err(got, want):
    want = want.detach().double().cpu()
    got = got.detach().double().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    return float((got - want).abs().max()) / max(float(want.abs().max()), 1e-30)


def randn(seed, *shape, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


# ------------------------------------------------------------------------------------- restatements (any dtype / device)
def dwconv(x, dw_w, dw_b):
    """x [K,H,W,C], dw_w [C,1,7,7] -> depthwise 7x7, padding 3, + bias, channels-last."""
    C = x.shape[-1]
    return F.conv2d(x.permute(0, 3, 1, 2), dw_w, dw_b, padding=3, groups=C).permute(0, 2, 3, 1)


def dwconv_norm(x, dw_w, dw_b, ln_w, ln_b, eps=1e-6):
    """-> (y, LayerNorm over C of y) with y = dwconv(x)."""
    y = dwconv(x, dw_w, dw_b)
    return y, F.layer_norm(y, (x.shape[-1],), ln_w, ln_b, eps)


def gelu_bias(proj, bias):
    return F.gelu(proj + bias)


def block(p, prefix, x):
    """ConvNeXtBlock on channels-last planes from a parameter dict (the module's names under `prefix`)."""
    g = lambda k: p[prefix + k]
    _, n = dwconv_norm(x, g("dwconv.weight"), g("dwconv.bias"), g("norm.weight"), g("norm.bias"))
    h = F.gelu(F.linear(n, g("pwconv1.weight"), g("pwconv1.bias")))
    return F.linear(h, g("pwconv2.weight"), g("pwconv2.bias")) + x


def down(p, prefix, x, stride):
    return F.conv2d(x.permute(0, 3, 1, 2), p[prefix + "down.weight"], p[prefix + "down.bias"], stride=stride,
                    padding=1).permute(0, 2, 3, 1)


def downsampler(p, prefix, x, stride):
    """-> [after block 0, after block 1, after the strided convolution] for channels-last planes x."""
    a = block(p, prefix + "blocks.0.", x)
    b = block(p, prefix + "blocks.1.", a)
    return [a, b, down(p, prefix, b, stride)]


def patch4_gather(x, stride):
    """x [K,H,W,C] -> [K*Ho*Wo, 16*C] tap-major: F.unfold's columns (channel-major) reordered.  A copy: exact in any dtype."""
    K, H, W, C = x.shape
    cols = F.unfold(x.permute(0, 3, 1, 2), kernel_size=4, padding=1, stride=stride)       # [K, C*16, L]
    return cols.view(K, C, 16, -1).permute(0, 3, 2, 1).reshape(-1, 16 * C)


def to(p, dtype, device="cpu"):
    return {k: v.to(device=device, dtype=dtype) for k, v in p.items()}


def planes_of(x5):
    """[F,3,C,H,W] -> channels-last planes [F*3,H,W,C]."""
    Fr, P, C, H, W = x5.shape
    return x5.permute(0, 1, 3, 4, 2).reshape(Fr * P, H, W, C)


# -------------------------------------------------------------------------------------------------------- seeded cases
# (K, H, W, C): 5 x 5 clips every tap set on two sides, 9 x 13 is off the 8 x 8 tile (four blocks per plane); the narrowest
# and the default width
DW_CASES = [(1, 5, 5, 64), (1, 9, 13, 64), (2, 9, 13, 256), (2, 5, 5, 256)]


@functools.lru_cache(maxsize=None)
def dw_case(K, H, W, C, seed=0):
    """fp32 inputs of dwconv + LayerNorm and the fp64 results (y, norm) -- computed once, shared, never modified."""
    x = randn(seed + 1, K, H, W, C)
    dw_w = randn(seed + 2, C, 1, 7, 7, scale=1.0 / 7)
    dw_b, ln_b = randn(seed + 3, C, scale=0.1), randn(seed + 5, C, scale=0.1)
    ln_w = 1.0 + randn(seed + 4, C, scale=0.1)
    args = (x, dw_w, dw_b, ln_w, ln_b)
    y, n = dwconv_norm(*(t.double() for t in args))
    return args, (y, n.reshape(-1, C))


@functools.lru_cache(maxsize=None)
def dw_backward_case(K, H, W, C, seed=0):
    """(inputs, grad_norm fp32, fp64 gradients (dx, d dw_w, d dw_b, d ln_w, d ln_b)) of dwconv + LayerNorm."""
    args, _ = dw_case(K, H, W, C, seed)
    g = randn(seed + 6, K * H * W, C)
    leaves = [t.double().requires_grad_(True) for t in args]
    _, n = dwconv_norm(*leaves)
    grads = torch.autograd.grad(n.reshape(-1, C), leaves, g.double())
    return args, g, tuple(t.detach() for t in grads)


def library_dw_backward(args, g, device="cpu"):
    """The library's fp32 autograd of the same expression."""
    leaves = [t.to(device).requires_grad_(True) for t in args]
    _, n = dwconv_norm(*leaves)
    return torch.autograd.grad(n.reshape(-1, args[0].shape[-1]), leaves, g.to(device))


GELU_ROWS = (1, 67)
GELU_INNER = 256


@functools.lru_cache(maxsize=None)
def gelu_case(rows, inner=GELU_INNER, seed=20):
    """(proj, bias, grad_out fp32; fp64 gelu(proj + bias), d proj, d bias).  proj spans the saturated tails too."""
    proj, bias, g = randn(seed, rows, inner, scale=3.0), randn(seed + 1, inner, scale=0.5), randn(seed + 2, rows, inner)
    leaves = [proj.double().requires_grad_(True), bias.double().requires_grad_(True)]
    out = gelu_bias(*leaves)
    d_proj, d_bias = torch.autograd.grad(out, leaves, g.double())
    return (proj, bias, g), (out.detach(), d_proj, d_bias)


@functools.lru_cache(maxsize=None)
def module_case(C=256, R=8, factor=3, frames=1, seed=40):
    """A seeded TriplaneDownsampler state_dict (reference names), fine planes [frames*3, R*factor, R*factor, C] at the
    magnitude of per-cell feature means, and the fp64 results of `downsampler`."""
    from helpers import seeded_params

    shapes = {}
    for b in range(2):
        for name, shape in (("dwconv.weight", [C, 1, 7, 7]), ("dwconv.bias", [C]), ("norm.weight", [C]), ("norm.bias", [C]),
                            ("pwconv1.weight", [4 * C, C]), ("pwconv1.bias", [4 * C]), ("pwconv2.weight", [C, 4 * C]),
                            ("pwconv2.bias", [C])):
            shapes[f"blocks.{b}.{name}"] = shape
    shapes["down.weight"], shapes["down.bias"] = [C, C, 4, 4], [C]
    p = seeded_params(shapes, "triplane_downsampler.")
    x = randn(seed, frames * 3, R * factor, R * factor, C)
    return p, x, [t.detach() for t in downsampler(to(p, torch.float64), "", x.double(), factor)]


def module_grads(p, x, g, factor=3):
    """Gradients of the restated downsampler's output (upstream gradient g) for the input and every parameter, in the
    dtype / on the device of p: {"input": ..., name: ...}."""
    leaves = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    leaf = x.to(next(iter(p.values()))).clone().requires_grad_(True)
    y = downsampler(leaves, "", leaf, factor)[2]
    grads = torch.autograd.grad(y, [leaf] + list(leaves.values()), g.to(y))
    return dict(zip(["input"] + list(leaves), (t.detach() for t in grads)))


@functools.lru_cache(maxsize=None)
def module_backward_case():
    """(upstream gradient fp32, fp64 gradients) of module_case()."""
    p, x, want = module_case()
    g = randn(41, *want[2].shape)
    return g, module_grads(to(p, torch.float64), x, g)


def measure_library(device="cpu"):
    """{kind: the library's fp32 error against the fp64 restatement, the largest over the tests' cases} on `device`."""
    from helpers import ref_fixture, seeded_params

    err = {k: 0.0 for k in LIBRARY_ERR}
    up = lambda kind, got, want: err.__setitem__(kind, max(err[kind], rel_err(got, want)))
    for case in DW_CASES:
        args, (y, n) = dw_case(*case)
        ly, ln = dwconv_norm(*(t.to(device) for t in args))
        up("conv", ly, y)
        up("norm", ln.reshape(n.shape), n)
        args, g, want = dw_backward_case(*case)
        got = library_dw_backward(args, g, device)
        up("dx", got[0], want[0])
        for a, b in zip(got[1:], want[1:]):
            up("dparam", a, b)
    for rows in GELU_ROWS:
        (proj, bias, g), (out, d_proj, d_bias) = gelu_case(rows)
        leaves = [proj.to(device).requires_grad_(True), bias.to(device).requires_grad_(True)]
        lo = gelu_bias(*leaves)
        lp, lb = torch.autograd.grad(lo, leaves, g.to(device))
        up("gelu", lo, out)
        up("dgelu", lp, d_proj)
        up("dparam", lb, d_bias)
    a, meta, _ = ref_fixture("stage1_downsampler")
    p = seeded_params(meta["params"], meta["param_prefix"])
    x = planes_of(a["x"])
    for got, want in zip(downsampler(to(p, torch.float32, device), "", x.to(device), 3),
                         downsampler(to(p, torch.float64), "", x.double(), 3)):
        up("block", got, want)
    p, x, want = module_case()
    for got, w in zip(downsampler(to(p, torch.float32, device), "", x.to(device), 3), want):
        up("block", got, w)
    g, want = module_backward_case()
    got = module_grads(to(p, torch.float32, device), x, g)
    for k in want:
        up("dmodule", got[k], want[k])
    return err


# ---------------------------------------------------------------- every built width, off-square tile grids, magnitudes
# The second case list of the stencil (tests/test_stage1_downsampler_widths_gpu.py; its conditions are asserted on the
# CPU by tests/test_stage1_downsampler_cases.py).  A case is (group, (K, H, W, C), options of wide_case as sorted pairs).
#   widths  every instantiation V = C / 64 = 1..8 on 19 x 27: a 3 x 4 tile grid, ragged on both axes, whose tiles (1, 1) and
#           (1, 2) have their whole 14 x 14 halo inside the plane; 12 tiles = one unrolled-by-8 pass of sum_parts_kernel and
#           a tail of three.  27 x 19 is the transpose.  17 x 17: 9 tiles (the unrolled body once, an empty tail) and 289
#           rows (the last LayerNorm chunk of 16 holds one row); K = 3 of them: 27 tiles across planes.
#   eps     var(y) ~ 1e-6 = eps: inputs x 1e-3, dwconv bias x 1e-4
#   large   inputs x 1e3, dwconv bias x 1e2
#   offset  dwconv bias 8 + 0.1 randn: |row mean| > 5 standard deviations, the cancellation of a one-pass variance
MAGNITUDES = {
    "eps": (("b_scale", 1e-4), ("eps", 1e-6), ("x_scale", 1e-3)),
    "large": (("b_scale", 1e2), ("x_scale", 1e3)),
    "offset": (("b_offset", 8.0),),
}
WIDE_GROUPS = ("widths", "eps", "large", "offset")
WIDE_KINDS = ("conv", "norm", "dx", "dparam")
WIDE_CASES = ([("widths", (1, 19, 27, C), ()) for C in range(64, 513, 64)]
              + [("widths", (1, 27, 19, 192), ()), ("widths", (1, 17, 17, 64), ()), ("widths", (3, 17, 17, 128), ())]
              + [(group, (1, 9, 13, C), MAGNITUDES[group]) for group in ("eps", "large", "offset") for C in (64, 192, 512)])

# (group, kind) -> the library's fp32 error against the fp64 restatement over the group's cases, measured by
# measure_library_wide() on the CPU and on the MI355X; the larger of the two, rounded up to one digit.  A test's bound is
# the figure x ORDER_FACTOR (bound_wide).  None of it comes from the HIP kernels, whose errors stand beside for comparison.
LIBRARY_ERR_WIDE = {                # library fp32: CPU / MI355X      HIP kernels on the MI355X
    ("widths", "conv"): 4e-7,       # 2.8e-7 / 3.1e-7                   2.8e-7
    ("widths", "norm"): 5e-7,       # 4.6e-7 / 3.2e-7                   3.2e-7
    ("widths", "dx"): 4e-7,         # 3.3e-7 / 3.1e-7                   3.2e-7
    ("widths", "dparam"): 1e-6,     # 9.0e-7 / 9.8e-7                   2.6e-7
    ("eps", "conv"): 3e-7,          # 2.3e-7 / 2.4e-7                   2.3e-7
    ("eps", "norm"): 3e-7,          # 2.8e-7 / 2.7e-7                   3.2e-7
    ("eps", "dx"): 3e-7,            # 2.1e-7 / 2.5e-7                   2.3e-7
    ("eps", "dparam"): 6e-7,        # 2.8e-7 / 5.2e-7                   2.0e-7
    ("large", "conv"): 3e-7,        # 2.6e-7 / 2.1e-7                   2.6e-7
    ("large", "norm"): 3e-7,        # 2.8e-7 / 2.7e-7                   2.8e-7
    ("large", "dx"): 3e-7,          # 2.6e-7 / 2.3e-7                   2.5e-7
    ("large", "dparam"): 6e-7,      # 3.2e-7 / 5.2e-7                   1.5e-7
    ("offset", "conv"): 1e-7,       # 9.1e-8 / 9.9e-8                   9.1e-8   (5.6e-7 with the bias first)
    ("offset", "norm"): 3e-6,       # 6.6e-7 / 2.6e-6                   6.8e-7   (the library on the MI355X: 4x the CPU's)
    ("offset", "dx"): 7e-7,         # 3.2e-7 / 6.4e-7                   2.5e-7
    ("offset", "dparam"): 6e-6,     # 7.3e-7 / 5.1e-6                   6.3e-7   (... 7x the CPU's)
}
# bias + GELU at the product's inner = 4 C = 1024 and at inner = 12 (no multiple of 8: fp32 output only).  The library's
# fp32 error there is inside LIBRARY_ERR's gelu / dgelu / dparam entries, which therefore apply unchanged:
#   gelu 8.8e-8 / 6.6e-8; 6.6e-8      dgelu 1.5e-7 / 8.6e-8; 8.6e-8      dparam (d bias) 1.3e-7 / 1.4e-7; 1.5e-7
#   (library fp32 on the CPU / on the MI355X; the HIP kernels on the MI355X)
GELU_WIDE = ((67, 1024), (5, 12))


def bound_wide(group, kind):
    return LIBRARY_ERR_WIDE[group, kind] * ORDER_FACTOR


def case_id(case):
    group, shape, _ = case
    return group + "-" + "x".join(map(str, shape))


@functools.lru_cache(maxsize=None)
def wide_tensors(K, H, W, C, x_scale=1.0, b_scale=1.0, b_offset=0.0, eps=1e-6, seed=100):
    x = randn(seed + 1, K, H, W, C, scale=x_scale)
    dw_w = randn(seed + 2, C, 1, 7, 7, scale=1.0 / 7)
    dw_b = b_offset + randn(seed + 3, C, scale=0.1 * b_scale)
    ln_w, ln_b = 1.0 + randn(seed + 4, C, scale=0.1), randn(seed + 5, C, scale=0.1)
    args = (x, dw_w, dw_b, ln_w, ln_b)
    g = randn(seed + 6, K * H * W, C)
    leaves = [t.double().requires_grad_(True) for t in args]
    y, n = dwconv_norm(*leaves, eps=eps)
    n = n.reshape(-1, C)
    grads = torch.autograd.grad(n, leaves, g.double())
    return args, eps, (y.detach(), n.detach()), g, tuple(t.detach() for t in grads)


def wide_case(case):
    """A case of WIDE_CASES -> (fp32 inputs (x, dw_w, dw_b, ln_w, ln_b), eps, fp64 (y, norm rows), grad_norm fp32, fp64
    gradients (dx, d dw_w, d dw_b, d ln_w, d ln_b)), generated like dw_case / dw_backward_case -- computed once, shared,
    never modified."""
    _, shape, options = case
    return wide_tensors(*shape, **dict(options))


def library_wide(case, device="cpu"):
    """The library's fp32 evaluation of a case: {kind: (results, fp64 references)}."""
    args, eps, (y, n), g, want = wide_case(case)
    leaves = [t.to(device).requires_grad_(True) for t in args]
    ly, ln = dwconv_norm(*leaves, eps=eps)
    ln = ln.reshape(n.shape)
    grads = torch.autograd.grad(ln, leaves, g.to(device))
    return {"conv": ([ly], [y]), "norm": ([ln], [n]), "dx": (grads[:1], want[:1]), "dparam": (grads[1:], want[1:])}


def measure_library_wide(device="cpu"):
    """{(group, kind): the library's fp32 error against the fp64 restatement, the largest over the group's cases} on
    `device`, and under ("gelu", kind) the same for GELU_WIDE."""
    err = {}
    up = lambda key, got, want: err.__setitem__(key, max(err.get(key, 0.0), rel_err(got, want)))
    for case in WIDE_CASES:
        for kind, (got, want) in library_wide(case, device).items():
            for a, b in zip(got, want):
                up((case[0], kind), a, b)
    for rows, inner in GELU_WIDE:
        (proj, bias, g), (out, d_proj, d_bias) = gelu_case(rows, inner)
        leaves = [proj.to(device).requires_grad_(True), bias.to(device).requires_grad_(True)]
        lo = gelu_bias(*leaves)
        lp, lb = torch.autograd.grad(lo, leaves, g.to(device))
        up(("gelu", "gelu"), lo, out)
        up(("gelu", "dgelu"), lp, d_proj)
        up(("gelu", "dparam"), lb, d_bias)
    return err
