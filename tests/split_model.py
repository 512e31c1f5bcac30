"""An independent statement, on CPU tensors, of the split-operand formats of the transformer step (include/amav.h,
amav_split_operand) and of the two row operations that write them (LayerNorm, GEGLU), for the GPU tests to
compare the kernels with.  Everything here is torch on the CPU: `.to(float16)` / `.to(bfloat16)` there are IEEE
round-to-nearest-even conversions that keep subnormals, whatever conversion instructions and denormal mode the device
uses.  tests/test_split_model.py checks this file against the formats' own claims."""
import torch
import torch.nn.functional as F

BF16X3, FP16X2 = 0, 1  # AMAV_SPLIT_BF16X3, AMAV_SPLIT_FP16X2 (test_split_model.py compares them with the header)
FP16_TARGET = 32768.0  # the caller of the fp16 x 2 format bounds |x * 2^e| by this


def split2(x, e=0):
    """fp32 x -> (h1, h2) fp16 with x * 2^e = h1 + h2 up to 2^-22 (relative) or 2^-25 (absolute, where h2 is an fp16
    subnormal): h1 the nearest fp16, h2 the nearest fp16 of the exact fp32 residual."""
    assert x.dtype == torch.float32 and not x.is_cuda and -126 <= e <= 126
    xs = x * 2.0 ** e
    h1 = xs.to(torch.float16)
    return h1, (xs - h1.float()).to(torch.float16)


def split3(x):
    """fp32 x -> (x1, x2, x3) bf16 with x = x1 + x2 + x3 up to 2^-23 |x| (exact where x3 does not underflow)."""
    assert x.dtype == torch.float32 and not x.is_cuda
    x1 = x.to(torch.bfloat16)
    r = x - x1.float()
    x2 = r.to(torch.bfloat16)
    return x1, x2, (r - x2.float()).to(torch.bfloat16)


def operand(x, fmt, weights=False, e=0):
    """x [rows, k] fp32 -> the K-concatenated operand of the split GEMM, small terms first:
         fp16 x 2   activations [h2|h1|h1]             weights [g1|g2|g1]             (K' = 3 k, of x * 2^e)
         bf16 x 3   activations [x3|x2|x1|x2|x1|x1]    weights [w1|w2|w3|w1|w2|w1]    (K' = 6 k; e is ignored)"""
    assert x.dim() == 2
    if fmt == FP16X2:
        h1, h2 = split2(x, e)
        parts = (h1, h2, h1) if weights else (h2, h1, h1)
    elif fmt == BF16X3:
        x1, x2, x3 = split3(x)
        parts = (x1, x2, x3, x1, x2, x1) if weights else (x3, x2, x1, x2, x1, x1)
    else:
        raise ValueError(f"unknown split format {fmt}")
    return torch.cat(parts, dim=1)


def bits(t):
    """The 16-bit patterns of an fp16 / bf16 tensor: torch.equal on these tells +0 from -0, which == does not."""
    assert t.dtype in (torch.float16, torch.bfloat16)
    return t.contiguous().view(torch.int16)


def layer_norm64(h, weight, bias, eps):
    """LayerNorm over the last axis in fp64 (biased variance, as nn.LayerNorm)."""
    h = h.double()
    mean = h.mean(-1, keepdim=True)
    var = ((h - mean) ** 2).mean(-1, keepdim=True)
    return (h - mean) / torch.sqrt(var + eps) * weight.double() + bias.double()


def geglu64(proj, bias=None):
    """proj [..., 2 * inner] (+ bias [2 * inner]) -> h * gelu(g) in fp64, exact-erf GELU, and the two fp64 halves."""
    p = proj.double() if bias is None else proj.double() + bias.double()
    h, g = p.chunk(2, dim=-1)
    return h * F.gelu(g), h, g


def edge_values(sweep=4083, seed=0):
    """1-D fp32: the values a split can get wrong, then `sweep` random ones over 13 decades.  +-0; the smallest fp16
    subnormal 2^-24; 2^-25 (a tie between 0 and it) and 3 * 2^-26 (just above that tie); the smallest normal fp16
    2^-14; 1 + 2^-11 (an fp16 rounding tie) and 1 + 2^-8 (a bf16 one); the fp16 x 2 target bound, both signs; the
    smallest fp32 subnormal.  All of magnitude <= 32768."""
    special = torch.tensor([0.0, -0.0, 2.0 ** -24, -2.0 ** -24, 2.0 ** -25, -2.0 ** -25, 3 * 2.0 ** -26, 2.0 ** -14,
                            1 + 2.0 ** -11, -(1 + 2.0 ** -11), 1 + 2.0 ** -8, FP16_TARGET, -FP16_TARGET, 2.0 ** -149],
                           dtype=torch.float64).float()
    g = torch.Generator().manual_seed(seed)
    s = (torch.randn(sweep, generator=g) * torch.logspace(-9, 4.4, sweep)).clamp(-FP16_TARGET, FP16_TARGET)
    return torch.cat([special, s])


def edge_matrix(rows, k, e=0, seed=0):
    """edge_values() tiled into [rows, k] (the special values first, so even k = 8 holds eight of them), times 2^-e --
    exact, save where it leaves fp32's range (clamped to its largest finite value, or rounded into its subnormals) --
    so that |x * 2^e| <= 32768 as the fp16 x 2 format requires."""
    v = edge_values(seed=seed)
    x = v.repeat(-(-rows * k // v.numel()))[:rows * k].reshape(rows, k)
    fmax = torch.finfo(torch.float32).max
    return (x.double() * 2.0 ** -e).clamp(-fmax, fmax).float()
