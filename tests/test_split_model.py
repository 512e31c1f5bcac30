"""tests/split_model.py against the formats' own claims (CPU only): the fp16 x 2 parts carry x * 2^e to
max(2^-22 |x 2^e|, 2^-25), the fp32 residual they are built from is exact, the bf16 x 3 parts carry 24 bits, the operand
layouts are the ones include/amav.h documents, and the edge list holds what the GPU tests rely on."""
import pytest
import torch

import split_model as sm


def _values():
    g = torch.Generator().manual_seed(1)
    sweep = torch.randn(400_000, generator=g) * torch.logspace(-9, 4.4, 400_000)
    return torch.cat([sm.edge_values(), sweep.clamp(-sm.FP16_TARGET, sm.FP16_TARGET)])


def test_format_constants_are_the_headers():
    from audio_motion_avatar_amd import _lib

    assert (sm.BF16X3, sm.FP16X2) == (_lib.DEFINES["AMAV_SPLIT_BF16X3"], _lib.DEFINES["AMAV_SPLIT_FP16X2"])


@pytest.mark.parametrize("e", [-126, -3, 0, 10, 126])
def test_split2_reconstructs_to_two_half_ulp_roundings(e):
    """|h1 + h2 - x 2^e| <= max(2^-22 |x 2^e|, 2^-25): two roundings to 11 bits, each half an ulp, and the floor of half
    the smallest fp16 subnormal where the residual falls below fp16's normal range.  Worst ratio over 400 000 values and
    the edge list: exactly 1.0 (x 2^e = 2^-25 rounds to 0; 0.5 at e = 126, where 2^-25 2^-126 is below fp32's range)."""
    x = (_values().double() * 2.0 ** -e).clamp(-3e38, 3e38).float()
    xs = x.double() * 2.0 ** e
    keep = xs.abs() <= sm.FP16_TARGET
    assert keep.float().mean() > 0.99
    h1, h2 = sm.split2(x, e)
    assert torch.isfinite(h1.float()).all() and torch.isfinite(h2.float()).all()
    err = (h1.double() + h2.double() - xs).abs()
    bound = torch.maximum(2.0 ** -22 * xs.abs(), torch.tensor(2.0 ** -25, dtype=torch.float64))
    ratio = float((err / bound)[keep].max())
    print(f"split2 e={e}: worst error / bound {ratio:.3f}")
    assert ratio <= 1.0
    # the residual the second part is rounded from is exact in fp32
    xs32 = x * 2.0 ** e
    assert torch.equal((xs32 - h1.float()).double(), xs32.double() - h1.double())


def test_split3_reconstructs_24_bits():
    """x1 + x2 + x3 = x to 2^-23 |x| + 1e-37, the bound test_split_operand_layouts_are_bit_exact holds the device to;
    both residuals are exact in fp32."""
    g = torch.Generator().manual_seed(2)
    x = torch.cat([_values(), torch.randn(100_000, generator=g) * torch.logspace(-30, 30, 100_000)])
    x1, x2, x3 = sm.split3(x)
    back = x1.double() + x2.double() + x3.double()
    assert ((back - x.double()).abs() <= x.double().abs() * 2.0 ** -23 + 1e-37).all()
    r1 = x - x1.float()
    assert torch.equal(r1.double(), x.double() - x1.double())
    assert torch.equal((r1 - x2.float()).double(), r1.double() - x2.double())


def test_rounding_ties_and_signed_zeros():
    h1, h2 = sm.split2(torch.tensor([1 + 2.0 ** -11, 2.0 ** -25, 3 * 2.0 ** -26, -0.0, 0.0, 2.0 ** -149]))
    assert h1.tolist() == [1.0, 0.0, 2.0 ** -24, 0.0, 0.0, 0.0]          # ties go to the even neighbour
    assert h2.tolist() == [2.0 ** -11, 0.0, 0.0, 0.0, 0.0, 0.0]          # residuals 2^-25 (a tie) and -2^-26 round to 0
    assert sm.bits(h1)[3].item() == -32768 and sm.bits(h1)[4].item() == 0   # -0 keeps its sign in h1
    x1, x2, x3 = sm.split3(torch.tensor([1 + 2.0 ** -8, -0.0]))
    assert (x1[0].item(), x2[0].item(), x3[0].item()) == (1.0, 2.0 ** -8, 0.0)
    assert sm.bits(x1)[1].item() == -32768


def test_operand_layouts():
    x = sm.edge_matrix(3, 8, e=5)
    h1, h2 = sm.split2(x, 5)
    act, wts = sm.operand(x, sm.FP16X2, e=5), sm.operand(x, sm.FP16X2, weights=True, e=5)
    assert act.shape == (3, 24) and act.dtype == torch.float16
    assert [torch.equal(sm.bits(act[:, 8 * i:8 * i + 8]), sm.bits(p)) for i, p in enumerate((h2, h1, h1))] == [True] * 3
    assert [torch.equal(sm.bits(wts[:, 8 * i:8 * i + 8]), sm.bits(p)) for i, p in enumerate((h1, h2, h1))] == [True] * 3
    x1, x2, x3 = sm.split3(x)
    act, wts = sm.operand(x, sm.BF16X3), sm.operand(x, sm.BF16X3, weights=True)
    assert act.shape == (3, 48) and act.dtype == torch.bfloat16
    for got, parts in ((act, (x3, x2, x1, x2, x1, x1)), (wts, (x1, x2, x3, x1, x2, x1))):
        assert all(torch.equal(sm.bits(got[:, 8 * i:8 * i + 8]), sm.bits(p)) for i, p in enumerate(parts))
    # the concatenated operands multiply to the kept partial products
    a, w = sm.operand(x, sm.FP16X2, e=5).double(), sm.operand(x, sm.FP16X2, weights=True, e=5).double()
    want = h2.double() @ h1.double().t() + h1.double() @ h2.double().t() + h1.double() @ h1.double().t()
    assert torch.isfinite(want).all() and torch.allclose(a @ w.t(), want, rtol=1e-12, atol=0)


def test_edge_values_hold_what_the_gpu_tests_rely_on():
    v = sm.edge_values()
    assert v.dtype == torch.float32 and torch.isfinite(v).all() and float(v.abs().max()) == sm.FP16_TARGET
    for special in (2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -26, 2.0 ** -14, 1 + 2.0 ** -11, 1 + 2.0 ** -8, 32768.0, -32768.0,
                    2.0 ** -149):
        assert (v[:14] == special).any(), special
    assert (v[:2] == 0).all() and torch.signbit(v[:2]).tolist() == [False, True]
    h1, h2 = sm.split2(v)
    sub = lambda h: (h != 0) & (h.float().abs() < 2.0 ** -14)
    assert sub(h1).sum() > 20 and (sub(h2) & ~sub(h1)).sum() > 200   # parts that are fp16 subnormals, of both kinds
    assert (v.abs() < 1e-8).any() and (v.abs() > 1e4).any()
    for rows, k, e in ((1, 8, 0), (3, 24, -126), (37, 520, 126), (37, 520, 10)):
        x = sm.edge_matrix(rows, k, e)
        assert x.shape == (rows, k) and torch.isfinite(x).all()
        assert float((x.double() * 2.0 ** e).abs().max()) <= sm.FP16_TARGET


def test_fp64_rows():
    g = torch.Generator().manual_seed(3)
    h, w, b = torch.randn(5, 768, generator=g), torch.randn(768, generator=g), torch.randn(768, generator=g)
    want = torch.nn.functional.layer_norm(h.double(), (768,), w.double(), b.double(), 1e-3)
    assert float((sm.layer_norm64(h, w, b, 1e-3) - want).abs().max()) <= 1e-13
    proj, bias = torch.randn(4, 24, generator=g) * 3, torch.randn(24, generator=g)
    y, hh, gg = sm.geglu64(proj, bias)
    p = proj.double() + bias.double()
    assert torch.equal(hh, p[:, :12]) and torch.equal(gg, p[:, 12:])
    assert float((y - hh * 0.5 * gg * (1 + torch.erf(gg * 0.5 ** 0.5))).abs().max()) <= 1e-14
    assert float(sm.geglu64(torch.tensor([[1.0, 1.0, -40.0, 40.0]]))[0].abs().max()) == 40.0  # saturated both ways
