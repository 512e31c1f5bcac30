"""The self-attention backward (csrc/attention_backward.hip) and the forward's row log-sum-exp against fp64 autograd of
the library's SDPA, on the fused-qkv layout the transformer feeds them.  Bound: max |error| <= 1e-5 * max |grad| per
tensor (q, k, v separately)."""
import pytest
import torch
import torch.nn.functional as F

import attention_cases as ac

pytestmark = pytest.mark.gpu

BOUND = 1e-5


def make_qkv(B, S, H, seed, q_mul=1.0, v_norms=False, pad=0):
    """[B,S,3*H*64] (+ pad columns: the fused projection read through a row stride)."""
    g = torch.Generator().manual_seed(seed)
    HD = H * 64
    x = torch.randn(B, S, 3 * HD + pad, generator=g)
    x[..., :HD] *= q_mul
    if v_norms:  # rows of v with norms spread over six decades
        x[..., 2 * HD:3 * HD] *= 10.0 ** (torch.rand(B, S, 1, generator=g) * 6 - 3)
    return x.cuda()[..., :3 * HD]


def fp64_reference(qkv, dout, H, dtype=torch.float64):
    """(out, lse, dqkv) of softmax(q k^T / 8) v by torch autograd in `dtype`."""
    B, S, C = qkv.shape
    x = qkv.detach().to(dtype).requires_grad_()
    q, k, v = (t.reshape(B, S, H, 64).transpose(1, 2) for t in x.split(C // 3, -1))
    o = F.scaled_dot_product_attention(q, k, v)
    o.backward(dout.to(dtype).reshape(B, S, H, 64).transpose(1, 2))
    lse = torch.logsumexp((q.detach() @ k.detach().transpose(-1, -2)) * 0.125, dim=-1)
    return o.detach().transpose(1, 2).reshape(B, S, -1), lse, x.grad


def grad_errors(got, ref, HD, qkv, dout):
    """max |got - ref| / max |ref| for dq, dk, dv.  dq and dk are sums of scale * dS * (k or q) whose terms cancel
    (exactly, at S = 1: dS = P (dP - delta) = 0), so their normaliser has a floor of 1e-2 of the proven term bound
    scale * max|k or q| * |dS|max, |dS| <= 2 max_i |dO_i| max_j |v_j|."""
    H = HD // 64
    x = qkv.detach().double().unflatten(-1, (3, H, 64))
    norm_do = float(dout.double().unflatten(-1, (H, 64)).norm(dim=-1).max())
    norm_v = float(x[..., 2, :, :].norm(dim=-1).max())
    out = []
    for i in range(3):
        g, r = got[..., i * HD:(i + 1) * HD].double(), ref[..., i * HD:(i + 1) * HD].double()
        floor = 0.0 if i == 2 else 1e-2 * 0.125 * float(x[..., 1 - i, :, :].abs().max()) * 2 * norm_do * norm_v
        out.append(float((g - r).abs().max()) / max(float(r.abs().max()), floor, 1e-300))
    return out


def run(qkv, dout, H):
    from audio_motion_avatar_amd import ops

    out, lse = ops.selfattn_lse(qkv, H)
    return out, lse, ops.selfattn_backward(qkv, out, lse, dout, H)


SHAPES = [(B, S, H) for S in (1, 2, 31, 63, 64, 65, 129, 1000) for H in (1, 8) for B in (1, 2)] + \
         [(1, 6304, 8), (2, 6304, 1)]


@pytest.mark.parametrize("B,S,H", SHAPES)
def test_gradients_match_fp64(B, S, H):
    qkv = make_qkv(B, S, H, seed=S * 10 + H + B, pad=12)  # read through the fused-projection row stride (+ padding)
    HD = H * 64
    dout = torch.randn(B, S, HD, generator=torch.Generator().manual_seed(S)).cuda()
    from audio_motion_avatar_amd import ops

    out, lse = ops.selfattn_lse(qkv, H)
    dest = torch.full((B, S, 3 * HD + 20), float("nan"), device="cuda")  # grads written with a padded row stride
    got = ops.selfattn_backward(qkv, out, lse, dout, H, grad_qkv=dest)
    assert torch.isnan(dest[..., 3 * HD:]).all()  # the padding stays untouched
    o64, lse64, ref = fp64_reference(qkv, dout, H)
    _, _, ref32 = fp64_reference(qkv, dout, H, torch.float32)
    err, err32 = grad_errors(got[..., :3 * HD], ref, HD, qkv, dout), grad_errors(ref32, ref, HD, qkv, dout)
    lse_err = float(((lse.double() - lse64).abs() / lse64.abs().clamp_min(1.0)).max())
    print(f"B={B} S={S} H={H}: dq/dk/dv error / max {['%.2e' % e for e in err]} (torch fp32 SDPA "
          f"{['%.2e' % e for e in err32]}); lse {lse_err:.2e}")
    assert lse_err <= 1e-6
    # the forward's output against the same fp64 reference: <= 4 x (CPU fp32 SDPA's error) + 2^-22 max |v|
    yard = ac.reference(ac.Case("qkv", *(t.cpu().contiguous() for t in qkv.split(HD, -1)), H))
    ac.check(out.cpu(), ac.Reference(o64.cpu(), yard.err32, yard.vmax), f"B={B} S={S} H={H}: out")
    assert torch.equal(out, ops.selfattn(qkv[..., :HD], qkv[..., HD:2 * HD], qkv[..., 2 * HD:], H))
    for e, e32 in zip(err, err32):
        assert e <= BOUND, (err, err32)
        assert e <= 4 * e32 + 2e-6, (err, err32)  # no worse than the library's fp32 backward


MAGNITUDES = {
    "peaked": dict(q_mul=10.0),      # near one-hot softmax rows
    "uniform": dict(q_mul=0.0),      # q = 0: every row the mean of v
    "v_norms": dict(v_norms=True),
}


@pytest.mark.parametrize("case", ["peaked", "uniform", "v_norms", "dout_1e3", "dout_1e-6"])
def test_gradients_across_magnitudes(case):
    B, S, H = 1, 1000, 2
    qkv = make_qkv(B, S, H, seed=7, **MAGNITUDES.get(case, {}))
    dmul = {"dout_1e3": 1e3, "dout_1e-6": 1e-6}.get(case, 1.0)
    dout = torch.randn(B, S, H * 64, generator=torch.Generator().manual_seed(8)).cuda() * dmul
    _, _, got = run(qkv, dout, H)
    _, _, ref = fp64_reference(qkv, dout, H)
    _, _, ref32 = fp64_reference(qkv, dout, H, torch.float32)
    err, err32 = grad_errors(got, ref, H * 64, qkv, dout), grad_errors(ref32, ref, H * 64, qkv, dout)
    print(f"{case}: dq/dk/dv error / max {['%.2e' % e for e in err]} (torch fp32 {['%.2e' % e for e in err32]})")
    if case == "uniform":  # q = 0: dk = scale dS^T q is exactly zero
        assert torch.equal(got[..., 64 * H:128 * H], torch.zeros_like(got[..., 64 * H:128 * H]))
    for e in err:
        assert e <= BOUND, err


def test_deterministic_and_batch_independent():
    H, S = 8, 1000
    qkv = make_qkv(2, S, H, seed=3)
    dout = torch.randn(2, S, H * 64, generator=torch.Generator().manual_seed(4)).cuda()
    out, lse, g1 = run(qkv, dout, H)
    from audio_motion_avatar_amd import ops

    g2 = ops.selfattn_backward(qkv, out, lse, dout, H)
    assert torch.equal(g1, g2)
    for b in range(2):  # the same forward state, one batch item at a time
        gb = ops.selfattn_backward(qkv[b:b + 1], out[b:b + 1], lse[b:b + 1], dout[b:b + 1], H)
        assert torch.equal(gb, g1[b:b + 1])


def test_zero_dout_gives_positive_zero_gradients():
    from audio_motion_avatar_amd import ops

    H, S = 2, 129
    qkv = make_qkv(1, S, H, seed=5)
    out, lse = ops.selfattn_lse(qkv, H)
    g = ops.selfattn_backward(qkv, out, lse, torch.zeros(1, S, H * 64, device="cuda"), H)
    assert torch.equal(g, torch.zeros_like(g)) and not torch.signbit(g).any()


def test_strided_and_contiguous_qkv_agree_bitwise():
    H, S = 8, 65
    strided = make_qkv(1, S, H, seed=9, pad=36)
    contig = strided.contiguous()
    assert strided.stride(1) != contig.stride(1)
    dout = torch.randn(1, S, H * 64, generator=torch.Generator().manual_seed(10)).cuda()
    a, b = run(strided, dout, H), run(contig, dout, H)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_autograd_function_matches_the_abi():
    from audio_motion_avatar_amd import ops

    H, S = 2, 100
    qkv = make_qkv(2, S, H, seed=11).contiguous().requires_grad_()
    dout = torch.randn(2, S, H * 64, generator=torch.Generator().manual_seed(12)).cuda()
    y = ops.selfattn_differentiable(qkv, H)
    y.backward(dout)
    _, _, g = run(qkv.detach(), dout, H)
    assert torch.equal(qkv.grad, g)
