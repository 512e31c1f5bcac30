"""Cross-attention on the MI355X (amav_crossattn_forward / amav_crossattn_backward through ops.crossattn*): Sq queries
over Sk keys in either order, read through padded row strides.

Forward: against float64 CPU SDPA under attention_cases' bound, with the CPU's float32 SDPA as the yardstick
    error <= 4 err32 + 2^-22 max |v|     and     error <= 2e-5 max(1, max |ref|),
and the row log-sum-exp under check_lse.
Backward: against float64 autograd of the library's SDPA under test_attention_backward_gpu.py's bounds, per tensor
    error <= 1e-5 max |grad| (grad_errors' floor for dq and dk)     and     error <= 4 (torch fp32 SDPA autograd's) + 2e-6.
"""
import pytest
import torch
import torch.nn.functional as F

import cross_attention_cases as cc
import test_attention_backward_gpu as sb   # BOUND and make_qkv

pytestmark = pytest.mark.gpu

D = cc.D


def _ops():
    from audio_motion_avatar_amd import ops

    return ops


def _split(B, Sq, Sk, H):
    from audio_motion_avatar_amd import _lib

    return _lib.lib().amav_crossattn_key_split(B, Sq, Sk, H)


def device_inputs(B, Sq, Sk, H):
    """q and the fused kv on the device, as views of row-padded buffers (q: + 12 floats, kv: + 20)."""
    q, kv = cc.inputs(B, Sq, Sk, H)
    HD = H * D
    qb = torch.full((B, Sq, HD + cc.Q_PAD), float("nan"), device="cuda")
    kvb = torch.full((B, Sk, 2 * HD + cc.KV_PAD), float("nan"), device="cuda")
    qb[..., :HD], kvb[..., :2 * HD] = q.cuda(), kv.cuda()
    return qb[..., :HD], kvb[..., :2 * HD]


# ---------------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("B,Sq,Sk,H", cc.SHAPES)
def test_forward_matches_fp64(B, Sq, Sk, H):
    ops, HD = _ops(), H * D
    q, kv = device_inputs(B, Sq, Sk, H)
    assert q.stride(1) == HD + cc.Q_PAD and kv.stride(1) == 2 * HD + cc.KV_PAD
    ref = cc.reference(B, Sq, Sk, H)
    label = f"cross B={B} Sq={Sq} Sk={Sk} H={H} split={_split(B, Sq, Sk, H)}"
    out, lse = ops.crossattn_lse(q, kv, H)
    assert out.shape == (B, Sq, HD) and lse.shape == (B, H, Sq)
    cc.check(out.cpu(), ref, label)
    cc.check_lse(lse.cpu(), ref, label)
    assert torch.equal(ops.crossattn(q, kv[..., :HD], kv[..., HD:], H), out)   # with and without the lse


def test_key_splits_taken():
    """The partial-state merge runs for the long key sweeps and not for the small shapes."""
    for Sq, Sk in cc.SMALL:
        for B, H in cc.BH:
            assert _split(B, Sq, Sk, H) == 1, (B, Sq, Sk, H)
    assert _split(1, 5, 1030, 1) > 1 and _split(2, 5, 1030, 3) > 1
    assert _split(1, 80, 4096, 8) > 1
    assert _split(*cc.REFERENCE_SHAPE) > 1


def test_known_answer():
    """Query i selects key (i + 7) mod 200 among 200 keys, 150 queries: `out` is that row of an asymmetric v."""
    case, sel = cc.known_answer_case(Sq=150, Sk=200, shift=7)
    assert int(sel[0]) == 7 and int(sel[149]) == 156
    out = _ops().crossattn(case.q.cuda(), case.k.cuda(), case.v.cuda(), 1, scale=case.scale).cpu()
    expected = case.v[:, sel]
    ref = cc.ac.reference(case)
    assert float((ref.out64 - expected.double()).abs().max()) <= 1e-12 * float(case.v.max())   # the construction holds
    cc.check(out, ref, case.name)
    assert float((out - expected).abs().max()) <= ref.bound


def test_v_zero_gives_zero():
    B, Sq, Sk, H = 2, 129, 200, 3
    q, kv = device_inputs(B, Sq, Sk, H)
    kv = kv.clone()
    kv[..., H * D:] = 0.0
    out, lse = _ops().crossattn_lse(q, kv, H)
    assert torch.equal(out, torch.zeros_like(out))
    cc.check_lse(lse.cpu(), cc.reference(B, Sq, Sk, H), "v = 0")   # the lse does not depend on v


# ------------------------------------------------------------------------------------- equals self-attention, Sq = Sk
@pytest.mark.parametrize("S", [65, 1025])
@pytest.mark.parametrize("arithmetic", ["f32", "split"])
def test_equals_self_attention_bitwise(arithmetic, S):
    """Self-attention is cross-attention with Sq = Sk over the thirds of one fused row: the forward, and the backward in
    either arithmetic, run the same kernels on the same rows."""
    ops, B, H = _ops(), 2, 3
    HD = H * D
    qkv = sb.make_qkv(B, S, H, seed=S, pad=12)
    dout = torch.randn(B, S, HD, generator=torch.Generator().manual_seed(S + 1)).cuda()
    out_s, lse_s = ops.selfattn_lse(qkv, H)
    dqkv = ops.selfattn_backward(qkv, out_s, lse_s, dout, H, arithmetic=arithmetic)
    q, kv = qkv[..., :HD], qkv[..., HD:]
    out, lse = ops.crossattn_lse(q, kv, H)
    assert torch.equal(out, out_s) and torch.equal(lse, lse_s)
    assert torch.equal(ops.crossattn(q, kv[..., :HD], kv[..., HD:], H), out_s)
    dq, dkv = ops.crossattn_backward(q, kv, out, lse, dout, H, arithmetic=arithmetic)
    assert torch.equal(dq, dqkv[..., :HD])
    assert torch.equal(dkv[..., :HD], dqkv[..., HD:2 * HD]) and torch.equal(dkv[..., HD:], dqkv[..., 2 * HD:])


# ---------------------------------------------------------------------------------------------------------- backward
def autograd_reference(q, kv, dout, H, dtype):
    """(dq, dkv) of softmax(q k^T / 8) v by torch autograd of the library's SDPA in `dtype`, on the device."""
    B, Sq, HD = q.shape
    x, y = q.detach().to(dtype).requires_grad_(), kv.detach().to(dtype).requires_grad_()
    heads = lambda t: t.reshape(B, t.shape[1], H, D).transpose(1, 2)
    o = F.scaled_dot_product_attention(heads(x), heads(y[..., :HD]), heads(y[..., HD:]))
    o.backward(heads(dout.to(dtype)))
    return x.grad, y.grad


def grad_errors(got, ref, q, kv, dout, H):
    """test_attention_backward_gpu.grad_errors for two row sets: max |got - ref| / max |ref| for (dq, dk, dv); dq and dk
    are sums of scale * dS * (k or q) whose terms cancel (exactly, with one key: dS = P (dP - delta) = 0), so their
    normaliser has the same floor, 1e-2 of the proven term bound scale * max|k or q| * 2 max_i |dO_i| max_j |v_j|."""
    HD = H * D
    norm_do = float(dout.double().unflatten(-1, (H, D)).norm(dim=-1).max())
    norm_v = float(kv[..., HD:].double().unflatten(-1, (H, D)).norm(dim=-1).max())
    other = (float(kv[..., :HD].abs().max()), float(q.abs().max()))   # dq's terms carry k, dk's carry q
    pairs = ((got[0], ref[0]), (got[1][..., :HD], ref[1][..., :HD]), (got[1][..., HD:2 * HD], ref[1][..., HD:]))
    out = []
    for i, (g, r) in enumerate(pairs):
        floor = 0.0 if i == 2 else 1e-2 * 0.125 * other[i] * 2 * norm_do * norm_v
        out.append(float((g.double() - r.double()).abs().max()) / max(float(r.abs().max()), floor, 1e-300))
    return out


@pytest.mark.parametrize("B,Sq,Sk,H", cc.SHAPES)
def test_gradients_match_fp64(B, Sq, Sk, H):
    ops, HD = _ops(), H * D
    q, kv = device_inputs(B, Sq, Sk, H)
    dout = cc.grad_out(B, Sq, Sk, H).cuda()
    out, lse = ops.crossattn_lse(q, kv, H)
    dq_dest = torch.full((B, Sq, HD + 12), float("nan"), device="cuda")      # destinations with padded row strides
    dkv_dest = torch.full((B, Sk, 2 * HD + 20), float("nan"), device="cuda")
    dq, dkv = ops.crossattn_backward(q, kv, out, lse, dout, H, grad_q=dq_dest, grad_kv=dkv_dest)
    assert dq.data_ptr() == dq_dest.data_ptr() and dkv.data_ptr() == dkv_dest.data_ptr()
    assert torch.isnan(dq_dest[..., HD:]).all() and torch.isnan(dkv_dest[..., 2 * HD:]).all()   # the padding stays untouched
    got = (dq_dest[..., :HD], dkv_dest[..., :2 * HD])
    assert all(bool(torch.isfinite(g).all()) for g in got)
    ref = autograd_reference(q, kv, dout, H, torch.float64)
    ref32 = autograd_reference(q, kv, dout, H, torch.float32)
    err, err32 = grad_errors(got, ref, q, kv, dout, H), grad_errors(ref32, ref, q, kv, dout, H)
    print(f"cross B={B} Sq={Sq} Sk={Sk} H={H}: dq/dk/dv error / max {['%.2e' % e for e in err]} (torch fp32 SDPA "
          f"{['%.2e' % e for e in err32]})")
    for e, e32 in zip(err, err32):
        assert e <= sb.BOUND, (err, err32)
        assert e <= 4 * e32 + 2e-6, (err, err32)   # no worse than the library's fp32 backward


# -------------------------------------------------------------------------------------------------------- properties
def _run(q, kv, dout, H):
    ops = _ops()
    out, lse = ops.crossattn_lse(q, kv, H)
    return (out, lse) + ops.crossattn_backward(q, kv, out, lse, dout, H)


def test_deterministic_and_batch_independent():
    B, Sq, Sk, H = 2, 200, 1030, 3
    q, kv = device_inputs(B, Sq, Sk, H)
    dout = cc.grad_out(B, Sq, Sk, H).cuda()
    ops = _ops()
    out, lse, dq, dkv = _run(q, kv, dout, H)
    dq2, dkv2 = ops.crossattn_backward(q, kv, out, lse, dout, H)
    assert torch.equal(dq, dq2) and torch.equal(dkv, dkv2)
    for b in range(B):   # the same forward state, one batch item at a time
        dqb, dkvb = ops.crossattn_backward(q[b:b + 1], kv[b:b + 1], out[b:b + 1], lse[b:b + 1], dout[b:b + 1], H)
        assert torch.equal(dqb, dq[b:b + 1]) and torch.equal(dkvb, dkv[b:b + 1])


def test_strided_and_contiguous_inputs_agree_bitwise():
    B, Sq, Sk, H = 1, 129, 200, 3
    q, kv = device_inputs(B, Sq, Sk, H)
    dout = cc.grad_out(B, Sq, Sk, H).cuda()
    qc, kvc = q.contiguous(), kv.contiguous()
    assert q.stride(1) != qc.stride(1) and kv.stride(1) != kvc.stride(1)
    for x, y in zip(_run(q, kv, dout, H), _run(qc, kvc, dout, H)):
        assert torch.equal(x, y)


def test_zero_dout_gives_positive_zero_gradients():
    B, Sq, Sk, H = 1, 129, 200, 3
    q, kv = device_inputs(B, Sq, Sk, H)
    _, _, dq, dkv = _run(q, kv, torch.zeros(B, Sq, H * D, device="cuda"), H)
    for g in (dq, dkv):
        assert torch.equal(g, torch.zeros_like(g)) and not torch.signbit(g).any()


def test_autograd_function_matches_the_abi():
    B, Sq, Sk, H = 2, 100, 130, 3
    q, kv = (t.contiguous().requires_grad_() for t in device_inputs(B, Sq, Sk, H))
    dout = cc.grad_out(B, Sq, Sk, H).cuda()
    y = _ops().crossattn_differentiable(q, kv, H)
    y.backward(dout)
    out, _, dq, dkv = _run(q.detach(), kv.detach(), dout, H)
    assert torch.equal(y.detach(), out) and torch.equal(q.grad, dq) and torch.equal(kv.grad, dkv)
