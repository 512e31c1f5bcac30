"""The attention backward on fp16 x 2 split products (csrc/attention_backward_split.hip, arithmetic="split" /
AMAV_ATTN_BACKWARD=split) for self- and cross-attention, against fp64 autograd of the library's SDPA under the bounds of
test_attention_backward_gpu.py: per tensor, max |error| <= 1e-5 max |grad| (grad_errors' floor for dq and dk) and
<= 4 x (torch fp32 SDPA autograd's error) + 2e-6.  The peaked softmax (q x 10), where the exact-fp32 backward already
sits at 7.3e-6 (inherited from the forward's L), is held to the second condition only."""
import pytest
import torch

import cross_attention_cases as cc
import test_attention_backward_gpu as sb
import test_cross_attention_gpu as xg

pytestmark = pytest.mark.gpu

BOUND = sb.BOUND
D = 64


def _ops():
    from audio_motion_avatar_amd import ops

    return ops


def _check(err, err32, peaked=False):
    for e, e32 in zip(err, err32):
        if not peaked:
            assert e <= BOUND, (err, err32)
        assert e <= 4 * e32 + 2e-6, (err, err32)   # no worse than the library's fp32 backward


# ------------------------------------------------------------------------------------------------------ self-attention
# the 16-row MFMA step, the 32-row tile and the 128-row workgroup, from below, at and above
SELF_S = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257)


@pytest.mark.parametrize("B,H", [(1, 1), (2, 3)])
@pytest.mark.parametrize("S", SELF_S)
def test_self_gradients_match_fp64(S, B, H):
    ops, HD = _ops(), H * D
    qkv = sb.make_qkv(B, S, H, seed=S * 10 + H + B, pad=12)   # read through a padded row stride
    assert qkv.stride(1) == 3 * HD + 12
    dout = torch.randn(B, S, HD, generator=torch.Generator().manual_seed(S)).cuda()
    out, lse = ops.selfattn_lse(qkv, H)
    dest = torch.full((B, S, 3 * HD + 20), float("nan"), device="cuda")   # written with a padded row stride
    got = ops.selfattn_backward(qkv, out, lse, dout, H, grad_qkv=dest, arithmetic="split")
    assert got.data_ptr() == dest.data_ptr()
    assert torch.isnan(dest[..., 3 * HD:]).all()   # the padding stays untouched
    assert torch.isfinite(dest[..., :3 * HD]).all()
    _, _, ref = sb.fp64_reference(qkv, dout, H)
    _, _, ref32 = sb.fp64_reference(qkv, dout, H, torch.float32)
    err, err32 = sb.grad_errors(dest[..., :3 * HD], ref, HD, qkv, dout), sb.grad_errors(ref32, ref, HD, qkv, dout)
    print(f"split B={B} S={S} H={H}: dq/dk/dv error / max {['%.2e' % e for e in err]} (torch fp32 SDPA "
          f"{['%.2e' % e for e in err32]})")
    _check(err, err32)


@pytest.mark.parametrize("case", ["peaked", "uniform", "v_norms", "dout_1e3", "dout_1e-6"])
def test_self_gradients_across_magnitudes(case):
    ops = _ops()
    B, S, H = 1, 1000, 2
    qkv = sb.make_qkv(B, S, H, seed=7, **sb.MAGNITUDES.get(case, {}))
    dmul = {"dout_1e3": 1e3, "dout_1e-6": 1e-6}.get(case, 1.0)
    dout = torch.randn(B, S, H * D, generator=torch.Generator().manual_seed(8)).cuda() * dmul
    out, lse = ops.selfattn_lse(qkv, H)
    got = ops.selfattn_backward(qkv, out, lse, dout, H, arithmetic="split")
    exact = ops.selfattn_backward(qkv, out, lse, dout, H, arithmetic="f32")
    _, _, ref = sb.fp64_reference(qkv, dout, H)
    _, _, ref32 = sb.fp64_reference(qkv, dout, H, torch.float32)
    err, err32 = sb.grad_errors(got, ref, H * D, qkv, dout), sb.grad_errors(ref32, ref, H * D, qkv, dout)
    errx = sb.grad_errors(exact, ref, H * D, qkv, dout)
    print(f"split {case}: dq/dk/dv error / max {['%.2e' % e for e in err]} (exact fp32 products "
          f"{['%.2e' % e for e in errx]}, torch fp32 {['%.2e' % e for e in err32]})")
    assert torch.isfinite(got).all()
    if case == "uniform":   # q = 0: dk = scale dS^T q is exactly zero
        assert torch.equal(got[..., D * H:2 * D * H], torch.zeros_like(got[..., D * H:2 * D * H]))
    _check(err, err32, peaked=case == "peaked")


# ----------------------------------------------------------------------------------------------------- cross-attention
CROSS = [(B, Sq, Sk, 2) for (Sq, Sk) in ((1, 1), (1, 129), (33, 1), (80, 257), (130, 31)) for B in (1, 2)] + \
        [(1, 80, 4096, 8)]


@pytest.mark.parametrize("B,Sq,Sk,H", CROSS)
def test_cross_gradients_match_fp64(B, Sq, Sk, H):
    ops, HD = _ops(), H * D
    q, kv = xg.device_inputs(B, Sq, Sk, H)   # k | v read in place from one fused, row-padded projection
    dout = cc.grad_out(B, Sq, Sk, H).cuda()
    out, lse = ops.crossattn_lse(q, kv, H)
    dq_dest = torch.full((B, Sq, HD + 12), float("nan"), device="cuda")
    dkv_dest = torch.full((B, Sk, 2 * HD + 20), float("nan"), device="cuda")   # dk | dv written fused
    dq, dkv = ops.crossattn_backward(q, kv, out, lse, dout, H, grad_q=dq_dest, grad_kv=dkv_dest, arithmetic="split")
    assert dq.data_ptr() == dq_dest.data_ptr() and dkv.data_ptr() == dkv_dest.data_ptr()
    assert torch.isnan(dq_dest[..., HD:]).all() and torch.isnan(dkv_dest[..., 2 * HD:]).all()
    got = (dq_dest[..., :HD], dkv_dest[..., :2 * HD])
    assert all(bool(torch.isfinite(g).all()) for g in got)
    ref = xg.autograd_reference(q, kv, dout, H, torch.float64)
    ref32 = xg.autograd_reference(q, kv, dout, H, torch.float32)
    err, err32 = xg.grad_errors(got, ref, q, kv, dout, H), xg.grad_errors(ref32, ref, q, kv, dout, H)
    print(f"split cross B={B} Sq={Sq} Sk={Sk} H={H}: dq/dk/dv error / max {['%.2e' % e for e in err]} (torch fp32 "
          f"SDPA {['%.2e' % e for e in err32]})")
    _check(err, err32)


# --------------------------------------------------------------------------------------------------------- determinism
def _self_case(B, S, H, seed, pad=0):
    qkv = sb.make_qkv(B, S, H, seed=seed, pad=pad)
    dout = torch.randn(B, S, H * D, generator=torch.Generator().manual_seed(seed + 1)).cuda()
    out, lse = _ops().selfattn_lse(qkv, H)
    return qkv, out, lse, dout


def test_two_calls_agree_bitwise():
    """Fixed-order sums and an order-independent (integer max) reduction of the operand scales.  A batch of two is NOT
    compared with two single calls: the scales are measured per call."""
    ops = _ops()
    qkv, out, lse, dout = _self_case(2, 1000, 3, seed=3)
    g1 = ops.selfattn_backward(qkv, out, lse, dout, 3, arithmetic="split")
    g2 = ops.selfattn_backward(qkv, out, lse, dout, 3, arithmetic="split")
    assert torch.equal(g1, g2)
    B, Sq, Sk, H = 2, 200, 1030, 3
    q, kv = xg.device_inputs(B, Sq, Sk, H)
    dout = cc.grad_out(B, Sq, Sk, H).cuda()
    out, lse = ops.crossattn_lse(q, kv, H)
    a = ops.crossattn_backward(q, kv, out, lse, dout, H, arithmetic="split")
    b = ops.crossattn_backward(q, kv, out, lse, dout, H, arithmetic="split")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_strided_and_contiguous_qkv_agree_bitwise():
    ops, H = _ops(), 8
    qkv, out, lse, dout = _self_case(1, 65, H, seed=9, pad=36)
    contig = qkv.contiguous()
    assert qkv.stride(1) != contig.stride(1)
    a = ops.selfattn_backward(qkv, out, lse, dout, H, arithmetic="split")
    b = ops.selfattn_backward(contig, out, lse, dout, H, arithmetic="split")
    assert torch.equal(a, b)


def test_zero_dout_gives_positive_zero_gradients():
    ops, H = _ops(), 2
    qkv, out, lse, _ = _self_case(1, 129, H, seed=5)
    g = ops.selfattn_backward(qkv, out, lse, torch.zeros(1, 129, H * D, device="cuda"), H, arithmetic="split")
    assert torch.equal(g, torch.zeros_like(g)) and not torch.signbit(g).any()
    B, Sq, Sk, H = 1, 129, 200, 3
    q, kv = xg.device_inputs(B, Sq, Sk, H)
    out, lse = ops.crossattn_lse(q, kv, H)
    for g in ops.crossattn_backward(q, kv, out, lse, torch.zeros(B, Sq, H * D, device="cuda"), H, arithmetic="split"):
        assert torch.equal(g, torch.zeros_like(g)) and not torch.signbit(g).any()


# ------------------------------------------------------------------------------------------------------------- routing
def _autograd_self(qkv, dout, H):
    x = qkv.detach().contiguous().requires_grad_()
    _ops().selfattn_differentiable(x, H).backward(dout)
    return x.grad


def _autograd_cross(q, kv, dout, H):
    x, y = q.detach().contiguous().requires_grad_(), kv.detach().contiguous().requires_grad_()
    _ops().crossattn_differentiable(x, y, H).backward(dout)
    return x.grad, y.grad


def test_environment_switch_routes_autograd(monkeypatch):
    ops, H = _ops(), 2
    qkv, out, lse, dout = _self_case(2, 100, H, seed=11)
    qkv = qkv.contiguous()
    B, Sq, Sk = 2, 80, 257
    q, kv = (t.contiguous() for t in xg.device_inputs(B, Sq, Sk, H))
    xdout = cc.grad_out(B, Sq, Sk, H).cuda()
    xout, xlse = ops.crossattn_lse(q, kv, H)
    want = {a: (ops.selfattn_backward(qkv, out, lse, dout, H, arithmetic=a),
                ops.crossattn_backward(q, kv, xout, xlse, xdout, H, arithmetic=a)) for a in ("f32", "split")}
    assert not torch.equal(want["f32"][0], want["split"][0])   # two arithmetics, not one kernel under two names

    monkeypatch.setenv("AMAV_ATTN_BACKWARD", "split")
    assert torch.equal(_autograd_self(qkv, dout, H), want["split"][0])
    dq, dkv = _autograd_cross(q, kv, xdout, H)
    assert torch.equal(dq, want["split"][1][0]) and torch.equal(dkv, want["split"][1][1])
    assert torch.equal(ops.selfattn_backward(qkv, out, lse, dout, H), want["split"][0])
    assert torch.equal(ops.selfattn_backward(qkv, out, lse, dout, H, arithmetic="f32"), want["f32"][0])

    monkeypatch.delenv("AMAV_ATTN_BACKWARD")
    assert torch.equal(_autograd_self(qkv, dout, H), want["f32"][0])
    dq, dkv = _autograd_cross(q, kv, xdout, H)
    assert torch.equal(dq, want["f32"][1][0]) and torch.equal(dkv, want["f32"][1][1])

    from audio_motion_avatar_amd._lib import AmavError
    monkeypatch.setenv("AMAV_ATTN_BACKWARD", "fp16")
    with pytest.raises(AmavError, match="AMAV_ATTN_BACKWARD"):
        ops.selfattn_backward(qkv, out, lse, dout, H)
    with pytest.raises(AmavError, match="AMAV_ATTN_BACKWARD"):
        ops.crossattn_backward(q, kv, xout, xlse, xdout, H)
    monkeypatch.delenv("AMAV_ATTN_BACKWARD")
    with pytest.raises(AmavError, match="arithmetic"):
        ops.selfattn_backward(qkv, out, lse, dout, H, arithmetic="bf16")
    with pytest.raises(AmavError, match="arithmetic"):
        ops.crossattn_backward(q, kv, xout, xlse, xdout, H, arithmetic="")

    # each arithmetic is within BOUND of fp64, so the two are within 2 BOUND of each other in the same measure
    for e in sb.grad_errors(want["split"][0], want["f32"][0], H * D, qkv, dout):
        assert e <= 2 * BOUND
    for e in xg.grad_errors(want["split"][1], want["f32"][1], q, kv, xdout, H):
        assert e <= 2 * BOUND


# ------------------------------------------------------------------------------------------------------- graph capture
def _capture(fn):
    """fn() captured into a HIP graph on a side stream, as test_properties_gpu.py captures other entry points."""
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            out = fn()
    torch.cuda.current_stream().wait_stream(side)
    return graph, out


def test_split_backward_is_hip_graph_capturable():
    """The header clear is a kernel and the scales never leave the device: one amav_selfattn_backward_split call
    captures into a HIP graph and replays bit-identically, with an eager call of the same entry point in between."""
    ops, H, S = _ops(), 2, 129
    qkv, out, lse, dout = _self_case(1, S, H, seed=13)
    call = lambda: ops.selfattn_backward(qkv, out, lse, dout, H, arithmetic="split")
    with torch.no_grad():
        eager = call().clone()
        torch.cuda.synchronize()
        graph, got = _capture(call)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(got, eager)
        got.zero_()
        again = call().clone()   # eager call of the same entry point between two replays
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(got, eager) and torch.equal(again, eager)
