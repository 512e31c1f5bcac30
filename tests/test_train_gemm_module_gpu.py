"""The transformer modules under autograd with AMAV_TRAIN_GEMM=split (transformer.train_linear):
gradients of the block and the two-layer Transformer1D_nn of test_transformer_training_rows_gpu.py (width 256, [2, 257, ...]:
514 rows, above the 256-row gate) and of many-key cross-attention against fp64 autograd on the CPU, with and without
gradient checkpointing, and the default setting left exactly where it was.  Bound: that file's 1e-5 max |grad| per
tensor."""
import copy

import pytest
import torch

from test_transformer_training_rows_gpu import TOL, _block, _compare, _net, block_reference, net_reference

pytestmark = pytest.mark.gpu


@pytest.fixture
def spy(monkeypatch):
    """Counts the calls of ops.linear_split_differentiable."""
    from audio_motion_avatar_amd import ops

    calls = []
    real = ops.linear_split_differentiable

    def counted(x, weight, *a, **k):
        calls.append((x.numel() // weight.shape[1], weight.shape[1], weight.shape[0]))
        return real(x, weight, *a, **k)

    monkeypatch.setattr(ops, "linear_split_differentiable", counted)
    return calls


def test_block_gradients_on_split_gemms(monkeypatch, spy):
    monkeypatch.setenv("AMAV_TRAIN_GEMM", "split")
    monkeypatch.delenv("AMAV_TRAIN_ROWS", raising=False)
    blk, inputs, up = _block()
    _compare(blk, inputs, up, block_reference(), "block 256 split GEMMs")
    # q|k|v, to_out, ff_in, ff_out; the single-key attn2 products have one row and stay on the library
    assert spy == [(514, 256, 768), (514, 256, 256), (514, 256, 2048), (514, 1024, 256)]


def test_two_layer_transformer_gradients_on_split_gemms(monkeypatch, spy):
    monkeypatch.setenv("AMAV_TRAIN_GEMM", "split")
    monkeypatch.delenv("AMAV_TRAIN_ROWS", raising=False)
    net, inputs, up = _net()
    _compare(net, inputs, up, net_reference(), "Transformer1D_nn 2 x 256 split GEMMs")
    assert len(spy) == 8


def test_checkpointed_transformer_gives_the_same_gradients(monkeypatch, spy):
    """.train() with gradient_checkpointing=True: every block's forward runs again in the backward (8 more calls, served
    by the memoised weight operands), and the gradients meet the same bound against fp64 and against the unchecked run."""
    monkeypatch.setenv("AMAV_TRAIN_GEMM", "split")
    monkeypatch.delenv("AMAV_TRAIN_ROWS", raising=False)
    net, inputs, up = _net()
    _compare(net, inputs, up, net_reference(), "Transformer1D_nn 2 x 256 split GEMMs, plain")
    plain = {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}
    assert len(spy) == 8
    net.zero_grad(set_to_none=True)
    net.train()
    net.gradient_checkpointing = True
    _compare(net, inputs, up, net_reference(), "Transformer1D_nn 2 x 256 split GEMMs, checkpointed")
    assert len(spy) == 8 + 16
    ckpt = {k: p.grad for k, p in net.named_parameters() if p.grad is not None}
    assert set(ckpt) == set(plain)
    for k, ref in plain.items():
        assert float((ckpt[k] - ref).abs().max()) <= TOL * float(ref.abs().max()), k


def _cross():
    from audio_motion_avatar_amd.transformer import Attention

    torch.manual_seed(11)
    attn = Attention(128, cross_attention_dim=96, heads=2, dim_head=64)
    g = torch.Generator().manual_seed(12)
    return attn, (torch.randn(1, 300, 128, generator=g), torch.randn(1, 260, 96, generator=g)), \
        torch.randn(1, 300, 128, generator=g)


def _cross_run(attn, inputs, up):
    xs = [x.detach().clone().requires_grad_() for x in inputs]
    attn.zero_grad(set_to_none=True)
    attn(*xs).backward(up)
    grads = {k: p.grad for k, p in attn.named_parameters()}
    grads["hidden"], grads["context"] = xs[0].grad, xs[1].grad
    return {k: v.detach().double().cpu() for k, v in grads.items()}


def test_cross_attention_gradients_on_split_gemms(monkeypatch, spy):
    """300 queries over 260 keys at dim_head 64 through Attention._forward_cross: to_q, the fused k | v projection and
    to_out are split products; the reference is fp64 SDPA autograd on the CPU."""
    attn, inputs, up = _cross()
    ref = _cross_run(copy.deepcopy(attn).double(), [x.double() for x in inputs], up.double())
    assert not spy
    monkeypatch.setenv("AMAV_TRAIN_GEMM", "split")
    monkeypatch.delenv("AMAV_CROSS_ATTN", raising=False)
    got = _cross_run(attn.cuda(), [x.cuda() for x in inputs], up.cuda())
    assert spy == [(300, 128, 128), (260, 96, 256), (300, 128, 128)]
    assert set(got) == set(ref)
    report = {k: float((got[k] - r).abs().max()) / float(r.abs().max()) for k, r in ref.items()}
    worst = max(report, key=report.get)
    print(f"traingemm| cross-attention 300 x 260: largest gradient error / max|grad| {report[worst]:.2e} ({worst}) = "
          f"{report[worst] / TOL:.3f} of the bound, {len(report)} tensors")
    assert report[worst] <= TOL, (worst, report[worst])


def test_default_is_f32_and_unchanged(monkeypatch, spy):
    """Unset and `f32` are the same path -- no split call, outputs and every gradient bit-identical."""
    monkeypatch.delenv("AMAV_TRAIN_ROWS", raising=False)
    blk, inputs, up = _block()
    blk = blk.cuda()

    def run():
        xs = [x.cuda().requires_grad_() for x in inputs]
        blk.zero_grad(set_to_none=True)
        y = blk(*xs)
        y.backward(up.cuda())
        grads = {k: p.grad.clone() for k, p in blk.named_parameters() if p.grad is not None}
        grads.update(out=y.detach(), input0=xs[0].grad, input1=xs[1].grad)
        return grads

    monkeypatch.delenv("AMAV_TRAIN_GEMM", raising=False)
    unset = run()
    monkeypatch.setenv("AMAV_TRAIN_GEMM", "f32")
    f32 = run()
    assert not spy
    assert set(unset) == set(f32)
    for k in unset:
        assert torch.equal(unset[k], f32[k]), k
