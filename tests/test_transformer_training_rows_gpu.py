"""The transformer block under autograd on the fused row kernels (transformer.py, BasicTransformerBlock.forward's
fused-rows branch) at width 256, where add_layernorm_kernel is built: gradients of a block and of
a two-layer Transformer1D_nn against fp64 autograd of oracle.transformer on the CPU, the AMAV_TRAIN_ROWS=library way
back, and the peak memory of one block.  Bound: max |error| <= 1e-5 max |grad| per tensor, the bound
tests/test_audio_net_training_gpu.py::test_one_transformer_block uses at width 128."""
import functools
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-5
# one audio key: softmax over it is 1, so norm2 and attn2.to_q / to_k are outside the differentiable graph
DISCONNECTED = re.compile(r"(^|transformer_blocks\.\d+\.)(norm2|attn2\.to_q|attn2\.to_k)\.")


def randomize(module, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in module.named_parameters():
            if p.dim() > 1:
                p.copy_(torch.randn(p.shape, generator=g) * (0.5 / p.shape[-1] ** 0.5))
            else:
                p.copy_(torch.randn(p.shape, generator=g) * 0.1 + (1.0 if "norm" in name and "weight" in name else 0.0))


def _block():
    from audio_motion_avatar_amd.transformer import BasicTransformerBlock

    blk = BasicTransformerBlock(256, 4, 64, cross_attention_dim=48)
    randomize(blk, 3)
    g = torch.Generator().manual_seed(4)
    inputs = [torch.randn(2, 257, 256, generator=g), torch.randn(2, 1, 48, generator=g)]
    return blk, inputs, torch.randn(2, 257, 256, generator=g)


def _net():
    from audio_motion_avatar_amd.transformer import Transformer1D_nn

    net = Transformer1D_nn(4, 64, in_channels=32, num_layers=2, cross_attention_dim=48)
    randomize(net, 5)
    g = torch.Generator().manual_seed(6)
    inputs = [torch.randn(2, 32, 257, generator=g), torch.randn(2, 1, 48, generator=g)]
    return net, inputs, torch.randn(2, 32, 257, generator=g)


def _oracle(module, inputs, up, fn):
    """fp64 autograd of the functional oracle on the CPU -> (grads of parameters by name, grads of inputs)."""
    p64 = {"m." + k: v.detach().double().requires_grad_() for k, v in module.state_dict().items()}
    x64 = [x.double().requires_grad_() for x in inputs]
    fn(p64, *x64).backward(up.double())
    return {k[2:]: v.grad for k, v in p64.items()}, [x.grad for x in x64]


@functools.lru_cache(maxsize=None)
def block_reference():
    from oracle import transformer as o_tr

    blk, inputs, up = _block()
    return _oracle(blk, inputs, up, lambda p, h, e: o_tr.transformer_block(p, "m.", h, e, 4))


@functools.lru_cache(maxsize=None)
def net_reference():
    from oracle import transformer as o_tr

    net, inputs, up = _net()
    return _oracle(net, inputs, up, lambda p, h, e: o_tr.transformer1d(p, "m.", h, e, 2, 4))


def _compare(module, inputs, up, reference, label):
    module = module.cuda()
    xs = [x.cuda().requires_grad_() for x in inputs]
    module(*xs).backward(up.cuda())
    ref_p, ref_x = reference
    report = {}
    for k, p in module.named_parameters():
        if DISCONNECTED.search(k):
            assert p.grad is None, k
            continue
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
        report[k] = float((p.grad.cpu().double() - ref_p[k]).abs().max()) / max(float(ref_p[k].abs().max()), 1e-30)
    for i, (x, r) in enumerate(zip(xs, ref_x)):
        report[f"input{i}"] = float((x.grad.cpu().double() - r).abs().max()) / max(float(r.abs().max()), 1e-30)
    worst = max(report, key=report.get)
    print(f"trainrows| {label}: largest gradient error / max|grad| {report[worst]:.2e} ({worst}) = "
          f"{report[worst] / TOL:.3f} of the bound, {len(report)} tensors")
    assert report[worst] <= TOL, (worst, report[worst])
    return report


def _count_new_ops(monkeypatch):
    from audio_motion_avatar_amd import ops

    calls = {"add_layernorm": 0, "geglu": 0}
    real_ln, real_geglu = ops.add_layernorm_differentiable, ops.geglu_differentiable

    def ln(*a, **k):
        calls["add_layernorm"] += 1
        return real_ln(*a, **k)

    def geglu(*a, **k):
        calls["geglu"] += 1
        return real_geglu(*a, **k)

    monkeypatch.setattr(ops, "add_layernorm_differentiable", ln)
    monkeypatch.setattr(ops, "geglu_differentiable", geglu)
    return calls


def test_block_gradients_on_the_fused_rows(monkeypatch):
    monkeypatch.delenv("AMAV_TRAIN_ROWS", raising=False)
    calls = _count_new_ops(monkeypatch)
    blk, inputs, up = _block()
    _compare(blk, inputs, up, block_reference(), "block 256 fused rows")
    assert calls == {"add_layernorm": 2, "geglu": 1}  # the branch under test ran


def test_two_layer_transformer_gradients_on_the_fused_rows(monkeypatch):
    monkeypatch.delenv("AMAV_TRAIN_ROWS", raising=False)
    calls = _count_new_ops(monkeypatch)
    net, inputs, up = _net()
    _compare(net, inputs, up, net_reference(), "Transformer1D_nn 2 x 256 fused rows")
    assert calls == {"add_layernorm": 4, "geglu": 2}


def test_library_rows_take_no_new_op_and_give_the_same_gradients(monkeypatch):
    from audio_motion_avatar_amd import ops

    def refuse(*a, **k):
        raise AssertionError("AMAV_TRAIN_ROWS=library must not reach the fused row ops")

    monkeypatch.setenv("AMAV_TRAIN_ROWS", "library")
    monkeypatch.setattr(ops, "add_layernorm_differentiable", refuse)
    monkeypatch.setattr(ops, "geglu_differentiable", refuse)
    blk, inputs, up = _block()
    _compare(blk, inputs, up, block_reference(), "block 256 library rows")
    net, inputs, up = _net()
    _compare(net, inputs, up, net_reference(), "Transformer1D_nn 2 x 256 library rows")


def _peak_increment(blk, x, ctx, up):
    for _ in range(2):  # the first pass warms the allocator and the GEMM workspaces
        for p in blk.parameters():
            p.grad = None
        x.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        blk(x, ctx).backward(up)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
    return peak


def test_fused_rows_lower_the_peak_memory_of_a_block(monkeypatch):
    """One block at [1, 1000, 512]: the fused rows keep proj instead of proj, gelu(gate) and the gated product's operands,
    so the peak-allocated increment over forward + backward is strictly below the library rows'."""
    from audio_motion_avatar_amd.transformer import BasicTransformerBlock

    blk = BasicTransformerBlock(512, 8, 64, cross_attention_dim=48)
    randomize(blk, 7)
    blk = blk.cuda()
    g = torch.Generator().manual_seed(8)
    x = torch.randn(1, 1000, 512, generator=g).cuda().requires_grad_()
    ctx, up = torch.randn(1, 1, 48, generator=g).cuda(), torch.randn(1, 1000, 512, generator=g).cuda()
    monkeypatch.setenv("AMAV_TRAIN_ROWS", "library")
    library = _peak_increment(blk, x, ctx, up)
    monkeypatch.delenv("AMAV_TRAIN_ROWS")
    fused = _peak_increment(blk, x, ctx, up)
    print(f"trainrows| block [1,1000,512] peak increment: fused {fused / 2 ** 20:.1f} MiB, library {library / 2 ** 20:.1f} MiB, "
          f"ratio {fused / library:.3f}")
    assert fused < library
