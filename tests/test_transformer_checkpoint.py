"""Gradient checkpointing of Transformer1D_nn (src/models/transformers.py:1044-1056): in .train() with autograd every
block is called through torch.utils.checkpoint.checkpoint(..., use_reentrant=False), so it keeps its input only and its
forward runs a second time in the backward; everywhere else nothing changes.  CPU: width 128, the library path."""
from types import SimpleNamespace

import pytest
import torch

from helpers import ref_fixture, toy_body


def _net(checkpointing, seed=0):
    from audio_motion_avatar_amd.transformer import Transformer1D_nn

    torch.manual_seed(seed)
    net = Transformer1D_nn(2, 64, in_channels=32, num_layers=3, cross_attention_dim=16, gradient_checkpointing=checkpointing)
    with torch.no_grad():  # LayerNorm / GroupNorm start at (1, 0): move them so that every gradient path is exercised
        for p in net.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    return net


def _inputs():
    g = torch.Generator().manual_seed(3)
    return torch.randn(2, 32, 40, generator=g), torch.randn(2, 1, 16, generator=g), torch.randn(2, 32, 40, generator=g)


def _count_block_forwards(net):
    calls = [0] * len(net.transformer_blocks)

    def hook(index):
        def pre(module, args):
            calls[index] += 1
        return pre

    for i, block in enumerate(net.transformer_blocks):
        block.register_forward_pre_hook(hook(i))
    return calls


def _step(net, no_grad=False):
    x, ctx, up = _inputs()
    x.requires_grad_(not no_grad)
    if no_grad:
        with torch.no_grad():
            net(x, ctx)
        return None
    net(x, ctx).backward(up)
    return x.grad


@pytest.mark.parametrize("checkpointing, mode, no_grad, forwards", [
    (True, "train", False, 2), (True, "eval", False, 1), (False, "train", False, 1), (True, "train", True, 1)])
def test_blocks_run_twice_only_when_checkpointed(checkpointing, mode, no_grad, forwards):
    net = getattr(_net(checkpointing), mode)()
    assert net.gradient_checkpointing is checkpointing
    if no_grad:  # without autograd a block's self-attention is the HIP kernel alone: count calls of stand-in blocks
        for block in net.transformer_blocks:
            block.forward = lambda h, ctx: h
    calls = _count_block_forwards(net)
    _step(net, no_grad)
    assert calls == [forwards] * 3


def test_checkpointed_gradients_equal_the_plain_run_bit_for_bit():
    plain, ckpt = _net(False, seed=5).train(), _net(True, seed=5).train()
    gx_plain, gx_ckpt = _step(plain), _step(ckpt)
    assert torch.equal(gx_plain, gx_ckpt)
    grads = dict(ckpt.named_parameters())
    for name, p in plain.named_parameters():
        q = grads[name]
        assert (p.grad is None) == (q.grad is None), name
        if p.grad is not None:
            assert torch.equal(p.grad, q.grad), name
    assert sum(p.grad is not None for p in plain.parameters()) > 40


def test_stage1_transformers_are_built_with_checkpointing():
    """triplane_net.py:116,364 of the reference: both stage-1 transformers are constructed with the flag."""
    from audio_motion_avatar_amd.smplx_decoder import SMPLXDecoder
    from audio_motion_avatar_amd.triplane_net import FeatureFusionNetwork, SMPLXTriplaneEncoder

    _, meta, _ = ref_fixture("stage1")
    cfg = SimpleNamespace(**meta["cfg"])
    body = toy_body(**meta["toy_body"])

    class Encoder(SMPLXTriplaneEncoder):
        def init_smplx_model(self):
            return body

    assert Encoder(cfg, SMPLXDecoder(cfg)).cross_attn.gradient_checkpointing is True
    assert FeatureFusionNetwork(cfg).transformer_cross.gradient_checkpointing is True


def test_audio_net_transformer_is_built_with_checkpointing():
    from audio_motion_avatar_amd.config import AudioNetConfig, ModelConfig
    from audio_motion_avatar_amd.triplane_audio_net import AudioTriplaneNet

    a = AudioNetConfig(triplane_feature_dim=32, transformer_layers=1, transformer_num_heads=2, transformer_head_dim=64)
    assert AudioTriplaneNet(ModelConfig(triplane_audio_net=a), renderer=None).transformer.gradient_checkpointing is True
