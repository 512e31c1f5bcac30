"""Gradient checkpointing of Transformer1D_nn on the MI355X: four layers at width 256, S = 1000, a single audio key, in
.train().  The checkpointed step recomputes every block's forward on the HIP Functions (self-attention, add + LayerNorm,
GEGLU); they are deterministic and keep no per-call state, so the recomputation repeats the forward and the gradients
are those of the plain step, at a lower peak memory.  Run for the fused rows and for AMAV_TRAIN_ROWS=library."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _net():
    from audio_motion_avatar_amd.transformer import Transformer1D_nn

    net = Transformer1D_nn(4, 64, in_channels=32, num_layers=4, cross_attention_dim=48, gradient_checkpointing=True)
    g = torch.Generator().manual_seed(9)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if p.dim() > 1:
                p.copy_(torch.randn(p.shape, generator=g) * (0.5 / p.shape[-1] ** 0.5))
            else:
                p.copy_(torch.randn(p.shape, generator=g) * 0.1 + (1.0 if "norm" in name and "weight" in name else 0.0))
    return net.cuda().train()


def _step(net, x, ctx, up, checkpointing):
    """-> (gradients by name, peak-allocated increment over forward + backward)"""
    net.gradient_checkpointing = checkpointing
    for p in net.parameters():
        p.grad = None
    x.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    net(x, ctx).backward(up)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    grads = {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}
    grads["input"] = x.grad.clone()
    return grads, peak


@pytest.mark.parametrize("rows", ["fused", "library"])
def test_checkpointed_step_gives_the_plain_gradients_at_a_lower_peak(rows, monkeypatch):
    if rows == "library":
        monkeypatch.setenv("AMAV_TRAIN_ROWS", "library")
    else:
        monkeypatch.delenv("AMAV_TRAIN_ROWS", raising=False)
    net = _net()
    g = torch.Generator().manual_seed(10)
    x = torch.randn(1, 32, 1000, generator=g).cuda().requires_grad_()
    ctx, up = torch.randn(1, 1, 48, generator=g).cuda(), torch.randn(1, 32, 1000, generator=g).cuda()
    _step(net, x, ctx, up, False)  # warms the allocator and the library's workspaces
    plain_a, peak_plain = _step(net, x, ctx, up, False)
    plain_b, _ = _step(net, x, ctx, up, False)
    ckpt, peak_ckpt = _step(net, x, ctx, up, True)
    assert set(ckpt) == set(plain_a) and len(plain_a) > 60
    worst = 0.0
    for k, ref in plain_a.items():
        noise = float((plain_b[k] - ref).abs().max())   # what two plain runs differ by in this process
        diff = float((ckpt[k] - ref).abs().max())
        if noise == 0.0:
            assert torch.equal(ckpt[k], ref), f"{k}: plain runs are bit-identical, the checkpointed run is {diff:.3e} off"
        else:
            worst = max(worst, diff / noise)
            assert diff <= 4.0 * noise, f"{k}: checkpointed {diff:.3e} vs run-to-run {noise:.3e}"
    identical = sum(torch.equal(plain_b[k], plain_a[k]) for k in plain_a)
    print(f"checkpoint| {rows} rows: {identical} of {len(plain_a)} gradients bit-identical between plain runs, worst "
          f"checkpointed / run-to-run elsewhere {worst:.2f}; peak increment checkpointed {peak_ckpt / 2 ** 20:.1f} MiB, "
          f"plain {peak_plain / 2 ** 20:.1f} MiB, ratio {peak_ckpt / peak_plain:.3f}")
    assert peak_ckpt < peak_plain
