"""The point refiner's opt-in training function (PointTransformerV3(batch_statistics=True) in .train(); DESIGN.md section
4.18): BatchNorm with batch statistics at all 13 sites, running-buffer updates, DropPath -- against oracle/ptv3.py with
its BatchNorm swapped for F.batch_norm(training=True) inside the test, in fp64 on the CPU.

Bound per tensor, the project's yardstick (tests/test_point_refiner_backward_gpu.py):
    max|got - ref64| <= max(4 * err32, 2e-5 * max|ref64|),   err32 = max|ref32 - ref64| of the oracle run in fp32."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

PCFG = dict(stride=(2, 2), enc_depths=(1, 1, 1), enc_channels=(32, 64, 128), enc_num_head=(2, 4, 4),
            enc_patch_size=(256, 256, 256), dec_depths=(1, 1), dec_channels=(64, 64), dec_num_head=(1, 2),
            dec_patch_size=(256, 256))
IN_CHANNELS = 48


def _mods():
    from audio_motion_avatar_amd import ops, point_transformer

    return ops, point_transformer


def _clouds(seed, Fc, N, extent=(0.3, 0.5, 0.2)):
    g = torch.Generator().manual_seed(seed)
    d = F.normalize(torch.randn(Fc, N, 3, generator=g), dim=-1)
    pts = d * torch.tensor(extent) * (1.0 + 0.05 * torch.randn(Fc, N, 1, generator=g))
    pts[:, N - N // 8:] = pts[:, : N // 8] + 0.002 * torch.randn(Fc, N // 8, 3, generator=g)  # shared voxels
    return pts + torch.randn(Fc, 1, 3, generator=g) * 0.3


def _check(name, got, g64, g32):
    g64 = g64.double()
    err = float((got.detach().cpu().double() - g64).abs().max())
    err32 = float((g32.double() - g64).abs().max())
    big = float(g64.abs().max())
    bound = max(4 * err32, 2e-5 * big)
    print(f"{name}: err {err:.3e}  err32 {err32:.3e}  max|g64| {big:.3e}  err/bound {err / max(bound, 1e-300):.3f}")
    assert err <= bound, (name, err, err32, big)
    return err / max(bound, 1e-300)


def _network(batch_statistics=True, drop_path=0.0, differentiable=True):
    _, pt = _mods()
    torch.manual_seed(0)
    net = pt.PointTransformerV3(in_channels=IN_CHANNELS, differentiable=differentiable, drop_path=drop_path,
                                batch_statistics=batch_statistics, **PCFG).eval()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_mean.normal_(0, 0.2)
                m.running_var.uniform_(0.5, 1.5)
    return net


def _bns(net):
    return {k: m for k, m in net.named_modules() if isinstance(m, torch.nn.BatchNorm1d)}


def _inputs(Fc, N):
    pts = _clouds(41, Fc, N)
    feat = torch.randn(Fc, N, IN_CHANNELS, generator=torch.Generator().manual_seed(42))
    dout = torch.randn(Fc * N, PCFG["dec_channels"][0], generator=torch.Generator().manual_seed(43))
    return pts, feat, dout


def _hip_grads(net, pts, feat, dout):
    net.zero_grad(set_to_none=True)
    x = feat.cuda().requires_grad_()
    out = net(pts.cuda(), x)
    out.backward(dout.cuda())
    return out.detach(), {k: v.grad.clone() for k, v in net.named_parameters()}, x.grad


def _oracle_train(monkeypatch_setattr, net, pts, feat, dout, dtype):
    """oracle.ptv3.ptv3_cloud with its `_bn` swapped for train-mode batch_norm on the same parameter dict
    -> (out, {name: grad}, d feat, {bn prefix: (batch mean, unbiased variance)})."""
    from oracle import ptv3 as o_pt

    stats = {}

    def bn_train(p, prefix, x, eps=1e-3):
        assert x.shape[0] >= 2, (prefix, x.shape)  # the deepest level keeps at least 2 voxels
        var, mean = torch.var_mean(x.detach(), 0, unbiased=True)
        stats[prefix] = (mean, var)
        return F.batch_norm(x, None, None, p[prefix + "weight"], p[prefix + "bias"], True, 0.0, eps)

    monkeypatch_setattr(o_pt, "_bn", bn_train)
    cfg = {k: list(PCFG[k]) for k in ("enc_depths", "enc_num_head", "enc_patch_size", "dec_depths", "dec_num_head",
                                      "dec_patch_size")}
    names = {k for k, _ in net.named_parameters()}
    p = {k: v.detach().cpu().to(dtype).requires_grad_(k in names) for k, v in net.state_dict().items()
         if v.is_floating_point()}
    x = feat.detach().clone().to(dtype).requires_grad_()
    out = o_pt.ptv3_cloud(p, "", o_pt.frame_grid(pts), x, cfg)
    out.backward(dout.to(dtype))
    return out.detach(), {k: p[k].grad for k in names}, x.grad, stats


_REFERENCE = {}


def _reference(monkeypatch):
    """The fp64 reference and the fp32 yardstick of the 700-point case, computed once for the module."""
    if not _REFERENCE:
        net = _network()
        pts, feat, dout = _inputs(1, 700)
        _REFERENCE["r"] = tuple(_oracle_train(monkeypatch.setattr, net, pts[0], feat[0], dout, t)
                                for t in (torch.float64, torch.float32))
    return _REFERENCE["r"]


def test_eval_is_unchanged():
    pts, feat, dout = _inputs(1, 700)
    off = _network(batch_statistics=False).cuda()
    want = _hip_grads(off, pts, feat, dout)
    on = _network(batch_statistics=True, drop_path=0.3).cuda().eval()
    before = {k: (m.running_mean.clone(), m.running_var.clone()) for k, m in _bns(on).items()}
    got = _hip_grads(on, pts, feat, dout)
    off_train = _hip_grads(off.train(), pts, feat, dout)  # the flag off: .train() changes nothing
    for other in (got, off_train):
        assert torch.equal(other[0], want[0]) and torch.equal(other[2], want[2])
        for k in want[1]:
            assert torch.equal(other[1][k], want[1][k]), k
    for k, m in _bns(on).items():  # .eval(): the buffers do not move
        assert torch.equal(m.running_mean, before[k][0]) and torch.equal(m.running_var, before[k][1])
        assert int(m.num_batches_tracked) == 0


def test_train_mode_matches_the_fp64_oracle(monkeypatch):
    (o64, p64, f64, _), (o32, p32, f32, _) = _reference(monkeypatch)
    net = _network().cuda().train()
    assert len(p64) == len(list(net.named_parameters())) > 100
    pts, feat, dout = _inputs(1, 700)
    out, grads, dfeat = _hip_grads(net, pts, feat, dout)
    worst = _check("forward", out, o64, o32)
    worst = max([worst] + [_check(k, grads[k], p64[k], p32[k]) for k in sorted(p64)])
    worst = max(worst, _check("d feat", dfeat[0], f64, f32))
    print(f"worst err / bound: {worst:.3f}")


def test_buffers_after_one_train_forward(monkeypatch):
    (_, _, _, s64), (_, _, _, s32) = _reference(monkeypatch)
    net = _network().cuda().train()
    bns = _bns(net)
    assert len(bns) == len(s64) == 1 + 2 + 2 * 2  # stem, poolings, both branches of the unpoolings (13 at five stages)
    old = {k: (m.running_mean.cpu().double(), m.running_var.cpu().double()) for k, m in bns.items()}
    pts, feat, dout = _inputs(1, 700)
    with torch.no_grad():
        net(pts.cuda(), feat.cuda())
    for k, m in bns.items():
        mom = m.momentum
        for i, (name, got) in enumerate((("running_mean", m.running_mean), ("running_var", m.running_var))):
            want64 = (1 - mom) * old[k][i] + mom * s64[k + "."][i]
            want32 = (1 - mom) * old[k][i] + mom * s32[k + "."][i].double()
            _check(f"{k}.{name}", got, want64, want32.float())
        assert int(m.num_batches_tracked) == 1, k
    net.eval()
    before = {k: (m.running_mean.clone(), m.running_var.clone()) for k, m in bns.items()}
    with torch.no_grad():
        net(pts.cuda(), feat.cuda())
    for k, m in bns.items():
        assert torch.equal(m.running_mean, before[k][0]) and torch.equal(m.running_var, before[k][1])
        assert int(m.num_batches_tracked) == 1


def test_a_statistic_is_over_every_cloud_of_the_call():
    _, pt = _mods()
    pts, feat, _ = _inputs(2, 420)

    def stem_mean(run):
        net = _network().cuda().train()
        net.embedding.stem.norm.momentum = 1.0
        with torch.no_grad():
            run(net)
        return net.embedding.stem.norm.running_mean.cpu().double()

    a = stem_mean(lambda net: net(pts[:1].cuda(), feat[:1].cuda()))
    b = stem_mean(lambda net: net(pts[1:].cuda(), feat[1:].cuda()))
    both = stem_mean(lambda net: net(pts.cuda(), feat.cuda()))
    scale = float(torch.maximum(a.abs(), b.abs()).max())
    assert float((both - (a + b) / 2).abs().max()) <= 2e-5 * scale
    assert float((both - a).abs().max()) > 1e-3 * scale and float((both - b).abs().max()) > 1e-3 * scale

    cfg = SimpleNamespace(input_dim=IN_CHANNELS, refiner_clouds_per_pass=1, refiner_batch_statistics=True,
                          differentiable_refiner=True, **PCFG)
    torch.manual_seed(0)
    enc = pt.PTv3Encoder(cfg).cuda().train()
    enc.point_transformer.embedding.stem.norm.momentum = 1.0
    enc.point_transformer.load_state_dict(_network().state_dict())
    with torch.no_grad():
        enc(pts.cuda(), feat.cuda())
    stem = enc.point_transformer.embedding.stem.norm
    assert int(stem.num_batches_tracked) == 1  # one pass
    assert float((stem.running_mean.cpu().double() - both).abs().max()) <= 2e-5 * scale


def test_one_pooled_row_is_refused_by_name():
    """A level whose pooling leaves one row: AmavError naming the level, raised before any BatchNorm kernel runs (the
    pooling module is called on a level of 8 points that share one voxel)."""
    from audio_motion_avatar_amd._lib import AmavError

    ops, pt = _mods()
    net = _network().cuda().train()
    pts = (0.001 * torch.rand(8, 3, generator=torch.Generator().manual_seed(1))).cuda()
    cloud_of = torch.zeros(8, dtype=torch.int32).cuda()
    grid, depth = ops.cloud_voxelize(pts, cloud_of, 1)
    level = pt.Level(grid, cloud_of, depth, np.full(1, 8), ops.cloud_codes(grid, cloud_of, depth))
    down = net.enc.enc2.down
    with pytest.raises(AmavError, match="pooling into level 2: 1 pooled row"):
        down(torch.randn(8, 64).cuda(), level, True, True)
    assert int(down.norm[0].num_batches_tracked) == 0
    bn = net.embedding.stem.norm
    bn.momentum = None
    with pytest.raises(AmavError, match="momentum"):
        pt._bn_gelu_train(torch.randn(16, 32).cuda(), bn, "stem")


def test_drop_path_is_seeded_and_off_in_eval():
    pts, feat, dout = _inputs(1, 700)
    net = _network(drop_path=0.3).cuda().train()
    rates = [net.enc.enc0.block0.drop_path, net.enc.enc1.block0.drop_path, net.enc.enc2.block0.drop_path]
    assert rates == pytest.approx([0.0, 0.15, 0.3]) and net.dec.dec1.block0.drop_path == pytest.approx(0.3)

    def run(seed):
        net.drop_path_generator = torch.Generator(device="cuda").manual_seed(seed)
        return _hip_grads(net, pts, feat, dout)

    a, b, c = run(5), run(5), run(6)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and all(torch.equal(a[1][k], b[1][k]) for k in a[1])
    assert not torch.equal(a[0], c[0])
    plain = _network(drop_path=0.0).cuda().eval()
    want = _hip_grads(plain, pts, feat, dout)
    got = _hip_grads(_network(drop_path=0.3).cuda().eval(), pts, feat, dout)  # fresh: the runs above moved net's buffers
    assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2])
    assert all(torch.equal(got[1][k], want[1][k]) for k in want[1])


def _block_case():
    ops, pt = _mods()
    pts = _clouds(41, 1, 300)
    cloud_of = torch.zeros(300, dtype=torch.int32).cuda()
    grid, depth = ops.cloud_voxelize(pts.reshape(300, 3).cuda(), cloud_of, 1)
    level = pt.Level(grid, cloud_of, depth, np.full(1, 300), ops.cloud_codes(grid, cloud_of, depth))
    blk = _network().cuda().train().enc.enc0.block0
    blk.drop_path = 0.25
    feat = torch.randn(300, 32, generator=torch.Generator().manual_seed(9)).cuda()
    return pt, blk, level, feat, torch.Generator(device="cuda")


def test_a_block_that_drops_every_row_keeps_the_cpe_branch_only(monkeypatch):
    pt, blk, level, feat, gen = _block_case()
    monkeypatch.setattr(pt, "_drop_path_mask", lambda n, rate, generator: torch.zeros(n, 1, device="cuda"))
    out = blk(feat, level, differentiable=True, drop_generator=gen)
    want = feat + blk.cpe[2](blk.cpe[1](blk.cpe[0](feat, level, True)))
    assert torch.equal(out, want)
    out.sum().backward()
    for mod in (blk.attn, blk.mlp, blk.norm1, blk.norm2):
        for p in mod.parameters():
            assert p.grad is not None and torch.equal(p.grad, torch.zeros_like(p.grad))
    assert float(blk.cpe[1].weight.grad.abs().max()) > 0


def test_a_block_that_keeps_every_row_scales_both_branches(monkeypatch):
    pt, blk, level, feat, gen = _block_case()
    monkeypatch.setattr(pt, "_drop_path_mask", lambda n, rate, generator: torch.ones(n, 1, device="cuda"))
    with torch.no_grad():
        out = blk(feat, level, differentiable=True, drop_generator=gen)
        x = feat + blk.cpe[2](blk.cpe[1](blk.cpe[0](feat, level, True)))
        x = x + blk.attn(blk.norm1(x), level, True) / 0.75
        want = x + blk.mlp(blk.norm2(x)) / 0.75
        plain = blk(feat, level, differentiable=True)  # no generator: the present path
    assert float((out - want).abs().max()) <= 1e-6 * float(want.abs().max())
    assert float((out - plain).abs().max()) > 1e-3 * float(want.abs().max())


def test_train_mode_network_trains():
    """16 Adam steps (lr 1e-3) on the MSE to a fixed random target at N = 300, batch statistics on: the loss at least
    halves (test_network_trains' bar), the running buffers move, and a following .eval() forward is finite."""
    torch.manual_seed(0)
    _, pt = _mods()
    net = pt.PointTransformerV3(in_channels=IN_CHANNELS, differentiable=True, drop_path=0.0, batch_statistics=True,
                                **PCFG).cuda().train()
    pts, feat, target = (t.cuda() for t in _inputs(1, 300))
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    losses = []
    for _ in range(16):
        opt.zero_grad(set_to_none=True)
        loss = F.mse_loss(net(pts, feat), target)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print("losses:", " ".join(f"{v:.4f}" for v in losses))
    assert losses[-1] < 0.5 * losses[0], losses
    for k, m in _bns(net).items():
        assert int(m.num_batches_tracked) == 16
        assert float(m.running_mean.abs().max()) > 0 and float((m.running_var - 1).abs().max()) > 0, k
    with torch.no_grad():
        assert bool(torch.isfinite(net.eval()(pts, feat)).all())
