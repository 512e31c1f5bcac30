#!/usr/bin/env python3
"""Times the trainable point refiner (PointTransformerV3(differentiable=True)) at the
reference's configuration -- the RendererConfig defaults, 8 clouds x 10 000 posed-body points, the 768-channel stem --
with HIP events (median of --iters): the inference forward, the differentiable forward, forward + backward and the peak
memory of a step; then each HIP operator's forward and backward on the network's own level-0 shapes (the stem
convolution, a block convolution, the patch attention, the pooling maximum) with the backward / forward ratio.  Prints one
JSON line per measurement.

    timeout -k 10 900 python tools/bench_refiner_backward.py [--clouds 8] [--points 10000] [--iters 5]

--train-mode measures the refiner's training function instead (batch_statistics=True, .train(), DESIGN.md section
4.18): forward + backward with the HIP BatchNorm kernels against AMAV_REFINER_BN=library, alternated round by round in
this one process, and each new kernel at the level-0 shape with its achieved bytes per second.

Per-kernel times come from a trace run of their own (one step, no event timing):

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_refiner_backward.py --once
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from audio_motion_avatar_amd import ops  # noqa: E402
from audio_motion_avatar_amd.config import RendererConfig  # noqa: E402
from audio_motion_avatar_amd.point_transformer import Level, PointTransformerV3, SubMConv3d  # noqa: E402

PCFG_KEYS = ("stride", "enc_depths", "enc_channels", "enc_num_head", "enc_patch_size", "dec_depths", "dec_channels",
             "dec_num_head", "dec_patch_size")


def timed(fn, iters):
    for _ in range(2):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return dict(median_ms=round(ms[len(ms) // 2], 3), min_ms=round(ms[0], 3))


def body_points(clouds, points):
    """Posed-body vertices of the configured body model, as the renderer hands them to the refiner."""
    from audio_motion_avatar_amd.renderer import Renderer
    from audio_motion_avatar_amd.synthetic import make_render_inputs

    cfg = RendererConfig(image_size=(64, 64), subdivide_steps=0, predict_smplx_params=False, num_gaussians=points,
                         device="cuda")
    r = Renderer(cfg).eval()
    _, smpl, _ = make_render_inputs(clouds, cfg, seed=42)
    with torch.no_grad():
        return ops.points_gather(r._posed_vertices(smpl), r._gather_idx).contiguous()


def network(rc):
    torch.manual_seed(0)
    net = PointTransformerV3(in_channels=3 * rc.triplane_feature_dim, differentiable=True,
                             **{k: tuple(getattr(rc, k)) for k in PCFG_KEYS}).eval()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_mean.normal_(0, 0.2)
                m.running_var.uniform_(0.5, 1.5)
    return net.cuda()


def ratio(res, fwd, bwd):
    res[bwd]["over_forward"] = round(res[bwd]["median_ms"] / max(res[fwd]["median_ms"], 1e-9), 2)


def network_bench(net, pts, feat, dout, iters):
    def forward_inference():
        with torch.no_grad():
            net(pts, feat)

    def step():
        net.zero_grad(set_to_none=True)
        x = feat.detach().requires_grad_()
        net(pts, x).backward(dout)

    res = dict(clouds=int(pts.shape[0]), points=int(pts.shape[1]), in_channels=int(feat.shape[2]), iters=iters)
    res["forward_inference"] = timed(forward_inference, iters)
    res["forward_differentiable"] = timed(lambda: net(pts, feat.detach().requires_grad_()), iters)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    res["forward_backward"] = timed(step, iters)
    res["peak_mem_gib"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
    res["backward_over_forward"] = round((res["forward_backward"]["median_ms"] - res["forward_differentiable"]["median_ms"])
                                         / res["forward_differentiable"]["median_ms"], 2)
    print(json.dumps(dict(kind="refiner_network", **res)), flush=True)


def operator_bench(rc, pts, feat, iters):
    Fc, N, _ = pts.shape
    n = Fc * N
    cloud_of = torch.arange(Fc, device="cuda", dtype=torch.int32).repeat_interleave(N)
    grid, depth = ops.cloud_voxelize(pts.reshape(n, 3), cloud_of, Fc)
    level = Level(grid, cloud_of, depth, np.full(Fc, N), ops.cloud_codes(grid, cloud_of, depth))
    g = torch.Generator().manual_seed(1)
    res = dict(clouds=Fc, points=N, iters=iters)
    C0 = rc.enc_channels[0]
    for name, cin, cout, k in (("stem_conv", feat.shape[2], C0, 5), ("block_conv", C0, C0, 3)):
        conv = SubMConv3d(cin, cout, k, bias=k == 3).cuda()
        x = (feat.reshape(n, -1) if k == 5 else torch.randn(n, cin, generator=g).cuda()).contiguous()
        dy = torch.randn(n, cout, generator=g).cuda()
        pairs = level.pairs(k)

        def backward(feat_grad):
            xg = x.detach().requires_grad_(feat_grad)
            conv.zero_grad(set_to_none=True)
            conv(xg, level, differentiable=True).backward(dy)

        with torch.no_grad():
            res[name + "_forward"] = timed(lambda: conv(x, level), iters)
        fwd = res[name + "_forward"]["median_ms"]
        for tag, feat_grad in (("_forward_backward", True), ("_forward_backward_weights_only", False)):
            t = timed(lambda: backward(feat_grad), iters)
            t["backward_over_forward"] = round((t["median_ms"] - fwd) / max(fwd, 1e-9), 2)
            res[name + tag] = t
        res[name + "_pairs"] = pairs.count
    heads, patch = rc.enc_num_head[0], rc.enc_patch_size[0]
    desc, max_patch = level.patches(patch)
    qkv = torch.randn(n, 3 * C0, generator=g).cuda()
    dy = torch.randn(n, C0, generator=g).cuda()
    out, lse = ops.patch_attention_lse(qkv, level.order[0], desc, heads, max_patch)
    res["attention_forward"] = timed(lambda: ops.patch_attention_lse(qkv, level.order[0], desc, heads, max_patch), iters)
    res["attention_backward"] = timed(
        lambda: ops.patch_attention_backward(qkv, level.order[0], desc, out, lse, dy, heads, max_patch), iters)
    ratio(res, "attention_forward", "attention_backward")
    _, _, seg = level.pool()
    C1 = rc.enc_channels[1]
    x = torch.randn(n, C1, generator=g).cuda()
    scale, shift = torch.rand(C1, generator=g).cuda() + 0.5, torch.randn(C1, generator=g).cuda()
    dy = torch.randn(seg.shape[0] - 1, C1, generator=g).cuda()
    res["cluster_max_forward"] = timed(lambda: ops.cluster_max(x, level.order[0], seg, scale, shift), iters)
    res["cluster_max_backward"] = timed(lambda: ops.cluster_max_backward(x, level.order[0], seg, scale, shift, dy), iters)
    ratio(res, "cluster_max_forward", "cluster_max_backward")
    res["cluster_sum"] = timed(lambda: ops.cluster_sum(x, level.order[0], seg), iters)
    print(json.dumps(dict(kind="refiner_operators", **res)), flush=True)


def train_mode_bench(rc, pts, feat, dout, iters, rounds=3):
    torch.manual_seed(0)
    net = PointTransformerV3(in_channels=3 * rc.triplane_feature_dim, differentiable=True, batch_statistics=True,
                             drop_path=0.0, **{k: tuple(getattr(rc, k)) for k in PCFG_KEYS}).cuda().train()

    def step():
        net.zero_grad(set_to_none=True)
        net(pts, feat.detach().requires_grad_()).backward(dout)

    res = dict(clouds=int(pts.shape[0]), points=int(pts.shape[1]), iters=iters, rounds=rounds, hip=[], library=[])
    for _ in range(rounds):  # A B A B ...: both sides see the same clocks and cache state
        for mode in ("hip", "library"):
            os.environ["AMAV_REFINER_BN"] = mode
            res[mode].append(timed(step, iters)["median_ms"])
    os.environ.pop("AMAV_REFINER_BN")
    res["hip_median_ms"], res["library_median_ms"] = (sorted(res[m])[rounds // 2] for m in ("hip", "library"))
    print(json.dumps(dict(kind="refiner_train_mode", **res)), flush=True)

    n, C = pts.shape[0] * pts.shape[1], rc.enc_channels[0]
    g = torch.Generator().manual_seed(3)
    x, dy = torch.randn(n, C, generator=g).cuda(), torch.randn(n, C, generator=g).cuda()
    w, b = torch.rand(C, generator=g).cuda() + 0.5, torch.randn(C, generator=g).cuda()
    mean, var = ops.bn_batch_stats(x)
    rstd = torch.rsqrt(var + 1e-3)
    cloud_of = torch.arange(pts.shape[0], device="cuda", dtype=torch.int32).repeat_interleave(pts.shape[1])
    grid, depth = ops.cloud_voxelize(pts.reshape(n, 3), cloud_of, pts.shape[0])
    level = Level(grid, cloud_of, depth, np.full(pts.shape[0], pts.shape[1]), ops.cloud_codes(grid, cloud_of, depth))
    _, _, seg = level.pool()
    m = seg.shape[0] - 1
    dm = torch.randn(m, C, generator=g).cuda()
    rows = n * C * 4
    ops_res = dict(rows=n, channels=C, clusters=m)
    for name, fn, nbytes in (
            ("bn_batch_stats", lambda: ops.bn_batch_stats(x), rows),
            ("bn_gelu_train_backward", lambda: ops.bn_gelu_train_backward(x, mean, rstd, w, b, dy), 5 * rows),
            ("cluster_max_raw", lambda: ops.cluster_max_raw(x, level.order[0], seg), rows + m * C * 4 + n * 8),
            ("cluster_max_route", lambda: ops.cluster_max_route(x, level.order[0], seg, dm), 2 * rows + m * C * 4 + n * 8)):
        t = timed(fn, max(iters, 20))
        t["floor_bytes"] = nbytes
        t["gb_per_s"] = round(nbytes / (t["median_ms"] * 1e-3) / 1e9, 1)
        ops_res[name] = t
    print(json.dumps(dict(kind="refiner_train_mode_operators", **ops_res)), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--clouds", type=int, default=8)
    ap.add_argument("--points", type=int, default=10000)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--once", action="store_true", help="one warm-up and one forward + backward step (for a kernel trace)")
    ap.add_argument("--train-mode", action="store_true", help="the batch-statistics training function, HIP against library")
    args = ap.parse_args()
    rc = RendererConfig()
    pts = body_points(args.clouds, args.points)
    net = network(rc)
    g = torch.Generator().manual_seed(2)
    feat = torch.randn(args.clouds, pts.shape[1], 3 * rc.triplane_feature_dim, generator=g).cuda()
    dout = torch.randn(args.clouds * pts.shape[1], net.out_channels, generator=g).cuda()
    if args.once:
        for _ in range(2):
            net.zero_grad(set_to_none=True)
            net(pts, feat.detach().requires_grad_()).backward(dout)
        torch.cuda.synchronize()
        return
    if args.train_mode:
        train_mode_bench(rc, pts, feat, dout, args.iters)
        return
    network_bench(net, pts, feat, dout, args.iters)
    operator_bench(rc, pts, feat, args.iters)


if __name__ == "__main__":
    main()
