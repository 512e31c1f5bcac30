#!/usr/bin/env python3
"""Times the stage-1 encoder's HIP backwards (amav_cell_max_backward, amav_cell_mean_backward,
amav_points_project_backward) next to their forwards at the stage-1 shape -- the configured body's vertices plus its face
centres, C = 256, R = 32, 128 image-feature channels at 512^2 -- against their HBM byte floors (bytes that must move /
6.3 TB/s, the achievable stream rate), with HIP events (median of --iters).  Then a full stage-1 training step
(TriplaneGaussianAvatar.training_step forward + backward, with a test view) at the reference's widths and its peak
memory, for each --frames count.  Prints one JSON line per measurement.

    timeout -k 10 600 python tools/bench_stage1_backward.py [--frames 1 4] [--iters 20]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from audio_motion_avatar_amd import ops  # noqa: E402

HBM_BYTES_PER_MS = 6.3e9  # 6.3 TB/s


def timed(fn, iters):
    for _ in range(3):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return dict(median_ms=round(ms[len(ms) // 2], 4), min_ms=round(ms[0], 4))


def floor_ms(nbytes):
    return round(nbytes / HBM_BYTES_PER_MS, 4)


def ops_bench(iters, frames):
    from audio_motion_avatar_amd.config import Stage1Config
    from audio_motion_avatar_amd.synthetic import make_render_inputs
    from audio_motion_avatar_amd.triplane_net import POINT_RADIUS_NDC, SMPLXTriplaneEncoder

    cfg = Stage1Config(subdivide_steps=0, device="cuda")
    enc = SMPLXTriplaneEncoder(cfg).cuda().eval()
    _, smpl, cam = make_render_inputs(frames, cfg, seed=3)
    with torch.no_grad():
        verts = enc.get_smplx_verts(smpl)
    B, N, _ = verts.shape
    C, R, Cimg, H, W = cfg.triplane_feature_dim, cfg.triplane_resolution, 128, 512, 512
    cells = R * R
    g = torch.Generator().manual_seed(0)
    cell_of = enc.cell_indices(verts)
    segs = ops.cell_segments(cell_of, cells)
    seg1 = (segs[0][:, 1].contiguous(), segs[1][:, 1].contiguous())
    feat = torch.randn(B, N, C, generator=g).cuda()
    dout = torch.randn(B, N, C, generator=g).cuda()
    dplane = torch.randn(B, C, cells, generator=g).cuda()
    img = torch.randn(B, Cimg, H, W, generator=g).cuda()
    pts = (verts + smpl["transl"].reshape(B, 1, 3)).contiguous()
    E, K = cam["extrinsic"].reshape(B, 4, 4), cam["intrinsic"].reshape(B, 3, 3)
    radius = POINT_RADIUS_NDC * min(H, W) / 2.0
    out, ws = ops._points_project(pts, E, K, img, radius)
    dproj = torch.randn(B, N, Cimg, generator=g).cuda()
    f32, i32 = 4, 4
    rows = B * N * C * f32
    res = dict(frames=B, points=N, channels=C, resolution=R, image=[Cimg, H, W], iters=iters)
    res["pool_forward"] = timed(lambda: ops.cell_pool_max(feat, cell_of, cells, segs), iters)
    # pool backward: feat + dout in, dfeat out; plus the indices (order, cell_of: 3 planes each)
    res["pool_backward"] = timed(lambda: ops.cell_pool_max_backward(feat, cell_of, cells, segs, dout), iters)
    res["pool_backward"]["floor_ms"] = floor_ms(3 * rows + 2 * 3 * B * N * i32)
    res["mean_forward"] = timed(lambda: ops.cell_splat_mean(feat, cell_of[:, 1].contiguous(), cells, seg1), iters)
    # mean backward (one plane): dplane in, dfeat out, order
    res["mean_backward"] = timed(lambda: ops.cell_splat_mean_backward(dplane, cells, seg1, N), iters)
    res["mean_backward"]["floor_ms"] = floor_ms(rows + B * C * cells * f32 + B * N * i32)
    res["project_forward"] = timed(lambda: ops.points_project(pts, E, K, img, radius), iters)
    # projection backward: the z-buffer in, the [B,C,H,W] gradient out (the won rows of dout are a fraction of it)
    res["project_backward"] = timed(lambda: ops.points_project_backward(dproj, ws, H, W), iters)
    res["project_backward"]["floor_ms"] = floor_ms(B * H * W * (8 + Cimg * f32))
    for k in ("pool_backward", "mean_backward", "project_backward"):
        res[k]["over_floor"] = round(res[k]["median_ms"] / max(res[k]["floor_ms"], 1e-9), 2)
    print(json.dumps(dict(kind="stage1_backward_ops", **res)), flush=True)


def step_bench(iters, frames):
    from audio_motion_avatar_amd.config import Stage1Config
    from audio_motion_avatar_amd.synthetic import init_random_heads, make_render_inputs
    from audio_motion_avatar_amd.triplane_net import TriplaneGaussianAvatar

    cfg = Stage1Config(subdivide_steps=0, device="cuda")
    torch.manual_seed(0)
    model = TriplaneGaussianAvatar(cfg).eval()
    init_random_heads(model.renderer)
    with torch.no_grad():
        for blk in model.smplx_triplane_encoder.blocks:
            blk.fc_1.weight.normal_(0, 0.02)
    H, W = cfg.image_size
    _, smpl, cam = make_render_inputs(frames, cfg, seed=5)
    _, _, test_cam = make_render_inputs(frames, cfg, seed=6)
    g = torch.Generator().manual_seed(1)
    ref = torch.rand(1, frames, 3, H, W, generator=g).cuda()
    test = torch.rand(1, frames, 3, H, W, generator=g).cuda()
    tokens = (torch.randn(1, frames, 4096, cfg.image_feature_dim, generator=g) * 0.5).cuda()

    def step():
        model.zero_grad(set_to_none=True)
        total, _ = model.training_step(ref, smpl, cam, tokens, test, test_cam)
        total.backward()

    step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t = timed(step, iters)
    peak = torch.cuda.max_memory_allocated()
    print(json.dumps(dict(kind="stage1_training_step", frames=frames, image=[H, W], iters=iters, **t,
                          peak_mem_gib=round(peak / 2 ** 30, 2))), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--step-iters", type=int, default=5)
    args = ap.parse_args()
    with torch.no_grad():
        ops_bench(args.iters, 1)
    for F in args.frames:
        step_bench(args.step_iters, F)


if __name__ == "__main__":
    main()
