#!/usr/bin/env python3
"""Stage-1 image-feature sampling, dense against grid, forward + backward under autograd:

  dense  ImageFeature.forward (Linear 1536 -> 125 on the 64 x 64 tokens, bilinear resize to the image, cat RGB) +
         ops.points_project_differentiable, then backward to the reducer's weights
  grid   ImageFeature.reduce + ops.points_project_grid_differentiable, then the same backward

at one frame of the configured body's vertices + face centres (31 161 points; 3 RGB + 125 reduced channels) and image
sizes 512^2 and 1024^2.  The two alternate in one process, --rounds times; per path and size one JSON line with the
median and minimum time of a forward + backward (HIP events) and the peak of torch.cuda.max_memory_allocated over it,
above what was allocated before (inputs and parameters).

    timeout -k 10 600 python tools/bench_stage1_sample.py [--sizes 512 1024] [--rounds 10] [--frames 1]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from audio_motion_avatar_amd import ops  # noqa: E402


def main():
    from audio_motion_avatar_amd.config import Stage1Config
    from audio_motion_avatar_amd.synthetic import make_render_inputs
    from audio_motion_avatar_amd.triplane_net import POINT_RADIUS_NDC, ImageFeature, SMPLXTriplaneEncoder

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--frames", type=int, default=1)
    args = ap.parse_args()

    torch.manual_seed(0)
    g = torch.Generator().manual_seed(0)
    imf = ImageFeature(1536).cuda()
    F = args.frames
    tokens = (torch.randn(1, F, 4096, 1536, generator=g) * 0.5).cuda()
    for size in args.sizes:
        cfg = Stage1Config(image_size=(size, size), subdivide_steps=0, device="cuda")
        enc = SMPLXTriplaneEncoder(cfg).cuda().eval()
        _, smpl, cam = make_render_inputs(F, cfg, seed=3)
        with torch.no_grad():
            verts = enc.get_smplx_verts(smpl)
        N = verts.shape[1]
        pts = (verts + smpl["transl"].reshape(F, 1, 3)).contiguous()
        E, K = cam["extrinsic"].reshape(F, 4, 4).float(), cam["intrinsic"].reshape(F, 3, 3).float()
        radius = POINT_RADIUS_NDC * size / 2.0
        rgb = torch.rand(1, F, 3, size, size, generator=g).cuda()
        dout = torch.randn(F, N, 128, generator=g).cuda()
        del enc

        def dense():
            feats = imf(rgb, tokens)
            return ops.points_project_differentiable(pts, E, K, feats.reshape(F, 128, size, size), radius)

        def grid():
            return ops.points_project_grid_differentiable(pts, E, K, rgb.reshape(F, 3, size, size), imf.reduce(tokens),
                                                          radius)

        def step(path):
            imf.zero_grad(set_to_none=True)
            path().backward(dout)

        paths = {"dense": dense, "grid": grid}
        with torch.no_grad():
            hit = int((grid() != 0).any(-1).sum())
        times, peaks = {k: [] for k in paths}, {k: 0 for k in paths}
        for name, path in paths.items():   # warm-up: the library's GEMM workspaces and the allocator's blocks
            step(path)
        for _ in range(args.rounds):
            for name, path in paths.items():
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                step(path)
                b.record()
                torch.cuda.synchronize()
                times[name].append(a.elapsed_time(b))
                peaks[name] = max(peaks[name], torch.cuda.max_memory_allocated() - base)
        for name in paths:
            ms = sorted(times[name])
            print(json.dumps(dict(kind="stage1_sample", path=name, image=[size, size], frames=F, points=N,
                                  points_hit=hit, channels=128, rounds=args.rounds, median_ms=round(ms[len(ms) // 2], 4),
                                  min_ms=round(ms[0], 4), peak_mem_mib=round(peaks[name] / 2 ** 20, 1))), flush=True)


if __name__ == "__main__":
    main()
