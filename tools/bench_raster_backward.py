#!/usr/bin/env python3
"""Times the rasterizer's forward and backward (amav_rasterize_forward / amav_rasterize_backward) with HIP events at
BASELINE configs[1] (250 frames x 10 000 Gaussians x 512^2) and at the stress shape (configs[4] per GPU: 32 frames x
50 000 Gaussians x 1024^2), on seeded random Gaussians of the bench's size range.  Prints one JSON line per shape.

    timeout -k 10 300 python tools/bench_raster_backward.py [--shape configs1|stress|both] [--iters 20]

Per-kernel times (seg_kernel, tile_grad_kernel, gauss_grad_kernel next to the forward's launches):

    timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d prof_bwd -o bwd -- \
        python tools/bench_raster_backward.py --iters 5

(prof_bwd/bwd_kernel_stats.csv then lists every kernel's calls and mean / min / max time.)
"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from audio_motion_avatar_amd import ops  # noqa: E402

SHAPES = {"configs1": (250, 10000, 512, 512, -4.9), "stress": (32, 50000, 1024, 1024, -5.2)}


def scene(F, N, H, W, log_scale, seed=7):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    xyz = rn(F, N, 3) * 0.3 + torch.tensor([0.0, 0.0, 2.5])
    rot = torch.nn.functional.normalize(rn(F, N, 4), dim=-1)
    scale = torch.exp(rn(F, N, 3) * 0.55 + log_scale)
    opacity = torch.sigmoid(rn(F, N, 1) * 1.5)
    color = torch.rand(F, N, 3, generator=g)
    K = torch.tensor([[float(W), 0, W / 2], [0, float(W), H / 2], [0, 0, 1.0]]).repeat(F, 1, 1)
    E = torch.eye(4).repeat(F, 1, 1)
    ang = rn(F) * 0.1
    E[:, 0, 0], E[:, 0, 2], E[:, 2, 0], E[:, 2, 2] = torch.cos(ang), torch.sin(ang), -torch.sin(ang), torch.cos(ang)
    attrs = [t.cuda() for t in (xyz, rot, scale, opacity, color)]
    return attrs, ops.camera_from_intrinsics(K.cuda(), E.cuda(), H, W)[:3]


def run(name, iters):
    F, N, H, W, log_scale = SHAPES[name]
    attrs, cam = scene(F, N, H, W, log_scale)
    first = ops.rasterize(*attrs, *cam, H, W, check_overflow=True)  # sizes the workspace (one sync)
    ws, max_frame = first["workspace"], first["max_frame"]
    go = torch.randn(F, H, W, 4, device="cuda")
    fwd = lambda: ops.rasterize(*attrs, *cam, H, W, workspace=ws, check_overflow=False, out_rgba=first["rgba"])  # noqa
    bwd = lambda: ops.rasterize_backward(*attrs, *cam, H, W, go, ws, max_frame)  # noqa: E731
    times = {}
    for what, fn in (("forward", fwd), ("backward", bwd)):
        for _ in range(3):
            fn()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
        for a, b in ev:
            a.record()
            fn()
            b.record()
        torch.cuda.synchronize()
        ms = sorted(a.elapsed_time(b) for a, b in ev)
        times[what] = dict(median_ms=ms[len(ms) // 2], min_ms=ms[0])
    total, mx, over = ws.status_full()
    print(json.dumps(dict(shape=name, frames=F, gaussians=N, height=H, width=W, instances=total, max_frame=mx,
                          overflow=over, iters=iters, **times,
                          backward_over_forward=round(times["backward"]["median_ms"] / times["forward"]["median_ms"], 2))),
          flush=True)
    assert not over and math.isfinite(times["backward"]["median_ms"])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", choices=["configs1", "stress", "both"], default="both")
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    with torch.no_grad():
        for name in (("configs1", "stress") if args.shape == "both" else (args.shape,)):
            run(name, args.iters)


if __name__ == "__main__":
    main()
