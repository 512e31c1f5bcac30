#!/usr/bin/env python3
"""Times the triplane decode's forward (region projection + sample decode) and backward (amav_triplane_decode_backward)
with HIP events at BASELINE configs[1] (250 frames x 10 000 Gaussians, C = 256, R = 32) and at the stress shape
(32 frames x 50 000 Gaussians, C = 512, R = 128).  The points are a posed synthetic body's (synthetic.make_render_inputs
through Renderer.get_smpl_vertices), so the projected regions are a real body's.  Prints one JSON line per shape.

    timeout -k 10 300 python tools/bench_decode_backward.py [--shape configs1|stress|both] [--iters 20]

Per-kernel times (point_kernel, texel_kernel, dtokens_kernel, dwplane_kernel, finalize_kernel next to the forward's):

    timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d prof_dec -o dec -- \
        python tools/bench_decode_backward.py --iters 5

(prof_dec/dec_kernel_stats.csv then lists every kernel's calls and mean / min / max time.)
"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from audio_motion_avatar_amd import ops  # noqa: E402

SHAPES = {"configs1": (250, 10000, 256, 32, 0), "stress": (32, 50000, 512, 128, 2)}


def inputs(name):
    from audio_motion_avatar_amd.config import RendererConfig
    from audio_motion_avatar_amd.renderer import Renderer
    from audio_motion_avatar_amd.synthetic import init_random_heads, make_render_inputs

    F, N, C, R, steps = SHAPES[name]
    cfg = RendererConfig(image_size=(64, 64), subdivide_steps=steps, num_gaussians=N, triplane_feature_dim=C,
                         triplane_resolution=R, predict_smplx_params=False, device="cuda")
    r = init_random_heads(Renderer(cfg).eval())
    tokens, smpl, _ = make_render_inputs(F, cfg, seed=42)
    points = r.get_smpl_vertices(smpl)
    wpl, wpt = r._head_weights()
    transl = smpl["transl"].reshape(F, 3)
    return tokens[0], wpl, wpt, points, transl, cfg


def run(name, iters):
    F, N, C, R, _ = SHAPES[name]
    tokens, wpl, wpt, points, transl, cfg = inputs(name)
    radius = cfg.radius
    boxes = ops.points_bbox(points)
    proj = ops.triplane_project(tokens, wpl, R, region=(boxes, radius))
    grec = torch.randn(F, N, 16, device="cuda")

    def fwd():
        b = ops.points_bbox(points)
        p = ops.triplane_project(tokens, wpl, R, region=(b, radius), out=proj)
        return ops.triplane_sample_decode(p, points, transl, radius, wpt)

    bwd = lambda: ops.triplane_decode_backward(tokens, wpl, wpt, points, proj, grec, radius, boxes=boxes)  # noqa: E731
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
    slab_mb = F * C * 3 * R * R * 4 / 1e6
    print(json.dumps(dict(shape=name, frames=F, gaussians=N, channels=C, resolution=R, iters=iters,
                          grad_slab_mb=round(slab_mb, 1), **times,
                          backward_over_forward=round(times["backward"]["median_ms"] / times["forward"]["median_ms"], 2))),
          flush=True)
    assert math.isfinite(times["backward"]["median_ms"])


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
