#!/usr/bin/env python3
"""Times the feature sampling's backward (amav_triplane_sample_features_backward: bin_kernel + texel_kernel +
point_kernel) with HIP events at the point refiner's shape, F = 8 frames, C = 256, R = 32, N = 10 000 and 30 000, and
next to it torch autograd of three F.grid_sample calls on the same inputs (the library path: float atomics, not
reproducible).  The points are a posed synthetic body's (Renderer.get_smpl_vertices), so the texel load is a real body's:
a fifth to a third of each plane.  The planes are the renderer's permuted view of a token slab.

    timeout -k 10 300 python tools/bench_sample_features_backward.py [--iters 50]

Operands are cold in the sense that matters here: grad_out (31 / 92 MB per frame) is 246 / 737 MB per call and is read
once per call from HBM; between two calls everything else that ran evicts it from the 4 MiB L2s, and at N = 30 000 it
exceeds the 256 MB Infinity Cache.  Three warm-up calls, then `iters` timed calls, each between its own pair of events;
median and minimum are printed, one JSON line per N.  Per-kernel times:

    timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d prof_sfb -o sfb -- \
        python tools/bench_sample_features_backward.py --iters 5
"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from audio_motion_avatar_amd import ops  # noqa: E402

F, C, R = 8, 256, 32


def inputs(N):
    from audio_motion_avatar_amd.config import RendererConfig
    from audio_motion_avatar_amd.renderer import Renderer
    from audio_motion_avatar_amd.synthetic import make_render_inputs

    cfg = RendererConfig(image_size=(64, 64), subdivide_steps=0 if N <= 10000 else 2, num_gaussians=N,
                         triplane_feature_dim=C, triplane_resolution=R, predict_smplx_params=False, device="cuda")
    r = Renderer(cfg).eval()
    tokens, smpl, _ = make_render_inputs(F, cfg, seed=42)
    with torch.no_grad():
        points = r.get_smpl_vertices(smpl).contiguous()
    planes = tokens[0].view(F, C, 3, R, R).permute(0, 2, 1, 3, 4)
    return planes, points, cfg.radius


def grid_sample_features(planes, points, radius):
    """Renderer.sample_from_triplane of the reference (src/models/renderer.py:292-317) with library calls."""
    u = torch.clamp(points / radius, -1, 1)
    feats = [torch.nn.functional.grid_sample(planes[:, p], u[..., list(axes)].unsqueeze(1), mode="bilinear",
                                             padding_mode="zeros", align_corners=False).squeeze(2).permute(0, 2, 1)
             for p, axes in enumerate(((0, 1), (0, 2), (1, 2)))]
    return torch.cat(feats, -1)


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


def run(N, iters):
    planes, points, radius = inputs(N)
    gout = torch.randn(F, N, 3 * C, device="cuda")
    hip = lambda: ops.triplane_sample_features_backward(planes, points, gout, radius)  # noqa: E731
    hip_planes = lambda: ops.triplane_sample_features_backward(planes, points, gout, radius, want_points=False)  # noqa: E731
    hip_points = lambda: ops.triplane_sample_features_backward(planes, points, gout, radius, want_planes=False)  # noqa: E731

    pl = planes.detach().clone().requires_grad_()  # a leaf in the same (permuted) layout
    pt = points.detach().clone().requires_grad_()
    with torch.enable_grad():
        feats = grid_sample_features(pl, pt, radius)

    def library():
        torch.autograd.grad(feats, (pl, pt), gout, retain_graph=True)

    times = dict(hip_backward=timed(hip, iters), hip_grad_planes_only=timed(hip_planes, iters),
                 hip_grad_points_only=timed(hip_points, iters), grid_sample_backward=timed(library, iters))
    # the library's result, for scale (its sums are atomic: the last bits change from run to run)
    g_hip, p_hip = hip()
    g_lib, p_lib = torch.autograd.grad(feats, (pl, pt), gout, retain_graph=True)
    diff = dict(grad_planes=float((g_hip - g_lib).abs().max() / g_lib.abs().max()),
                grad_points=float((p_hip - p_lib).abs().max() / p_lib.abs().max()))
    print(json.dumps(dict(frames=F, points=N, channels=C, resolution=R, iters=iters,
                          grad_out_mb=round(F * N * 3 * C * 4 / 1e6, 1), **times,
                          hip_over_library=round(times["hip_backward"]["median_ms"] /
                                                 times["grid_sample_backward"]["median_ms"], 3),
                          max_rel_difference_to_library=diff)), flush=True)
    assert math.isfinite(times["hip_backward"]["median_ms"])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--points", type=int, nargs="*", default=[10000, 30000])
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    for n in args.points:
        run(n, args.iters)


if __name__ == "__main__":
    main()
