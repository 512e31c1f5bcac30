#!/usr/bin/env python3
"""Times the SMPL-X LBS forward (amav_lbs_forward_parts) and backward (amav_lbs_backward), and the gather forward and
backward (amav_points_gather(_backward), 10 000 points of a once-subdivided body), with HIP events (median of --iters)
at 250 frames (BASELINE configs[1]) and at 6 frames (the reference's training window) on the synthetic SMPL-X body.
Prints one JSON line per frame count.

    timeout -k 10 300 python tools/bench_lbs_backward.py [--frames 250 6] [--iters 20]

Per-kernel times (joint_chain_kernel, vposed_kernel, dfeat_kernel, joint_grad_kernel, chain_backward_kernel next to the
forward's):

    timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d prof_lbs -o lbs -- \\
        python tools/bench_lbs_backward.py --iters 5

(prof_lbs/lbs_kernel_stats.csv then lists every kernel's calls and mean / min / max time.)
"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from audio_motion_avatar_amd import ops  # noqa: E402


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


def run(F, iters, body, idx, csr):
    g = torch.Generator().manual_seed(F)
    pose = (torch.randn(F, 165, generator=g) * 0.3).cuda()
    coeffs = torch.randn(F, 20, generator=g).cuda()
    parts = [pose[:, :3], pose[:, 3:66], pose[:, 66:69], pose[:, 69:72], pose[:, 72:75], pose[:, 75:120], pose[:, 120:]]
    cparts = [coeffs[:, :10], coeffs[:, 10:]]
    tables = body.device_tables()
    gv = torch.randn(F, body.num_verts, 3, generator=g).cuda()
    verts = ops.lbs_forward_parts(tables, parts, cparts, pose_mean=body.pose_mean)
    gpts = torch.randn(F, idx.shape[0], 3, generator=g).cuda()
    times = dict(
        lbs_forward=timed(lambda: ops.lbs_forward_parts(tables, parts, cparts, pose_mean=body.pose_mean), iters),
        lbs_backward=timed(lambda: ops.lbs_backward(tables, parts, cparts, gv, pose_mean=body.pose_mean), iters),
        gather_forward=timed(lambda: ops.points_gather(verts, idx), iters),
        gather_backward=timed(lambda: ops.points_gather_backward(gpts, csr, body.num_verts), iters))
    KB = 20 + 54 * 9
    flop = 2 * 2 * F * KB * 3 * body.num_verts  # v_posed recompute + the transposed product
    print(json.dumps(dict(frames=F, verts=body.num_verts, points=int(idx.shape[0]), iters=iters,
                          blend_gflop=round(flop / 1e9, 2), **times,
                          backward_over_forward=round(times["lbs_backward"]["median_ms"] /
                                                      times["lbs_forward"]["median_ms"], 2))), flush=True)
    assert math.isfinite(times["lbs_backward"]["median_ms"])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, nargs="+", default=[250, 6])
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    from audio_motion_avatar_amd.body_model import BodyModel, build_subdivision_table

    body = BodyModel.synthetic_model(seed=42, device="cuda")
    table = torch.as_tensor(build_subdivision_table(body.faces, body.num_verts, 1))
    idx = table[torch.randperm(table.shape[0], generator=torch.Generator().manual_seed(42))[:10000]].contiguous().cuda()
    csr = ops.points_gather_csr(idx, body.num_verts)
    with torch.no_grad():
        for F in args.frames:
            run(F, args.iters, body, idx, csr)


if __name__ == "__main__":
    main()
