#!/usr/bin/env python3
"""Diagnostic: what the mesh overlay costs (ops.mesh_overlay: the five launches of csrc/mesh.hip -- fill, project, setup +
small faces, large faces, resolve) at 512 x 512 with the synthetic body (10 475 vertices and its faces) posed at random,
for 6 and for 48 frames per call, over 3-channel frames.

One process; after a warm-up the variants alternate in rounds, every round timing `repeats` calls one by one between
device events.  Reported per variant: the median over rounds of the round medians in ms per call and per frame, the
spread (max - min) of the round medians, and next to it the byte floor of DESIGN.md section 4.21 per pixel -- 8 B key
fill, 8 B key read, 12 B frame read (16 B for RGBA frames), 12 B store -- plus 12 B read and 12 B written per vertex and
28 B per face (ids and shade), at the 6.29 TB/s a float4 copy reaches on the MI355X.  There is no earlier path to compare
with, hence no threshold.  `all_large` runs the same call with small_box = 0 (every face through the wave-per-face tier):
what the tiering buys.  large_share_of_all_faces: the faces that took the large tier, of all F x T faces (the lengths of the
deferred lists, read from the workspace's last slab).  Prints one JSON line.

usage: time_mesh_overlay.py [rounds] [repeats]"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from audio_motion_avatar_amd import _lib, ops  # noqa: E402

COPY_TB_PER_S = 6.29  # float4 copy, measured
H = W = 512


def call_ms(step, repeats):
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def scene(F):
    from audio_motion_avatar_amd.body_model import BodyModel
    from audio_motion_avatar_amd.config import RendererConfig
    from audio_motion_avatar_amd.synthetic import make_render_inputs

    body = BodyModel.synthetic_model(seed=42, device="cuda")
    _, smpl, cam = make_render_inputs(F, RendererConfig(image_size=(H, W), device="cuda"), seed=1, device="cuda")
    verts = body(**{k: v.reshape(F, -1) for k, v in smpl.items()}).vertices
    faces = torch.as_tensor(body.faces).to("cuda", torch.int32)
    frames = torch.rand(F, H, W, 3, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
    return dict(vertices=verts, faces=faces, K=cam["intrinsic"][0], E=cam["extrinsic"][0], transl=smpl["transl"][0],
                frames=frames)


def variant(s, small_box):
    F, V, T = s["vertices"].shape[0], s["vertices"].shape[1], s["faces"].shape[0]
    ws = torch.empty(_lib.lib().amav_mesh_overlay_workspace_bytes(F, V, T, H, W), dtype=torch.uint8, device="cuda")
    step = lambda: ops.mesh_overlay(s["vertices"], s["faces"], s["K"], s["E"], H, W, frames=s["frames"], transl=s["transl"],
                                    workspace=ws, small_box=small_box, want_face_index=True)
    return step, ws


if __name__ == "__main__":
    if not torch.cuda.is_available():
        raise SystemExit("time_mesh_overlay.py needs an MI355X")
    given = [int(a) for a in sys.argv[1:] if a.isdigit()]
    rounds, repeats = (given + [5, 5][len(given):])[:2]
    res = {"rounds": rounds, "repeats": repeats, "image": [H, W]}
    paths, info = {}, {}
    for F in (6, 48):
        s = scene(F)
        V, T = s["vertices"].shape[1], s["faces"].shape[0]
        for name, small_box in ((f"frames_{F}", None), (f"frames_{F}_all_large", 0)):
            paths[name], ws = variant(s, small_box)
            info[name] = (F, V, T, ws)
    for step in paths.values():
        for _ in range(3):
            out = step()
    torch.cuda.synchronize()
    medians = {name: [] for name in paths}
    for _ in range(rounds):
        for name, step in paths.items():
            medians[name].append(call_ms(step, repeats))
    for name, m in medians.items():
        F, V, T, ws = info[name]
        ms = statistics.median(m)
        floor_bytes = F * (H * W * (8 + 8 + 12 + 12) + V * 24 + T * 28)
        floor_ms = floor_bytes / (COPY_TB_PER_S * 1e12) * 1e3
        out = paths[name]()
        torch.cuda.synchronize()
        counters = ws[ws.numel() - (12 * F + 255) // 256 * 256:][:4 * F].view(torch.int32)  # the deferred lists' lengths [F]
        covered = int((out["face_index"] >= 0).sum())
        res[name] = {"vertices": V, "faces": T, "ms": round(ms, 4), "ms_per_frame": round(ms / F, 5),
                     "spread_ms": round(max(m) - min(m), 4), "floor_ms": round(floor_ms, 4),
                     "floor_ms_per_frame": round(floor_ms / F, 5), "fraction_of_copy_rate": round(floor_ms / ms, 3),
                     "deferred_faces_per_frame": round(int(counters[:F].sum()) / F, 2),
                     "large_share_of_all_faces": round(int(counters[:F].sum()) / (F * T), 5),
                     "dropped_near_guard": out["status"].sum(dim=0).tolist(),
                     "covered_pixel_share": round(covered / (F * H * W), 4)}
    print(json.dumps(res))
