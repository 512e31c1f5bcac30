#!/usr/bin/env python3
"""Diagnostic: the Motion-JPEG output path against the raw rgb24 path it stands beside, on a 48-frame 512 x 512 clip of
the synthetic body (mostly background) and on uniform noise (the encoder's worst case).

    compare (default)  alternating in one process: ops.jpeg_encode into a reused buffer + copy of the STREAM to pinned
                       host memory, against ops.frames_to_rgb8 + copy of the raw bytes; bytes per frame at qualities
                       75 / 90 / 100; the encode alone with and without the rasterizer's tile hint (device events)
    --kernels          a few encodes of each workload and nothing else: run under `rocprofv3 --kernel-trace --stats`
                       for the per-kernel times (profiles/jpeg_encode_kernel_stats.csv)
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from audio_motion_avatar_amd import ops  # noqa: E402
from audio_motion_avatar_amd.config import RendererConfig  # noqa: E402
from audio_motion_avatar_amd.renderer import Renderer  # noqa: E402
from audio_motion_avatar_amd.synthetic import init_random_heads, make_render_inputs  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=48)
ap.add_argument("--size", type=int, default=512)
ap.add_argument("--rounds", type=int, default=30)
ap.add_argument("--kernels", action="store_true")
ap.add_argument("--json", help="also write the figures there")
args = ap.parse_args()
F, H, W = args.frames, args.size, args.size

cfg = RendererConfig(image_size=(H, W), subdivide_steps=0, predict_smplx_params=False, device="cuda")
r = init_random_heads(Renderer(cfg).eval())
tokens, smpl, cam = make_render_inputs(F, cfg, seed=42)
ws = [None]
with torch.no_grad():
    rendered, _ = r.render_tokens(tokens[0], smpl, cam, workspaces=ws)
rendered = rendered.contiguous()
hint = ws[0].tile_counts()
noise = torch.rand(F, H, W, 4, generator=torch.Generator().manual_seed(0)).cuda()
raw_bytes = F * H * W * 3
print(f"{F} frames of {W}x{H}; background tiles by the rasterizer's hint: {float((hint == 0).float().mean()):.3f}")

stream = torch.empty(raw_bytes * 2, dtype=torch.uint8, device="cuda")  # noise at quality 100 exceeds the raw size
offsets = torch.empty(F + 1, dtype=torch.int64, device="cuda")
status = torch.zeros(1, dtype=torch.int32, device="cuda")


def encode(frames, quality=90, tile_hint=None):
    ops.jpeg_encode_into(frames, stream, quality=quality, tile_hint=tile_hint, frame_offsets=offsets, status=status)


if args.kernels:
    for frames, h in ((rendered, None), (rendered, hint), (noise, None)):
        for _ in range(5):
            encode(frames, tile_hint=h)
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    sys.exit(0)

result = {"frames": F, "height": H, "width": W, "raw_bytes_per_frame": H * W * 3, "bytes_per_frame": {}, "ms_per_clip": {}}
for name, frames in (("rendered", rendered), ("noise", noise)):
    for q in (75, 90, 100):
        encode(frames, q)
        result["bytes_per_frame"][f"{name}_q{q}"] = int(offsets[-1].item()) / F
assert int(status.item()) == 0
# the hint changes no byte
encode(rendered, 90, hint)
with_hint = stream[:int(offsets[-1].item())].clone()
encode(rendered, 90)
assert torch.equal(with_hint, stream[:int(offsets[-1].item())])

host_stream = torch.empty(raw_bytes * 2, dtype=torch.uint8).pin_memory()
host_raw = torch.empty(raw_bytes, dtype=torch.uint8).pin_memory()
dense = torch.empty(F, H, W, 3, dtype=torch.uint8, device="cuda")


def jpeg_path(frames, tile_hint=None):
    encode(frames, 90, tile_hint)
    n = int(offsets[-1].item())  # the single synchronisation: the size
    host_stream[:n].copy_(stream[:n], non_blocking=True)
    torch.cuda.synchronize()


def raw_path(frames):
    ops.frames_to_rgb8(frames, out=dense)
    host_raw.copy_(dense.view(-1), non_blocking=True)
    torch.cuda.synchronize()


def alternate(pairs, rounds):
    times = {k: [] for k, _ in pairs}
    for i in range(rounds + 3):
        for k, fn in pairs:
            t0 = time.perf_counter()
            fn()
            if i >= 3:
                times[k].append((time.perf_counter() - t0) * 1e3)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def events(fn, rounds):
    out = []
    for i in range(rounds + 3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= 3:
            out.append(a.elapsed_time(b))
    return statistics.median(out), min(out), max(out)


end_to_end = alternate([("rendered: jpeg encode + stream to host", lambda: jpeg_path(rendered)),
                        ("rendered: jpeg encode (hint) + stream to host", lambda: jpeg_path(rendered, hint)),
                        ("rendered: rgb8 + raw bytes to host", lambda: raw_path(rendered)),
                        ("noise: jpeg encode + stream to host", lambda: jpeg_path(noise)),
                        ("noise: rgb8 + raw bytes to host", lambda: raw_path(noise))], args.rounds)
device_only = {"rendered: encode, no hint": events(lambda: encode(rendered), args.rounds),
               "rendered: encode, tile hint": events(lambda: encode(rendered, 90, hint), args.rounds),
               "noise: encode": events(lambda: encode(noise), args.rounds),
               "rendered: frames_to_rgb8": events(lambda: ops.frames_to_rgb8(rendered, out=dense), args.rounds)}
for title, table in (("end to end (host clock, synchronised), ms per clip: median min max", end_to_end),
                     ("device only (events), ms per clip: median min max", device_only)):
    print(title)
    for k, (med, lo, hi) in table.items():
        print(f"  {k:48s} {med:8.3f} {lo:8.3f} {hi:8.3f}   ({med / F * 1e3:7.1f} us per frame)")
        result["ms_per_clip"][k] = med
print("bytes per frame:", json.dumps(result["bytes_per_frame"]), "raw", H * W * 3)
if args.json:
    with open(args.json, "w") as fh:
        json.dump(result, fh, indent=1)
