#!/usr/bin/env python3
"""Diagnostic: the PNG output path on a 48-frame 512 x 512 clip of the synthetic body (fp32 RGBA as rendered) and its
masks (uint8 grey, alpha > 0.5), against a Pillow save loop fed by a download of the raw frames, alternating in one
process.

    time     png.save_clip's device part (ops.png_encode_into, device events) and its whole (frames on the device ->
             files on disk), against frames_to_rgb8 + download + Image.save at compress_level 1 and 6
    size     bytes per frame, against Pillow at both levels and against zlib.compress(filtered scanlines, 1) on the very
             bytes the device deflates (taken from the files' IDAT payloads)
    phases   the deflate waves' time by phase and the input rate per wave, summed over both runs of the pieces; only
             with a stamped build of the library (not the product build; the stamps slow the waves a little):
                 cd audio-motion-avatar_amd/csrc && touch png_encode.hip && \
                 make CXXFLAGS="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -DAMAV_PNG_STAMPS"
             (then `touch png_encode.hip && make` again)
    --kernels  a few encodes and nothing else: run under `rocprofv3 --kernel-trace --stats` for the per-kernel times
"""
import argparse
import ctypes
import json
import os
import statistics
import struct
import sys
import tempfile
import time
import zlib

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from audio_motion_avatar_amd import _lib, ops, png  # noqa: E402
from audio_motion_avatar_amd.config import RendererConfig  # noqa: E402
from audio_motion_avatar_amd.renderer import Renderer  # noqa: E402
from audio_motion_avatar_amd.synthetic import init_random_heads, make_render_inputs  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=48)
ap.add_argument("--size", type=int, default=512)
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--kernels", action="store_true")
ap.add_argument("--json", help="also write the figures there")
args = ap.parse_args()
F, H, W = args.frames, args.size, args.size

cfg = RendererConfig(image_size=(H, W), subdivide_steps=0, predict_smplx_params=False, device="cuda")
r = init_random_heads(Renderer(cfg).eval())
tokens, smpl, cam = make_render_inputs(F, cfg, seed=42)
with torch.no_grad():
    rendered, _ = r.render_tokens(tokens[0], smpl, cam, workspaces=[None])
rendered = rendered.contiguous()
masks = ((rendered[..., 3] > 0.5).to(torch.uint8) * 255).contiguous()
workloads = {"rendered": (rendered, 3), "masks": (masks, 1)}
stream = torch.empty(ops.png_stream_bound(F, H, W, 3), dtype=torch.uint8, device="cuda")
offsets = torch.empty(F + 1, dtype=torch.int64, device="cuda")
status = torch.empty(F, dtype=torch.int32, device="cuda")


def encode(frames):
    ops.png_encode_into(frames, stream, frame_offsets=offsets, status=status)


stamped = hasattr(_lib.lib(), "amav_debug_png_stamps")


if args.kernels:
    for frames, _ in workloads.values():
        for _ in range(5):
            encode(frames)
    torch.cuda.synchronize()
    sys.exit(0)


def events(fn, rounds):
    out = []
    for i in range(rounds + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= 2:
            out.append(a.elapsed_time(b))
    return statistics.median(out)


def alternate(pairs, rounds):
    times = {k: [] for k, _ in pairs}
    for i in range(rounds + 1):
        for k, fn in pairs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            if i >= 1:
                times[k].append((time.perf_counter() - t0) * 1e3)
    return {k: statistics.median(v) for k, v in times.items()}


def pillow_loop(frames, channels, level, directory):
    from PIL import Image

    host = (ops.frames_to_rgb8(frames) if frames.dtype == torch.float32 else frames).cpu().numpy()
    for i in range(F):
        Image.fromarray(host[i]).save(os.path.join(directory, f"{i:05d}.png"), compress_level=level)


def idat(blob):
    at, parts = 8, []
    while at < len(blob):
        n, kind = struct.unpack(">I4s", blob[at:at + 8])
        if kind == b"IDAT":
            parts.append(blob[at + 8:at + 8 + n])
        at += 12 + n
    return b"".join(parts)


result = {"frames": F, "height": H, "width": W}
with tempfile.TemporaryDirectory() as tmp:
    for name, (frames, channels) in workloads.items():
        dirs = {k: os.path.join(tmp, f"{name}_{k}") for k in ("device", "pillow1", "pillow6")}
        for d in dirs.values():
            os.makedirs(d)
        device_ms = events(lambda: encode(frames), args.rounds)
        files_ms = alternate([("save_clip", lambda: png.save_clip(dirs["device"], frames)),
                              ("pillow level 1", lambda: pillow_loop(frames, channels, 1, dirs["pillow1"])),
                              ("pillow level 6", lambda: pillow_loop(frames, channels, 6, dirs["pillow6"]))], max(2, args.rounds // 3))
        size = {k: sum(os.path.getsize(os.path.join(d, n)) for n in os.listdir(d)) / F for k, d in dirs.items()}
        filtered = [zlib.decompress(idat(open(os.path.join(dirs["device"], f"{i:05d}.png"), "rb").read())) for i in range(F)]
        size["zlib level 1 on the same filtered bytes"] = sum(len(zlib.compress(b, 1)) for b in filtered) / F
        size["zlib level 6 on the same filtered bytes"] = sum(len(zlib.compress(b, 6)) for b in filtered) / F
        size["device IDAT payload"] = sum(len(idat(open(os.path.join(dirs["device"], f"{i:05d}.png"), "rb").read())) for i in range(F)) / F
        size["raw"] = H * W * channels
        result[name] = {"device_ms_per_clip": device_ms, "ms_per_clip_to_files": files_ms, "bytes_per_frame": size,
                        "stamped_build": stamped}
        if stamped:
            buf = (ctypes.c_ulonglong * 4)()
            _lib.lib().amav_debug_png_stamps(buf)  # clear what the runs above left
            encode(frames)
            _lib.lib().amav_debug_png_stamps(buf)
            ticks, total = list(buf), sum(buf)
            waves = 2 * F * -(-len(filtered[0]) // ops.DEFLATE_PIECE)  # every piece is run twice
            names = ("load + match finding + parse", "histograms", "code construction + choice", "emission + crc + copy")
            result[name].update(phase_share={k: t / total for k, t in zip(names, ticks)}, waves=waves,
                                wave_us=total * 10e-3 / waves,  # 100 MHz ticks
                                wave_input_MB_per_s=2 * F * len(filtered[0]) / (total * 10e-9) / 1e6)
        print(name, json.dumps(result[name], indent=1))
if args.json:
    with open(args.json, "w") as fh:
        json.dump(result, fh, indent=1)
