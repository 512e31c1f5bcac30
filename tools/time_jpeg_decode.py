#!/usr/bin/env python3
"""Diagnostic: what the device JPEG decoder costs (ops.jpeg_decode: marker search, entropy decode, IDCT, colour -- the
four launches of csrc/jpeg_decode.hip) on a 48-frame 512 x 512 clip of the synthetic body, encoded by the project's own
encoder at quality 90, 4:2:0, with one MCU row per restart interval (32 intervals per frame) and, for the record, without
restart markers (one interval per frame: one lane decodes the whole frame).

One process; after a warm-up the variants alternate in rounds, every round timing `repeats` calls one by one.
  decode            ops.jpeg_decode on a stream already on the device, chw_f32 output       (device events)
  levels            ops.jpeg_decode_levels, the first two stages alone; pixels = decode - levels  (device events)
  upload_decode     the copy of records + stream from host memory, then the decode           (device events)
  host_to_tensor    parse the headers, pack the records, copy, decode, synchronise: load_clip without the file  (wall clock)
  pillow_to_tensor  what there was before: Pillow decodes every frame on the host, the raw bytes are copied up, the device
                    converts to fp32 [F,3,H,W] / 255                                          (wall clock)
Reported per variant: the median over rounds of the round medians in ms per call and per frame and the spread (max - min)
of the round medians; and the bytes that cross the host link either way.  There is no earlier device path to compare
with, hence no threshold.  Prints one JSON line.

usage: time_jpeg_decode.py [rounds] [repeats]"""
import io
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from audio_motion_avatar_amd import mjpeg, ops  # noqa: E402

F, H, W = 48, 512, 512


def event_ms(step, repeats):
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def wall_ms(step, repeats):
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t = time.perf_counter()
        step()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return statistics.median(out)


def rendered_clip():
    from audio_motion_avatar_amd.config import RendererConfig
    from audio_motion_avatar_amd.renderer import Renderer
    from audio_motion_avatar_amd.synthetic import init_random_heads, make_render_inputs

    cfg = RendererConfig(image_size=(H, W), subdivide_steps=0, predict_smplx_params=False, device="cuda")
    r = init_random_heads(Renderer(cfg).eval())
    tokens, smpl, cam = make_render_inputs(F, cfg, seed=42)
    with torch.no_grad():
        frames, _ = r.render_tokens(tokens[0], smpl, cam, workspaces=[None])
    return frames.contiguous()


def host_clip(frames, restart_rows):
    stream, offsets = ops.jpeg_encode(frames, quality=90, subsampling="420", restart_rows=restart_rows)
    data = stream.cpu().numpy().tobytes()
    return [data[int(a):int(b)] for a, b in zip(offsets[:-1], offsets[1:])]


def packed(jpegs):
    """(host uint8 tensor: records then frames, bytes of the record table, the records' geometry)"""
    headers = [mjpeg.parse_jpeg(j)[0] for j in jpegs]
    offsets, at = [], 0
    for j in jpegs:
        offsets.append(at)
        at += len(j)
    records = mjpeg.frame_records(headers, offsets)
    host = torch.cat([records.table, torch.frombuffer(bytearray(b"".join(jpegs)), dtype=torch.uint8)])
    return host, records.table.numel(), records


def decode_from(host, table_bytes, records, out):
    dev = host.cuda()
    return ops.jpeg_decode(dev[table_bytes:], ops.JpegRecords(dev[:table_bytes], records.height, records.width, records.sampling),
                           layout="chw_f32", out=out)


def pillow_to_tensor(jpegs):
    import numpy as np
    from PIL import Image

    raw = np.stack([np.asarray(Image.open(io.BytesIO(j)).convert("RGB")) for j in jpegs])
    return torch.from_numpy(raw).cuda().permute(0, 3, 1, 2).float() / 255.0


if __name__ == "__main__":
    if not torch.cuda.is_available():
        raise SystemExit("time_jpeg_decode.py needs an MI355X")
    given = [int(a) for a in sys.argv[1:] if a.isdigit()]
    rounds, repeats = (given + [5, 5][len(given):])[:2]
    frames = rendered_clip()
    res = {"rounds": rounds, "repeats": repeats, "frames": F, "image": [H, W], "quality": 90, "subsampling": "420",
           "raw_rgb8_bytes_per_frame": H * W * 3}
    out = torch.empty(F, 3, H, W, device="cuda")
    paths, timers = {}, {}
    for rr in (1, 0):
        jpegs = host_clip(frames, rr)
        host, table_bytes, records = packed(jpegs)
        dev = host.cuda()
        stream, table = dev[table_bytes:], ops.JpegRecords(dev[:table_bytes], records.height, records.width, records.sampling)
        tag = f"restart_rows_{rr}"
        res[tag] = {"jpeg_bytes_per_frame": round(sum(len(j) for j in jpegs) / F), "record_bytes_per_frame": table_bytes // F}
        paths[tag + ": decode"] = lambda stream=stream, table=table: ops.jpeg_decode(stream, table, layout="chw_f32", out=out)
        paths[tag + ": levels"] = lambda stream=stream, table=table: ops.jpeg_decode_levels(stream, table)
        if rr:
            paths[tag + ": upload_decode"] = lambda host=host, n=table_bytes, records=records: decode_from(host, n, records, out)
            paths[tag + ": host_to_tensor"] = lambda jpegs=jpegs: decode_from(*packed(jpegs), out)
            paths[tag + ": pillow_to_tensor"] = lambda jpegs=jpegs: pillow_to_tensor(jpegs)
        _, status = ops.jpeg_decode(stream, table, layout="chw_f32", out=out)
        want = pillow_to_tensor(jpegs)
        res[tag]["status_nonzero"] = int((status != 0).sum())
        res[tag]["max_abs_difference_to_pillow_levels"] = round(float((out - want).abs().max()) * 255.0, 3)
    for name in paths:
        timers[name] = wall_ms if name.endswith("_to_tensor") else event_ms
    for step in paths.values():
        for _ in range(2):
            step()
    torch.cuda.synchronize()
    medians = {name: [] for name in paths}
    for _ in range(rounds):
        for name, step in paths.items():
            medians[name].append(timers[name](step, repeats))
    for name, m in medians.items():
        tag, what = name.split(": ")
        ms = statistics.median(m)
        res[tag][what] = {"ms": round(ms, 4), "ms_per_frame": round(ms / F, 5), "spread_ms": round(max(m) - min(m), 4),
                          "clock": "wall" if timers[name] is wall_ms else "device events"}
    for tag in ("restart_rows_1", "restart_rows_0"):
        res[tag]["pixels_ms"] = round(res[tag]["decode"]["ms"] - res[tag]["levels"]["ms"], 4)
    print(json.dumps(res))
