#!/usr/bin/env python3
"""Diagnostic: what the device PNG decoder costs (ops.png_decode: inflate, then unfilter + convert -- the two launches of
csrc/png_decode.hip) on the clip DESIGN 4.24 uses: 48 frames at 512 x 512 of the synthetic body, written by Pillow at its
default compression level as RGB files, and their masks (alpha > 1/2) as mode "L" files.

One process; after a warm-up the variants alternate in rounds, every round timing `repeats` calls one by one.
  decode_frames / decode_masks   ops.png_decode on bytes already on the device, hwc_u8 output        (device events)
  inflate_frames / inflate_masks ops.inflate of the same zlib streams alone; unfilter = decode - inflate (device events)
  inflate_one_frame              ops.inflate of the first frame's stream alone: one wave's rate        (device events)
  host_to_clip      parse the files, pack, copy up, two decodes, ops.prepare_frames, synchronise: load_training_clip
                    without the file reads                                                              (wall clock)
  pillow_to_clip    what there was before: Pillow decodes every file on the host, the raw bytes are copied up, then
                    ops.prepare_frames                                                                  (wall clock)
Reported per variant: the median over rounds of the round medians in ms per call and the spread (max - min) of the round
medians; the bytes that cross the host link either way; inflate rates in output MB/s.  Prints one JSON line.

usage: time_png_decode.py [rounds] [repeats]"""
import io
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from audio_motion_avatar_amd import ops, png  # noqa: E402
from time_jpeg_decode import F, H, W, event_ms, rendered_clip, wall_ms  # noqa: E402

CROP = 1024


def png_files(frames):
    """Rendered fp32 RGBA [F,H,W,4] -> (RGB files, mask files) as Pillow writes them by default."""
    from PIL import Image

    rgba = frames.clamp(0, 1).cpu().numpy()
    rgb = (rgba[..., :3] * 255.0 + 0.5).astype(np.uint8)
    mask = ((rgba[..., 3] > 0.5) * 255).astype(np.uint8)
    out = ([], [])
    for f in range(rgb.shape[0]):
        for k, im in enumerate((Image.fromarray(rgb[f]), Image.fromarray(mask[f]))):
            buf = io.BytesIO()
            im.save(buf, "PNG")
            out[k].append(buf.getvalue())
    return out


def inflate_records(files):
    """The zlib streams of `files` as ops.inflate takes them: (stream bytes on the host, int64 [N,5], output bytes)."""
    blob, rows, at, out_at = bytearray(), [], 0, 0
    for data in files:
        h = png.parse_png(data)
        z = png.zlib_stream(data, h)
        channels = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}[h.color_type]
        need = h.height * (1 + (h.width * channels * h.bit_depth + 7) // 8)
        rows.append([at, at + len(z), out_at, need, 1])
        blob += z
        at += len(z)
        out_at += (need + 15) // 16 * 16
    return torch.frombuffer(blob, dtype=torch.uint8), torch.tensor(rows, dtype=torch.int64), out_at


def host_to_clip(rgb_files, mask_files):
    rgb, s0 = png.load_clip(rgb_files, mode="rgb", layout="hwc_u8", check=False)
    mask, s1 = png.load_clip(mask_files, mode="l", layout="hwc_u8", check=False)
    out = ops.prepare_frames(rgb, mask, crop_size=CROP)
    assert not torch.cat([s0, s1]).cpu().any()  # the one read-back
    return out


def pillow_to_clip(rgb_files, mask_files):
    from PIL import Image

    rgb = np.stack([np.asarray(Image.open(io.BytesIO(d)).convert("RGB")) for d in rgb_files])
    mask = np.stack([np.asarray(Image.open(io.BytesIO(d)).convert("L")) for d in mask_files])
    return ops.prepare_frames(torch.from_numpy(rgb).cuda(), torch.from_numpy(mask).cuda(), crop_size=CROP)


if __name__ == "__main__":
    if not torch.cuda.is_available():
        raise SystemExit("time_png_decode.py needs an MI355X")
    given = [int(a) for a in sys.argv[1:] if a.isdigit()]
    rounds, repeats = (given + [5, 5][len(given):])[:2]
    rgb_files, mask_files = png_files(rendered_clip())
    res = {"rounds": rounds, "repeats": repeats, "frames": F, "image": [H, W], "crop": CROP,
           "raw_bytes_per_frame": H * W * 4, "png_bytes_per_frame": round(sum(map(len, rgb_files + mask_files)) / F),
           "rgb_png_bytes_per_frame": round(sum(map(len, rgb_files)) / F), "mask_png_bytes_per_frame": round(sum(map(len, mask_files)) / F)}
    paths, out_bytes = {}, {}
    for tag, files, mode in (("frames", rgb_files, "rgb"), ("masks", mask_files, "l")):
        host, table_bytes, h, w = png.pack_clip(files)
        dev = host.cuda()
        stream, records = dev[table_bytes:], ops.PngRecords(dev[:table_bytes], h, w)
        out = torch.empty((F, H, W, 3) if mode == "rgb" else (F, H, W), dtype=torch.uint8, device="cuda")
        paths["decode_" + tag] = lambda s=stream, r=records, m=mode, o=out: ops.png_decode(s, r, mode=m, layout="hwc_u8", out=o)
        zhost, rows, total = inflate_records(files)
        zdev, raw = zhost.cuda(), torch.empty(total, dtype=torch.uint8, device="cuda")
        paths["inflate_" + tag] = lambda z=zdev, r=rows, o=raw: ops.inflate(z, r, out=o)
        out_bytes["inflate_" + tag] = int(rows[:, 3].sum())
        if tag == "frames":
            paths["inflate_one_frame"] = lambda z=zdev, r=rows[:1], o=raw: ops.inflate(z, r, out=o)
            out_bytes["inflate_one_frame"] = int(rows[0, 3])
        got, status = ops.png_decode(stream, records, mode=mode, layout="hwc_u8", out=out)
        from PIL import Image

        want = np.stack([np.asarray(Image.open(io.BytesIO(d)).convert("RGB" if mode == "rgb" else "L")) for d in files])
        res[tag + "_equal_pillow"] = bool(np.array_equal(got.cpu().numpy(), want)) and not bool(status.any())
    paths["host_to_clip"] = lambda: host_to_clip(rgb_files, mask_files)
    paths["pillow_to_clip"] = lambda: pillow_to_clip(rgb_files, mask_files)
    a, b = host_to_clip(rgb_files, mask_files), pillow_to_clip(rgb_files, mask_files)
    res["clips_equal"] = all(torch.equal(x, y) for x, y in zip(a, b))
    timers = {name: wall_ms if name.endswith("_to_clip") else event_ms for name in paths}
    for step in paths.values():
        for _ in range(2):
            step()
    torch.cuda.synchronize()
    medians = {name: [] for name in paths}
    for _ in range(rounds):
        for name, step in paths.items():
            medians[name].append(timers[name](step, repeats))
    for name, m in medians.items():
        ms = statistics.median(m)
        res[name] = {"ms": round(ms, 4), "spread_ms": round(max(m) - min(m), 4),
                     "clock": "wall" if timers[name] is wall_ms else "device events"}
        if name in out_bytes:
            res[name]["output_MB_per_s"] = round(out_bytes[name] / ms / 1e3, 1)
    for tag in ("frames", "masks"):
        res["unfilter_" + tag + "_ms"] = round(res["decode_" + tag]["ms"] - res["inflate_" + tag]["ms"], 4)
    print(json.dumps(res))
