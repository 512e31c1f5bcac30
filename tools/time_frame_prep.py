#!/usr/bin/env python3
"""Diagnostic: what the training-clip frame preparation costs (ops.prepare_frames: mask composite, pad, box, crop, resize;
csrc/frame_prep.hip) on 512 x 512 frames with a 1024 x 1024 crop, 8 and 48 frames per call, uint8 frames and masks as
mjpeg.load_clip(layout="hwc_u8") leaves them.

One process; after a warm-up the variants alternate in rounds, every round timing `repeats` calls one by one.
  hip     ops.prepare_frames into preallocated outputs: three launches, no host synchronisation       (device events)
  hip_boxes  the same call with neither image output: table initialisation, box reduction, box arithmetic  (device events)
  torch   the same steps with torch operators on the device, frame by frame because the crop box decides tensor
          shapes: composite, pad, any / nonzero with .item() reads of the box, slice, pad, interpolate  (wall clock)
  numpy   the reference's CPU path, through the NumPy model of the tests, on two frames                 (wall clock)
Reported per variant: the median over rounds of the round medians in ms per call and per frame and the spread (max - min)
of the round medians.  For `hip` also the bytes that must move (12 B x (S^2 + Hp Wp) written, the frame and the mask read
once), the rate that makes, and its fraction of the 6.29 TB/s a float4 copy reaches on this chip.
`torch` divides by 255 with a reciprocal on the device, so its values differ from the dataset's in the last bit; the
largest difference to `hip` is printed, and the boxes must be equal.  Prints one JSON line.

usage: time_frame_prep.py [rounds] [repeats] [pad_ratio]
       time_frame_prep.py --kernels      ten 48-frame calls of `hip` and nothing else, for per-kernel times in a run of its own:
           rocprofv3 --kernel-trace --stats --output-format csv -d prof_prep -o prep -- python tools/time_frame_prep.py --kernels"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import frame_prep_cases as fc  # noqa: E402
import frame_prep_model as fm  # noqa: E402
from audio_motion_avatar_amd import ops  # noqa: E402

H = W = 512
S = 1024
COPY_RATE = 6.29e12


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


def clip(n):
    masks = np.stack([fc.blob(256 + 3 * (f % 16), 230 + 5 * (f % 9), 180 + f % 7, 90 + 2 * (f % 11), H, W) for f in range(n)])
    return fc.frames(n, H, W), masks


def torch_path(frames, masks, pad_ratio):
    n = frames.shape[0]
    hp, wp, oy, ox = ops.padded_size(H, W, pad_ratio)
    img = frames.permute(0, 3, 1, 2).float() / 255.0
    m = (masks.float() / 255.0)[:, None]
    images = torch.ones(n, 3, hp, wp, device=frames.device)
    images[:, :, oy:oy + H, ox:ox + W] = img * m + (1 - m)
    cropped, boxes = [], []
    for f in range(n):
        rows, cols = (masks[f] != 0).any(dim=1).nonzero(), (masks[f] != 0).any(dim=0).nonzero()
        if rows.numel():
            y0, y1, x0, x1 = rows[0].item(), rows[-1].item(), cols[0].item(), cols[-1].item()
            py, px = int((y1 - y0) * 0.2), int((x1 - x0) * 0.2)
            y0, y1, x0, x1 = max(0, y0 - py), min(H - 1, y1 + py), max(0, x0 - px), min(W - 1, x1 + px)
            half, cy, cx = max(y1 - y0, x1 - x0) // 2, (y0 + y1) // 2, (x0 + x1) // 2
            y0, y1, x0, x1 = max(0, cy - half), min(H - 1, cy + half), max(0, cx - half), min(W - 1, cx + half)
        else:
            y0, y1, x0, x1 = 0, hp - 1, 0, wp - 1
        crop = images[f:f + 1, :, y0:y1 + 1, x0:x1 + 1]
        h, w = crop.shape[2:]
        side = max(h, w)
        left, top = (side - w) // 2, (side - h) // 2
        square = torch.nn.functional.pad(crop, (left, side - w - left, top, side - h - top), value=1.0)
        cropped.append(torch.nn.functional.interpolate(square, size=(S, S), mode="bilinear", align_corners=True))
        boxes.append([y0, y1, x0, x1, side])
    return images, torch.cat(cropped), boxes


if __name__ == "__main__":
    if not torch.cuda.is_available():
        raise SystemExit("time_frame_prep.py needs an MI355X")
    if "--kernels" in sys.argv:
        host_frames, host_masks = clip(48)
        frames, masks = torch.from_numpy(host_frames).cuda(), torch.from_numpy(host_masks).cuda()
        out_i, out_c = torch.empty(48, 3, H, W, device="cuda"), torch.empty(48, 3, S, S, device="cuda")
        for _ in range(10):
            ops.prepare_frames(frames, masks, crop_size=S, out_images=out_i, out_cropped=out_c)
        torch.cuda.synchronize()
        raise SystemExit(0)
    given = [a for a in sys.argv[1:]]
    rounds, repeats = (int(a) for a in (given + ["5", "5"][len(given):])[:2])
    pad_ratio = float(given[2]) if len(given) > 2 else 0.0
    hp, wp, _, _ = ops.padded_size(H, W, pad_ratio)
    res = {"rounds": rounds, "repeats": repeats, "image": [H, W], "padded": [hp, wp], "crop_side": S, "pad_ratio": pad_ratio,
           "hip_launches": 3, "hip_host_synchronisations": 0}
    paths, timers, frames_of = {}, {}, {}
    for n in (8, 48):
        host_frames, host_masks = clip(n)
        frames, masks = torch.from_numpy(host_frames).cuda(), torch.from_numpy(host_masks).cuda()
        out_i, out_c = torch.empty(n, 3, hp, wp, device="cuda"), torch.empty(n, 3, S, S, device="cuda")
        tag = f"frames_{n}"
        paths[tag + ": hip"] = lambda frames=frames, masks=masks, out_i=out_i, out_c=out_c: ops.prepare_frames(
            frames, masks, pad_ratio=pad_ratio, crop_size=S, out_images=out_i, out_cropped=out_c)
        paths[tag + ": hip_boxes"] = lambda frames=frames, masks=masks: ops.prepare_frames(
            frames, masks, pad_ratio=pad_ratio, crop_size=S, images=False, cropped=False)
        paths[tag + ": torch"] = lambda frames=frames, masks=masks: torch_path(frames, masks, pad_ratio)
        case = dict(frames=host_frames[:2], masks=host_masks[:2], pad_ratio=pad_ratio)
        paths[tag + ": numpy"] = lambda case=case: fm.prepare(case, S)
        frames_of.update({tag + ": hip": n, tag + ": hip_boxes": n, tag + ": torch": n, tag + ": numpy": 2})
        _, _, boxes = paths[tag + ": hip"]()
        images_t, cropped_t, boxes_t = paths[tag + ": torch"]()
        assert boxes.tolist() == boxes_t, "the torch composition found other boxes"
        need = 12 * (S * S + hp * wp) + H * W * 3 + H * W
        res[tag] = {"bytes_needed_per_frame": need, "max_abs_hip_minus_torch": {
            "images": float((out_i - images_t).abs().max()), "cropped": float((out_c - cropped_t).abs().max())}}
        del images_t, cropped_t
    for name in paths:
        timers[name] = event_ms if ": hip" in name else wall_ms
    for name, step in paths.items():
        for _ in range(1 if name.endswith("numpy") else 2):
            step()
    torch.cuda.synchronize()
    medians = {name: [] for name in paths}
    for _ in range(rounds):
        for name, step in paths.items():
            medians[name].append(timers[name](step, 1 if name.endswith("numpy") else repeats))
    for name, m in medians.items():
        tag, what = name.split(": ")
        ms = statistics.median(m)
        res[tag][what] = {"ms": round(ms, 4), "ms_per_frame": round(ms / frames_of[name], 5), "spread_ms": round(max(m) - min(m), 4),
                          "frames_timed": frames_of[name], "clock": "device events" if timers[name] is event_ms else "wall"}
    for n in (8, 48):
        r = res[f"frames_{n}"]
        rate = r["bytes_needed_per_frame"] * n / (r["hip"]["ms"] * 1e-3)
        r["hip"]["needed_TB_per_second"] = round(rate / 1e12, 3)
        r["hip"]["fraction_of_float4_copy_rate"] = round(rate / COPY_RATE, 3)
        r["torch_over_hip"] = round(r["torch"]["ms"] / r["hip"]["ms"], 2)
        r["numpy_over_hip_per_frame"] = round(r["numpy"]["ms_per_frame"] / r["hip"]["ms_per_frame"], 1)
    print(json.dumps(res))
