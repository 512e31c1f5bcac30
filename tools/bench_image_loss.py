#!/usr/bin/env python3
"""Diagnostic: the fused HIP image loss (losses.image_losses: csrc/image_loss.hip) against the library path
(losses.l1_loss + losses.ssim, what AMAV_IMAGE_LOSS=library keeps) -- forward plus backward of l1 + 0.1 (1 - ssim) at
the shapes the two training steps hand to it: the stage-2 window (B = 1, T_output frames of the default image_size) and
stage 1's views (B = 1, 4 frames and 1 frame, each scored once for the train and once for the test views).  The inputs
are laid out as the steps deliver them: x a [..., :3] view of RGBA frames that require a gradient, y a permuted
[B,T,3,H,W] target.

One process; the two sides alternate in rounds (HIP, library, HIP, library, ...), every round timing `repeats` calls
between HIP events after a warm-up, so that drift of the machine lands on both sides.  Reported per side: the median over
rounds of the round medians, the spread (max - min) of the round medians, and the peak allocated bytes above what is
allocated before the call.  The fused kernels alone are timed the same way and set against their algorithmic traffic
(forward 8 B read + 12 B written per element, backward 20 B read + 4 B written).  Unless --no-step: one whole training
step (forward + backward) of each stage under either setting, which puts the loss's share of a step on record.
Prints one JSON line.

usage: bench_image_loss.py [rounds] [repeats] [--no-step]"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from audio_motion_avatar_amd import losses, ops  # noqa: E402
from audio_motion_avatar_amd.config import ModelConfig  # noqa: E402
from bench_cross_attention import SIDES, alternate, round_median  # noqa: E402

_CFG = ModelConfig()
SHAPES = {"stage2_window": (1, _CFG.triplane_audio_net.triplane_output_frames, *_CFG.renderer.image_size, 3),
          "stage1_views_4": (1, 4, *_CFG.renderer.image_size, 3),
          "stage1_views_1": (1, 1, *_CFG.renderer.image_size, 3)}


def loss_numbers(shape, rounds, repeats):
    B, T, H, W, C = shape
    g = torch.Generator().manual_seed(0)
    rgba = torch.rand(B, T, H, W, C + 1, generator=g).cuda().requires_grad_()
    video = torch.rand(B, T, C, H, W, generator=g).cuda()
    y = video.permute(0, 1, 3, 4, 2)

    def fused():
        rgba.grad = None
        l1, s = losses.image_losses(rgba[..., :C], y)
        (l1 + 0.1 * (1 - s)).backward()

    def library():
        rgba.grad = None
        x = rgba[..., :C]
        (losses.l1_loss(x, y) + 0.1 * (1 - losses.ssim(x, y))).backward()

    peaks = {side: 0 for side in SIDES}
    current = {}

    def before(side):
        if current:   # close the previous side's window
            peaks[current["side"]] = max(peaks[current["side"]], torch.cuda.max_memory_allocated() - current["base"])
        rgba.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        current.update(side=side, base=torch.cuda.memory_allocated())

    res = alternate({"hip": fused, "library": library}, rounds, repeats, before=before)
    before("hip")   # closes the last window
    for side in SIDES:
        res[side]["peak_bytes"] = peaks[side]
    res["speedup"] = round(res["library"]["ms"] / res["hip"]["ms"], 2)

    # the two kernels alone, against their algorithmic traffic
    x = rgba.detach()[..., :C].reshape(-1, H, W, C)
    yn = y.reshape(-1, H, W, C)
    elements = x.numel()
    _, maps = ops.image_loss_sums(x, yn, True)
    ones = torch.ones(x.shape[0], device="cuda")
    kernels = {"forward": (lambda: ops.image_loss_sums(x, yn, True), 20),
               "forward_no_grad": (lambda: ops.image_loss_sums(x, yn, False), 8),
               "backward": (lambda: ops.image_loss_backward(x, yn, maps, ones, ones), 24)}
    res["kernels"] = {}
    for name, (fn, bytes_per_element) in kernels.items():
        for _ in range(3):
            fn()
        m = [round_median(fn, repeats) for _ in range(rounds)]
        ms = statistics.median(m)
        res["kernels"][name] = {"ms": round(ms, 4), "spread_ms": round(max(m) - min(m), 4),
                                "algorithmic_bytes": elements * bytes_per_element,
                                "tb_per_s": round(elements * bytes_per_element / (ms * 1e-3) / 1e12, 3)}
    res["shape"] = list(shape)
    return res


def step_numbers(step, rounds, repeats):
    """One whole training step under the default and under AMAV_IMAGE_LOSS=library."""
    def before(side):
        if side == "library":
            os.environ["AMAV_IMAGE_LOSS"] = "library"
        else:
            os.environ["AMAV_IMAGE_LOSS"] = "hip"

    res = alternate({side: step for side in SIDES}, rounds, repeats, before=before)
    os.environ.pop("AMAV_IMAGE_LOSS", None)
    res["saved_ms"] = round(res["library"]["ms"] - res["hip"]["ms"], 3)
    res["saved_share_of_library_step"] = round(res["saved_ms"] / res["library"]["ms"], 4)
    return res


if __name__ == "__main__":
    if not torch.cuda.is_available():
        raise SystemExit("bench_image_loss.py needs an MI355X")
    numbers = [int(a) for a in sys.argv[1:] if a.isdigit()]
    rounds, repeats = (numbers + [5, 5][len(numbers):])[:2]
    res = {"rounds": rounds, "repeats": repeats,
           "loss": {name: loss_numbers(shape, rounds, repeats) for name, shape in SHAPES.items()}}
    if "--no-step" not in sys.argv:
        from bench_attention_backward import stage2_step
        from bench_cross_attention import stage1_step

        step2, info = stage2_step()
        res["training_step"] = {"stage2": {**step_numbers(step2, rounds, max(2, repeats // 2)), **info}}
        del step2
        torch.cuda.empty_cache()
        res["training_step"]["stage1_4_frames"] = step_numbers(stage1_step(4), rounds, max(2, repeats // 2))
    print(json.dumps(res))
