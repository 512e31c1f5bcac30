#!/usr/bin/env python3
"""Diagnostic: the SMPL-X parameter term on the fused HIP kernels (csrc/smplx_params.hip; AMAV_SMPLX_PARAMS=hip) against
the library path (the torch statements of smplx_decoder.py and losses.smplx_param_loss; the default), forward plus
backward, at the sizes the training steps hand to it:

    conversion    rot6d -> axis-angle of a [12,55,6] tensor that requires a gradient (one SMPLXDecoder call of stage 2)
    loss_stage2   one smplx_param_loss at F = 12 frames, the pred rotations being slices of one [12,55,3] tensor as the
                  decoder returns them (harness.py training_step)
    loss_stage1   the pair of calls of stage 1 (triplane_net.py training_step: two predictions against one target),
                  one backward for their sum

What these calls cost is host dispatch and launch latency, not arithmetic, so every sample is `calls` back-to-back calls
between two device events, divided by `calls`; the host is synchronised before each sample.  One process; the two sides
alternate in rounds (HIP, library, HIP, library, ...) after a warm-up, so drift of the machine lands on both.  Reported
per side: the median over rounds of the round medians and the spread (max - min) of the round medians, in milliseconds per
call.  Unless --no-step: one whole stage-2 training step (forward + backward, reference configuration) with the switch
either way.  The figure to read is hip against library of the same run.  Prints one JSON line.

usage: bench_smplx_params.py [rounds] [repeats] [calls] [--no-step]"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from audio_motion_avatar_amd import losses, ops  # noqa: E402
from audio_motion_avatar_amd.smplx_decoder import matrix_to_axis_angle, rotation_6d_to_matrix  # noqa: E402
from bench_cross_attention import SIDES, alternate  # noqa: E402

FRAMES = 12
JOINTS = {"global_orient": (0, 1), "body_pose": (1, 22), "left_hand_pose": (22, 37), "right_hand_pose": (37, 52),
          "jaw_pose": (52, 53), "leye_pose": (53, 54), "reye_pose": (54, 55)}


def batched(fn, calls):
    def run():
        for _ in range(calls):
            fn()
    return run


def per_call(res, calls):
    for side in SIDES:
        res[side] = {k: round(v / calls, 5) for k, v in res[side].items()}
    res["library_over_hip"] = round(res["library"]["ms"] / res["hip"]["ms"], 2)
    return res


def conversion_numbers(rounds, repeats, calls):
    g = torch.Generator().manual_seed(0)
    d6 = torch.randn(FRAMES, 55, 6, generator=g).cuda().requires_grad_()
    up = torch.randn(FRAMES, 55, 3, generator=g).cuda()

    def fused():
        d6.grad = None
        ops.rot6d_to_axis_angle_differentiable(d6).backward(up)

    def library():
        d6.grad = None
        matrix_to_axis_angle(rotation_6d_to_matrix(d6)).backward(up)

    res = alternate({"hip": batched(fused, calls), "library": batched(library, calls)}, rounds, repeats)
    return {**per_call(res, calls), "shape": [FRAMES, 55, 6]}


def prediction(seed):
    """A decoder output at F = 12: rotations as slices of one [12,55,3] leaf, betas / expression / transl as leaves."""
    g = torch.Generator().manual_seed(seed)
    aa = (0.5 * torch.randn(FRAMES, 55, 3, generator=g)).cuda().requires_grad_()
    pred = {k: (aa[:, lo] if hi - lo == 1 else aa[:, lo:hi]) for k, (lo, hi) in JOINTS.items()}
    leaves = [aa]
    for k, width in (("betas", 10), ("expression", 10), ("transl", 3)):
        pred[k] = (0.5 * torch.randn(FRAMES, width, generator=g)).cuda().requires_grad_()
        leaves.append(pred[k])
    return pred, leaves


def loss_numbers(predictions, rounds, repeats, calls):
    preds = [prediction(10 + i) for i in range(predictions)]
    g = torch.Generator().manual_seed(1)
    gt = {k: (p.detach() + 0.3 * torch.randn(p.shape, generator=g).cuda()).contiguous() for k, p in preds[0][0].items()}

    def run(term):
        for _, leaves in preds:
            for leaf in leaves:
                leaf.grad = None
        sum(term(pred, gt)[0] for pred, _ in preds).backward()

    res = alternate({"hip": batched(lambda: run(losses.smplx_param_losses), calls),
                     "library": batched(lambda: run(losses.smplx_param_loss), calls)}, rounds, repeats)
    return {**per_call(res, calls), "frames": FRAMES, "loss_calls": predictions}


def step_numbers(rounds, repeats):
    """One whole stage-2 training step with AMAV_SMPLX_PARAMS either way (decoder conversion and loss term together)."""
    from bench_attention_backward import stage2_step

    step, info = stage2_step()

    def before(side):
        os.environ["AMAV_SMPLX_PARAMS"] = side

    res = alternate({side: step for side in SIDES}, rounds, repeats, before=before)
    os.environ.pop("AMAV_SMPLX_PARAMS", None)
    res["saved_ms"] = round(res["library"]["ms"] - res["hip"]["ms"], 3)
    res["saved_share_of_library_step"] = round(res["saved_ms"] / res["library"]["ms"], 4)
    return {**res, **info}


if __name__ == "__main__":
    if not torch.cuda.is_available():
        raise SystemExit("bench_smplx_params.py needs an MI355X")
    numbers = [int(a) for a in sys.argv[1:] if a.isdigit()]
    rounds, repeats, calls = (numbers + [5, 5, 20][len(numbers):])[:3]
    res = {"rounds": rounds, "repeats": repeats, "calls_per_sample": calls,
           "conversion": conversion_numbers(rounds, repeats, calls),
           "loss_stage2": loss_numbers(1, rounds, repeats, calls),
           "loss_stage1": loss_numbers(2, rounds, repeats, calls)}
    if "--no-step" not in sys.argv:
        res["training_step_stage2"] = step_numbers(rounds, max(2, repeats // 2))
    print(json.dumps(res))
