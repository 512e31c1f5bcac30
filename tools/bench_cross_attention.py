#!/usr/bin/env python3
"""Diagnostic: the HIP cross-attention (ops.crossattn_lse / ops.crossattn_backward) against the library's SDPA
(AMAV_CROSS_ATTN=library) at the two stage-1 shapes -- the fusion network's (B, Sq, Sk, H) = (1, 3152, 4096, 8) and the
SMPL-X predictor's (1, 80, 4096, 8) -- forward and backward, and one stage-1 training step
(TriplaneGaussianAvatar.training_step forward + backward at the reference widths, B = 1) for 1 and for 4 frames, in ms
and peak allocated GiB.

One process; the two sides alternate in rounds (HIP, library, HIP, library, ...), every round timing `repeats` calls
between HIP events after a warm-up, so that drift of the machine lands on both sides.  Reported per side: the median over
rounds of the round medians, and the spread (max - min) of the round medians.  Prints one JSON line.

usage: bench_cross_attention.py [rounds] [repeats] [--no-step]"""
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from audio_motion_avatar_amd import _lib, ops  # noqa: E402

SHAPES = {"fusion": (1, 3152, 4096, 8), "smplx_predictor": (1, 80, 4096, 8)}
SIDES = ("hip", "library")


def round_median(fn, repeats):
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def alternate(fns, rounds, repeats, before=None):
    """fns: side -> callable.  -> side -> {"ms": median of the round medians, "spread_ms": their max - min}"""
    for side in SIDES:   # warm-up: code objects, library algorithm choices, the allocator
        if before:
            before(side)
        for _ in range(2):
            fns[side]()
    torch.cuda.synchronize()
    medians = {side: [] for side in SIDES}
    for _ in range(rounds):
        for side in SIDES:
            if before:
                before(side)
            medians[side].append(round_median(fns[side], repeats))
    return {side: {"ms": round(statistics.median(m), 4), "spread_ms": round(max(m) - min(m), 4)}
            for side, m in medians.items()}


def attention_numbers(B, Sq, Sk, H, rounds, repeats):
    g = torch.Generator().manual_seed(0)
    HD = H * 64
    q = torch.randn(B, Sq, HD, generator=g).cuda()
    kv = torch.randn(B, Sk, 2 * HD, generator=g).cuda()
    dout = torch.randn(B, Sq, HD, generator=g).cuda()
    out, lse = ops.crossattn_lse(q, kv, H)
    dq, dkv = torch.empty_like(q), torch.empty_like(kv)
    heads = lambda t: t.reshape(B, t.shape[1], H, 64).transpose(1, 2)
    qh, kh, vh = (heads(t).detach().requires_grad_() for t in (q, kv[..., :HD], kv[..., HD:]))
    doh = heads(dout)
    state = {}

    def lib_forward():
        state["o"] = F.scaled_dot_product_attention(qh, kh, vh)

    def lib_backward():
        qh.grad = kh.grad = vh.grad = None
        state["o"].backward(doh, retain_graph=True)

    lib_forward()
    fwd = alternate({"hip": lambda: ops.crossattn_lse(q, kv, H), "library": lib_forward}, rounds, repeats)
    bwd = alternate({"hip": lambda: ops.crossattn_backward(q, kv, out, lse, dout, H, grad_q=dq, grad_kv=dkv),
                     "library": lib_backward}, rounds, repeats)
    return {"shape": [B, Sq, Sk, H], "key_split": _lib.lib().amav_crossattn_key_split(B, Sq, Sk, H),
            "forward": fwd, "backward": bwd}


def stage1_step(frames):
    """-> step(): one TriplaneGaussianAvatar.training_step forward + backward at the reference widths (C = 256, R = 32,
    4096 x 1536 image tokens, 8 fusion + 4 SMPL-X layers, 512^2 views), B = 1, `frames` frames, seeded inputs."""
    from audio_motion_avatar_amd.config import Stage1Config
    from audio_motion_avatar_amd.synthetic import init_random_heads, make_render_inputs
    from audio_motion_avatar_amd.triplane_net import TriplaneGaussianAvatar

    torch.manual_seed(0)
    cfg = Stage1Config(subdivide_steps=0, device="cuda")
    model = TriplaneGaussianAvatar(cfg).eval()
    init_random_heads(model.renderer)
    with torch.no_grad():
        for blk in model.smplx_triplane_encoder.blocks:
            blk.fc_1.weight.normal_(0, 0.02)
    Hh, Ww = cfg.image_size
    _, smpl, cam = make_render_inputs(frames, cfg, seed=12, batch=1)
    _, _, test_cam = make_render_inputs(frames, cfg, seed=13, batch=1)
    g = torch.Generator().manual_seed(12)
    ref = torch.rand(1, frames, 3, Hh, Ww, generator=g).cuda()
    test = torch.rand(1, frames, 3, Hh, Ww, generator=g).cuda()
    tokens = (torch.randn(1, frames, 4096, cfg.image_feature_dim, generator=g) * 0.5).cuda()

    def step():
        model.zero_grad(set_to_none=True)
        total, _ = model.training_step(ref, smpl, cam, tokens, test, test_cam)
        total.backward()

    return step


def training_step_numbers(frames, rounds, repeats):
    step = stage1_step(frames)
    peaks = {side: 0 for side in SIDES}
    current = {}

    def before(side):
        if current:   # close the previous side's window
            peaks[current["side"]] = max(peaks[current["side"]], torch.cuda.max_memory_allocated())
        if side == "library":
            os.environ["AMAV_CROSS_ATTN"] = "library"
        else:
            os.environ.pop("AMAV_CROSS_ATTN", None)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        current["side"] = side

    res = alternate({side: step for side in SIDES}, rounds, repeats, before=before)
    before("hip")   # closes the last window
    os.environ.pop("AMAV_CROSS_ATTN", None)
    for side in SIDES:
        res[side]["peak_gib"] = round(peaks[side] / 2 ** 30, 2)
    res["frames"] = frames
    return res


if __name__ == "__main__":
    if not torch.cuda.is_available():
        raise SystemExit("bench_cross_attention.py needs an MI355X")
    numbers = [int(a) for a in sys.argv[1:] if a.isdigit()]
    rounds, repeats = (numbers + [5, 5][len(numbers):])[:2]
    res = {"rounds": rounds, "repeats": repeats,
           "attention": {name: attention_numbers(*shape, rounds, repeats) for name, shape in SHAPES.items()}}
    if "--no-step" not in sys.argv:
        res["training_step"] = [training_step_numbers(frames, rounds, max(2, repeats // 2)) for frames in (1, 4)]
    print(json.dumps(res))
