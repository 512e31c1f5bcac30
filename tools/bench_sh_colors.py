#!/usr/bin/env python3
"""Diagnostic: the spherical-harmonic colour kernels (ops.sh_colors and its backward) at degree 3, 250 x 10 000 and
6 x 30 000 Gaussians, dense and with a frame-stride-0 `sh`, against the same statements as torch operators on the
device (what the reference's Python runs); and render_batch at bench.py's render shape (250 frames of the synthetic
body's 10 000 Gaussians at 512 x 512) with args.rgb=False, degree 3, against args.rgb=True.

One process; every shape is warmed up, then the candidates alternate round by round; times are device events, medians
over the rounds with the spread (min .. max).  "GB/s" is the bytes that must move (inputs read once per frame row they
are used in, outputs written once) over the median time, to be read next to the ~6.3 TB/s a float4 copy reaches.

    python tools/bench_sh_colors.py [--rounds 30] [--json out.json] [--no-render]
"""
import argparse
import json
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sh_model  # noqa: E402
from audio_motion_avatar_amd import ops, renderer  # noqa: E402
from audio_motion_avatar_amd.config import RendererConfig  # noqa: E402
from audio_motion_avatar_amd.synthetic import init_random_heads, make_render_inputs  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=30)
ap.add_argument("--degree", type=int, default=3)
ap.add_argument("--json", help="also write the figures there")
ap.add_argument("--no-render", action="store_true")
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_sh_colors.py measures on the GPU; none is visible")
DEG, KC = args.degree, (args.degree + 1) ** 2


def torch_colors(means3d, sh, campos, degree):
    """The statements of renderer.py:541-545 / eval_sh as torch operators on the device (tests/sh_model.py in fp32)."""
    return sh_model.colors(means3d, sh.reshape(sh.shape[0], sh.shape[1], -1, 3), campos, degree)


def alternate(candidates, rounds, warmup=3):
    """candidates: {name: fn}; every round runs each once, timed by device events -> {name: (median, min, max)} ms."""
    times = {k: [] for k in candidates}
    for i in range(warmup + rounds):
        for k, fn in candidates.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if i >= warmup:
                times[k].append(a.elapsed_time(b))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def kernel_case(F, N, shared):
    g = torch.Generator().manual_seed(1)
    Fs = 1 if shared else F
    means3d = ((torch.rand(F, N, 3, generator=g) - 0.5) * 1.6).cuda()
    sh = (torch.randn(Fs, N, 3 * KC, generator=g) * 0.5).cuda().expand(F, -1, -1)
    campos = (torch.nn.functional.normalize(torch.randn(F, 3, generator=g), dim=-1) * 2.6).cuda()
    go = torch.randn(F, N, 3, generator=g).cuda()
    used = 3 * (DEG + 1) ** 2
    fwd_bytes = 4 * F * N * (3 + used + 3)              # means3d + the record + the colours
    bwd_bytes = 4 * F * N * (3 + used + 3 + used + 3)   # + grad_colors in, grad_sh and grad_means3d out
    sh_leaf = sh.detach().clone().requires_grad_() if not shared else sh[:1].detach().clone().requires_grad_()
    p_leaf = means3d.detach().clone().requires_grad_()

    def torch_backward():
        s = sh_leaf if not shared else sh_leaf.expand(F, -1, -1)
        out = torch_colors(p_leaf, s, campos, DEG)
        torch.autograd.grad((out * go).sum(), [sh_leaf, p_leaf])

    got = alternate({"hip forward": lambda: ops.sh_colors(means3d, sh, campos, DEG),
                     "torch forward": lambda: torch_colors(means3d, sh, campos, DEG),
                     "hip backward": lambda: ops.sh_colors_backward(means3d, sh, campos, DEG, go),
                     "torch forward+backward": torch_backward}, args.rounds)
    err = (ops.sh_colors(means3d, sh, campos, DEG) - torch_colors(means3d, sh, campos, DEG)).abs().max().item()
    row = {"F": F, "N": N, "shared_sh": shared, "max_abs_difference_to_torch": err, "bytes_forward": fwd_bytes,
           "bytes_backward": bwd_bytes}
    for k, (med, lo, hi) in got.items():
        row[k] = {"ms": med, "min": lo, "max": hi}
    row["hip forward"]["GB_per_s"] = fwd_bytes / row["hip forward"]["ms"] / 1e6
    row["hip backward"]["GB_per_s"] = bwd_bytes / row["hip backward"]["ms"] / 1e6
    return row


result = {"degree": DEG, "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "kernels": []}
for F, N in ((250, 10000), (6, 30000)):
    for shared in (False, True):
        row = kernel_case(F, N, shared)
        result["kernels"].append(row)
        print(json.dumps(row))

if not args.no_render:
    F, H, W = 250, 512, 512
    cfg = RendererConfig(image_size=(H, W), subdivide_steps=0, predict_smplx_params=False, device="cuda")
    r = init_random_heads(renderer.Renderer(cfg).eval())
    tokens, smpl, cam = make_render_inputs(F, cfg, seed=42)
    with torch.no_grad():
        _, packed = r.render_tokens(tokens[0], smpl, cam, workspaces=[None])
    g = {k: v.contiguous() for k, v in renderer.Renderer.unpack_gaussians(packed).items() if k != "shs"}
    N = g["xyz"].shape[1]
    gen = torch.Generator().manual_seed(2)
    sh = torch.randn(F, N, 3 * KC, generator=gen) * 0.2
    sh[..., :3] = renderer.RGB2SH(g["color"].cpu())
    g_sh = dict(g, color=sh.cuda())
    K, E = cam["intrinsic"], cam["extrinsic"]
    rgb_args = types.SimpleNamespace(image_size=(H, W), rgb=True, sh_degree=DEG)
    sh_args = types.SimpleNamespace(image_size=(H, W), rgb=False, sh_degree=DEG)
    ws = {k: None for k in ("rgb", "sh")}

    def render(which, gaussians, a):
        # the first call sizes the workspace (one host sync for the overflow check); the timed ones reuse it unchecked
        with torch.no_grad():
            _, ws[which] = renderer.render_batch(gaussians, K, E, a, workspace=ws[which], return_workspace=True,
                                                 check_overflow=ws[which] is None)

    render("rgb", g, rgb_args)
    render("sh", g_sh, sh_args)
    got = alternate({"render_batch rgb=True": lambda: render("rgb", g, rgb_args),
                     "render_batch rgb=False": lambda: render("sh", g_sh, sh_args)}, args.rounds)
    result["render"] = {"F": F, "N": N, "H": H, "W": W,
                        **{k: {"ms": med, "min": lo, "max": hi} for k, (med, lo, hi) in got.items()}}
    print(json.dumps(result["render"]))
if args.json:
    with open(args.json, "w") as fh:
        json.dump(result, fh, indent=1)
