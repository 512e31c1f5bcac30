#!/usr/bin/env python3
"""Diagnostic: time of the TriplaneUpsampler (renderer.py:377-417) at the reference defaults (4 blocks, C=256,
32^2 -> 512^2, three planes per frame) and of the default-config frame (upsampler + refiner at 30 000 points).

    python tools/bench_upsampler.py [frames] [--backward] [--full-frames N] [--training-step] [--conv library|hip|both]

--backward: forward + backward of the upsampler under autograd (loss = weighted sum of the features sampled at the
body's points), windowed (forward_tokens_windowed(differentiable=True)) against full planes (forward_tokens, on
--full-frames frames, default 1), each with torch.cuda.max_memory_allocated and, for the windowed path, the share of the
time spent in the two window-cutting kernels (HIP events around ops.windows_cut / ops.windows_cut_backward).
--conv: only the windowed evaluation, with its tile stages on the library's convolutions (the mosaic images) or on the HIP
3x3 cell convolution (AMAV_UPSAMPLER_CONV).  `both` alternates the two in one process on one plan
and prints ms per frame for each, the largest difference inside the active tiles and, for the HIP launches, their
HIP-event time and the FLOP they issue (3 partial products x 2 M 9 C_in C_out) against the dense 16-bit MFMA peak.
--backward --conv library|hip|both: forward + backward of the windowed evaluation with its tile stages' gradients on the
library or on the HIP backward (AMAV_UPSAMPLER_CONV_GRAD); `both` alternates the two in one
process on one plan: ms per frame (median, range) and peak allocated memory for each, and, for the HIP path, HIP-event
times of its data-gradient and weight-gradient launches replayed one by one, with the FLOP they issue.
--training-step: one full stage-2 AudioDrivenAvatar.training_step, forward + backward, at the reference's default
renderer.yaml (upsampler + refiner, 30 000 points, every differentiable_* flag on) with its peak allocated memory.
"""
import os
import sys
import time

import torch

if os.environ.get("AMAV_CONV_BENCHMARK"):
    torch.backends.cudnn.benchmark = True  # MIOpen find mode: search the convolution kernels per shape

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from audio_motion_avatar_amd.config import RendererConfig  # noqa: E402
from audio_motion_avatar_amd.renderer import Renderer  # noqa: E402
from audio_motion_avatar_amd.synthetic import init_random_heads, make_render_inputs  # noqa: E402

from audio_motion_avatar_amd import ops  # noqa: E402

_positional = [a for i, a in enumerate(sys.argv[1:], 1)
               if not a.startswith("--") and sys.argv[i - 1] not in ("--full-frames", "--conv")]
F = int(_positional[0]) if _positional else 2
FULL_FRAMES = int(sys.argv[sys.argv.index("--full-frames") + 1]) if "--full-frames" in sys.argv else 1
CONV = sys.argv[sys.argv.index("--conv") + 1] if "--conv" in sys.argv else None
if CONV not in (None, "library", "hip", "both"):
    sys.exit("--conv takes library, hip or both")
MFMA_16BIT_PEAK_TFLOPS = 2516.6  # bench.py: dense fp16 MFMA, 32x32x16 in 32 cycles per SIMD, 1024 SIMDs, 2.4 GHz


def training_step():
    """tools/bench_attention_backward.py's training step with the reference's default renderer configuration."""
    from audio_motion_avatar_amd.config import ModelConfig
    from audio_motion_avatar_amd.harness import AudioDrivenAvatar

    mcfg = ModelConfig()
    rc = mcfg.renderer
    rc.upsample_triplane, rc.no_point_refiner, rc.subdivide_steps = True, False, 2
    rc.differentiable_smplx = rc.differentiable_refiner = rc.differentiable_refine_points = True
    rc.differentiable_upsampler = True
    model = AudioDrivenAvatar(mcfg)
    init_random_heads(model.renderer)
    model = model.cuda().eval()
    with torch.no_grad():
        model.renderer.point_refiner[-1].weight.normal_(0, 0.005)
    a = mcfg.triplane_audio_net
    T = a.triplane_output_frames
    _, smpl, cam = make_render_inputs(T, rc, seed=1)
    g = torch.Generator().manual_seed(2)
    tri = torch.randn(1, a.triplane_input_frames, a.triplane_feature_dim, 3 * a.triplane_resolution ** 2, generator=g)
    st = torch.randn(1, a.triplane_input_frames, a.smpl_token_dim, a.smpl_token_len, generator=g) * 0.2
    audio = torch.randn(1, T, a.audio_feature_dim, generator=g)
    target = torch.rand(1, T, 3, *rc.image_size, generator=g)
    tri, st, audio, target = (t.cuda() for t in (tri, st, audio, target))

    def step():
        model.zero_grad(set_to_none=True)
        loss, _ = model.training_step(tri, st, audio, cam, target, smpl)
        loss.backward()

    up = model.renderer.triplane_upsampler
    full_plane_calls, full = [], up.forward_tokens
    up.forward_tokens = lambda *args, **kw: (full_plane_calls.append(1), full(*args, **kw))[1]  # the fallback, if taken
    step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    reps = 2
    for _ in range(reps):
        step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / reps
    missing = [k for k, p in up.named_parameters() if p.grad is None]
    print(f"stage-2 training_step, reference default renderer ({T} frames, {model.renderer.num_verts} points, upsampler + "
          f"refiner under autograd): {dt * 1e3:.0f} ms, peak allocated {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB; "
          f"full-plane fallbacks in {reps + 1} steps: {len(full_plane_calls)}; upsampler parameters without a gradient: "
          f"{missing}", flush=True)


if "--training-step" in sys.argv:
    training_step()
    sys.exit(0)
cfg = RendererConfig(image_size=(512, 512), subdivide_steps=0, predict_smplx_params=False, upsample_triplane=True,
                     num_upsample_blocks=4, device="cuda")
r = init_random_heads(Renderer(cfg).eval())
tokens, smpl, cam = make_render_inputs(F, cfg, seed=42)
up = r.triplane_upsampler


def flops():
    c, res, total = cfg.triplane_feature_dim, cfg.triplane_resolution, 0.0
    for i in range(cfg.num_upsample_blocks):
        res *= 2
        total += 3 * (2.0 * res * res * c * c * 9) + (2.0 * (res // 2) ** 2 * c * c if i == 0 else 0.0)
    return 3 * total  # three planes


def compare_conv():
    """The windowed evaluation under AMAV_UPSAMPLER_CONV = library / hip, alternating on one plan."""
    modes = ("library", "hip") if CONV == "both" else (CONV,)
    R, rounds = cfg.triplane_resolution, 5
    launches = []  # (start event, stop event, issued FLOP) of every HIP convolution
    conv = ops.conv3x3_cells

    def timed_conv(x, weights_split, cout, *a, **k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        y = conv(x, weights_split, cout, *a, **k)
        e1.record()
        launches.append((e0, e1, 3 * 2.0 * y.shape[0] * y.shape[1] * y.shape[2] * 9 * x.shape[3] * cout))
        return y

    ops.conv3x3_cells = timed_conv
    with torch.no_grad():
        pts = r.get_smpl_vertices(smpl)
        plan = up.plan_windows(pts, R, cfg.radius)
        slabs, times = {}, {m: [] for m in modes}
        for m in modes:  # warm-up: kernel selection of the library, prepared weights of the HIP path
            os.environ["AMAV_UPSAMPLER_CONV"] = m
            for _ in range(2):
                slabs[m] = up.forward_tokens_windowed(tokens[0], R, plan).clone()
        torch.cuda.synchronize()
        launches.clear()
        for _ in range(rounds):
            for m in modes:
                os.environ["AMAV_UPSAMPLER_CONV"] = m
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                up.forward_tokens_windowed(tokens[0], R, plan)
                torch.cuda.synchronize()
                times[m].append((time.perf_counter() - t0) * 1e3 / F)
    os.environ.pop("AMAV_UPSAMPLER_CONV", None)
    ops.conv3x3_cells = conv
    tiles = sum(len(w["tiles"]) for w in plan if w["tiles"] is not None)
    print(f"windowed upsampler, {F} frames, {tiles} active tiles, {rounds} alternating rounds (median, min .. max):")
    for m in modes:
        t = sorted(times[m])
        print(f"  {m:8s} {t[len(t) // 2]:7.2f} ms per frame ({t[0]:.2f} .. {t[-1]:.2f})")
    if launches:
        ms = sum(a.elapsed_time(b) for a, b, _ in launches) / rounds
        flop = sum(f for _, _, f in launches) / rounds
        tf = flop / (ms * 1e-3) / 1e12
        print(f"  hip convolutions: {len(launches) // rounds} launches, {ms / F:.2f} ms per frame by HIP events (the operand sweep "
              f"included), {flop / F / 1e12:.3f} TFLOP issued per frame -> {tf:.0f} TFLOP/s = "
              f"{tf / MFMA_16BIT_PEAK_TFLOPS * 100:.1f} % of the 16-bit MFMA peak ({MFMA_16BIT_PEAK_TFLOPS:.0f}); "
              f"fp32-equivalent {tf / 3:.0f} TFLOP/s")
    if CONV == "both":
        r_out, t = R * 2 ** cfg.num_upsample_blocks, 4 * 2 ** cfg.num_upsample_blocks
        a, b = (slabs[m].view(F, -1, 3, r_out, r_out) for m in modes)
        err = max(float((a[f, :, p, ty * t:(ty + 1) * t, tx * t:(tx + 1) * t]
                         - b[f, :, p, ty * t:(ty + 1) * t, tx * t:(tx + 1) * t]).abs().max())
                  for p, w in enumerate(plan) if w["tiles"] is not None for f, ty, tx in w["tiles"].tolist())
        print(f"  max |library - hip| inside the active tiles {err:.2e} (largest |value| {float(a.abs().max()):.2e})")


def compare_conv_grad():
    """Forward + backward of the windowed evaluation under AMAV_UPSAMPLER_CONV_GRAD = library / hip, alternating on one
    plan; then every HIP backward call of one step replayed alone: its data gradient (with the column sums and the
    operand's row kernel) and its weight gradient under HIP events."""
    modes = ("library", "hip") if CONV == "both" else (CONV,)
    R, rounds = cfg.triplane_resolution, 3
    r_out = R * 2 ** cfg.num_upsample_blocks
    with torch.no_grad():
        pts = r.get_smpl_vertices(smpl).contiguous()
        plan = up.plan_windows(pts, R, cfg.radius)
    tok = tokens[0].clone().requires_grad_()
    weights = torch.randn(F, pts.shape[1], 3 * cfg.triplane_feature_dim, generator=torch.Generator().manual_seed(3)).cuda()

    def step():
        r.zero_grad(set_to_none=True)
        tok.grad = None
        slab = up.forward_tokens_windowed(tok, R, plan, differentiable=True)
        planes = slab.view(F, -1, 3, r_out, r_out).permute(0, 2, 1, 3, 4)
        (ops.triplane_sample_features_differentiable(planes, pts, cfg.radius) * weights).sum().backward()

    times, peaks = {m: [] for m in modes}, {m: 0.0 for m in modes}
    for m in modes:
        os.environ["AMAV_UPSAMPLER_CONV_GRAD"] = m
        step()
    for _ in range(rounds):
        for m in modes:
            os.environ["AMAV_UPSAMPLER_CONV_GRAD"] = m
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            step()
            torch.cuda.synchronize()
            times[m].append((time.perf_counter() - t0) * 1e3 / F)
            peaks[m] = max(peaks[m], torch.cuda.max_memory_allocated() / 2 ** 30)
    tiles = sum(len(w["tiles"]) for w in plan if w["tiles"] is not None)
    print(f"windowed upsampler, forward + backward, {F} frames per call, {tiles} active tiles, {rounds} alternating rounds "
          f"(median, min .. max):")
    for m in modes:
        t = sorted(times[m])
        print(f"  {m:8s} {t[len(t) // 2]:7.2f} ms per frame ({t[0]:.2f} .. {t[-1]:.2f}), peak allocated {peaks[m]:.2f} GiB", flush=True)
    if "hip" in modes:
        os.environ["AMAV_UPSAMPLER_CONV_GRAD"] = "hip"
        backward, recorded = ops.conv3x3_cells_backward, []
        ops.conv3x3_cells_backward = lambda *a, **k: (recorded.append((a, k)), backward(*a, **k))[1]
        step()
        ops.conv3x3_cells_backward = backward
        torch.cuda.synchronize()
        totals = {"data": [0.0, 0.0], "weight": [0.0, 0.0]}  # ms, FLOP
        with torch.no_grad():
            for a, k in recorded:
                K, H, W, cout = a[0].shape
                flop = 3 * 2.0 * K * H * W * 9 * a[1].shape[3] * cout
                parts = {"data": dict(k, want_weight=False), "weight": dict(k, want_x=False, want_bias=False, want_prologue=False)}
                for name, kw in parts.items():
                    if not (kw["want_x"] or kw["want_weight"] or kw["want_bias"] or kw["want_prologue"]):
                        continue
                    backward(*a, **kw)  # warm-up
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    backward(*a, **kw)
                    e1.record()
                    torch.cuda.synchronize()
                    totals[name][0] += e0.elapsed_time(e1)
                    totals[name][1] += flop if (name == "weight" or kw["want_x"] or kw["want_prologue"]) else 0.0
        for name, (ms, flop) in totals.items():
            tf = flop / max(ms, 1e-9) / 1e9
            print(f"  hip {name} gradient: {len(recorded)} calls, {ms / F:.2f} ms per frame by HIP events (sweeps, column sums and "
                  f"workspace allocation included), {flop / F / 1e12:.3f} TFLOP issued per frame -> {tf:.0f} TFLOP/s = "
                  f"{tf / MFMA_16BIT_PEAK_TFLOPS * 100:.1f} % of the 16-bit MFMA peak ({MFMA_16BIT_PEAK_TFLOPS:.0f})")
    os.environ.pop("AMAV_UPSAMPLER_CONV_GRAD", None)


if CONV:
    compare_conv_grad() if "--backward" in sys.argv else compare_conv()
    sys.exit(0)

with torch.no_grad():
    for _ in range(2):
        out = up.forward_tokens(tokens[0], cfg.triplane_resolution)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    reps = 3
    for _ in range(reps):
        out = up.forward_tokens(tokens[0], cfg.triplane_resolution)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / reps / F
print(f"TriplaneUpsampler, full planes: {dt * 1e3:.1f} ms per frame, {flops() / 1e12:.2f} TFLOP per frame -> "
      f"{flops() / dt / 1e12:.1f} TFLOP/s; output {tuple(out.shape)}")

# windowed: blocks 1..3 on the bounding box of the active tiles, the last block on the active tiles only
with torch.no_grad():
    pts = r.get_smpl_vertices(smpl)
    plan = up.plan_windows(pts, cfg.triplane_resolution, cfg.radius)
    for _ in range(2):
        win = up.forward_tokens_windowed(tokens[0], cfg.triplane_resolution, plan)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        plan = up.plan_windows(pts, cfg.triplane_resolution, cfg.radius)
        win = up.forward_tokens_windowed(tokens[0], cfg.triplane_resolution, plan)
    torch.cuda.synchronize()
    dw = (time.perf_counter() - t0) / reps / F
    R = cfg.triplane_resolution
    cells = sum((w["crop"][1] - w["crop"][0]) * (w["crop"][3] - w["crop"][2]) for w in plan) / (3 * R * R)
    tiles = sum(int(w["mask"].sum()) for w in plan) / (3 * F * (R // 4) ** 2)
    r_out, t = R * 16, 64
    fv, wv = out.view(F, -1, 3, r_out, r_out), win.view(F, -1, 3, r_out, r_out)
    err = max(float((fv[f, :, p, ty * t:(ty + 1) * t, tx * t:(tx + 1) * t] - wv[f, :, p, ty * t:(ty + 1) * t, tx * t:(tx + 1) * t]).abs().max())
              for p, w in enumerate(plan) for f, ty, tx in torch.nonzero(w["mask"]).tolist())
print(f"windowed: {dw * 1e3:.1f} ms per frame; crops {[w['crop'] for w in plan]} = {cells * 100:.0f} % of the cells for blocks 1-3, "
      f"{tiles * 100:.0f} % of the tiles for block 4 (tiled: {[w['tiles'] is not None for w in plan]}); "
      f"max |full - windowed| inside the active tiles {err:.2e}")

if "--backward" in sys.argv:
    del out, win, fv, wv
    r.triplane_upsampler._slab = None
    torch.cuda.empty_cache()
    R, radius = cfg.triplane_resolution, cfg.radius
    r_out = R * 2 ** cfg.num_upsample_blocks
    cut_events = []

    def timed_op(fn):
        def wrapper(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            res = fn(*a, **k)
            e1.record()
            cut_events.append((e0, e1))
            return res
        return wrapper

    ops.windows_cut, ops.windows_cut_backward = timed_op(ops.windows_cut), timed_op(ops.windows_cut_backward)

    def run(label, frames, upsample):
        g = torch.Generator().manual_seed(3)
        tok = tokens[0, :frames].clone().requires_grad_()
        points = pts[:frames].contiguous()
        weights = torch.randn(frames, points.shape[1], 3 * cfg.triplane_feature_dim, generator=g).cuda()

        def step():
            r.zero_grad(set_to_none=True)
            tok.grad = None
            slab = upsample(tok, points)
            planes = slab.view(frames, -1, 3, r_out, r_out).permute(0, 2, 1, 3, 4)
            (ops.triplane_sample_features_differentiable(planes, points, radius) * weights).sum().backward()

        step()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        cut_events.clear()
        t0 = time.perf_counter()
        for _ in range(reps):
            step()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / reps
        cut = sum(a.elapsed_time(b) for a, b in cut_events) / reps
        print(f"{label}: forward + backward {dt * 1e3 / frames:.1f} ms per frame ({frames} frames per call), peak allocated "
              f"{torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB; window cut kernels {cut:.2f} ms per call = "
              f"{cut / (dt * 1e3) * 100:.2f} % of it ({len(cut_events) // reps} launches)", flush=True)
        return {k: p.grad.clone() for k, p in up.named_parameters()}, tok.grad.clone()

    def windowed(tok, points):
        with torch.no_grad():
            plan = up.plan_windows(points, R, radius)
        return up.forward_tokens_windowed(tok, R, plan, differentiable=True)

    gw, tw = run("windowed, autograd", F, windowed)
    gw2, tw2 = run("windowed, autograd (again)", F, windowed)
    same = all(torch.equal(gw[k], gw2[k]) for k in gw) and torch.equal(tw, tw2)
    print(f"two windowed runs bit-identical: {same}" + ("" if same else "; worst relative difference " + format(max(
        float((gw[k] - gw2[k]).abs().max() / gw[k].abs().max().clamp_min(1e-30)) for k in gw), ".2e")), flush=True)
    del gw, gw2, tw, tw2
    torch.cuda.empty_cache()
    run("full planes, autograd", min(F, FULL_FRAMES), lambda tok, points: up.forward_tokens(tok, R))
