#!/usr/bin/env python3
"""Diagnostic: the self-attention backward at the reference shape (B = 1, S = 6304, H = 8, D = 64) -- forward with the
row log-sum-exp, backward, and the backward's three kernels (delta pre-pass, key-major dK/dV, query-major dQ) -- and one
full stage-2 training step (AudioDrivenAvatar.training_step forward + backward, 6 output frames, 8 layers, 512^2
frames, B = 1) with its peak allocated memory.  Times are medians over repeats between HIP events; the per-kernel split
is the profiler's device time of each kernel, median over the same repeats.  Prints one JSON line.

--arithmetics [rounds]: instead, the exact-fp32 backward and the fp16 x 2 split-product backward (arithmetic="f32" /
"split") alternating in one process, `rounds` rounds (default 3) of medians of 10 calls each, at the
self-attention reference shape and the two stage-1 cross-attention shapes (Sq = 3152 and 80 over Sk = 4096, B = 1,
H = 8): per arithmetic the median over the rounds, the spread between them and the per-kernel split; with --step also
the stage-2 training step under AMAV_ATTN_BACKWARD=f32 and =split, alternating."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from audio_motion_avatar_amd import ops  # noqa: E402


def timed(fn, repeats, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def kernel_split(fn, repeats):
    """median device ms per call of each kernel whose name mentions attn_bwd (torch.profiler)."""
    from torch.profiler import ProfilerActivity, profile

    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(repeats):
            fn()
        torch.cuda.synchronize()
    times = {}
    for e in prof.events():
        if e.device_type.name == "CUDA" and "attn_bwd" in e.name:
            key = e.name.split("(")[0].split("<")[0].split("::")[-1]  # "void ns::kernel<64, ns::Rows>(...)" -> kernel
            times.setdefault(key, []).append(e.device_time / 1e3 if hasattr(e, "device_time") else e.cuda_time / 1e3)
    return {k: round(statistics.median(v), 4) for k, v in times.items()}


def attention_numbers(repeats):
    B, S, H = 1, 6304, 8
    g = torch.Generator().manual_seed(0)
    qkv = torch.randn(B, S, 3 * H * 64, generator=g).cuda()
    dout = torch.randn(B, S, H * 64, generator=g).cuda()
    out, lse = ops.selfattn_lse(qkv, H)
    grad = torch.empty(B, S, 3 * H * 64, device="cuda")
    fwd = timed(lambda: ops.selfattn_lse(qkv, H), repeats)
    bwd = timed(lambda: ops.selfattn_backward(qkv, out, lse, dout, H, grad_qkv=grad), repeats)
    split = kernel_split(lambda: ops.selfattn_backward(qkv, out, lse, dout, H, grad_qkv=grad), repeats)
    flop = 10.0 * B * H * S * S * 64
    return {"forward_lse_ms": round(fwd, 4), "backward_ms": round(bwd, 4), "backward_kernels_ms": split,
            "backward_tflops_fp32": round(flop / (bwd * 1e-3) / 1e12, 1)}


def alternate(sides, rounds, repeats=10):
    """{name: fn} timed in turn, `rounds` times -> {name: {"ms": median of the rounds, "spread_ms": max - min}}."""
    seen = {name: [] for name in sides}
    for _ in range(rounds):
        for name, fn in sides.items():
            seen[name].append(timed(fn, repeats))
    return {name: {"ms": round(statistics.median(v), 4), "spread_ms": round(max(v) - min(v), 4)} for name, v in seen.items()}


def arithmetic_numbers(rounds):
    """f32 and split backwards alternating at (B, Sq, Sk, H) = the self-attention reference shape and the two stage-1
    cross-attention shapes."""
    H, HD = 8, 8 * 64
    g = torch.Generator().manual_seed(0)
    res = {}
    S = 6304
    qkv = torch.randn(1, S, 3 * HD, generator=g).cuda()
    dout = torch.randn(1, S, HD, generator=g).cuda()
    out, lse = ops.selfattn_lse(qkv, H)
    grad = torch.empty(1, S, 3 * HD, device="cuda")
    sides = {a: (lambda a=a: ops.selfattn_backward(qkv, out, lse, dout, H, grad_qkv=grad, arithmetic=a))
             for a in ("f32", "split")}
    res[f"self_{S}"] = alternate(sides, rounds)
    for a, fn in sides.items():
        res[f"self_{S}"][a]["kernels_ms"] = kernel_split(fn, 10)
    for Sq, Sk in ((3152, 4096), (80, 4096)):
        q = torch.randn(1, Sq, HD, generator=g).cuda()
        kv = torch.randn(1, Sk, 2 * HD, generator=g).cuda()
        xdout = torch.randn(1, Sq, HD, generator=g).cuda()
        xout, xlse = ops.crossattn_lse(q, kv, H)
        dq, dkv = torch.empty(1, Sq, HD, device="cuda"), torch.empty(1, Sk, 2 * HD, device="cuda")
        sides = {a: (lambda a=a: ops.crossattn_backward(q, kv, xout, xlse, xdout, H, grad_q=dq, grad_kv=dkv, arithmetic=a))
                 for a in ("f32", "split")}
        res[f"cross_{Sq}x{Sk}"] = alternate(sides, rounds)
        for a, fn in sides.items():
            res[f"cross_{Sq}x{Sk}"][a]["kernels_ms"] = kernel_split(fn, 10)
    return res


def arithmetic_step_numbers(rounds):
    """The stage-2 training step under AMAV_ATTN_BACKWARD=f32 and =split (read per call), alternating."""
    step, info = stage2_step()

    def under(value):
        def run():
            os.environ["AMAV_ATTN_BACKWARD"] = value
            try:
                return step()
            finally:
                os.environ.pop("AMAV_ATTN_BACKWARD", None)
        return run

    under("f32")()
    torch.cuda.synchronize()
    return {**alternate({"f32": under("f32"), "split": under("split")}, rounds, repeats=3), **info}


def stage2_step(train_transformer=False):
    """-> (step, info): step() runs one AudioDrivenAvatar.training_step forward + backward at the reference configuration
    (B = 1) on seeded inputs.  The model is in .eval(); train_transformer puts .train() on audio_triplane.transformer
    alone (its blocks are then checkpointed; the reducer's dropout stays off, so the loss is the same)."""
    from audio_motion_avatar_amd.config import ModelConfig
    from audio_motion_avatar_amd.harness import AudioDrivenAvatar
    from audio_motion_avatar_amd.synthetic import init_random_heads, make_render_inputs

    torch.manual_seed(0)  # the same weights in every process
    cfg = ModelConfig()
    cfg.renderer.differentiable_smplx = True
    model = AudioDrivenAvatar(cfg)
    init_random_heads(model.renderer)
    model = model.cuda().eval()
    if train_transformer:
        model.audio_triplane.transformer.train()
    a, r = cfg.triplane_audio_net, cfg.renderer
    T = a.triplane_output_frames
    _, smpl, cam = make_render_inputs(T, r, seed=1)
    g = torch.Generator().manual_seed(2)
    tri = torch.randn(1, a.triplane_input_frames, a.triplane_feature_dim, 3 * a.triplane_resolution ** 2, generator=g)
    st = torch.randn(1, a.triplane_input_frames, a.smpl_token_dim, a.smpl_token_len, generator=g) * 0.2
    audio = torch.randn(1, T, a.audio_feature_dim, generator=g)
    Hh, Ww = r.image_size
    target = torch.rand(1, T, 3, Hh, Ww, generator=g)
    tri, st, audio, target = (t.cuda() for t in (tri, st, audio, target))

    def step():
        model.zero_grad(set_to_none=True)
        loss, _ = model.training_step(tri, st, audio, cam, target, smpl)
        loss.backward()
        return loss

    return step, {"frames": T, "layers": a.transformer_layers, "image": list(r.image_size)}


def training_step_numbers(repeats):
    step, info = stage2_step()
    step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    ms = timed(step, repeats, warmup=1)
    return {"training_step_ms": round(ms, 2), "training_step_peak_gib": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2),
            **info}


if __name__ == "__main__":
    if "--arithmetics" in sys.argv:
        at = sys.argv.index("--arithmetics")
        rounds = int(sys.argv[at + 1]) if len(sys.argv) > at + 1 and sys.argv[at + 1].isdigit() else 3
        res = {"attention_backward_arithmetics": arithmetic_numbers(rounds)}
        if "--step" in sys.argv:
            res["training_step_ms"] = arithmetic_step_numbers(rounds)
        print(json.dumps(res))
        sys.exit(0)
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 10
    res = {"attention": attention_numbers(repeats)}
    if "--no-step" not in sys.argv:
        res["training_step"] = training_step_numbers(max(3, repeats // 3))
    print(json.dumps(res))
