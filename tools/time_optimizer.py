#!/usr/bin/env python3
"""Diagnostic: what the tail of a training step costs -- the clip of the global gradient norm plus the Adam update -- on
three paths over the same parameters and seeded random gradients:

  library        optim.Adam(backend="library"): torch.nn.utils.clip_grad_norm_ + the library's default (foreach) Adam,
                 the only path before csrc/optimizer.hip
  library_fused  clip_grad_norm_ + torch.optim.Adam(fused=True)
  hip            optim.Adam(backend="hip"): amav_grad_norm_clip + amav_adam_step, three launches
  hip_launches   those three launches alone, over tables built once: `hip` without step()'s walk over the parameters
  hip_norm_launches  the two launches of the norm alone (4 B per parameter)

Parameter sets: `model` = AudioDrivenAvatar at the default config (every parameter), and `survey` = SURVEY.md's estimate
of the reference's trainable set, 2e8 fp32 parameters in 400 equal tensors (--no-survey skips it).

One process; after a warm-up of every path the three alternate in rounds, every round timing `repeats` steps one by one
between device events (a step's time includes the gaps the host leaves between its launches: that is what the training
loop waits for).  Reported per path: the median over rounds of the round medians and the spread (max - min) of the round
medians.  Next to `hip`: the traffic model of DESIGN.md section 4.20 -- 4 B per parameter for the norm, 28 B for the update
-- at the 6.29 TB/s a float4 copy reaches on the MI355X, and the fraction of that rate the step achieves.
Prints one JSON line.

--data-parallel: the data-parallel step instead ("Data-parallel step"), on the `model` set in a
one-rank RCCL group -- what the step costs a rank apart from the wire, which one GPU cannot show:

  hip                optim.Adam(backend="hip") as above
  hip_data_parallel  optim.Adam(backend="hip", process_group=<the one-rank group>): pack + all-reduce + the three launches
  pack_launch        amav_grads_pack alone over tables built once: 8 B per parameter (a read and a write)

The same rounds, the same events; next to pack_launch its fraction of the float4 copy rate.

usage: time_optimizer.py [rounds] [repeats] [--no-survey] [--data-parallel]"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from audio_motion_avatar_amd import ops, optim  # noqa: E402

COPY_TB_PER_S = 6.29    # float4 copy, measured
BYTES_PER_PARAM = 4 + 28


def step_ms(step, repeats):
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def library_fused(params):
    opt = torch.optim.Adam(params, lr=1e-4, fused=True)

    def step():
        torch.nn.utils.clip_grad_norm_(params, 1.0)
        opt.step()
    return step


def launches_only(params, chunk):
    """The two entry points over tables built once from `params`, their gradients and a fresh state."""
    state = [(torch.zeros_like(p), torch.zeros_like(p)) for p in params]
    tensors, chunk_table = ops.optimizer_tables([p.numel() for p in params], [0] * len(params), chunk)
    for t, p, (m, v) in zip(tensors, params, state):
        t.param, t.grad, t.exp_avg, t.exp_avg_sq = p.data_ptr(), p.grad.data_ptr(), m.data_ptr(), v.data_ptr()
    tables = (ops.optimizer_table_to_device(tensors, "cuda"), len(tensors), ops.optimizer_table_to_device(chunk_table, "cuda"),
              len(chunk_table), chunk)
    partial, norm = torch.empty(len(chunk_table), dtype=torch.float64, device="cuda"), torch.empty(2, device="cuda")
    groups = [ops.optimizer_group(1e-4, (0.9, 0.999), 1e-8, 0.0, 10)]

    def step():
        ops.grad_norm_clip(*tables, 1.0, partial=partial, norm=norm)
        ops.adam_step(*tables, groups, coef=norm[1:])
        return state   # kept alive by the closure
    return step, lambda: ops.grad_norm_clip(*tables, 1.0, partial=partial, norm=norm)


def pack_only(params, chunk):
    """amav_grads_pack over tables built once from the gradients of `params`, into a bucket of its own."""
    tensors, chunk_table = ops.optimizer_tables([p.numel() for p in params], [0] * len(params), chunk)
    for t, p in zip(tensors, params):
        t.grad = p.grad.data_ptr()
    offsets, total = ops.bucket_offsets([p.numel() for p in params])
    bucket = torch.zeros(total, device="cuda")
    offsets_dev = torch.tensor(offsets, dtype=torch.int64, device="cuda")
    tables = (ops.optimizer_table_to_device(tensors, "cuda"), len(tensors), ops.optimizer_table_to_device(chunk_table, "cuda"),
              len(chunk_table), chunk)
    return lambda: ops.grads_pack(*tables, offsets_dev, bucket, scale=1.0)


def rounds_of(paths, rounds, repeats):
    """Warm every path up, then let them alternate -> {name: the round medians}."""
    for step in paths.values():   # warm-up: code objects, the state, the tables, the allocator
        for _ in range(3):
            step()
    torch.cuda.synchronize()
    medians = {name: [] for name in paths}
    for _ in range(rounds):
        for name, step in paths.items():
            medians[name].append(step_ms(step, repeats))
    return medians


def data_parallel_numbers(params, rounds, repeats):
    import tempfile

    import torch.distributed as dist

    g = torch.Generator(device="cuda").manual_seed(0)
    for p in params:
        p.grad = torch.randn(p.shape, generator=g, device="cuda") * 1e-3
    with tempfile.TemporaryDirectory() as d:
        dist.init_process_group("nccl", init_method=f"file://{os.path.join(d, 'rendezvous')}", rank=0, world_size=1)
        try:
            paths = {"hip": optim.Adam(params, lr=1e-4, backend="hip").step,
                     "hip_data_parallel": optim.Adam(params, lr=1e-4, backend="hip", process_group=dist.group.WORLD).step,
                     "pack_launch": pack_only(params, ops.OPTIM_CHUNK)}
            medians = rounds_of(paths, rounds, repeats)
        finally:
            dist.destroy_process_group()
    count = sum(p.numel() for p in params)
    res = {"tensors": len(params), "parameters": count}
    for name, m in medians.items():
        ms = statistics.median(m)
        res[name] = {"ms": round(ms, 4), "spread_ms": round(max(m) - min(m), 4)}
    ms, model_ms = res["pack_launch"]["ms"], count * 8 / (COPY_TB_PER_S * 1e12) * 1e3
    res["pack_launch"].update(model_ms_at_copy_rate=round(model_ms, 4), tb_per_s=round(count * 8 / (ms * 1e-3) / 1e12, 3),
                              fraction_of_copy_rate=round(model_ms / ms, 3))
    return res


def numbers(params, rounds, repeats):
    g = torch.Generator(device="cuda").manual_seed(0)
    for p in params:
        p.grad = torch.randn(p.shape, generator=g, device="cuda") * 1e-3
    paths = {"library": optim.Adam(params, lr=1e-4, backend="library").step, "library_fused": library_fused(params),
             "hip": optim.Adam(params, lr=1e-4, backend="hip").step}
    paths["hip_launches"], paths["hip_norm_launches"] = launches_only(params, ops.OPTIM_CHUNK)
    medians = rounds_of(paths, rounds, repeats)
    count = sum(p.numel() for p in params)
    res = {"tensors": len(params), "parameters": count}
    for name, m in medians.items():
        ms = statistics.median(m)
        res[name] = {"ms": round(ms, 4), "spread_ms": round(max(m) - min(m), 4)}
        if name.startswith("hip"):
            nbytes = count * (4 if name == "hip_norm_launches" else BYTES_PER_PARAM)
            model_ms = nbytes / (COPY_TB_PER_S * 1e12) * 1e3
            res[name].update(model_ms_at_copy_rate=round(model_ms, 4), tb_per_s=round(nbytes / (ms * 1e-3) / 1e12, 3),
                             fraction_of_copy_rate=round(model_ms / ms, 3))
    return res


if __name__ == "__main__":
    if not torch.cuda.is_available():
        raise SystemExit("time_optimizer.py needs an MI355X")
    numbers_given = [int(a) for a in sys.argv[1:] if a.isdigit()]
    rounds, repeats = (numbers_given + [5, 5][len(numbers_given):])[:2]
    from audio_motion_avatar_amd.harness import AudioDrivenAvatar

    res = {"rounds": rounds, "repeats": repeats, "chunk": ops.OPTIM_CHUNK}
    model = AudioDrivenAvatar()
    if "--data-parallel" in sys.argv:
        res["model_data_parallel"] = data_parallel_numbers([p for p in model.parameters() if p.requires_grad], rounds, repeats)
        print(json.dumps(res))
        raise SystemExit(0)
    res["model"] = numbers([p for p in model.parameters() if p.requires_grad], rounds, repeats)
    del model
    torch.cuda.empty_cache()
    if "--no-survey" not in sys.argv:
        g = torch.Generator(device="cuda").manual_seed(1)
        survey = [torch.nn.Parameter(torch.randn(500_000, generator=g, device="cuda")) for _ in range(400)]
        res["survey"] = numbers(survey, rounds, repeats)
    print(json.dumps(res))
