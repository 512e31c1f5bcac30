#!/usr/bin/env python3
"""Diagnostic: training the audio transformer on the fused row kernels and with gradient checkpointing (DESIGN.md section
4.15).  Prints one JSON line with
  * HIP-event times of the three backward entry points of csrc/attention_rows_backward.hip at the reference shape (rows =
    6304, dim = 512, inner = 2048) next to their algorithmic byte floors (bytes each must read and write once);
  * the stage-2 training step of tools/bench_attention_backward.py (forward + backward, B = 1) in four settings: library
    or fused rows (AMAV_TRAIN_ROWS) x eval or .train() on audio_triplane.transformer alone (checkpointed blocks; the
    reducer's dropout stays off, so all four compute the same loss).  Every setting runs in a fresh child process, the
    settings alternating over --rounds rounds, one warm-up and --steps timed steps each; ms is the median over all timed
    steps of a setting, spread the range of its per-round medians, peak the largest max_memory_allocated.
Only the children open the GPU, one at a time."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

SETTINGS = [("library", "eval"), ("fused", "eval"), ("library", "checkpointed"), ("fused", "checkpointed")]
ROWS, DIM, INNER = 6304, 512, 2048


def kernel_numbers(repeats, batch=20):
    import torch

    from audio_motion_avatar_amd import ops

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(batch):
                fn()
            b.record()
            torch.cuda.synchronize()
            out.append(a.elapsed_time(b) / batch)
        return statistics.median(out)

    g = torch.Generator().manual_seed(0)
    rand = lambda *shape: torch.randn(*shape, generator=g).cuda()
    proj, bias, dout = rand(ROWS, 2 * INNER), rand(2 * INNER), rand(ROWS, INNER)
    h, w, dnorm, dh_out = rand(1, ROWS, DIM), rand(DIM), rand(1, ROWS, DIM), rand(1, ROWS, DIM)
    dproj = ops.geglu_backward(proj, bias, dout)
    cases = {
        "geglu_backward": (lambda: ops.geglu_backward(proj, bias, dout), 5 * ROWS * INNER * 4),
        "add_layernorm_backward": (lambda: ops.add_layernorm_backward(h, w, 1e-5, dnorm, dh_out), 4 * ROWS * DIM * 4),
        "rows_colsum_4096": (lambda: ops.rows_colsum(dproj), (ROWS + 1) * 2 * INNER * 4),
        "rows_colsum_512": (lambda: ops.rows_colsum(h[0]), (ROWS + 1) * DIM * 4),
    }
    res = {}
    for name, (fn, floor_bytes) in cases.items():
        ms = timed(fn)
        res[name] = {"ms": round(ms, 4), "floor_bytes": floor_bytes, "gb_per_s": round(floor_bytes / (ms * 1e-3) / 1e9, 1)}
    return res


def step_numbers(mode, steps):
    import torch

    from bench_attention_backward import stage2_step

    step, info = stage2_step(train_transformer=(mode == "checkpointed"))
    loss = float(step().detach())  # warm-up
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    times = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return {"ms": times, "peak_gib": torch.cuda.max_memory_allocated() / 2 ** 30, "loss": loss, **info}


def child(args_list, env=None):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + args_list, env=env, check=True,
                         stdout=subprocess.PIPE, text=True).stdout
    return json.loads(out.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=3, help="timed steps per child (at least 3)")
    ap.add_argument("--rounds", type=int, default=2, help="children per setting")
    ap.add_argument("--repeats", type=int, default=10, help="timed batches per kernel")
    ap.add_argument("--no-step", action="store_true", help="kernel times only")
    ap.add_argument("--child", nargs="+", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        if args.child[0] == "kernels":
            print(json.dumps(kernel_numbers(int(args.child[1]))))
        else:
            print(json.dumps(step_numbers(args.child[0], int(args.child[1]))))
        return
    res = {"shape": {"rows": ROWS, "dim": DIM, "inner": INNER}, "kernels": child(["kernels", str(args.repeats)])}
    if not args.no_step:
        runs = {s: [] for s in SETTINGS}
        for _ in range(max(1, args.rounds)):
            for rows, mode in SETTINGS:
                runs[rows, mode].append(child([mode, str(max(3, args.steps))], dict(os.environ, AMAV_TRAIN_ROWS=rows)))
        res["training_step"] = {}
        for (rows, mode), rs in runs.items():
            medians = [statistics.median(r["ms"]) for r in rs]
            res["training_step"][f"{rows}_{mode}"] = {
                "ms": round(statistics.median([t for r in rs for t in r["ms"]]), 2),
                "round_medians_ms": [round(m, 2) for m in medians], "spread_ms": round(max(medians) - min(medians), 2),
                "peak_gib": round(max(r["peak_gib"] for r in rs), 2), "loss": rs[0]["loss"]}
        res["training_step"]["config"] = {k: rs[0][k] for k in ("frames", "layers", "image")}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
