#!/usr/bin/env python3
"""Diagnostic: linear layers under autograd on bf16 x 3 split products.  Prints one JSON line with
  * per reference projection at rows = 6304 (512 -> 1536, 512 -> 512, 512 -> 4096, 2048 -> 512) the HIP-event times of
    forward, dgrad and wgrad on the split path -- its split kernels included, the memoised weight operands excluded --
    next to the library's fp32 products (for wgrad also its two split kernels alone, its bf16 GEMM alone, and that GEMM
    with the contraction cut by hand into 12 and 24 slices: torch.bmm + a sum), the backward as
    ops.linear_split_differentiable runs it (both operands of the gradient from one read) next to the two fp32 products,
    and whether two identical backward calls give a bit-identical dW;
  * the transposing split kernel alone on the [6304, N] gradients, with and without the row-major operand, next to its byte
    floor (4 B read + 12 B, or 24 B, written per element);
  * the stage-2 training step of tools/bench_transformer_training.py with AMAV_TRAIN_GEMM=f32 and =split, in eval mode and
    with checkpointed blocks.  Every setting runs in a fresh child process, the settings alternating over --rounds
    rounds, one warm-up and --steps timed steps each; ms is the median over all timed steps of a setting.
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

SETTINGS = [("f32", "eval"), ("split", "eval"), ("f32", "checkpointed"), ("split", "checkpointed")]
ROWS = 6304
PROJECTIONS = [("qkv", 512, 1536), ("to_out", 512, 512), ("ff_in", 512, 4096), ("ff_out", 2048, 512)]


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
        return round(statistics.median(out) * 1e3, 1)  # us

    g = torch.Generator().manual_seed(0)
    rand = lambda *shape: torch.randn(*shape, generator=g).cuda()
    mm = lambda a, b: torch.mm(a, b.t(), out_dtype=torch.float32)
    res = {"products_us": {}, "split_transposed": {}}
    for name, K, N in PROJECTIONS:
        x, w, up = rand(ROWS, K), rand(N, K) * K ** -0.5, rand(ROWS, N)
        ws, wt = ops.split_operand(w, weights=True), ops.split_operand_transposed(w, weights=True)
        xr, wr = x.clone().requires_grad_(), w.clone().requires_grad_()

        def backward(fn):
            y = fn(xr, wr)
            return lambda: torch.autograd.grad(y, (xr, wr), up, retain_graph=True)

        split_bwd = backward(lambda a, b: ops.linear_split_differentiable(a, b, None, lambda: ws, lambda: wt))
        dw_a, dw_b = split_bwd()[1], split_bwd()[1]
        res["products_us"][name] = {
            "K": K, "N": N,
            "forward": {"split": timed(lambda: mm(ops.split_operand(x), ws)), "f32": timed(lambda: torch.mm(x, w.t()))},
            "dgrad": {"split": timed(lambda: mm(ops.split_operand(up), wt)), "f32": timed(lambda: torch.mm(up, w))},
            "wgrad": {"split": timed(lambda: mm(ops.split_operand_transposed(up),
                                                ops.split_operand_transposed(x, weights=True))),
                      "f32": timed(lambda: torch.mm(up.t(), x)), **sliced_wgrad(timed, ops, up, x)},
            "backward": {"split": timed(split_bwd), "f32": timed(backward(torch.nn.functional.linear))},
            "dW_bit_identical_between_calls": bool(torch.equal(dw_a, dw_b))}
        for also_rows in (False, True):
            us = timed(lambda: ops.split_operand_transposed(up, also_rows=also_rows))
            floor = ROWS * N * (4 + (24 if also_rows else 12))
            res["split_transposed"][f"{ROWS}x{N}" + ("+rows" if also_rows else "")] = {
                "us": us, "floor_bytes": floor, "gb_per_s": round(floor / (us * 1e-6) / 1e9, 1)}
    return res


def sliced_wgrad(timed, ops, up, x):
    """The wgrad contraction cut by hand into 12 and 24 slices (torch.bmm over strided views of both transposed
    operands, then a sum over the slices): what a split-K of the library's bf16 GEMM would buy.  Not on the product path.
    -> us of the two split kernels alone, of the one bf16 GEMM alone, and of bmm + sum per slice count."""
    import torch

    gt, xt = ops.split_operand_transposed(up), ops.split_operand_transposed(x, weights=True)
    splits = lambda: (ops.split_operand_transposed(up), ops.split_operand_transposed(x, weights=True))
    res = {"split_kernels": timed(splits),
           "gemm_alone": timed(lambda: torch.mm(gt, xt.t(), out_dtype=torch.float32))}
    for slices in (12, 24):
        length = gt.shape[1] // slices
        if gt.shape[1] % slices or length % 8:
            continue
        a = gt.view(gt.shape[0], slices, length).transpose(0, 1)
        b = xt.view(xt.shape[0], slices, length).permute(1, 2, 0)
        res[f"gemm_alone_{slices}_slices"] = timed(lambda: torch.bmm(a, b, out_dtype=torch.float32).sum(0))
    return res


def child(args_list, env=None):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + args_list, env=env, check=True,
                         stdout=subprocess.PIPE, text=True).stdout
    return json.loads(out.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=3, help="timed steps per child (at least 3)")
    ap.add_argument("--rounds", type=int, default=2, help="children per setting")
    ap.add_argument("--repeats", type=int, default=10, help="timed batches per kernel")
    ap.add_argument("--no-step", action="store_true", help="product and kernel times only")
    ap.add_argument("--child", nargs="+", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        if args.child[0] == "kernels":
            print(json.dumps(kernel_numbers(int(args.child[1]))))
        else:
            from bench_transformer_training import step_numbers

            print(json.dumps(step_numbers(args.child[0], int(args.child[1]))))
        return
    res = {"rows": ROWS, **child(["kernels", str(args.repeats)])}
    if not args.no_step:
        runs = {s: [] for s in SETTINGS}
        for _ in range(max(1, args.rounds)):
            for gemm, mode in SETTINGS:
                runs[gemm, mode].append(child([mode, str(max(3, args.steps))], dict(os.environ, AMAV_TRAIN_GEMM=gemm)))
        res["training_step"] = {}
        for (gemm, mode), rs in runs.items():
            medians = [statistics.median(r["ms"]) for r in rs]
            res["training_step"][f"{gemm}_{mode}"] = {
                "ms": round(statistics.median([t for r in rs for t in r["ms"]]), 2),
                "round_medians_ms": [round(m, 2) for m in medians], "spread_ms": round(max(medians) - min(medians), 2),
                "peak_gib": round(max(r["peak_gib"] for r in rs), 2), "loss": rs[0]["loss"]}
        res["training_step"]["config"] = {k: rs[0][k] for k in ("frames", "layers", "image")}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
