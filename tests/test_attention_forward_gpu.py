"""The self-attention forward (csrc/attention.hip, through the C ABI) against float64 SDPA on the CPU: all three kernels
(amav_set_option("attn", default = fp16 x 2 | bf16 | f32)), sequence-length edges, both key-split regimes and forced
splits, magnitudes and online-softmax bookkeeping, proven bounds, and exact properties.

Inputs, reference, yardstick and bound come from attention_cases.py; the bound, for every variant and every case inside
the documented envelope, over every output element:

    max |out - sdpa64|  <=  4 err32 + 2^-22 max |v|      (err32: the CPU's float32 SDPA against float64)
                        <=  2e-5 max(1, max |sdpa64|)     (the ceiling of tests/test_attention_gpu.py)

Every test prints its figures (error, error / err32, error / max |v|, the split that ran) before it asserts."""
import contextlib
import functools
import os
import subprocess
import sys
import tempfile
import time

import pytest
import torch

import attention_cases as ac

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def variant(name):
    from audio_motion_avatar_amd import ops

    ops.set_option("attn", name)
    try:
        yield
    finally:
        ops.set_option("attn", "default")


def fused(case, pad=12):
    """The case's q, k, v as views of one [B, S, 3 H 64 + pad] device buffer: read through the fused-projection row
    stride, as the transformer does."""
    HD = case.heads * ac.D
    B, S, _ = case.q.shape
    buf = torch.cat([case.q, case.k, case.v, torch.zeros(B, S, pad)], dim=-1).cuda()
    return buf[..., :3 * HD], (buf[..., :HD], buf[..., HD:2 * HD], buf[..., 2 * HD:3 * HD])


def run(case, name, qkv=None):
    from audio_motion_avatar_amd import ops

    q, k, v = qkv if qkv is not None else fused(case)[1]
    with variant(name):
        return ops.selfattn(q, k, v, case.heads, scale=case.scale, bounds=case.bounds).cpu()


def library_nsplit(B, S, H):
    """The key split the library takes for this shape, from amav_selfattn_workspace_bytes under the f32 variant."""
    from audio_motion_avatar_amd import _lib

    with variant("f32"):
        return ac.nsplit_from_workspace_bytes(int(_lib.lib().amav_selfattn_workspace_bytes(B, S, H, ac.D)), B, S, H)


@functools.lru_cache(maxsize=None)
def unit(B, S, H):
    case = ac.unit_case(B, S, H)
    return case, ac.reference(case, lse=True)


@functools.lru_cache(maxsize=None)
def magnitude(name, B, S, H):
    case = ac.magnitude_case(name, B, S, H)
    return case, ac.reference(case, lse=True)


def check_default_lse(case, ref, out, label):
    """selfattn_lse on the same fused buffer: lse against fp64 logsumexp, out bit-equal to selfattn's."""
    from audio_motion_avatar_amd import ops

    out2, lse = ops.selfattn_lse(fused(case)[0], case.heads, scale=case.scale)
    ac.check_lse(lse.cpu(), ref, label)
    assert torch.equal(out2.cpu(), out), f"{label}: selfattn and selfattn_lse differ"


# ------------------------------------------------------------------------------------------- a. shapes x variants
@pytest.mark.parametrize("name", ac.VARIANTS)
@pytest.mark.parametrize("B,S,H", ac.SHAPES)
def test_shapes(B, S, H, name):
    """Unit randn at every tail length of the 64-key tile and the 32-key MFMA half, one and several (batch, head)
    slices, and the key-split regime (the split the library took is printed)."""
    case, ref = unit(B, S, H)
    out = run(case, name)
    label = f"{name} {case.name} nsplit={library_nsplit(B, S, H)}"
    ac.check(out, ref, label)
    if name == "default":
        check_default_lse(case, ref, out, label)


def test_shapes_cover_both_split_regimes_and_a_padded_round():
    """Over the shape list the library took one key slice and several, and at least once several slices whose count
    (nsplit H B) is not a multiple of 8: the main kernels' grid is padded to 8 slices per round there."""
    took = {shape: library_nsplit(*shape) for shape in ac.SHAPES}
    for (B, S, H), n in took.items():
        print(f"B={B} S={S} H={H}: nsplit={n}, {n * H * B} slices, tail of {S % 64} keys")
    assert any(n == 1 for n in took.values()) and any(n > 1 for n in took.values())
    assert any(n > 1 and (n * H * B) % 8 != 0 for (B, S, H), n in took.items())


# ----------------------------------------------------------------------- b. magnitudes and softmax bookkeeping
@pytest.mark.parametrize("name", ac.VARIANTS)
@pytest.mark.parametrize("B,S,H", [(1, 1000, 2), (2, 193, 3)])   # split with a 40-key tail; one slice, 1-key tail
@pytest.mark.parametrize("case_name", ac.MAGNITUDE_NAMES)
def test_magnitudes_and_bookkeeping(case_name, B, S, H, name):
    """Every case of attention_cases.MAGNITUDE_NAMES under the bound; one of them without the 2e-5 ceiling
    (attention_cases.CEILING_WAIVED: the float32 yardstick itself is twice above it)."""
    case, ref = magnitude(case_name, B, S, H)
    out = run(case, name)
    label = f"{name} {case.name} nsplit={library_nsplit(B, S, H)}"
    waived = (case_name, (B, S, H)) in ac.CEILING_WAIVED
    if waived:
        assert ref.err32 > ref.ceiling   # the reason of the waiver: the float32 yardstick itself is above the ceiling
    ac.check(out, ref, label, ceiling=not waived)
    if case_name in ac.ZERO_OUTPUT:
        assert torch.equal(out, torch.zeros_like(out))
    if name == "default":
        check_default_lse(case, ref, out, label)


# ------------------------------------------------------------------------------- c. proven bounds (fp16 x 2 kernel)
@functools.lru_cache(maxsize=None)
def bounds_reference(magnitudes):
    return ac.reference(ac.bounds_case(magnitudes, 1.0, "qkv"))


@pytest.mark.parametrize("magnitudes", list(ac.BOUNDS_MAGNITUDES))
@pytest.mark.parametrize("target", ac.BOUNDS_TARGETS)
@pytest.mark.parametrize("slack", ac.BOUNDS_SLACKS)
def test_proven_bounds(slack, target, magnitudes):
    """Bounds up to FP16_MAX_OVERSHOOT above the magnitudes, on all operands and on one at a time: the same bound as
    measured scaling, not a widened one."""
    case = ac.bounds_case(magnitudes, slack, target)
    ac.check(run(case, "default"), bounds_reference(magnitudes), "default " + case.name)


@pytest.mark.parametrize("edge", ac.BOUNDS_EDGES)
def test_proven_bound_edges(edge):
    case = ac.bounds_edge_case(edge)
    ac.check(run(case, "default"), ac.reference(case), "default " + case.name)


def test_slack_beyond_the_envelope_stays_under_the_ceiling():
    """Bounds 2^20 above the magnitudes (the transformer never exceeds 2^12): the documented degradation.  Finite and
    under the 2e-5 ceiling is all that is asserted; error / err32 is printed."""
    case = ac.bounds_case("unit", ac.BOUNDS_OUTSIDE, "qkv")
    ac.check(run(case, "default"), bounds_reference("unit"), "default " + case.name, envelope=False)


# ------------------------------------------------------------------------------------------ d. exact properties
PROPERTY_SHAPE = (1, 1000, 2)


@pytest.mark.parametrize("name", ac.VARIANTS)
@pytest.mark.parametrize("a,b", [(0, 7), (13, 0), (-40, 40), (40, -25)])
def test_power_of_two_invariance(a, b, name):
    """selfattn(q 2^a, k 2^-a, v 2^b) == selfattn(q, k, v) 2^b, bit for bit: every pre-scale of all three kernels is a
    power of two and the softmax scale multiplies q before any split, so only exponents change."""
    case, _ = unit(*PROPERTY_SHAPE)
    base = run(case, name)
    scaled = ac.Case("scaled", case.q * 2.0 ** a, case.k * 2.0 ** -a, case.v * 2.0 ** b, case.heads)
    assert torch.equal(run(scaled, name), base * 2.0 ** b)


@pytest.mark.parametrize("name", ac.VARIANTS)
def test_permuting_the_queries_permutes_the_rows(name):
    """A query's column of every MFMA depends on no other query, and a skipped rescale multiplies by exactly 1."""
    case, _ = unit(*PROPERTY_SHAPE)
    perm = torch.randperm(case.q.shape[1], generator=torch.Generator().manual_seed(11))
    permuted = ac.Case("permuted", case.q[:, perm].contiguous(), case.k, case.v, case.heads)
    assert torch.equal(run(permuted, name), run(case, name)[:, perm])


BOUNDS_FOR_PARTS = (8.0, 8.0, 8.0)   # the fp16 x 2 scales are per call: fixed bounds give a part of a call the same ones


def _part_vs_whole(name, whole_case, whole_ref, part_case, part_ref, rows, cols, what):
    """`part_case` is batch item / head `rows`, `cols` of `whole_case`, run as a call of its own: bit-equal where both
    calls take the same key split; otherwise each side within the bound, and the difference printed."""
    with_bounds = lambda c: ac.Case(c.name, c.q, c.k, c.v, c.heads, bounds=BOUNDS_FOR_PARTS)
    whole, part = run(with_bounds(whole_case), name), run(with_bounds(part_case), name)
    n_whole, n_part = library_nsplit(*whole_case.shape), library_nsplit(*part_case.shape)
    diff = float((whole[rows, :, cols] - part).abs().max())
    print(f"{name} {what}: whole {whole_case.shape} nsplit={n_whole}, part {part_case.shape} nsplit={n_part}, "
          f"difference {diff:.3e}")
    if n_whole == n_part:
        assert torch.equal(whole[rows, :, cols], part)
    else:
        ac.check(whole, whole_ref, f"{name} {what} whole")
        ac.check(part, part_ref, f"{name} {what} part")


@pytest.mark.parametrize("name", ac.VARIANTS)
@pytest.mark.parametrize("B,S,H", [(2, 500, 3), (2, 1100, 2), (2, 2081, 3)])   # at 256 CUs: 1 = 1, 2 = 2, 2 vs 4 slices
def test_batch_items_are_independent(B, S, H, name):
    case, ref = unit(B, S, H)
    for b in range(B):
        part = ac.Case(f"{case.name}[b={b}]", case.q[b:b + 1], case.k[b:b + 1], case.v[b:b + 1], H)
        _part_vs_whole(name, case, ref, part, ac.reference(part), slice(b, b + 1), slice(None), f"batch item {b}")


@pytest.mark.parametrize("name", ac.VARIANTS)
@pytest.mark.parametrize("B,S,H", [(2, 500, 3), (1, 2081, 3), (3, 1100, 5)])   # at 256 CUs: 1 = 1, 4 = 4, 1 vs 2 slices
def test_heads_are_independent(B, S, H, name):
    case, ref = unit(B, S, H)
    for h in range(H):
        cols = slice(h * ac.D, (h + 1) * ac.D)
        part = ac.Case(f"{case.name}[h={h}]", case.q[..., cols].contiguous(), case.k[..., cols].contiguous(),
                       case.v[..., cols].contiguous(), 1)
        _part_vs_whole(name, case, ref, part, ac.reference(part), slice(None), cols, f"head {h}")


@pytest.mark.parametrize("name", ac.VARIANTS)
def test_deterministic_and_stride_independent(name):
    case, _ = unit(*PROPERTY_SHAPE)
    _, qkv = fused(case, pad=36)
    first = run(case, name, qkv)
    assert torch.equal(run(case, name, qkv), first)
    contiguous = tuple(t.contiguous() for t in qkv)
    assert contiguous[0].stride(1) != qkv[0].stride(1)
    assert torch.equal(run(case, name, contiguous), first)


@pytest.mark.parametrize("name", ac.VARIANTS)
@pytest.mark.parametrize("scale", [1.0, 0.5, 0.125])
def test_known_answer_with_a_shifted_diagonal(scale, name):
    """S = 200 (a 8-key tail), query i attends key (i + 1) mod S only: the output is v rolled by one row, to the product
    precision of the split formats (the one-hot row leaves no other error)."""
    case = ac.known_answer_case(scale)
    ref = ac.reference(case)
    out = run(case, name)
    ac.check(out, ref, f"{name} {case.name}")
    assert float((out - case.v.roll(-1, dims=1)).abs().max()) <= ac.FLOOR * ref.vmax


# ------------------------------------------------------------------------------- forced key splits, child processes
# The slowest child of the first run on an MI355X (library load, four shapes, three variants) took 2.5 s; ten times that
# covers a busy shared machine.
CHILD_TIMEOUT_S = 25


@pytest.fixture(scope="module")
def forced_children():
    """One child process at a time, one per forced split; stops at the first child that does not exit 0 (a timeout or a
    signal included): later children are not started."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    child = os.path.join(root, "tests", "attention_forced_split_child.py")
    results, failure = {}, None
    for forced in ac.FORCED_SPLITS:
        with tempfile.NamedTemporaryFile(suffix=".pt") as f:
            t0 = time.time()
            try:
                proc = subprocess.run([sys.executable, child, f.name], env=dict(os.environ, AMAV_ATTN_SPLIT=str(forced)),
                                      cwd=root, capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
                code, output = proc.returncode, proc.stdout + proc.stderr
            except subprocess.TimeoutExpired as e:
                code, output = "timeout", f"{e.stdout or ''}{e.stderr or ''}"
            print(f"AMAV_ATTN_SPLIT={forced}: child exit {code} after {time.time() - t0:.1f} s")
            if code != 0:
                failure = f"child AMAV_ATTN_SPLIT={forced} ended with {code}; later children not started\n{output[-4000:]}"
                break
            results[forced] = torch.load(f.name, weights_only=False)
    return results, failure


@pytest.mark.parametrize("forced", ac.FORCED_SPLITS)
def test_forced_key_splits(forced_children, forced):
    """Every key split from 1 to 16 slices, uneven slices and a slice of one valid key included: the bound for all
    three variants, the lse bound, selfattn == selfattn_lse and the split-out operand == split_operand(out), all
    computed in the same child.  Where the forced split exceeds the tile count the library takes its own choice."""
    results, failure = forced_children
    assert forced in results, failure
    got = results[forced]
    assert got["forced"] == str(forced)
    for (B, S, H), rec in got["shapes"].items():
        case, ref = unit(B, S, H)
        n = ac.nsplit_from_workspace_bytes(rec["workspace_bytes_f32"], B, S, H)
        for name in ac.VARIANTS:
            ac.check(rec[name], ref, f"forced {forced} {name} {case.name} nsplit={n}")
        ac.check_lse(rec["lse"], ref, f"forced {forced} {case.name} nsplit={n}")
        assert torch.equal(rec["lse_out"], rec["default"])
        assert rec["split_out"].dtype == torch.float16 and torch.equal(rec["split_out"], rec["split_want"])
        others = [results[f]["shapes"][(B, S, H)]["default"] for f in results if f != forced]
        if others:
            print(f"forced {forced} {case.name}: default differs from the other children by at most "
                  f"{max(float((o - rec['default']).abs().max()) for o in others):.3e}")
