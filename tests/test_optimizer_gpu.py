"""amav_grad_norm_clip / amav_adam_step through ops, against the fp64 oracle of the clipped Adam step.

Fixture: six tensors of 1, 63, 64, 65, 4097 and 3 * 4096 + 5 elements, seeded normal parameters, gradient i scaled by
10^(i - 3): the norm (~1.1e4) makes the clip active and the tensors differ by six decades.  Bounds: the norm within
2^-17 of the fp64 one (the design condition of DESIGN.md section 4.20), the coefficient exactly the fp32 expression of
the kernel's own norm, and p, m, v within 4 x the distance of the library's own fp32 single-tensor run on the CPU from
the same fp64 run, per tensor and quantity (optimizer_cases.py)."""
import pytest
import torch

import optimizer_cases as oc

pytestmark = pytest.mark.gpu

CHUNKS = (64, 4096)   # hundreds of partials (the second stage runs past its 256 lanes) / one chunk for most tensors


def _same_bits(a, b, quantities="pmv"):
    return all(torch.equal(x, y) for sa, sb in zip(a, b) for q in quantities for x, y in zip(sa[q], sb[q]))


@pytest.mark.parametrize("chunk", CHUNKS)
def test_norm_and_coefficient(chunk):
    oracle, _ = oc.reference(oc.PLAIN)
    run = oc.run_kernels(oc.PLAIN, chunk)
    for step, (got, want) in enumerate(zip(run, oracle)):
        rel = abs(float(got["norm"].double()) - float(want["norm"])) / float(want["norm"])
        print(f"chunk {chunk} step {step}: norm {float(got['norm']):.6e}, relative error {rel:.2e} (bound {oc.NORM_BOUND:.2e})")
        assert rel <= oc.NORM_BOUND
        assert 1e3 < float(got["norm"]) and float(got["coef"]) < 1e-3                 # the clip is active
        assert torch.equal(got["coef"], oc.clip_coefficient(got["norm"], torch.tensor(oc.PLAIN.max_norm)))


@pytest.mark.parametrize("chunk", CHUNKS)
def test_three_steps_against_the_fp64_oracle(chunk):
    oc.check_against_oracle(oc.PLAIN, oc.run_kernels(oc.PLAIN, chunk), f"chunk {chunk}")


def test_weight_decay_and_a_second_group():
    oc.check_against_oracle(oc.COVERAGE, oc.run_kernels(oc.COVERAGE, 4096), "weight decay, two groups")


def test_coefficient_one_is_the_unclipped_step():
    """Gradients whose norm is below max_norm: the coefficient is exactly 1 and the step equals, bit for bit, the one
    with no coefficient at all."""
    clipped = oc.run_kernels(oc.QUIET, 4096)
    assert all(float(s["coef"]) == 1.0 and 0 < float(s["norm"]) < 1 for s in clipped)
    assert _same_bits(clipped, oc.run_kernels(oc.QUIET, 4096, clip=False))
    oc.check_against_oracle(oc.QUIET, clipped, "coefficient 1")


@pytest.mark.parametrize("chunk", CHUNKS)
def test_two_runs_have_the_same_bits(chunk):
    first = oc.run_kernels(oc.PLAIN, chunk)
    for other in (oc.run_kernels(oc.PLAIN, chunk), oc.run_kernels(oc.PLAIN, chunk, rebuild_tables=True)):
        assert _same_bits(first, other)
        assert all(torch.equal(a["norm"], b["norm"]) and torch.equal(a["coef"], b["coef"]) for a, b in zip(first, other))


def test_unaligned_views_and_a_three_element_tensor():
    """A parameter and a gradient that start one float past a 16-byte boundary, next to a tensor of 3 elements: the same
    bound, and (run_kernels) nothing written outside any tensor."""
    run = oc.run_kernels(oc.ALIGNMENT, 64, misaligned={("p", 1), ("g", 2)})
    oc.check_against_oracle(oc.ALIGNMENT, run, "unaligned")
    oracle, _ = oc.reference(oc.ALIGNMENT)
    for got, want in zip(run, oracle):
        assert abs(float(got["norm"].double()) - float(want["norm"])) / float(want["norm"]) <= oc.NORM_BOUND
    assert _same_bits(run, oc.run_kernels(oc.ALIGNMENT, 64))     # the 16-byte path computes the same values


def test_zeroing_the_gradients_in_the_same_pass():
    plain, zeroed = oc.run_kernels(oc.PLAIN, 4096), oc.run_kernels(oc.PLAIN, 4096, zero_grad=True)
    assert _same_bits(plain, zeroed)
    assert all(bool((g == 0).all()) for s in zeroed for g in s["g"])
    assert all(bool((g != 0).any()) for s in plain for g in s["g"])                 # without the flag they are only read


def test_nothing_to_update():
    """No tensors: the norm is 0, the coefficient 1, and the update has nothing to launch."""
    from audio_motion_avatar_amd import ops

    empty = torch.empty(0, dtype=torch.uint8, device="cuda")
    norm = ops.grad_norm_clip(empty, 0, empty, 0, 64, 1.0, norm=torch.full((2,), oc.SENTINEL, device="cuda"))
    assert norm.tolist() == [0.0, 1.0]
    ops.adam_step(empty, 0, empty, 0, 64, [])
    torch.cuda.synchronize()
