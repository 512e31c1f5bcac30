"""The case list of attention_cases.py against a torch model of the default kernel's fp16 x 2 arithmetic, on the CPU.

It proves on any machine, without a GPU and without the HIP library, that the bound the GPU tests assert
(max |out - sdpa64| <= 4 err32 + 2^-22 max |v|) is satisfiable by a correct implementation on every input they use, and
it catches a later edit of the case list that leaves the envelope the kernel documents.  Sizes are reduced (S <= 512);
the model's sums are float64, so it carries the format's error and none of the fp32 accumulation error."""
import pytest
import torch

import attention_cases as ac

MODEL_SHAPES = ((1, 500, 2), (2, 193, 3))   # the GPU test's (1, 1000, 2) halved, and its single-slice shape


def run(case):
    ref = ac.reference(case)
    out = ac.model_fp16x2(case)
    return out, ref, ac.check(out, ref, "model " + case.name, envelope=case.in_envelope)


@pytest.mark.parametrize("B,S,H", [(1, 1, 1), (2, 33, 3), (1, 64, 1), (2, 129, 3), (1, 512, 2)])
def test_unit_shapes(B, S, H):
    run(ac.unit_case(B, S, H))


@pytest.mark.parametrize("B,S,H", MODEL_SHAPES)
@pytest.mark.parametrize("name", ac.MAGNITUDE_NAMES)
def test_magnitude_cases_are_inside_the_bound(name, B, S, H):
    out, _, _ = run(ac.magnitude_case(name, B, S, H))
    if name in ac.ZERO_OUTPUT:
        assert torch.equal(out, torch.zeros_like(out))


@pytest.mark.parametrize("B,S,H", [(1, 500, 2), (1, 1000, 2)])
def test_bookkeeping_cases_do_what_their_names_say(B, S, H):
    """rising: the running maximum moves in every 64-key tile; falling: only in the first; late_spike_one_lane: one
    query peaks at the last key, every other at key 0; first_key_only: key 0 leads by more than 60."""

    def scores(case):
        sp = lambda t: t.view(B, S, H, 64).transpose(1, 2).double()
        return sp(case.q) @ sp(case.k).transpose(-1, -2) * 0.125   # [B, H, query, key]

    tile_max = lambda s: torch.stack([s[..., t:t + 64].max(-1).values for t in range(0, S, 64)], -1)
    running = tile_max(scores(ac.magnitude_case("rising", B, S, H))).cummax(-1).values
    assert bool((running[..., 1:] > running[..., :-1]).all())
    running = tile_max(scores(ac.magnitude_case("falling", B, S, H))).cummax(-1).values
    assert bool((running[..., 1:] == running[..., :1]).all())
    arg = scores(ac.magnitude_case("late_spike_one_lane", B, S, H)).argmax(-1)
    b, h, i = ac.late_spike_query(B, S, H)
    assert int(arg[b, h, i]) == S - 1
    arg[b, h, i] = 0
    assert int(arg.abs().max()) == 0
    s = scores(ac.magnitude_case("first_key_only", B, S, H))
    assert float((s[..., :1] - s[..., 1:]).min()) > 60.0


@pytest.mark.parametrize("magnitudes", list(ac.BOUNDS_MAGNITUDES))
@pytest.mark.parametrize("target", ac.BOUNDS_TARGETS)
@pytest.mark.parametrize("slack", ac.BOUNDS_SLACKS)
def test_proven_bounds_are_inside_the_bound(slack, target, magnitudes):
    case = ac.bounds_case(magnitudes, slack, target, 1, 500, 2)
    assert case.in_envelope
    run(case)


@pytest.mark.parametrize("edge", ac.BOUNDS_EDGES)
def test_bound_edges_are_inside_the_bound(edge):
    run(ac.bounds_edge_case(edge, 1, 500, 2))


def test_slack_beyond_the_envelope_degrades_as_documented():
    """Bounds 2^20 above the magnitudes (FP16_MAX_OVERSHOOT is 2^12): residuals fall into fp16's subnormals and the
    result loses bits -- still under the 2e-5 ceiling, which is all that is asserted; error / err32 is printed."""
    case = ac.bounds_case("unit", ac.BOUNDS_OUTSIDE, "qkv", 1, 500, 2)
    assert not case.in_envelope
    _, ref, (err, ratio, _) = run(case)
    assert err > ref.bound / 4   # the case does leave the envelope: otherwise it tests nothing


@pytest.mark.parametrize("scale", [1.0, 0.5, 0.125])
def test_known_answer(scale):
    case = ac.known_answer_case(scale)
    out, ref, _ = run(case)
    want = case.v.roll(-1, dims=1)
    assert float((out - want).abs().max()) <= ac.FLOOR * ref.vmax


def test_nsplit_arithmetic():
    for B, S, H, n in ((1, 6304, 8, 5), (2, 2081, 3, 2), (1, 65, 1, 2), (1, 1, 1, 1)):
        nbytes = 256 if n == 1 else (n * B * H * S * 66 * 4 + 255) // 256 * 256
        assert ac.nsplit_from_workspace_bytes(nbytes, B, S, H) == n
