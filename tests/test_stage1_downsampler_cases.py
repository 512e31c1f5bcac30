"""The second case list of the TriplaneDownsampler stencil (downsampler_cases.WIDE_CASES) reaches what it was built for,
checked on the CPU alone: these conditions, not a GPU run, decided the shapes and magnitudes, which the kernel tests of
tests/test_stage1_downsampler_widths_gpu.py rely on.

    * every instantiation V = C / 64 = 1..8 of dwconv7_layernorm_kernel / layernorm_backward_kernel is present;
    * one plane has different tile counts on its two axes, both at least 3, and its transpose is present, so a kernel that
      decoded a tile index with the counts swapped cannot pass; it has tiles whose 14 x 14 halo lies wholly inside;
    * 9, 12 and 27 tiles: sum_parts_kernel's unrolled-by-8 body exactly once, once with a tail, three times with a tail;
    * one case leaves a single row in the last 16-row chunk of the LayerNorm backward;
    * in the `eps` group dropping eps moves the normalised rows by more than 0.1 of their maximum;
    * in the `offset` group every row's |mean| is more than 5 of its standard deviations;
    * the library's fp32 evaluation on the CPU is inside LIBRARY_ERR_WIDE for every case: the yardstick stays inside the
      figure the bounds are built from.
"""
import pytest
import torch

import downsampler_cases as dc

TILE, HALO, ROW_CHUNK, UNROLL = 8, 3, 16, 8          # csrc/convnext.hip: kTile, the 7 x 7 stencil's reach, kRowChunk


def tiles_of(n):
    return (n + TILE - 1) // TILE


def tile_count(shape):
    K, H, W, _ = shape
    return K * tiles_of(H) * tiles_of(W)


def interior_tiles(H, W):
    """Tiles (ty, tx) whose halo [8 t - 3, 8 t + 10] lies inside the plane on both axes."""
    inside = lambda t, n: TILE * t - HALO >= 0 and TILE * t + TILE - 1 + HALO <= n - 1
    return [(ty, tx) for ty in range(tiles_of(H)) for tx in range(tiles_of(W)) if inside(ty, H) and inside(tx, W)]


SHAPES = [shape for _, shape, _ in dc.WIDE_CASES]


def test_case_list_is_well_formed():
    assert len(set(dc.WIDE_CASES)) == len(dc.WIDE_CASES)
    assert {group for group, _, _ in dc.WIDE_CASES} == set(dc.WIDE_GROUPS)
    assert set(dc.LIBRARY_ERR_WIDE) == {(g, k) for g in dc.WIDE_GROUPS for k in dc.WIDE_KINDS}
    assert dc.ORDER_FACTOR == 4.0 and dc.bound_wide("widths", "dparam") == 4.0 * dc.LIBRARY_ERR_WIDE["widths", "dparam"]
    for group, (K, H, W, C), options in dc.WIDE_CASES:
        assert options == dc.MAGNITUDES.get(group, ())
        args, eps, (y, n), g, grads = dc.wide_case((group, (K, H, W, C), options))
        assert args[0].shape == (K, H, W, C) and all(t.dtype == torch.float32 for t in args + (g,))
        assert y.dtype == n.dtype == torch.float64 and n.shape == g.shape == (K * H * W, C)
        assert [t.shape for t in grads] == [t.shape for t in args] and eps == 1e-6
    # the existing lists and their table are as they were
    assert dc.DW_CASES == [(1, 5, 5, 64), (1, 9, 13, 64), (2, 9, 13, 256), (2, 5, 5, 256)]
    assert (dc.GELU_ROWS, dc.GELU_INNER) == ((1, 67), 256)
    assert dc.LIBRARY_ERR == {"conv": 3e-7, "norm": 4e-7, "gelu": 2e-7, "block": 3e-6, "dx": 3e-7, "dparam": 5e-7,
                              "dgelu": 2e-7, "dmodule": 2e-6}


def test_every_built_width_is_present_in_every_role():
    assert {C // 64 for _, _, _, C in SHAPES} == set(range(1, 9))
    off_square = {C for K, H, W, C in SHAPES if (K, H, W) == (1, 19, 27)}
    assert off_square == set(range(64, 513, 64))
    # the narrowest, an inexact 1 / C and the widest in every magnitude group
    for group in ("eps", "large", "offset"):
        assert {shape[3] for g, shape, _ in dc.WIDE_CASES if g == group} == {64, 192, 512}


def test_tile_grids():
    grids = {(tiles_of(H), tiles_of(W)) for _, H, W, _ in SHAPES}
    assert (3, 4) in grids and (4, 3) in grids
    assert (1, 19, 27, 192) in SHAPES and (1, 27, 19, 192) in SHAPES          # the same width both ways round
    assert 19 % TILE and 27 % TILE                                            # ragged in both directions
    assert interior_tiles(19, 27) == [(1, 1), (1, 2)] and interior_tiles(27, 19) == [(1, 1), (2, 1)]
    assert not any(interior_tiles(H, W) for H, W in ((5, 5), (9, 13), (17, 17)))   # new: no earlier case had one
    counts = {tile_count(shape) for shape in SHAPES}
    assert {9, 12, 27} <= counts
    # sum_parts_kernel: the first partial, then bodies of 8, then the tail
    loops = {n: ((n - 1) // UNROLL, (n - 1) % UNROLL) for n in (9, 12, 27)}
    assert loops == {9: (1, 0), 12: (1, 3), 27: (3, 2)}
    assert any(K > 1 and tile_count((K, H, W, C)) == 27 for K, H, W, C in SHAPES)  # tiles ascending across planes


def test_a_last_row_chunk_of_one_row():
    rows = {K * H * W for K, H, W, _ in SHAPES}
    assert 289 in rows and 289 % ROW_CHUNK == 1
    assert any(r % ROW_CHUNK == 1 for r in rows)
    assert any(-(-r // ROW_CHUNK) > UNROLL + 1 for r in rows)    # the LayerNorm partials drive the unrolled body too


@pytest.mark.parametrize("case", [c for c in dc.WIDE_CASES if c[0] == "eps"], ids=dc.case_id)
def test_eps_is_visible(case):
    args, eps, (y, n), _, _ = dc.wide_case(case)
    C = y.shape[-1]
    var = float(y.var(-1, unbiased=False).mean())
    assert 0.3 * eps < var < 3 * eps, var
    without = dc.dwconv_norm(*(t.double() for t in args), eps=0.0)[1].reshape(-1, C)
    moved = float((without - n).abs().max()) / float(n.abs().max())
    print(f"{dc.case_id(case)}: var(y) {var:.2e}; eps = 0 moves the rows by {moved:.2f} of max |norm|")
    assert moved > 0.1
    # eps outside the square root -- 1 / (sqrt(var) + eps) -- is as visible
    mean, v = y.mean(-1, keepdim=True), y.var(-1, unbiased=False, keepdim=True)
    outside = ((y - mean) / (v.sqrt() + eps) * args[3].double() + args[4].double()).reshape(-1, C)
    assert float((outside - n).abs().max()) / float(n.abs().max()) > 0.1


@pytest.mark.parametrize("case", [c for c in dc.WIDE_CASES if c[0] == "offset"], ids=dc.case_id)
def test_offset_rows_have_a_mean_far_from_zero(case):
    _, _, (y, _), _, _ = dc.wide_case(case)
    ratio = float((y.mean(-1).abs() / y.std(-1, unbiased=False)).min())
    print(f"{dc.case_id(case)}: smallest |row mean| / row deviation {ratio:.2f}")
    assert ratio > 5.0


def test_magnitudes_of_the_small_and_large_groups():
    for group, scale in (("eps", 1e-3), ("large", 1e3)):
        for case in (c for c in dc.WIDE_CASES if c[0] == group):
            args, _, (y, _), _, _ = dc.wide_case(case)
            assert 3 * scale < float(args[0].abs().max()) < 6 * scale
            assert 0.5 * scale < float(y.std()) < 2 * scale


@pytest.mark.parametrize("case", dc.WIDE_CASES, ids=dc.case_id)
def test_library_fp32_on_the_cpu_is_inside_its_figure(case):
    for kind, (got, want) in dc.library_wide(case).items():
        err = max(dc.rel_err(a, b) for a, b in zip(got, want))
        print(f"{dc.case_id(case)}: library fp32 {kind} error {err:.3e} (figure {dc.LIBRARY_ERR_WIDE[case[0], kind]:.0e})")
        assert err <= dc.LIBRARY_ERR_WIDE[case[0], kind]


def test_gelu_at_the_product_width_stays_inside_the_existing_figures():
    for rows, inner in dc.GELU_WIDE:
        (proj, bias, g), (out, d_proj, d_bias) = dc.gelu_case(rows, inner)
        leaves = [proj.clone().requires_grad_(True), bias.clone().requires_grad_(True)]
        lo = dc.gelu_bias(*leaves)
        lp, lb = torch.autograd.grad(lo, leaves, g)
        for kind, a, b in (("gelu", lo, out), ("dgelu", lp, d_proj), ("dparam", lb, d_bias)):
            err = dc.rel_err(a, b)
            print(f"gelu ({rows}, {inner}): library fp32 {kind} error {err:.3e} (figure {dc.LIBRARY_ERR[kind]:.0e})")
            assert err <= dc.LIBRARY_ERR[kind]
    assert dc.GELU_WIDE == ((67, 1024), (5, 12)) and 12 % 8 and 1024 == 4 * 256
