"""The windowed triplane upsampler as an autograd graph (TriplaneUpsampler.forward_tokens_windowed(differentiable=True),
DESIGN.md section 4.14), on the CPU in fp64: its gradients against those of full-plane forward_tokens, the CPU
formulation of ops.windows_cut_differentiable, and the slab it writes."""
import pytest
import torch

import upsampler_cases as uc


@pytest.mark.parametrize("box", sorted(uc.BOXES))
@pytest.mark.parametrize("n_blocks,R", uc.CASES)
def test_windowed_gradients_equal_full_plane_gradients_in_fp64(n_blocks, R, box):
    """d loss / d coarse tokens and every upsampler parameter, loss = random-weighted sum of the features sampled at
    the points: windowed (differentiable=True) against full planes, both fp64 on the CPU.

    Bound: 1e-12 of max |grad| per tensor -- fp64 rounding of sums taken in another order (the two evaluations feed
    the same operands to convolutions over different images), about 100x over the 6.2e-15 measured for this
    construction."""
    want = uc.reference_gradients(n_blocks, R, box)
    up = uc.make_upsampler(n_blocks).double()
    tokens, points, weights = (t.double() for t in uc.make_inputs(n_blocks, R, box))
    plan = uc.fresh_plan(up, points, R)
    g = R // up.TILE_CELLS
    for w in plan:  # tiles, some of them inactive, in every plane
        assert w["tiles"] is not None and len(w["tiles"]) > 0 and bool((~w["mask"]).any())
    if box == "border":
        assert any(int(w["tiles"][:, 1:].min()) == 0 or int(w["tiles"][:, 1:].max()) == g - 1 for w in plan)
    assert up.windows_contain(plan, points, R, uc.RADIUS)
    tok = tokens.clone().requires_grad_()
    slab = up.forward_tokens_windowed(tok, R, plan, differentiable=True)
    assert slab.requires_grad and slab.dtype == torch.float64
    uc.oracle_loss(slab, points, weights, R * 2 ** n_blocks).backward()
    got = uc.gradients(up, tok)
    assert set(got) == set(want) and len(got) == len(list(up.parameters())) + 1
    worst = 0.0
    for name in sorted(want):
        err = uc.relative_error(got[name], want[name])
        worst = max(worst, err)
        assert float(want[name].abs().max()) > 0 and err <= 1e-12, (name, err)
    print(f"blocks {n_blocks} R {R} {box}: worst relative gradient error {worst:.2e}")


def _pad_unfold_index(x, tiles, y0, x0, level_scale, pad, size, tile_cells=4):
    """The formulation the inference path of forward_tokens_windowed cuts its windows with."""
    f_idx, ty, tx = tiles[:, 0], tiles[:, 1], tiles[:, 2]
    step = tile_cells * level_scale
    xp = torch.nn.functional.pad(x, (pad, pad, pad, pad)) if pad else x
    ay, ax = -(-(y0 * level_scale) // step), -(-(x0 * level_scale) // step)
    wv = xp[:, :, ay * step - y0 * level_scale:].unfold(2, size, step).permute(0, 1, 2, 4, 3)
    wv = wv[..., ax * step - x0 * level_scale:].unfold(4, size, step)
    return wv[f_idx, :, ty - ay, :, tx - ax, :]


@pytest.mark.parametrize("level_scale,pad,size", ((2, 3, 14), (2, 1, 10), (4, 2, 20), (4, 0, 16), (1, 0, 4)))
def test_cpu_windows_cut_is_the_pad_unfold_index_formulation(level_scale, pad, size):
    """Values and gradients, exactly: integer-valued data, so the transposes' sums do not round.  A crop of input
    cells [y0, y1) x [x0, x1) at `level_scale` texels per cell, windows of the tiles inside it, overlapping by 2 pad."""
    from audio_motion_avatar_amd import ops

    y0, y1, x0, x1, g = 3, 15, 0, 10, 4
    tiles = torch.tensor([[0, 1, 0], [0, 1, 1], [0, 2, 1], [1, 2, 0], [1, 2, 1], [1, 1, 1]])  # frame, tile row, tile column
    gen = torch.Generator().manual_seed(size)
    x = torch.randint(-8, 9, (2, 3, (y1 - y0) * level_scale, (x1 - x0) * level_scale), generator=gen).double()
    xa, xb = x.clone().requires_grad_(), x.clone().requires_grad_()
    want = _pad_unfold_index(xa, tiles, y0, x0, level_scale, pad, size)
    step = 4 * level_scale
    off_y, off_x = -y0 * level_scale - pad, -x0 * level_scale - pad
    frame, oy, ox = tiles[:, 0].int(), (tiles[:, 1] * step + off_y).int(), (tiles[:, 2] * step + off_x).int()
    lattice = ops.windows_lattice(frame, oy, ox, step, off_y, off_x, 2, g, g)
    assert lattice[3].dtype == torch.int32 and sorted(lattice[3][lattice[3] >= 0].tolist()) == list(range(len(tiles)))
    got = ops.windows_cut_differentiable(xb, frame, oy, ox, size, lattice)
    assert got.shape == (len(tiles), 3, size, size) and torch.equal(got, want)
    cot = torch.randint(-8, 9, got.shape, generator=gen).double()
    want.backward(cot)
    got.backward(cot)
    assert torch.equal(xb.grad, xa.grad)
    # windows that leave the source on every side read zeros (the library kernel's contract, on the CPU too)
    oy2, ox2 = torch.tensor([-5, x.shape[2] - 3], dtype=torch.int32), torch.tensor([-2, x.shape[3] - 1], dtype=torch.int32)
    fr2 = torch.tensor([1, 0], dtype=torch.int32)
    far = ops.windows_cut_differentiable(x, fr2, oy2, ox2, size, (1, 0, 0, None))  # any corner lies on a lattice of step 1
    m = size + 8
    padded = torch.nn.functional.pad(x, (m, m, m, m))
    for k in range(2):
        ref = padded[fr2[k], :, oy2[k] + m:oy2[k] + m + size, ox2[k] + m:ox2[k] + m + size]
        assert torch.equal(far[k], ref)
    assert ops.windows_cut_differentiable(x, fr2[:0], oy2[:0], ox2[:0], size, (1, 0, 0, None)).shape == (0, 3, size, size)


def test_differentiable_never_touches_the_cached_slab():
    n_blocks, R = 2, 16
    up = uc.make_upsampler(n_blocks)
    tokens, points, _ = uc.make_inputs(n_blocks, R, "off_centre")
    plan = uc.fresh_plan(up, points, R)
    tok = tokens.clone().requires_grad_()
    first = up.forward_tokens_windowed(tok, R, plan, differentiable=True)
    assert not hasattr(up, "_slab")  # the autograd path does not create the cache either
    with torch.no_grad():
        cached = up.forward_tokens_windowed(tokens, R, plan)
    assert cached is up._slab
    up._slab.fill_(7.0)  # whatever the cache holds ...
    version = up._slab._version
    second = up.forward_tokens_windowed(tok, R, plan, differentiable=True)
    # ... is neither returned nor written, and every call has a slab of its own, zero outside the active tiles
    assert second is not up._slab and second.data_ptr() != up._slab.data_ptr() and second.data_ptr() != first.data_ptr()
    assert up._slab._version == version and bool((up._slab == 7.0).all())
    assert torch.equal(first, second) and second.requires_grad
    r_out, tile = R * 2 ** n_blocks, 4 * 2 ** n_blocks
    sv = second.detach().view(uc.F, uc.C, 3, R // 4, tile, R // 4, tile)
    for p, w in enumerate(plan):
        outside = ~w["mask"]
        assert bool(outside.any()) and bool((sv[:, :, p].permute(0, 2, 4, 1, 3, 5)[outside] == 0).all())
    assert second.shape == (uc.F, uc.C, 3 * r_out * r_out)
    with pytest.raises(ValueError, match="out"):
        up.forward_tokens_windowed(tok, R, plan, out=torch.zeros_like(second), differentiable=True)


def test_the_flag_is_off_by_default():
    from audio_motion_avatar_amd.config import RendererConfig

    assert RendererConfig().differentiable_upsampler is False
