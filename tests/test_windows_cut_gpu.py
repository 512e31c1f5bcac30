"""The window cutting kernels of the windowed upsampler (csrc/tile_windows.hip: amav_windows_cut and its transpose) on
the device, at the smallest geometries that can go wrong.

Forward: a cut copies, so it must EQUAL slices of the zero-padded source.
Transpose: against an fp64 index_put_(accumulate=True) model.  An element covered by m windows is an m-term fp32 sum
added in a fixed order: |got - exact| <= (m - 1) * 2^-24 * sum |terms| (every partial sum is bounded by sum |terms|, each
of the m - 1 additions rounds once); with m <= 1 nothing rounds and the element must be exact, an uncovered one +0.0.
Two calls must agree bit for bit (no atomics)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _lattice_case(F, C, h, w, step, size, off, A, B, positions, seed, shuffle=True):
    """positions: (frame, a, b) lattice positions that hold a window -> x, the windows' arguments and the lattice."""
    from audio_motion_avatar_amd import ops

    g = torch.Generator().manual_seed(seed)
    pos = torch.tensor(positions, dtype=torch.long).reshape(-1, 3)
    if shuffle and len(pos) > 1:  # window indices in another order than the lattice's
        pos = pos[torch.randperm(len(pos), generator=g)]
    frame = pos[:, 0].int().cuda()
    oy, ox = (pos[:, 1] * step + off[0]).int().cuda(), (pos[:, 2] * step + off[1]).int().cuda()
    x = torch.randn(F, C, h, w, generator=g).cuda()
    lattice = ops.windows_lattice(frame, oy, ox, step, off[0], off[1], F, A, B)
    return x, frame, oy, ox, lattice


def _cut_reference(x, frame, oy, ox, size):
    F, C, h, w = x.shape
    corners = torch.stack([oy, ox]).cpu()
    m = size + (int(corners.abs().max()) if corners.numel() else 0)
    padded = torch.nn.functional.pad(x, (m, m, m, m))
    wins = [padded[f, :, y + m:y + m + size, xx + m:xx + m + size] for f, y, xx in
            zip(frame.tolist(), oy.tolist(), ox.tolist())]
    return torch.stack(wins) if wins else x.new_zeros(0, C, size, size)


def _transpose_model(gw, frame, oy, ox, shape):
    """-> (fp64 sums, fp64 sums of |terms|, number of covering windows), each of `shape`, by index_put_ with accumulate."""
    F, C, h, w = shape
    K, _, size, _ = gw.shape
    dev = gw.device
    total, mass = torch.zeros(shape, dtype=torch.float64, device=dev), torch.zeros(shape, dtype=torch.float64, device=dev)
    count = torch.zeros(shape, dtype=torch.float64, device=dev)
    if K == 0:
        return total, mass, count
    r = torch.arange(size, device=dev)
    y = (oy.long()[:, None] + r)[:, None, :, None].expand(K, C, size, size)
    xx = (ox.long()[:, None] + r)[:, None, None, :].expand(K, C, size, size)
    f = frame.long()[:, None, None, None].expand(K, C, size, size)
    c = torch.arange(C, device=dev)[None, :, None, None].expand(K, C, size, size)
    ok = (y >= 0) & (y < h) & (xx >= 0) & (xx < w)
    idx = (f[ok], c[ok], y[ok], xx[ok])
    terms = gw.double()[ok]
    total.index_put_(idx, terms, accumulate=True)
    mass.index_put_(idx, terms.abs(), accumulate=True)
    count.index_put_(idx, torch.ones_like(terms), accumulate=True)
    return total, mass, count


def _check(x, frame, oy, ox, size, lattice, seed, max_cover):
    from audio_motion_avatar_amd import ops

    K, shape = frame.numel(), tuple(x.shape)
    got = ops.windows_cut(x, frame, oy, ox, size)
    assert got.shape == (K, shape[1], size, size) and torch.equal(got, _cut_reference(x, frame, oy, ox, size))
    g = torch.Generator().manual_seed(seed + 1)
    gw = torch.randn(got.shape, generator=g).cuda()
    gx = ops.windows_cut_backward(gw, lattice, shape)
    again = ops.windows_cut_backward(gw, lattice, shape)
    assert torch.equal(gx.view(torch.int32), again.view(torch.int32))
    total, mass, count = _transpose_model(gw, frame, oy, ox, shape)
    assert int(count.max()) == max_cover, (int(count.max()), max_cover)
    err = (gx.double() - total).abs()
    bound = (count - 1).clamp_min(0) * 2.0 ** -24 * mass
    worst = float((err / bound.clamp_min(1e-300))[count > 1].max()) if bool((count > 1).any()) else 0.0
    print(f"K {K} shape {shape} size {size}: cover <= {int(count.max())}, uncovered {int((count == 0).sum())}, "
          f"max err / bound {worst:.3f}, max err {float(err.max()):.3e}")
    assert bool((err <= bound).all())
    single = count <= 1
    assert torch.equal(gx[single].double(), total[single])        # one term or none: exact
    uncovered = gx[count == 0]
    assert bool((uncovered == 0).all()) and not bool(torch.signbit(uncovered).any())  # +0.0
    return got, gw, gx


def test_three_windows_per_axis_over_one_element():
    """C = 3, 9 x 13, step 4, size 10, offset -3: rows -3, 1, 5 all cover y = 5 .. 6 (columns alike): nine windows on one
    element, windows over every border and corner; through the autograd Function too."""
    from audio_motion_avatar_amd import ops

    positions = [(0, a, b) for a in range(3) for b in range(4)]
    x, frame, oy, ox, lattice = _lattice_case(1, 3, 9, 13, 4, 10, (-3, -3), 3, 4, positions, seed=1)
    _, gw, gx = _check(x, frame, oy, ox, 10, lattice, 1, max_cover=9)
    xr = x.clone().requires_grad_()
    out = ops.windows_cut_differentiable(xr, frame, oy, ox, 10, lattice)
    assert torch.equal(out, ops.windows_cut(x, frame, oy, ox, 10))
    out.backward(gw)
    assert torch.equal(xr.grad, gx)


def test_all_windows_in_the_second_frame():
    positions = [(1, a, b) for a in range(3) for b in range(4) if (a + b) % 3]
    x, frame, oy, ox, lattice = _lattice_case(2, 3, 9, 13, 4, 10, (-3, -3), 3, 4, positions, seed=2)
    _, _, gx = _check(x, frame, oy, ox, 10, lattice, 2, max_cover=6)
    assert not bool(gx[0].any())


def test_windows_over_each_border_and_a_corner():
    """A lattice of step 1 (any corner): windows of 6 hanging over the top, bottom, left and right edge, over two corners,
    and one that covers the whole 5 x 7 source."""
    off = (-8, -8)
    corners = [(-3, 1), (3, 1), (0, -4), (0, 5), (-2, -3), (2, 4)]
    positions = [(0, y - off[0], x - off[1]) for y, x in corners]
    x, frame, oy, ox, lattice = _lattice_case(1, 2, 5, 7, 1, 6, off, 16, 18, positions, seed=3)
    _check(x, frame, oy, ox, 6, lattice, 3, max_cover=3)
    positions = [(0, 0, 0)]
    x, frame, oy, ox, lattice = _lattice_case(1, 2, 5, 7, 1, 9, (-2, -1), 1, 1, positions, seed=4)
    _check(x, frame, oy, ox, 9, lattice, 4, max_cover=1)


def test_one_window_and_none():
    x, frame, oy, ox, lattice = _lattice_case(2, 3, 9, 13, 4, 10, (-3, -3), 3, 4, [(0, 1, 2)], seed=5)
    _check(x, frame, oy, ox, 10, lattice, 5, max_cover=1)
    x, frame, oy, ox, lattice = _lattice_case(2, 3, 9, 13, 4, 10, (-3, -3), 3, 4, [], seed=6)
    assert frame.numel() == 0 and bool((lattice[3] == -1).all())
    _, _, gx = _check(x, frame, oy, ox, 10, lattice, 6, max_cover=0)
    assert not bool(gx.any())


@pytest.mark.parametrize("h,w,step,size,off,positions,cover", (
    (32, 48, 16, 22, -3, [(0, 0, 0), (0, 0, 1), (0, 1, 1), (1, 1, 2), (1, 0, 2), (1, 1, 1)], 3),
    (64, 64, 32, 36, -2, [(0, 0, 0), (0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 1, 1)], 4)))
def test_the_reference_defaults_shapes_at_small_extent(h, w, step, size, off, positions, cover):
    """C = 256 with the two cuts of the reference's 4-block upsampler (cells of 16 + 6 texels into block n - 1, padded
    tiles of 32 + 4 into block n): neighbouring windows overlap by 6 / 4 texels, up to four of them around a lattice
    corner."""
    A, B = h // step, w // step
    x, frame, oy, ox, lattice = _lattice_case(2, 256, h, w, step, size, (off, off), A, B, positions, seed=size)
    _check(x, frame, oy, ox, size, lattice, size, max_cover=cover)


def test_offsets_past_2_31_elements():
    """F C h w = 3 * 2^30 elements: the last frame's offsets need 64 bits in both kernels.  Only that frame is filled and
    compared (one channel of the transpose against the model); frame 0 holds no window and must come back all zero."""
    from audio_motion_avatar_amd import ops

    F, C, h, w, step, size = 3, 64, 4096, 4096, 32, 36
    x = torch.empty(F, C, h, w, device="cuda")
    assert x.numel() > 2 ** 31
    g = torch.Generator(device="cuda").manual_seed(9)
    x[2].normal_(generator=g)
    pos = torch.tensor([(2, 127, 127), (2, 127, 126), (2, 0, 0), (1, 5, 5)])
    frame, oy, ox = pos[:, 0].int().cuda(), (pos[:, 1] * step - 2).int().cuda(), (pos[:, 2] * step - 2).int().cuda()
    lattice = ops.windows_lattice(frame, oy, ox, step, -2, -2, F, 128, 128)
    got = ops.windows_cut(x, frame, oy, ox, size)
    last = x[2:3]
    zero = torch.zeros(3, dtype=torch.int32, device="cuda")
    assert torch.equal(got[:3], _cut_reference(last, zero, oy[:3], ox[:3], size))
    gw = torch.randn(got.shape, generator=g, device="cuda")
    gx = ops.windows_cut_backward(gw, lattice, x.shape)
    c = C - 1
    total, _, count = _transpose_model(gw[:3, c:c + 1], zero, oy[:3], ox[:3], (1, 1, h, w))
    assert int(count.max()) == 2
    err = (gx[2, c].double() - total[0, 0]).abs()
    assert float(err.max()) <= 2.0 ** -24 * float(gw.abs().max()) * 2 and bool(gx[2, c][count[0, 0] == 0].eq(0).all())
    assert torch.equal(gx[2, c][count[0, 0] == 1].double(), total[0, 0][count[0, 0] == 1])
    assert not bool(gx[0].any()) and int((gx[1] != 0).sum()) > 0
