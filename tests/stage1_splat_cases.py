"""Inputs and CPU restatements for the forward kernels of csrc/splat.hip (tests/test_stage1_splat_model.py checks them
against the oracle, tests/test_stage1_splat_gpu.py holds the kernels to them).  Nothing here loads the HIP library.

Restatements: pool_local_fp32, cell_mean_seq_fp32, cell_mean_fp64 (+ cell_mean_bound), project_fp32 (+ expected_features).
Case builders: cells_case, project_scene, lattice_scene, ties_scene, near_plane_scene.  Every builder is seeded,
returns plain CPU tensors and asserts, on the restatements alone, that the case still has the edge it was built for."""
import functools
import math

import numpy as np
import torch

from oracle import triplane_net as o_tn

f32 = np.float32
U = 2.0 ** -24          # unit roundoff of fp32
RADIUS = 1.4            # the encoder's cube half-width (config.radius)
PLANES = ("xy", "xz", "yz")


# ---------------------------------------------------------------------------------------------------- restatements
def _segments(cell_row, cells):
    """int [N] -> (order: point ids stably sorted by cell, seg: int64 [cells + 1] run offsets)"""
    order = np.argsort(cell_row, kind="stable")
    seg = np.zeros(cells + 1, dtype=np.int64)
    seg[1:] = np.cumsum(np.bincount(cell_row, minlength=cells))
    return order, seg


def pool_local_fp32(feat, cell_of, cells):
    """feat fp32 [B,N,C], cell_of int [B,3,N] -> fp32 [B,N,C]: per plane the channel-wise maximum over the points of
    the point's cell (an empty cell reads 0, no point ever gathers one), summed as (m_xy + m_xz) + m_yz in fp32."""
    F, cell = feat.numpy(), cell_of.numpy().astype(np.int64)
    B, N, C = F.shape
    out = np.empty((B, N, C), dtype=f32)
    for b in range(B):
        gathered = []
        for p in range(3):
            order, seg = _segments(cell[b, p], cells)
            full = seg[1:] > seg[:-1]
            m = np.maximum.reduceat(F[b][order], seg[:-1][full], axis=0)          # one row per non-empty cell
            gathered.append(m[(np.cumsum(full) - 1)[cell[b, p]]])
        out[b] = (gathered[0] + gathered[1]) + gathered[2]
    return torch.from_numpy(out)


def cell_mean_seq_fp32(feat, cell_of, cells):
    """feat fp32 [B,N,C], cell_of int [B,N] -> fp32 [B,C,cells]: per cell the fp32 sum of its points' rows taken one
    after the other in ascending point id (np.cumsum is sequential), then one fp32 division by the count; 0 if empty."""
    F, cell = feat.numpy(), cell_of.numpy().astype(np.int64)
    B, N, C = F.shape
    out = np.zeros((B, C, cells), dtype=f32)
    for b in range(B):
        order, seg = _segments(cell[b], cells)
        for k in np.flatnonzero(seg[1:] > seg[:-1]):
            rows = F[b][order[seg[k]:seg[k + 1]]]
            out[b, :, k] = np.cumsum(rows, axis=0, dtype=f32)[-1] / f32(len(rows))
    return torch.from_numpy(out)


def cell_mean_fp64(feat, cell_of, cells):
    """The same mean in fp64, for the non-empty cells only (the product grid is mostly empty)
    -> (where int64 [M,2]: (b, cell) of every non-empty cell, mean fp64 [M,C], abs_sum fp64 [M,C] = sum |x_i| over the
    cell, count int64 [B,cells])"""
    F, cell = feat.numpy().astype(np.float64), cell_of.numpy().astype(np.int64)
    B, N, C = F.shape
    where, mean, abs_sum = [], [], []
    count = np.zeros((B, cells), dtype=np.int64)
    for b in range(B):
        order, seg = _segments(cell[b], cells)
        count[b] = seg[1:] - seg[:-1]
        full = np.flatnonzero(count[b])
        where.append(np.stack([np.full_like(full, b), full], axis=1))
        mean.append(np.add.reduceat(F[b][order], seg[full], axis=0) / count[b][full, None])
        abs_sum.append(np.add.reduceat(np.abs(F[b][order]), seg[full], axis=0))
    return tuple(torch.from_numpy(np.concatenate(x)) for x in (where, mean, abs_sum)) + (torch.from_numpy(count),)


def cell_mean_bound(abs_sum, n):
    """abs_sum [M,C], n [M] points per cell -> n * 2**-24 * (abs_sum / n): a sequential fp32 sum of n terms is within
    (n - 1) u sum|x_i| of the exact one to first order, the division adds one more rounding of the mean."""
    n = n[:, None].double()
    return n * U * (abs_sum / n)


def at_cells(planes, where):
    """planes [B,C,cells], where [M,2] -> [M,C]"""
    return planes[where[:, 0], :, where[:, 1]]


def _camera(points, w2c, K):
    """The fp32 operations of oracle.triplane_net.points_projection in its order, for all points at once -> Z, u, v"""
    P, E, k = (t.numpy().astype(f32) for t in (points, w2c, K))
    x, y, z = P[..., 0], P[..., 1], P[..., 2]

    def row(i):
        e = E[:, i, :, None]
        return ((e[:, 0] * x + e[:, 1] * y) + e[:, 2] * z) + e[:, 3]

    X, Y, Z = row(0), row(1), row(2)
    with np.errstate(all="ignore"):
        u = (k[:, 0, 0, None] * X) / Z + k[:, 0, 2, None]
        v = (k[:, 1, 1, None] * Y) / Z + k[:, 1, 2, None]
    assert Z.dtype == f32 and u.dtype == f32 and v.dtype == f32
    return Z, u, v


def _span(centre, r, size):
    """first and last pixel whose centre can lie within r of `centre` along one axis, clamped to [0, size - 1]"""
    lo, hi = math.ceil(f32(f32(centre - r) - f32(0.5))), math.floor(f32(f32(centre + r) - f32(0.5)))
    return max(0, lo), min(size - 1, hi)


def rasterise_fp32(points, w2c, K, H, W, radius_px):
    """-> (ids int64 [B,H,W]: the point each pixel belongs to or -1, depth fp32 [B,H,W], contested int64 [B,H,W]: how
    many points cover the pixel at exactly the winning depth).  A disc is tested as one array per point."""
    Z, u, v = _camera(points, w2c, K)
    B, N = Z.shape
    r, half = f32(radius_px), f32(0.5)
    r2 = f32(r * r)
    ids = np.full((B, H, W), -1, dtype=np.int64)
    depth = np.full((B, H, W), np.inf, dtype=f32)
    contested = np.zeros((B, H, W), dtype=np.int64)
    for second_pass in (False, True):
        for b in range(B):
            for n in range(N):
                z = Z[b, n]
                if not z > 0 or not (np.isfinite(u[b, n]) and np.isfinite(v[b, n])):
                    continue
                (x0, x1), (y0, y1) = _span(u[b, n], r, W), _span(v[b, n], r, H)
                if x0 > x1 or y0 > y1:
                    continue
                dx = (np.arange(x0, x1 + 1).astype(f32) + half) - u[b, n]
                dy = (np.arange(y0, y1 + 1).astype(f32) + half) - v[b, n]
                inside = ((dx * dx)[None, :] + (dy * dy)[:, None]) < r2
                zb, ib = depth[b, y0:y1 + 1, x0:x1 + 1], ids[b, y0:y1 + 1, x0:x1 + 1]
                if second_pass:
                    contested[b, y0:y1 + 1, x0:x1 + 1] += inside & (z == zb)
                    continue
                wins = inside & ((z < zb) | ((z == zb) & (n < ib)))
                zb[wins], ib[wins] = z, n
    return ids, depth, contested


def project_fp32(points, w2c, K, H, W, radius_px):
    """points [B,N,3], w2c [B,4,4], K [B,3,3] -> pixel_of int64 [B,N]: the LAST pixel (y * W + x) of which the point is
    the nearest one inside its disc, lowest id among equal depths; -1 if there is none.  A point behind the camera or
    whose u or v is not finite claims nothing."""
    ids = rasterise_fp32(points, w2c, K, H, W, radius_px)[0]
    B, N = points.shape[:2]
    pixel_of = np.full((B, N), -1, dtype=np.int64)
    for b in range(B):
        flat = ids[b].reshape(-1)
        won = np.flatnonzero(flat >= 0)
        np.maximum.at(pixel_of[b], flat[won], won)
    return torch.from_numpy(pixel_of)


def expected_features(features, pixel_of):
    """features [B,C,H,W], pixel_of [B,N] -> [B,N,C]: the claimed pixel's feature column, zeros for -1"""
    B, C = features.shape[:2]
    flat = features.reshape(B, C, -1)
    got = flat.gather(2, pixel_of.clamp_min(0)[:, None, :].expand(B, C, -1)).permute(0, 2, 1)
    return torch.where((pixel_of >= 0)[..., None], got, torch.zeros(())).contiguous()


# ------------------------------------------------------------------------------------------------ cell-reduction cases
CLAMPED = torch.tensor([[1.4, -1.4, 0.0],       # on two faces
                        [5.0, 0.0, -5.0],       # far outside: clamped onto an edge
                        [-1.4, 1.4, 1.4],       # corner: the last cell of yz
                        [-1.4, -1.4, 0.3]])     # cell 0 of xy


@functools.lru_cache(maxsize=None)
def cells_case(C, N, R, kind="randn", layout="random", offset=0.0, B=3):
    """-> dict(feat fp32 [B,N,C], cell_of int32 [B,3,N], cells, R).  Treat the tensors as read-only: the case is cached.

    kind: "randn" | "ties" (integers in -3..3 on every second point) | "negative" (one cell all negative in every
    channel) | "scaled" (channels alternately * 2**100 and * 2**-100).  layout: "random" (vertices through
    oracle.cell_indices, the first ones clamped onto faces and corners) | "corner" (every point in the LAST cell of
    plane 0 and the FIRST of plane 1)."""
    cells = R * R
    g = torch.Generator().manual_seed(1000 * C + 10 * N + R)
    verts = torch.randn(B, N, 3, generator=g) * 0.5
    k = min(N, len(CLAMPED))
    verts[:, :k] = CLAMPED[:k]
    index = o_tn.cell_indices(verts, RADIUS, R)
    cell_of = torch.stack([index[key][:, 0] for key in PLANES], dim=1).to(torch.int32)
    if layout == "corner":
        cell_of[:, 0] = cells - 1
        cell_of[:, 1] = 0
    assert int(cell_of.min()) >= 0 and int(cell_of.max()) < cells
    count = torch.stack([torch.stack([torch.bincount(cell_of[b, p].long(), minlength=cells) for p in range(3)])
                         for b in range(B)])                                       # [B,3,cells]

    feat = torch.randn(B, N, C, generator=g)
    if kind == "ties":
        feat[:, ::2] = torch.randint(-3, 4, (B, (N + 1) // 2, C), generator=g).float()
        assert not bool(torch.signbit(feat[feat == 0]).any())                      # no -0.0
    elif kind == "negative":
        for b in range(B):
            in_cell = cell_of[b, 0] == cell_of[b, 0, N // 2]
            feat[b, in_cell] = -feat[b, in_cell].abs() - 0.5
        assert all(bool((feat[b, cell_of[b, 0] == cell_of[b, 0, N // 2]] < 0).all()) for b in range(B))
    elif kind == "scaled":
        feat[..., 0::2] *= 2.0 ** 100
        feat[..., 1::2] *= 2.0 ** -100
        assert bool(torch.isfinite(feat).all()) and float(feat.abs().min()) > 2.0 ** -126   # all normal numbers
    else:
        assert kind == "randn"
    feat = feat + offset

    if layout == "random" and R > 1 and N > 1:
        assert not torch.equal(cell_of[0], cell_of[1])                             # per batch item
        if N > len(CLAMPED):
            assert not torch.equal(cell_of[:, 0], cell_of[:, 1]) and not torch.equal(cell_of[:, 1], cell_of[:, 2])
    if layout == "corner":
        assert bool((count[:, 0, cells - 1] == N).all()) and bool((count[:, 1, 0] == N).all())
    if R == 1:
        assert bool((count == N).all())                                            # one segment of all points
    if R == 96 and layout == "random":
        assert float((count == 0).float().mean()) >= 0.8                           # the product grid is mostly empty
        for b in range(B):
            assert bool((count[b, :, 0] == 0).any()) and bool((count[b, :, -1] == 0).any())
            assert bool((count[b] == 1).any())
    return dict(feat=feat, cell_of=cell_of, cells=cells, R=R)


CELL_WIDTHS = (1, 63, 64, 65, 255, 256, 257, 512)
CELL_GRIDS = (1, 6, 96)
# every C with N = 701, every N with C = 65 and C = 257; on each of the three grids
CELL_SHAPES = tuple((C, 701) for C in CELL_WIDTHS) + tuple((C, N) for C in (65, 257) for N in (1, 5, 1029))
CELL_CASES = (tuple((C, N, R) for R in CELL_GRIDS for C, N in CELL_SHAPES)
              + tuple((257, 701, R, kind) for R in CELL_GRIDS for kind in ("ties", "negative", "scaled"))
              + ((65, 701, 96, "randn", "corner"),)
              + ((65, 4099, 1, "randn", "random", 1000.0),))     # one long segment with a common offset


def cells_id(key):
    return "-".join(f"{n}{v}" for n, v in zip(("C", "N", "R", "", "", "plus"), key))


# ------------------------------------------------------------------------------------------------- projection cases
def _rotation(about_y, about_x, about_z):
    cy, sy, cx, sx = math.cos(about_y), math.sin(about_y), math.cos(about_x), math.sin(about_x)
    Ry = torch.tensor([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = torch.tensor([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Rz = torch.tensor([[math.cos(about_z), -math.sin(about_z), 0], [math.sin(about_z), math.cos(about_z), 0], [0, 0, 1]])
    return (Rz @ Rx @ Ry).float()


PROJECT_SCENES = ((1029, 50, 70, 0.18), (1029, 50, 70, 0.5), (257, 64, 48, 0.18), (1029, 33, 19, 4.86),
                  (255, 17, 300, 2.5), (1, 1, 1, 0.6))


@functools.lru_cache(maxsize=None)
def project_scene(N, H, W, radius_px, seed=0):
    """-> dict(points [2,N,3], w2c [2,4,4], K [2,3,3], H, W, radius_px, pixel_of): item 0 looks down the axis from a
    shifted position, item 1 is rotated about y, x and z and shifted, so every entry of its extrinsic is non-zero but the
    last row's; fx != fy and the principal point is off-centre.  Read-only: cached."""
    B = 2
    g = torch.Generator().manual_seed(seed + 7 * N + H)
    points = torch.randn(B, N, 3, generator=g) * torch.tensor([0.55, 0.55, 0.3]) + torch.tensor([0.0, 0.0, 2.0])
    if N > 8:
        points[:, 3:6, 2] = -1.0                                                   # behind the camera
    if N == 1:
        points[:] = torch.tensor([0.0, 0.0, 2.0])
    E = torch.eye(4).repeat(B, 1, 1)
    E[0, :3, 3] = torch.tensor([0.1, -0.05, 0.2])
    E[1, :3, :3] = _rotation(0.3, 0.2, 0.1)                      # a roll too: two axes alone leave one entry zero
    E[1, :3, 3] = torch.tensor([-0.55, 0.4, 0.15])
    if N == 1:                                                                     # keep the one point on the axis
        E[1, :3, 3] = points[1, 0] - E[1, :3, :3] @ points[1, 0]
    K = torch.tensor([[0.9 * W, 0, 0.45 * W], [0, 1.1 * H, 0.55 * H], [0, 0, 1]]).repeat(B, 1, 1)
    K[1, 0, 0] *= 1.1
    pixel_of = project_fp32(points, E, K, H, W, radius_px)

    assert bool((E[1, :3] != 0).all()) and float(K[0, 0, 0]) != float(K[0, 1, 1])
    assert float(K[0, 0, 2]) != W / 2 and float(K[0, 1, 2]) != H / 2
    hit = pixel_of >= 0
    if (N, H, W) == (1, 1, 1):
        assert bool(hit[0, 0])
    else:
        assert int(hit.sum()) >= 20 and int((~hit).sum()) >= 20, (int(hit.sum()), int((~hit).sum()))
        assert bool(hit[0].any()) and bool(hit[1].any())
        assert not bool(hit[:, 3:6].any())
    return dict(points=points, w2c=E, K=K, H=H, W=W, radius_px=radius_px, pixel_of=pixel_of)


def scene_features(scene, C, seed=0):
    g = torch.Generator().manual_seed(seed + C)
    return torch.randn(scene["points"].shape[0], C, scene["H"], scene["W"], generator=g)


LATTICE_K = ((64.0, 0.0, 12.0), (0.0, 64.0, 8.0), (0.0, 0.0, 1.0))
LATTICE_H, LATTICE_W, LATTICE_R = 16, 24, 2.5


def _lattice_point(u, v, Z):
    """the point that projects to exactly (u, v) at depth Z under LATTICE_K and the identity extrinsic (Z = 2, 4)"""
    return [(u - 12.0) * Z / 64.0, (v - 8.0) * Z / 64.0, Z]


def lattice_scene():
    """One item, identity extrinsic, u = 32 X + 12 and v = 32 Y + 8 exact at Z = 2.  Points by id:
    0 (8, 4.5)    1 the same at Z = 4    2, 3 identical at (20, 10.5)    4 (0, 0)    5 (24, 16)    6 (-5, -5)
    7 on the axis at Z = 1e-30    8 on the axis at Z = 2    9, 10 [+-0.1, 0.1, 1e-30]
    11 (-1, 8) left    12 (25, 4) right    13 (16, -1) top    14 (4, 17) bottom"""
    pts = [_lattice_point(8, 4.5, 2.0), _lattice_point(8, 4.5, 4.0), _lattice_point(20, 10.5, 2.0),
           _lattice_point(20, 10.5, 2.0), _lattice_point(0, 0, 2.0), _lattice_point(24, 16, 2.0),
           _lattice_point(-5, -5, 2.0), [0.0, 0.0, 1e-30], [0.0, 0.0, 2.0], [0.1, 0.1, 1e-30], [-0.1, 0.1, 1e-30],
           _lattice_point(-1, 8, 2.0), _lattice_point(25, 4, 2.0), _lattice_point(16, -1, 2.0),
           _lattice_point(4, 17, 2.0)]
    points = torch.tensor(pts, dtype=torch.float32)[None]
    scene = dict(points=points, w2c=torch.eye(4)[None], K=torch.tensor(LATTICE_K)[None], H=LATTICE_H, W=LATTICE_W,
                 radius_px=LATTICE_R)
    Z, u, v = _camera(points, scene["w2c"], scene["K"])
    assert u[0, 0] == 8 and v[0, 0] == 4.5 and u[0, 1] == 8 and v[0, 1] == 4.5 and u[0, 5] == 24 and v[0, 5] == 16
    assert abs(float(u[0, 9])) > 1e30 and abs(float(u[0, 10])) > 1e30 and np.isfinite(u).all() and np.isfinite(v).all()
    return scene


@functools.lru_cache(maxsize=None)
def ties_scene():
    """One item, identity extrinsic: 200 points at exactly Z = 2 with overlapping discs, then points 0..49 again as
    ids 200..249."""
    g = torch.Generator().manual_seed(5)
    H, W, r = 24, 32, 2.5
    points = torch.empty(1, 250, 3)
    points[0, :200, :2] = (torch.rand(200, 2, generator=g) - 0.5) * torch.tensor([1.0, 0.75])
    points[0, :200, 2] = 2.0
    points[0, 200:] = points[0, :50]
    E = torch.eye(4)[None]
    K = torch.tensor([[60.0, 0, 15.0], [0, 62.0, 13.0], [0, 0, 1]])[None]
    ids, depth, contested = rasterise_fp32(points, E, K, H, W, r)
    pixel_of = project_fp32(points, E, K, H, W, r)
    assert bool((depth[ids >= 0] == 2.0).all())
    # pixels inside two or more DIFFERENT discs at the same depth (a copy alone makes a count of 2)
    low = rasterise_fp32(points[:, :200], E, K, H, W, r)[2]
    assert int((low >= 2).sum()) >= 10 and bool((contested >= low).all())
    assert bool((pixel_of[0, 200:] == -1).all()) and int((pixel_of[0, :50] >= 0).sum()) >= 10
    return dict(points=points, w2c=E, K=K, H=H, W=W, radius_px=r, pixel_of=pixel_of)


@functools.lru_cache(maxsize=None)
def near_plane_scene(overflow=False):
    """Two items whose extrinsics do not rotate (so camera Z is the point's own z, exactly): 300 ordinary points, then
    points a hair in front of the camera plane with lateral offsets of both signs, on it (0, -0.0) and behind it.
    overflow=True appends points whose u or v overflows fp32 to +-inf (outside what the oracle can evaluate).
    -> the scene, plus `base`: the same scene without the appended points."""
    g = torch.Generator().manual_seed(11)
    B, N0, H, W, r = 2, 300, 40, 56, 2.5
    base = torch.randn(B, N0, 3, generator=g) * torch.tensor([0.5, 0.4, 0.3]) + torch.tensor([0.0, 0.0, 2.0])
    near = [[sx * ox, sy * oy, z] for z in (1e-30, 1e-20, 1e-6)
            for sx, sy, ox, oy in ((1, 1, 0.1, 0.1), (-1, 1, 0.1, 0.2), (1, -1, 0.3, 0.1), (-1, -1, 0.2, 0.2),
                                   (1, 1, 0.1, 0.0))]
    near.append([-0.1, 0.0, 1e-30])                                                # 16 in front
    other = [[0.0, 0.0, 0.0], [0.1, -0.1, 0.0], [0.0, 0.0, -0.0], [-0.1, 0.1, -0.0], [0.0, 0.0, -1e-30],
             [0.1, 0.1, -2.0]]
    extra = near + other
    if overflow:
        extra = extra + [[1.0, 0.0, 2e-38], [-1.0, 0.0, 2e-38], [0.0, 1.0, 2e-38], [0.0, -1.0, 2e-38],
                         [1.0, -1.0, 2e-38]]
    extra = torch.tensor(extra, dtype=torch.float32)
    points = torch.cat([base, extra[None].expand(B, -1, -1)], dim=1).contiguous()
    E = torch.eye(4).repeat(B, 1, 1)
    E[1, :2, 3] = torch.tensor([0.1, -0.05])
    K = torch.tensor([[60.0, 0, 26.0], [0, 62.0, 21.0], [0, 0, 1]]).repeat(B, 1, 1)
    pixel_of = project_fp32(points, E, K, H, W, r)
    base_pixel_of = project_fp32(base, E, K, H, W, r)

    Z, u, v = _camera(points, E, K)
    assert len(near) == 16 and bool((Z[:, N0:N0 + 16] > 0).all()) and bool((Z[:, N0 + 16:N0 + 22] <= 0).all())
    huge = np.maximum(np.abs(u[:, N0:N0 + 16]), np.abs(v[:, N0:N0 + 16]))
    assert bool((huge > 2.0 ** 31).any(axis=0).sum() >= 10) and float(huge.min()) > 1e5   # beyond int, all off screen
    finite = np.isfinite(u[:, N0:N0 + 16]).all() and np.isfinite(v[:, N0:N0 + 16]).all()
    assert finite
    if overflow:
        assert bool((~np.isfinite(u[:, N0 + 22:]) | ~np.isfinite(v[:, N0 + 22:])).all())
    assert bool((pixel_of[:, N0:] == -1).all()) and torch.equal(pixel_of[:, :N0], base_pixel_of)
    assert int((base_pixel_of >= 0).sum()) >= 20
    return dict(points=points, w2c=E, K=K, H=H, W=W, radius_px=r, pixel_of=pixel_of,
                base=dict(points=base, w2c=E, K=K, H=H, W=W, radius_px=r, pixel_of=base_pixel_of))
