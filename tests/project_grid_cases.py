"""Inputs, CPU restatements and error bounds for amav_points_project_grid and its backward (csrc/splat.hip,
csrc/splat_backward.hip, csrc/grid_bilinear.h).  tests/test_project_grid_model.py holds the restatements to fp64 and to
the oracle, tests/test_project_grid_gpu.py holds the kernels to them.  Nothing here loads the HIP library.

The op: the point -> pixel selection of points_projection (stage1_splat_cases.project_fp32 / rasterise_fp32), then for a
point that claims pixel (y, x) channels 0..2 = rgb[:, y, x] and channel 3 + c = the grid [Gh,Gw,Cg] resized to H x W as
F.interpolate(mode="bilinear", align_corners=False) defines it, at (y, x).  Per axis, in fp32:

    scale = G / size;  s = scale * (i + 0.5) - 0.5;  s = max(s, 0);  i0 = min(int(s), G - 1);  i1 = i0 + (i0 < G - 1)
    l = s - i0;  h = 1 - l;            value = hy * (hx * g00 + lx * g01) + ly * (hx * g10 + lx * g11)

The backward is the gradient of the dense path: index_put credits EVERY pixel a point wins, so a node sums, over the won
pixels that have it as a corner, weight * grad_out[winner]: in ascending pixel index and corners 00, 01, 10, 11, every
weight one fp32 product (wy * wx), every term one fp32 product added to the running fp32 sum.

Error bounds, with u = 2**-24 (stated per function below):
  * the source coordinate s is computed with three roundings at magnitude |s| + 0.5 <= G, so it is off by at most
    delta = 3 u (|s| + 1); l = s - i0 is exact.  The interpolant is piecewise linear in s with slope at most the largest
    difference of neighbouring nodes, and every node's weight (a hat function of s) has slope at most 1 -- also across a
    cell boundary, where the fp32 and the exact s may choose different cells;
  * a value passes through at most six roundings (h, four products / sums on its way, the last sum): 7 u sum(w |g|);
  * a node's gradient: every term's weight is off by at most delta_x + delta_y + 4 u (two h's, the product, the product
    with g), and a sequential sum of n terms adds (n - 1) u sum |w g|.
"""
import functools

import numpy as np
import torch

import stage1_splat_cases as sc

f32 = np.float32
U = sc.U


# --------------------------------------------------------------------------------------------------------- one axis
def axis_fp32(size, G):
    """-> (i0, i1 int64 [size], l, h fp32 [size]): the kernels' arithmetic, one rounding per operation"""
    i = np.arange(size).astype(f32)
    scale = f32(f32(G) / f32(size))
    s = scale * (i + f32(0.5)) - f32(0.5)
    s = np.where(s < 0, f32(0), s).astype(f32)
    i0 = np.minimum(s.astype(np.int64), G - 1)
    i1 = i0 + (i0 < G - 1)
    l = s - i0.astype(f32)
    h = f32(1) - l
    assert s.dtype == f32 and l.dtype == f32 and h.dtype == f32
    return i0, i1, l, h


def axis_fp64(size, G):
    """-> (i0, i1, l, h fp64, delta fp64 [size]: the bound of the fp32 coordinate's error, 3 u (|s| + 1))"""
    i = np.arange(size).astype(np.float64)
    raw = (G / size) * (i + 0.5) - 0.5
    s = np.maximum(raw, 0.0)
    i0 = np.minimum(s.astype(np.int64), G - 1)
    i1 = i0 + (i0 < G - 1)
    l = s - i0
    return i0, i1, l, 1.0 - l, 3.0 * U * (np.abs(raw) + 1.0)


def _corners(ay, ax, y, x):
    """the four (node row, node column, weight factors) of pixels (y, x) in the order 00, 01, 10, 11"""
    return ((ay[0][y], ax[0][x], ay[3][y], ax[3][x]), (ay[0][y], ax[1][x], ay[3][y], ax[2][x]),
            (ay[1][y], ax[0][x], ay[2][y], ax[3][x]), (ay[1][y], ax[1][x], ay[2][y], ax[2][x]))


# ---------------------------------------------------------------------------------------------------------- forward
def forward_fp32(rgb, grid, pixel_of):
    """rgb fp32 [B,3,H,W], grid fp32 [B,Gh,Gw,Cg], pixel_of int64 [B,N] -> fp32 [B,N,3+Cg], the kernel's operations"""
    B, _, H, W = rgb.shape
    _, Gh, Gw, Cg = grid.shape
    ay, ax = axis_fp32(H, Gh), axis_fp32(W, Gw)
    out = np.zeros((B, pixel_of.shape[1], 3 + Cg), dtype=f32)
    for b in range(B):
        hit = (pixel_of[b] >= 0).numpy()
        p = pixel_of[b].numpy()[hit]
        y, x = p // W, p % W
        g = grid[b].numpy()
        (y0, x0, hy, hx), (_, x1, _, lx), (y1, _, ly, _), _ = _corners(ay, ax, y, x)
        hy, hx, ly, lx = (w[:, None] for w in (hy, hx, ly, lx))
        value = hy * (hx * g[y0, x0] + lx * g[y0, x1]) + ly * (hx * g[y1, x0] + lx * g[y1, x1])
        assert value.dtype == f32
        out[b, hit, :3] = rgb[b].numpy().reshape(3, -1)[:, p].T
        out[b, hit, 3:] = value
    return torch.from_numpy(out)


def forward_fp64(rgb, grid, pixel_of):
    """-> (value fp64 [B,N,3+Cg], bound fp64 [B,N,3+Cg]; the RGB channels are copies: bound 0).
    bound = delta_x Dx + delta_y Dy + 7 u sum(w |g|), Dx / Dy the frame's largest difference of neighbouring nodes along
    the axis per channel."""
    B, _, H, W = rgb.shape
    _, Gh, Gw, Cg = grid.shape
    ay, ax = axis_fp64(H, Gh), axis_fp64(W, Gw)
    N = pixel_of.shape[1]
    out, bound = np.zeros((B, N, 3 + Cg)), np.zeros((B, N, 3 + Cg))
    for b in range(B):
        hit = (pixel_of[b] >= 0).numpy()
        p = pixel_of[b].numpy()[hit]
        y, x = p // W, p % W
        g = grid[b].numpy().astype(np.float64)
        Dy = np.abs(np.diff(g, axis=0)).max(axis=(0, 1)) if Gh > 1 else np.zeros(Cg)
        Dx = np.abs(np.diff(g, axis=1)).max(axis=(0, 1)) if Gw > 1 else np.zeros(Cg)
        (y0, x0, hy, hx), (_, x1, _, lx), (y1, _, ly, _), _ = _corners(ay, ax, y, x)
        hy, hx, ly, lx = (w[:, None] for w in (hy, hx, ly, lx))
        out[b, hit, :3] = rgb[b].numpy().astype(np.float64).reshape(3, -1)[:, p].T
        out[b, hit, 3:] = hy * (hx * g[y0, x0] + lx * g[y0, x1]) + ly * (hx * g[y1, x0] + lx * g[y1, x1])
        a = np.abs(g)
        mass = hy * (hx * a[y0, x0] + lx * a[y0, x1]) + ly * (hx * a[y1, x0] + lx * a[y1, x1])
        bound[b, hit, 3:] = ax[4][x][:, None] * Dx + ay[4][y][:, None] * Dy + 7.0 * U * mass
    return torch.from_numpy(out), torch.from_numpy(bound)


# --------------------------------------------------------------------------------------------------------- backward
def backward_fp32(dout, ids, Gh, Gw):
    """dout fp32 [B,N,3+Cg], ids int64 [B,H,W] (rasterise_fp32: every pixel's winner or -1) -> (grad_grid fp32
    [B,Gh,Gw,Cg], grad_rgb fp32 [B,3,H,W], reached bool [B,Gh,Gw]: the nodes that receive a term).  The kernel's order:
    pixels one after the other in ascending index, corners 00, 01, 10, 11, w = wy * wx, sum = sum + w * g."""
    B, H, W = ids.shape
    Cg = dout.shape[2] - 3
    ay, ax = axis_fp32(H, Gh), axis_fp32(W, Gw)
    d = dout.numpy()
    grad = np.zeros((B, Gh, Gw, Cg), dtype=f32)
    rgb = np.zeros((B, 3, H * W), dtype=f32)
    reached = np.zeros((B, Gh, Gw), dtype=bool)
    for b in range(B):
        flat = ids[b].reshape(-1)
        won = np.flatnonzero(flat >= 0)
        rgb[b][:, won] = d[b, flat[won], :3].T
        for p in won:
            g = d[b, flat[p], 3:]
            for cy, cx, wy, wx in _corners(ay, ax, p // W, p % W):
                w = f32(wy * wx)
                grad[b, cy, cx] = grad[b, cy, cx] + w * g
                reached[b, cy, cx] = True
    assert grad.dtype == f32
    return torch.from_numpy(grad), torch.from_numpy(rgb.reshape(B, 3, H, W)), torch.from_numpy(reached)


def backward_fp64(dout, ids, Gh, Gw):
    """-> (grad_grid fp64 [B,Gh,Gw,Cg], bound fp64 [B,Gh,Gw,Cg]).
    bound[node] = sum over the pixels that reach the node, in fp64 or in fp32 arithmetic, of (delta_x + delta_y + 4 u)
    |g|, plus (n + 2) u sum |w g| for the node's n terms."""
    B, H, W = ids.shape
    Cg = dout.shape[2] - 3
    ay, ax = axis_fp64(H, Gh), axis_fp64(W, Gw)
    ay32, ax32 = axis_fp32(H, Gh), axis_fp32(W, Gw)
    grad, mass, slack = (np.zeros((B, Gh, Gw, Cg)) for _ in range(3))
    terms = np.zeros((B, Gh, Gw))
    for b in range(B):
        flat = ids[b].reshape(-1)
        won = np.flatnonzero(flat >= 0)
        y, x = won // W, won % W
        g = dout[b].numpy().astype(np.float64)[flat[won], 3:]
        e = (ax[4][x] + ay[4][y] + 4.0 * U)[:, None] * np.abs(g)
        for cy, cx, wy, wx in _corners(ay, ax, y, x):
            w = (wy * wx)[:, None]
            np.add.at(grad[b], (cy, cx), w * g)
            np.add.at(mass[b], (cy, cx), w * np.abs(g))
            np.add.at(slack[b], (cy, cx), e)
            np.add.at(terms[b], (cy, cx), 1.0)
        other = (ay32[0][y] != ay[0][y]) | (ax32[0][x] != ax[0][x])       # the fp32 coordinate chose another cell
        for cy, cx, _, _ in _corners(ay32, ax32, y[other], x[other]):
            np.add.at(slack[b], (cy, cx), e[other])
            np.add.at(terms[b], (cy, cx), 1.0)
    return torch.from_numpy(grad), torch.from_numpy(slack + (terms[..., None] + 2.0) * U * mass)


# ------------------------------------------------------------------------------------------------------------ cases
def _scene(name):
    if name == "lattice":
        return sc.lattice_scene()
    if name == "ties":
        return sc.ties_scene()
    if name == "near_plane":
        return sc.near_plane_scene()
    return sc.project_scene(*name)


RANDOM, LONG, ONE = (1029, 50, 70, 0.5), (255, 17, 300, 2.5), (1, 1, 1, 0.6)
assert RANDOM in sc.PROJECT_SCENES and LONG in sc.PROJECT_SCENES and ONE in sc.PROJECT_SCENES
WIDTHS = (1, 61, 64, 65, 125, 129)   # 3 + Cg on either side of the 64- and 128-lane strides
# (scene, (Gh, Gw), Cg): every width on one scene, every scene at Cg = 125
CASES = (tuple((RANDOM, (4, 5), Cg) for Cg in WIDTHS)          # ratios 12.5 and 14
         + ((RANDOM, (50, 70), 125),                           # identity scale: the value is the node itself
            (RANDOM, (1, 1), 125),
            (LONG, (32, 8), 125),                              # rows down-sampled (32 nodes for 17 pixels)
            ("lattice", (4, 5), 125), ("ties", (4, 5), 125), ("near_plane", (4, 5), 125),
            (ONE, (2, 2), 125)))


def case_id(key):
    scene, (Gh, Gw), Cg = key
    name = scene if isinstance(scene, str) else "x".join(str(v) for v in scene)
    return f"{name}-grid{Gh}x{Gw}-Cg{Cg}"


@functools.lru_cache(maxsize=None)
def winners(scene_key):
    """-> ids int64 ndarray [B,H,W] of the scene: every pixel's winner or -1 (stage1_splat_cases.rasterise_fp32)"""
    s = _scene(scene_key)
    return sc.rasterise_fp32(s["points"], s["w2c"], s["K"], s["H"], s["W"], s["radius_px"])[0]


@functools.lru_cache(maxsize=None)
def case(key):
    """-> dict(scene, pixel_of [B,N], ids [B,H,W], rgb [B,3,H,W], grid [B,Gh,Gw,Cg], dout [B,N,3+Cg], Gh, Gw, Cg).
    Read-only: cached.  Asserts, on the CPU restatements alone, that the case still has its edges."""
    scene_key, (Gh, Gw), Cg = key
    scene = _scene(scene_key)
    H, W = scene["H"], scene["W"]
    B, N = scene["points"].shape[:2]
    pixel_of = scene["pixel_of"] if "pixel_of" in scene else sc.project_fp32(
        scene["points"], scene["w2c"], scene["K"], H, W, scene["radius_px"])
    ids = winners(scene_key)
    g = torch.Generator().manual_seed(100 * Gh + 10 * Gw + Cg)
    rgb = torch.rand(B, 3, H, W, generator=g)
    grid = torch.randn(B, Gh, Gw, Cg, generator=g)
    dout = torch.randn(B, N, 3 + Cg, generator=g)

    hit = pixel_of >= 0
    won = int((ids >= 0).sum())
    assert bool(hit.any()) and won >= int(hit.sum())
    for b in range(B):   # the claimed pixel is the last one the point wins
        flat = ids[b].reshape(-1)
        p = pixel_of[b][hit[b]].numpy()
        assert (flat[p] == np.flatnonzero(hit[b].numpy())).all()
    ay, ax = axis_fp32(H, Gh), axis_fp32(W, Gw)
    edges = set()
    if bool((~hit).any()):
        edges.add("missed points")
    if won > int(hit.sum()):
        edges.add("won but not claimed")
    ys, xs = np.nonzero((ids >= 0).any(axis=0))
    for name, axis, at, size, G in (("rows", ay, ys, H, Gh), ("columns", ax, xs, W, Gw)):
        raw = (G / size) * (at + 0.5) - 0.5
        if (raw < 0).any():
            edges.add(f"first half-cell of the {name}")        # s clamped to 0: l == 0 exactly
            assert (axis[2][at[raw < 0]] == 0).all()
        if (axis[0][at] == axis[1][at]).any():
            edges.add(f"equal nodes in the {name}")            # i0 == i1 == G - 1: two terms for one node
            assert (axis[0][at[axis[0][at] == axis[1][at]]] == G - 1).all()
    reached = backward_fp32(torch.zeros(B, N, 4), ids, Gh, Gw)[2]
    if not bool(reached.all()):
        edges.add("nodes out of reach")
    return dict(scene=scene, pixel_of=pixel_of, ids=ids, rgb=rgb, grid=grid, dout=dout, Gh=Gh, Gw=Gw, Cg=Cg,
                edges=frozenset(edges), reached=reached)


# the edges every case must still have (checked in tests/test_project_grid_model.py)
ALL_BORDERS = {"first half-cell of the rows", "first half-cell of the columns", "equal nodes in the rows",
               "equal nodes in the columns"}
# (at a radius of 0.5 pixel a disc holds one pixel centre at most: RANDOM has no pixel that is won but not claimed)
EDGES = {
    (RANDOM, (4, 5)): {"missed points"} | ALL_BORDERS,
    (RANDOM, (50, 70)): {"missed points", "nodes out of reach", "equal nodes in the rows", "equal nodes in the columns"},
    (RANDOM, (1, 1)): {"missed points", "equal nodes in the rows", "equal nodes in the columns"},
    (LONG, (32, 8)): {"missed points", "won but not claimed", "nodes out of reach", "equal nodes in the columns",
                      "first half-cell of the columns"},
    ("lattice", (4, 5)): {"missed points", "won but not claimed", "nodes out of reach"} | ALL_BORDERS,
    ("ties", (4, 5)): {"missed points", "won but not claimed"} | ALL_BORDERS,
    ("near_plane", (4, 5)): {"missed points", "won but not claimed"} | ALL_BORDERS,
    (ONE, (2, 2)): set(),   # one pixel, s = 0.5 on both axes: all four nodes, a quarter each
}
