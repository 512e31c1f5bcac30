"""numpy restatement of the mesh overlay (include/amav.h, amav_mesh_overlay; csrc/mesh.hip): a model the tests compare
the kernels with, not a test.  fp64 projection, int64 coverage on GIVEN snapped coordinates with the top-left fill rule,
fp64 perspective-correct depth, the lowest face id on exact ties, the Lambert shade, and for every pixel a near-tie
flag: the two nearest covering faces differ in depth by less than NEAR_TIE relative, so fp32 depths may order them
either way."""
import numpy as np

SNAP = 256          # snapped units per pixel
GUARD = 1 << 22     # snapped units: 16384 px
NEAR_TIE = 1e-5     # relative depth difference under which the winner of a pixel is not compared


def project(vertices, K, E, transl=None):
    """vertices [V,3], K [3,3], E [4,4] world-to-camera (OpenCV), transl [3] or None -> (p_cam [V,3], uv [V,2]) fp64."""
    p = np.asarray(vertices, np.float64)
    if transl is not None:
        p = p + np.asarray(transl, np.float64)
    E, K = np.asarray(E, np.float64), np.asarray(K, np.float64)
    pc = p @ E[:3, :3].T + E[:3, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        uv = np.stack([K[0, 0] * pc[:, 0] / pc[:, 2] + K[0, 2], K[1, 1] * pc[:, 1] / pc[:, 2] + K[1, 2]], axis=1)
    return pc, uv


def snap(uv):
    """Pixels -> int64 units of 1/256 px, round to nearest even (rintf)."""
    return np.rint(np.clip(np.nan_to_num(np.asarray(uv, np.float64) * SNAP, nan=-2.0 ** 30), -2.0 ** 30, 2.0 ** 30)).astype(np.int64)


def doubled_area(xy):
    """xy [...,3,2] int64 -> (x1-x0)(y2-y0) - (x2-x0)(y1-y0); NEGATIVE for a front face (y points down)."""
    a, b, c = xy[..., 0, :], xy[..., 1, :], xy[..., 2, :]
    return (b[..., 0] - a[..., 0]) * (c[..., 1] - a[..., 1]) - (c[..., 0] - a[..., 0]) * (b[..., 1] - a[..., 1])


def _edge(a, b, px, py):
    """Edge function of a -> b at the points (px, py), and whether the edge owns the points lying exactly on it when the
    interior is where the function is positive: a left edge (the interior to its right, the function grows with x) or a
    top edge (horizontal, the interior below it, the function grows with y; y points down)."""
    dx, dy = int(b[0] - a[0]), int(b[1] - a[1])
    e = dx * (py - int(a[1])) - dy * (px - int(a[0]))
    left, top = -dy > 0, dy == 0 and dx > 0
    return e, left or top


def coverage(tri, H, W):
    """tri [3,2] int64 snapped (x, y) -> (rows, cols, w [n,3] int64 edge values, doubled area > 0) of the pixel centres
    (256 c + 128, 256 r + 128) the face owns under the top-left rule; either winding.  None for a zero area."""
    tri = np.asarray(tri, np.int64)
    area2 = int(doubled_area(tri))
    if area2 == 0:
        return None
    if area2 < 0:  # make the interior the positive side of every edge
        tri = tri[[0, 2, 1]]
    c0 = max(0, -((128 - int(tri[:, 0].min())) // SNAP))          # ceil((min - 128) / 256)
    c1 = min(W - 1, (int(tri[:, 0].max()) - 128) // SNAP)
    r0 = max(0, -((128 - int(tri[:, 1].min())) // SNAP))
    r1 = min(H - 1, (int(tri[:, 1].max()) - 128) // SNAP)
    if c1 < c0 or r1 < r0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, 3), np.int64), abs(area2)
    rr, cc = np.meshgrid(np.arange(r0, r1 + 1, dtype=np.int64), np.arange(c0, c1 + 1, dtype=np.int64), indexing="ij")
    px, py = SNAP * cc + 128, SNAP * rr + 128
    inside = np.ones(rr.shape, bool)
    w = []
    for k in range(3):  # the edge opposite vertex k
        e, owns = _edge(tri[(k + 1) % 3], tri[(k + 2) % 3], px, py)
        inside &= (e >= 0) if owns else (e > 0)
        w.append(e)
    w = np.stack(w, axis=-1)[inside]
    if area2 < 0:
        w = w[:, [0, 2, 1]]  # back to the caller's vertex order
    return rr[inside], cc[inside], w, abs(area2)


def rasterize(screen, z, faces, H, W, znear=0.05, cull_backfaces=True):
    """screen [V,2] int64 snapped coordinates, z [V] fp64 camera depth, faces [T,3] -> dict:
    face_index int32 [H,W] (-1: uncovered), depth fp64 [H,W] (0: uncovered), near_tie bool [H,W], status (near drops,
    guard-band drops), kept bool [T] (rasterized: not dropped, not culled, non-zero area), front bool [T]."""
    screen, z, faces = np.asarray(screen, np.int64), np.asarray(z, np.float64), np.asarray(faces, np.int64)
    T = faces.shape[0]
    best = np.full((H, W), np.inf)
    second = np.full((H, W), np.inf)
    winner = np.full((H, W), -1, np.int32)
    near = ~(z[faces] >= znear).all(axis=1)
    guard = ~near & (np.abs(screen[faces]).reshape(T, 6).max(axis=1) > GUARD)
    area2 = doubled_area(np.where((near | guard)[:, None, None], 0, screen[faces]))
    front = area2 < 0
    kept = ~near & ~guard & (area2 != 0) & (front | (not cull_backfaces))
    tri = screen[faces]
    # faces whose box holds no pixel centre are skipped without a visit
    lo, hi = tri.min(axis=1), tri.max(axis=1)
    c0, c1 = np.maximum(0, -((128 - lo[:, 0]) // SNAP)), np.minimum(W - 1, (hi[:, 0] - 128) // SNAP)
    r0, r1 = np.maximum(0, -((128 - lo[:, 1]) // SNAP)), np.minimum(H - 1, (hi[:, 1] - 128) // SNAP)
    for t in np.nonzero(kept & (c1 >= c0) & (r1 >= r0))[0]:
        rows, cols, w, a2 = coverage(tri[t], H, W)
        if rows.size == 0:
            continue
        b = w.astype(np.float64) / float(a2)
        d = 1.0 / (b / z[faces[t]]).sum(axis=1)
        old, old_id = best[rows, cols], winner[rows, cols]
        wins = (d < old) | ((d == old) & (t < old_id))  # ascending t: the second clause never holds; kept for clarity
        second[rows, cols] = np.where(wins, old, np.minimum(second[rows, cols], d))
        best[rows, cols] = np.where(wins, d, old)
        winner[rows, cols] = np.where(wins, t, old_id)
    covered = winner >= 0
    depth = np.where(covered, best, 0.0)
    with np.errstate(invalid="ignore"):
        near_tie = covered & np.isfinite(second) & ((second - best) < NEAR_TIE * best)
    return {"face_index": winner, "depth": depth, "near_tie": near_tie, "status": (int(near.sum()), int(guard.sum())),
            "kept": kept, "front": front}


def shade(p_cam, faces, k, front=None):
    """Lambert shade of every face under the camera's headlight l = (0, 0, -1): min(1, k max(0, n . l)), n the unit
    normal (p1 - p0) x (p2 - p0) in camera space, reversed for the faces where `front` is False.  -> fp64 [T,3]."""
    p = np.asarray(p_cam, np.float64)[np.asarray(faces, np.int64)]
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    length = np.linalg.norm(n, axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        ndotl = np.where(length > 0, -n[:, 2] / length, 0.0)
    if front is not None:
        ndotl = np.where(front, ndotl, -ndotl)
    return np.minimum(1.0, np.asarray(k, np.float64)[None, :] * np.maximum(0.0, ndotl)[:, None])


def shade_k(base_color=(0.8, 0.8, 0.8), light_intensity=5.0):
    return 0.96 * np.asarray(base_color, np.float64) * light_intensity / np.pi


def render(vertices, faces, K, E, H, W, transl=None, screen=None, znear=0.05, cull_backfaces=True):
    """One frame of the model; `screen`: snapped coordinates to use instead of the model's own (the kernel's
    out_screen).  -> rasterize()'s dict plus p_cam, uv, screen."""
    pc, uv = project(vertices, K, E, transl)
    sc = snap(uv) if screen is None else np.asarray(screen, np.int64)
    out = rasterize(sc, pc[:, 2], faces, H, W, znear, cull_backfaces)
    out.update(p_cam=pc, uv=uv, screen=sc)
    return out
