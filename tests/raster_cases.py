"""Deterministic rasterizer scenes that put a tile list of a chosen length and depth pattern into a chosen tile, and
the oracle results the GPU parity tests share.  No GPU involved: test_raster_cases.py checks with the oracle alone that
every scene reaches the classes it is built for.

All cameras are E = identity, so the view depth of a Gaussian is its z exactly and depth relations (ties, clusters)
are decided by the inputs.  A scene is a dict of RAW decoder outputs (xyz, rot, scale, opacity, color as [F, N, *]
tensors, the values Renderer.unpack_gaussians views in a packed record buffer), K, E, H, W and `counts`, the intended
list length of every tile ([F, tiles]).  `activated(scene)` gives the same Gaussians as the rasterizer's activated
inputs, `raw(scene)` the packed [F, N, 16] record buffer.

Sort paths of rasterizer.hip and the list lengths that choose them (kSortCap 512, kPrepCap 256, kBucketMax 16,
kBigLdsCap 2048, kBigBucketMax 32):
    wave's first tile (`!ready`)    n <= 64 rank_sort<1>; bucket_sort<2|3|4|6|8> for n <= 128|192|256|384|512, and when
                                    a bucket of 512 holds more than 16 keys rank_sort<2|3|4> (n <= 256) or
                                    wave_bitonic_sort (n > 256)
    sorted under the previous tile  (`sort_prefetched`, n <= 256, only a wave's second and later tiles) n <= 64
                                    rank_sort<1>; 256 buckets, and when one holds more than 16 keys rank_sort<4>
    sort_big_kernel                 n > 512: 2048 buckets (n <= 2048, no bucket above 32 keys), else the LDS bitonic
                                    network (n <= 2048), else the in-place global network
A wave's first queue position is static (the blend grid is 16 waves per CU, one eighth of it per queue), so the
second group is reached only by a launch with more tiles in a queue than the queue has waves: `train_scene`.
"""
import functools
import math

import numpy as np
import torch

LADDER = (0, 1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 383, 384, 385, 511, 512, 513, 1000, 2047,
          2048, 2049, 2600)
LADDER_N = 2600
LADDER_F = 96
DEPTHS = ("spread", "clustered", "equal")
# (F, first frame) of the launches below the fused frame count: frame 51 has 2600 Gaussians, frames 20 .. 25 have 513,
# 1000, 2047, 2048, 2049 and 2600.  Chosen, like the seed, so that the oracle flags < 0.5 % of each launch's pixels.
LADDER_SUBSETS = ((1, 51), (6, 20), (95, 20))
SEED = 20260
FOCAL = 128.0       # pixels: a 3-pixel footprint at z = 3 stays below the activation's scale cap of 0.1
SCALE_BIAS = 3.9    # the activations of renderer.py:532-547 (oracle.rasterizer.render_one)
Z_TIE = 2.5
TILE = 16
QUEUES = 8          # rasterizer.hip kQueues: tile (f, row band) feeds queue (band + f) % 8
WAVES_PER_CU = 16   # rasterizer.hip render_grid(): 4 * kRenderWavesPerSimd one-wave blocks per CU
PREP_LADDER = tuple(n for n in LADDER if 0 < n <= 256)   # the lengths sort_prefetched takes
TRAIN_FILL = 300    # list length of the train's leading frames (one bucket class, above kPrepCap)


def _depths(g, n, kind):
    """z of n live Gaussians.  spread: a permutation of linspace(2.2, 3.0, n) -- one binade, so the depth word of the
    sort key is linear in z and no bucket of 256, 512 or 2048 collects more than ceil(n / buckets) + 1 keys.
    clustered: ceil(0.7 n) share z = 2.5 exactly, the rest are spread, all at random positions.  equal: all 2.5."""
    if kind == "equal":
        return torch.full((n,), Z_TIE)
    if kind == "spread":
        return torch.linspace(2.2, 3.0, n)[torch.randperm(n, generator=g)]
    if kind != "clustered":
        raise ValueError(f"depths: {kind!r}")
    tied = n - (3 * n) // 10
    z = torch.cat([torch.full((tied,), Z_TIE), torch.linspace(2.2, 3.0, n - tied)])
    return z[torch.randperm(n, generator=g)]


def _footprint(n, cap):
    """Pixel sigma of the 3-D part of a footprint (the rasterizer adds 0.3 to the variance), so that a pixel of a tile
    with n Gaussians sees a summed alpha of about 2.5: the blend neither saturates nor leaves the order immaterial."""
    var = 2.5 * TILE * TILE / (max(n, 1) * 0.175 * 2.0 * math.pi) - 0.3
    return min(cap, max(0.25, math.sqrt(max(var, 0.0))))


def _tile_gaussians(g, n, kind, x0, y0, cx, cy, cap, inside):
    """Raw attributes of n Gaussians whose centres fall into the tile at pixel origin (x0, y0) of an image with
    principal point (cx, cy).  inside: keep the whole 3-sigma square inside the tile (so it enters this list only)."""
    u = lambda *s: torch.rand(*s, generator=g)
    z = _depths(g, n, kind)
    sig = _footprint(n, cap)
    jitter = 0.75 + 0.5 * u(n, 3)                                  # mildly anisotropic, at most 1.25 sigma
    # 1.3: the projection's off-axis terms widen a footprint by a few percent at these fields of view
    margin = math.ceil(3.0 * math.sqrt((1.3 * 1.25 * sig) ** 2 + 0.3)) if inside else 1.0
    px = x0 + margin + (TILE - 2 * margin) * u(n)
    py = y0 + margin + (TILE - 2 * margin) * u(n)
    xyz = torch.stack([(px + 0.5 - cx) * z / FOCAL, (py + 0.5 - cy) * z / FOCAL, z], 1)
    scale = torch.log(sig * jitter * z[:, None] / FOCAL) + SCALE_BIAS
    rot = torch.nn.functional.normalize(torch.randn(n, 4, generator=g), dim=-1)
    alpha = 0.05 + 0.25 * u(n, 1)                                  # peak alpha
    color = u(n, 3) * 1.4 - 0.2                                    # exercises the colour clamp
    return dict(xyz=xyz, rot=rot, scale=scale, opacity=torch.log(alpha / (1 - alpha)), color=color)


def _culled(n):
    """n records behind the camera (z = -1)."""
    return dict(xyz=torch.tensor([0.0, 0.0, -1.0]).repeat(n, 1), rot=torch.tensor([1.0, 0, 0, 0]).repeat(n, 1),
                scale=torch.zeros(n, 3), opacity=torch.zeros(n, 1), color=torch.zeros(n, 3))


def _assemble(frames, counts, H, W):
    F = len(frames)
    scene = {k: torch.stack([fr[k] for fr in frames]) for k in ("xyz", "rot", "scale", "opacity", "color")}
    K = torch.tensor([[FOCAL, 0, W / 2], [0, FOCAL, H / 2], [0, 0, 1.0]]).repeat(F, 1, 1)
    scene.update(K=K, E=torch.eye(4).repeat(F, 1, 1), H=H, W=W, counts=torch.tensor(counts, dtype=torch.int32))
    return scene


def _frame(g, N, tiles, H, W, cap, inside):
    """One frame: `tiles` = [(n, kind, x0, y0)], then culled records up to N, the live ones at shuffled ids."""
    parts = [_tile_gaussians(g, n, kind, x0, y0, W / 2, H / 2, cap, inside) for n, kind, x0, y0 in tiles if n > 0]
    live = sum(n for n, *_ in tiles)
    assert live <= N
    parts.append(_culled(N - live))
    perm = torch.randperm(N, generator=g)
    return {k: torch.cat([p[k] for p in parts])[perm] for k in parts[0]}


def ladder_lengths(F=LADDER_F):
    return [LADDER[f % len(LADDER)] for f in range(F)]


def ladder_scene(depths, seed=SEED, F=LADDER_F, lengths=None, N=LADDER_N):
    """F frames of one 16 x 16 image (one tile): frame f has lengths[f] live Gaussians (default: LADDER, cyclically),
    all inside the image, the other records culled."""
    lengths = ladder_lengths(F) if lengths is None else list(lengths)
    frames = []
    for f, n in enumerate(lengths):
        g = torch.Generator().manual_seed(seed * 1000003 + 7919 * DEPTHS.index(depths) + f)
        frames.append(_frame(g, N, [(n, depths, 0, 0)], TILE, TILE, 3.0, inside=False))
    return _assemble(frames, [[n] for n in lengths], TILE, TILE)


MIXED_LENGTHS = (5, 40, 64, 70, 130, 200, 250, 260, 300, 400, 500, 520, 600, 900)


def mixed_scene(seed=SEED, F=97, N=1500):
    """48 x 32 frames (3 x 2 tiles): every tile of a frame holds a list of its own length (drawn from MIXED_LENGTHS, at
    most N per frame) and depth pattern (spread or clustered), each Gaussian inside one tile only, so lists of different
    length classes meet in one frame's queue buckets."""
    H, W = 2 * TILE, 3 * TILE
    frames, counts = [], []
    for f in range(F):
        g = torch.Generator().manual_seed(seed * 1000003 + 104729 + f)
        order = torch.randperm(len(MIXED_LENGTHS), generator=g).tolist()
        ns, left = [], N
        for t in range(6):
            n = next((MIXED_LENGTHS[i] for i in order[t:] + order[:t] if MIXED_LENGTHS[i] <= left), 0)
            ns.append(n)
            left -= n
        tiles = [(n, ("spread", "clustered")[(t + f) % 2], TILE * (t % 3), TILE * (t // 3)) for t, n in enumerate(ns)]
        frames.append(_frame(g, N, tiles, H, W, 1.2, inside=True))
        counts.append(ns)
    return _assemble(frames, counts, H, W)


def train_waves(compute_units):
    """Waves of the blend kernel per queue (render_grid(): 16 one-wave blocks per CU, dealt over the 8 queues)."""
    return compute_units * WAVES_PER_CU // QUEUES


def train_lengths(lead):
    """`lead` frames of TRAIN_FILL Gaussians per queue, then every length of PREP_LADDER twice in every queue
    (13 lengths, 8 queues, frame f feeds queue f % 8: 208 consecutive frames meet every pair twice)."""
    tail = 2 * QUEUES * len(PREP_LADDER)
    return [TRAIN_FILL] * (QUEUES * lead) + [PREP_LADDER[i % len(PREP_LADDER)] for i in range(tail)]


def train_scene(depths, lead, seed=SEED):
    """The launch that reaches sort_prefetched.  A queue hands its tiles out longest bucket first and a wave's first
    position is static, so with `lead` >= train_waves() frames of TRAIN_FILL Gaussians per queue every wave starts on
    one of those, and the PREP_LADDER frames behind them are all taken as second or later tiles: sorted under the
    previous tile.  The leading frames are copies of one frame (N = TRAIN_FILL records per frame)."""
    lengths = train_lengths(lead)
    nlead = QUEUES * lead
    tail = ladder_scene(depths, seed + 1, lengths=[TRAIN_FILL] + lengths[nlead:], N=TRAIN_FILL)
    pick = torch.cat([torch.zeros(nlead, dtype=torch.long), torch.arange(1, len(lengths) - nlead + 1)])
    scene = {k: (v[pick] if torch.is_tensor(v) else v) for k, v in tail.items()}
    scene["lead"] = nlead
    return scene


# ---- forms of a scene ----------------------------------------------------------------------------------------
_ATTRS = ("xyz", "rot", "scale", "opacity", "color")


def activated(scene):
    """The scene as the rasterizer's activated inputs: oracle.rasterizer.render_one's activations, in its fp32 ops."""
    out = dict(scene)
    out["scale"] = torch.min(torch.exp(scene["scale"] - SCALE_BIAS), torch.tensor(0.1))
    out["opacity"] = torch.sigmoid(scene["opacity"])
    out["color"] = torch.clamp(scene["color"], 0.0, 1.0)
    return out


def raw(scene):
    """The packed [F, N, 16] record buffer Renderer.unpack_gaussians views: xyz | opacity | rot | scale | color | pad."""
    F, N = scene["xyz"].shape[:2]
    rec = torch.zeros(F, N, 16, device=scene["xyz"].device)
    rec[..., 0:3], rec[..., 3:4], rec[..., 4:8] = scene["xyz"], scene["opacity"], scene["rot"]
    rec[..., 8:11], rec[..., 12:15] = scene["scale"], scene["color"]
    return rec


def take(scene, start, F):
    """Frames start, start + 1, ... (cyclically) of a scene, F of them."""
    idx = (torch.arange(F) + start) % scene["xyz"].shape[0]
    return {k: (v[idx] if torch.is_tensor(v) else v) for k, v in scene.items()}


def reverse_ties(scene):
    """The scene with the Gaussians of every frame's largest equal-depth group stored in reverse id order: the same
    Gaussians and depths, but every tie between two of them is broken the other way."""
    out = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in scene.items()}
    for f in range(scene["xyz"].shape[0]):
        z = scene["xyz"][f, :, 2]
        vals, cnt = torch.unique(z[z > 0], return_counts=True)
        if len(vals) == 0 or cnt.max() < 2:
            continue
        ids = torch.nonzero(z == vals[cnt.argmax()]).reshape(-1)
        for k in _ATTRS:
            out[k][f, ids] = scene[k][f, ids.flip(0)]
    return out


# ---- oracle results, computed once per process ---------------------------------------------------------------------
def oracle_activated(scene):
    """Per-frame oracle results of the activated scene (helpers.oracle_frames)."""
    from helpers import oracle_frames

    return oracle_frames(activated(scene), np.float32)


def oracle_product(scene, instances=None):
    """Per-frame references of the product launch: oracle.rasterizer.render_batch(full=True) on the raw scene (the
    activations, the colour clamp and clamp(0, 1) of the image), as the dicts raster_parity.compare_small reads."""
    from oracle import rasterizer as orc

    gauss = {k: scene[k][None] for k in _ATTRS}
    img, alpha, unstable = orc.render_batch(gauss, scene["K"][None], scene["E"][None], (scene["H"], scene["W"]), full=True)
    ref = [dict(color=img[0, f].permute(2, 0, 1).numpy(), alpha=alpha[0, f].numpy(),
                unstable=unstable[0, f].numpy().astype(np.uint8)) for f in range(img.shape[1])]
    if instances is not None:
        for r, n in zip(ref, instances):
            r["instances"] = int(n)
    return ref


@functools.lru_cache(maxsize=None)
def ladder_case(depths):
    """(scene, activated oracle frames, product references) of the 96-frame ladder."""
    scene = ladder_scene(depths)
    act = oracle_activated(scene)
    return scene, act, oracle_product(scene, [r["instances"] for r in act])


@functools.lru_cache(maxsize=None)
def mixed_case():
    scene = mixed_scene()
    act = oracle_activated(scene)
    return scene, act, oracle_product(scene, [r["instances"] for r in act])


def pick(ref, start, F):
    """The references of take(scene, start, F)."""
    return [ref[(start + i) % len(ref)] for i in range(F)]


def tile_lists(scene):
    """Per-tile list lengths [F, tiles] by the oracle's torch preprocess (tile rectangles of the visible Gaussians)."""
    from oracle import camera
    from oracle import rasterizer as orc

    act = activated(scene)
    H, W = scene["H"], scene["W"]
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    counts = torch.zeros(act["xyz"].shape[0], gy * gx, dtype=torch.int32)
    for f in range(act["xyz"].shape[0]):
        view, proj, tx, ty, _ = camera.camera_setup(scene["K"][f], scene["E"][f], H, W)
        g = orc.preprocess_torch(act["xyz"][f], act["rot"][f], act["scale"][f], act["opacity"][f], view, proj, tx, ty, H, W)
        x0, y0, x1, y1 = g["rect"]
        for t in range(gy * gx):
            hit = g["visible"] & (x0 <= t % gx) & (t % gx < x1) & (y0 <= t // gx) & (t // gx < y1)
            counts[f, t] = int(hit.sum())
    return counts
