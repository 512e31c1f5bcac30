"""Oracle parity of the rasterizer forward on the launch the product runs, and on every sort path.

test_raster_gpu.py compares against the C oracle through run_hip(): five separate, already activated tensors with radii
and inverse depth requested, i.e. preprocess_kernel<false> / bin_kernel<true, false> without the LDS stash and
render_kernel<true>.  The renderer launches something else: views of one packed [F, N, 16] record buffer, activations
and the colour clamp inside the kernels, no radii (so the binning block keeps its records in LDS) and no inverse depth
(render_kernel<false>).  Here that launch, and the branches between the two, are compared with the oracle on the scenes
of raster_cases.py, whose frames put a tile list of every length class and depth pattern in front of the sorts
(test_raster_cases.py shows with the oracle alone that they do), under the rules of raster_parity.py.

Bit-for-bit relations on the same inputs then tie every branch to the configuration that test_raster_gpu.py anchors:
inverse depth on / off, radii on / off (stash off / on), packed / unpacked, one launch of 96 frames / sixteen of 6
(fused binning block / projection launch + sliced binning), and a second run of each.

Which sort orders a list follows from its length, its depths and whether it is a wave's first tile (raster_cases.py's
docstring).  A wave's first queue position is static and the blend grid has 512 waves per queue on 256 CUs, so in a
96-frame launch of one-tile frames EVERY list is a first tile: the ladder drives the `!ready` sorts and sort_big_kernel
only.  The sorts a wave runs under its previous tile (sort_prefetched) need more tiles in a queue than it has waves:
test_short_lists_sorted_under_the_previous_tile.
"""
import functools
import os

import numpy as np
import pytest
import torch

import raster_cases as rc
from raster_parity import compare_small

pytestmark = pytest.mark.gpu
DEV = "cuda"
ATTRS = ("xyz", "rot", "scale", "opacity", "color")


def camera(scene):
    from audio_motion_avatar_amd import ops

    return ops.camera_from_intrinsics(scene["K"].to(DEV), scene["E"].to(DEV), scene["H"], scene["W"])[:3]


def views(rec):
    """The five attribute views of a packed record buffer, in rasterize()'s order."""
    from audio_motion_avatar_amd.renderer import Renderer

    g = Renderer.unpack_gaussians(rec)
    return [g[k] for k in ATTRS]


def rasterize(scene, attrs, cam=None, workspace=None, **kw):
    """One launch; afterwards the tile lists must be the scene's (the scene reached its classes, not a kernel check)."""
    from audio_motion_avatar_amd import ops

    view, proj, tanfov = camera(scene) if cam is None else cam
    out = ops.rasterize(*attrs, view, proj, tanfov, scene["H"], scene["W"], workspace=workspace, **kw)
    torch.cuda.synchronize()
    if scene.get("counts") is not None:
        assert out["workspace"].tile_counts().cpu().tolist() == scene["counts"].flatten().tolist()
    return out


def product(scene, rec=None, **kw):
    """The renderer's launch: packed raw records, activations and clamp in the kernels, no radii, no inverse depth."""
    rec = rc.raw(scene).to(DEV) if rec is None else rec
    return rasterize(scene, views(rec), apply_activations=True, clamp_output=True, **kw)


def unpacked(scene, **kw):
    """Five separate contiguous activated tensors (test_raster_gpu.run_hip's inputs)."""
    act = rc.activated(scene)
    return rasterize(scene, [act[k].to(DEV).contiguous() for k in ATTRS], **kw)


@functools.lru_cache(maxsize=None)
def ladder_anchor(depths):
    """The configuration test_raster_gpu.py anchors (unpacked, activated, radii and inverse depth) on the ladder."""
    return unpacked(rc.ladder_case(depths)[0], want_inv_depth=True, want_radii=True)


def clamped(rgba):
    return torch.cat([rgba[..., :3].clamp(0.0, 1.0), rgba[..., 3:]], dim=-1)


# ---- oracle parity --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depths", rc.DEPTHS)
def test_product_launch(depths):
    scene, _, prod = rc.ladder_case(depths)
    out = product(scene)
    assert out["inv_depth"] is None and out["radii"] is None
    compare_small(f"product[{depths}]", prod, out)


@pytest.mark.parametrize("depths", rc.DEPTHS)
def test_unpacked_without_radii_and_inverse_depth(depths):
    """bin_kernel<true, false> with the stash, render_kernel<false>."""
    scene, act, _ = rc.ladder_case(depths)
    compare_small(f"unpacked_plain[{depths}]", act, unpacked(scene))


@pytest.mark.parametrize("F,start", rc.LADDER_SUBSETS)
@pytest.mark.parametrize("depths", rc.DEPTHS)
def test_product_launch_below_the_fused_frame_count(depths, F, start):
    """preprocess_kernel<true> and the sliced binning (16, 16 and 3 slices): the first F frames of the ladder rotated
    so that the long lists fall inside them (raster_cases.LADDER_SUBSETS)."""
    scene, _, prod = rc.ladder_case(depths)
    out = product(rc.take(scene, start, F))
    compare_small(f"product_F{F}[{depths}]", rc.pick(prod, start, F), out)


@pytest.mark.parametrize("depths", rc.DEPTHS)
def test_anchored_configuration(depths):
    """rgb, alpha, inverse depth, radii (exactly) and the instance total."""
    _, act, _ = rc.ladder_case(depths)
    out = ladder_anchor(depths)
    assert out["inv_depth"] is not None and out["radii"] is not None
    compare_small(f"anchored[{depths}]", act, out)


def test_mixed_lengths_in_one_frame():
    """97 frames of 3 x 2 tiles whose lists differ in length class and depth pattern: the queue buckets of one frame."""
    scene, _, prod = rc.mixed_case()
    out = product(scene)
    present = set(out["workspace"].tile_counts().cpu().tolist())
    assert present >= set(rc.MIXED_LENGTHS)
    compare_small("product_mixed", prod, out)


def test_shared_gaussians_packed():
    """frame_stride = 0 (render_multi_view) through the packed path: one frame's records, 96 cameras."""
    base = rc.take(rc.ladder_case("clustered")[0], 20, 1)  # 513 Gaussians, 360 of them at one depth
    F = 96
    scene = {k: (v.expand(F, *v.shape[1:]).clone() if torch.is_tensor(v) else v) for k, v in base.items()}
    shift = torch.arange(F)
    scene["K"][:, 0, 2] += ((shift % 5) - 2) * 0.37
    scene["K"][:, 1, 2] += ((shift % 7) - 3) * 0.29
    scene["counts"] = None  # the lists are the oracle's to say: a camera may push a Gaussian out of the image
    instances = [r["instances"] for r in rc.oracle_activated(scene)]
    ref = rc.oracle_product(scene, instances)
    rec = rc.raw(base).to(DEV)
    assert rec.shape[0] == 1
    out = product(scene, rec.expand(F, -1, -1))
    assert out["workspace"].tile_counts().cpu().tolist() == instances and min(instances) > 500
    compare_small("product_shared", ref, out)


# ---- bit-for-bit relations -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depths", rc.DEPTHS)
def test_branches_agree_bit_for_bit(depths):
    scene, _, _ = rc.ladder_case(depths)
    anchor = ladder_anchor(depths)["rgba"]
    act = rc.activated(scene)
    # inverse depth off (render_kernel<false>), radii still on (no stash)
    no_depth = unpacked(scene, want_radii=True)
    assert torch.equal(no_depth["rgba"], anchor), "inverse depth on / off"
    assert torch.equal(no_depth["radii"], ladder_anchor(depths)["radii"])
    # radii off as well: the binning block keeps its records in LDS
    plain = unpacked(scene)
    assert torch.equal(plain["rgba"], anchor), "radii on / off (stash off / on)"
    with_depth = unpacked(scene, want_inv_depth=True)
    assert torch.equal(with_depth["rgba"], anchor) and torch.equal(with_depth["inv_depth"], ladder_anchor(depths)["inv_depth"])
    # the same activated values as views of one record buffer: bin_kernel<true, true>
    packed = rasterize(scene, views(rc.raw(act).to(DEV)))
    assert torch.equal(packed["rgba"], anchor), "packed / unpacked"
    # a second run of each
    assert torch.equal(unpacked(scene, want_inv_depth=True, want_radii=True)["rgba"], anchor)
    assert torch.equal(unpacked(scene)["rgba"], anchor)
    assert torch.equal(rasterize(scene, views(rc.raw(act).to(DEV)))["rgba"], anchor)
    # the colour clamp is exact
    assert torch.equal(unpacked(scene, clamp_output=True)["rgba"], clamped(anchor))


@pytest.mark.parametrize("depths", rc.DEPTHS)
def test_product_launch_agrees_bit_for_bit(depths):
    """The product launch against the same raw values unpacked, with radii (no stash), with inverse depth, in launches
    of 6 frames, and run again."""
    scene, _, _ = rc.ladder_case(depths)
    rec = rc.raw(scene).to(DEV)
    cam = camera(scene)
    ref = product(scene, rec, cam=cam)["rgba"]
    assert torch.equal(product(scene, rec, cam=cam)["rgba"], ref), "second run"
    raw_unpacked = rasterize(scene, [scene[k].to(DEV).contiguous() for k in ATTRS], cam=cam, apply_activations=True,
                             clamp_output=True)
    assert torch.equal(raw_unpacked["rgba"], ref), "packed / unpacked"
    assert torch.equal(product(scene, rec, cam=cam, want_radii=True)["rgba"], ref), "radii on / off (stash off / on)"
    assert torch.equal(product(scene, rec, cam=cam, want_inv_depth=True)["rgba"], ref), "inverse depth on / off"
    for s in range(0, rc.LADDER_F, 6):
        part = product(rc.take(scene, s, 6), rec[s:s + 6], cam=[c[s:s + 6] for c in cam])
        assert torch.equal(part["rgba"], ref[s:s + 6]), f"frames {s}..{s + 5} launched on their own"


# ---- the stash boundary --------------------------------------------------------------------------------------
# rasterize_forward(): with one tile the binning block needs bin_lds = (2 * 1 + 48 + 3 * 8 * 18) * 4 = 1928 B of LDS and
# the stash 8 + 8 N more; it is used while that fits 160 KiB (and no radii are asked for)
BIN_LDS = (2 * 1 + 48 + 3 * rc.QUEUES * 18) * 4
STASH_MAX_N = (160 * 1024 - BIN_LDS - 8) // 8


@functools.lru_cache(maxsize=None)
def boundary_case():
    lengths = [(300, 257, 256, 193, 129, 65, 64, 299, 1, 0, 2)[f % 11] for f in range(96)]
    scene = rc.ladder_scene("clustered", rc.SEED + 2, lengths=lengths, N=300)
    ids = torch.sort(torch.randperm(20233, generator=torch.Generator().manual_seed(5))[:300]).values
    return scene, ids


def spread_out(scene, ids, N, frames=None):
    """The scene's records stored at `ids` (ascending: id order, hence tie order, is kept) among N, the rest culled."""
    out = dict(scene)
    for k in ATTRS:
        src = scene[k] if frames is None else scene[k][frames]
        full = rc._culled(1)[k].to(src.device).expand(src.shape[0], N, -1).clone()
        full[:, ids.to(src.device)] = src
        out[k] = full
    for k in ("K", "E", "counts"):
        out[k] = scene[k] if frames is None else scene[k][frames]
    return out


@pytest.mark.parametrize("N", [20233, 20234, STASH_MAX_N, STASH_MAX_N + 1])
def test_stash_boundary(N):
    """The stash holds up to N = 20238 Gaussians per frame; one more and the binning records go through memory.  Both
    sides of that boundary (and 20233 / 20234, where a bin_lds of 1968 B would put it), with radii on (never a stash) and
    off, must give the same frames bit for bit; frames 0, 47 and 95 are compared with the oracle."""
    from audio_motion_avatar_amd import ops

    assert STASH_MAX_N == 20238 and BIN_LDS + 8 + 8 * STASH_MAX_N <= 160 * 1024 < BIN_LDS + 8 + 8 * (STASH_MAX_N + 1)
    scene, ids = boundary_case()
    dev_scene = {k: (v.to(DEV) if torch.is_tensor(v) and k != "counts" else v) for k, v in scene.items()}
    wide = spread_out(dev_scene, ids, N)
    rec = rc.raw(wide)
    assert rec.is_cuda and rec.shape == (96, N, 16)
    cam = camera(scene)
    ws = lambda: ops.RasterWorkspace(96, N, 16, 16, 96 * 512, DEV)
    off = product(wide, rec, cam=cam, workspace=ws())
    on = product(wide, rec, cam=cam, workspace=ws(), want_radii=True)
    assert torch.equal(off["rgba"], on["rgba"]), "radii on / off"
    assert torch.equal(product(wide, rec, cam=cam, workspace=ws())["rgba"], off["rgba"]), "second run"
    # the same Gaussians without the culled records between them
    assert torch.equal(product(scene)["rgba"], off["rgba"]), "N = 300 / N at the stash boundary"
    frames = [0, 47, 95]
    few = spread_out(scene, ids, N, frames)
    act = rc.oracle_activated(few)
    assert [r["instances"] for r in act] == [int(scene["counts"][f]) for f in frames]
    compare_small(f"product_stash_N{N}", rc.oracle_product(few), off, frames=frames)
    for f, r in zip(frames, act):
        assert np.array_equal(on["radii"][f].cpu().numpy(), r["radii"]), f"frame {f} radii"


# ---- the sorts under the previous tile -------------------------------------------------------------------------------
@pytest.mark.parametrize("depths", rc.DEPTHS)
def test_short_lists_sorted_under_the_previous_tile(depths):
    """sort_prefetched: rank_sort<1> (n <= 64), the 256-bucket form (spread) and its rank_sort<4> fallback (clustered,
    equal).  Every queue starts with more 300-Gaussian frames than it has waves, so all the frames of 1 .. 256 Gaussians
    behind them are second or later tiles of their waves (raster_cases.train_scene)."""
    per_cu = int(os.environ.get("AMAV_RENDER_WAVES", rc.WAVES_PER_CU))
    waves = torch.cuda.get_device_properties(0).multi_processor_count * per_cu // rc.QUEUES
    lead = max(rc.train_waves(256), waves) + 8
    scene = rc.train_scene(depths, lead)
    nlead, F = scene["lead"], scene["xyz"].shape[0]
    assert nlead // rc.QUEUES >= waves
    out = product(scene)
    rgba = out["rgba"]
    assert torch.equal(rgba[:nlead], rgba[nlead - 1:nlead].expand(nlead, -1, -1, -1)), "copies of one frame differ"
    tail = rc.take(scene, nlead - 1, F - nlead + 1)
    compare_small(f"product_train[{depths}]", rc.oracle_product(tail), out, frames=range(nlead - 1, F))
    # the same frames as the first tiles of their waves: the `!ready` sorts
    alone = product(tail)
    assert torch.equal(alone["rgba"], rgba[nlead - 1:]), "sorted under the previous tile / as a wave's first tile"
