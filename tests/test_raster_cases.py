"""The scenes of raster_cases.py reach what they are built for, checked with the CPU oracle alone: these conditions,
not a GPU run, decided the scene parameters (footprint, opacity, seed), which are frozen.

Per scene and seed the GPU tests use:
    * the oracle's instance count of every frame is the intended list length (one tile: the list of that tile);
    * fewer than 0.5 % of the launch's pixels are flagged `unstable` (pooled; single 16 x 16 frames reach 1.2 %);
    * the blend reaches the back of the list: on at least half of a frame's covered pixels the oracle's alpha stays
      below 1 - 1e-4 (frames of 65 Gaussians and more), else the blend stops before the order matters;
    * the order matters: storing the equal-depth Gaussians in reverse id order changes at least 5 % of the covered
      pixels of a frame by more than TOL (clustered and equal scenes), so a wrong tie order would be seen.
"""
import numpy as np
import pytest
import torch

import raster_cases as rc
from raster_parity import FLAG_CAP, TOL


def _flag_share(ref):
    return sum(int((r["unstable"] != 0).sum()) for r in ref) / sum(r["unstable"].size for r in ref)


def _reach(r):
    covered = r["alpha"] > 0
    return float((r["alpha"][covered] < 1 - 1e-4).mean())


@pytest.mark.parametrize("depths", rc.DEPTHS)
def test_ladder_reaches_every_length_class(depths):
    scene, act, prod = rc.ladder_case(depths)
    lengths = rc.ladder_lengths()
    assert scene["xyz"].shape == (rc.LADDER_F, rc.LADDER_N, 3) and (scene["H"], scene["W"]) == (16, 16)
    assert lengths[:26] == list(rc.LADDER) and all(lengths.count(n) >= 3 for n in rc.LADDER)
    assert [r["instances"] for r in act] == lengths
    assert scene["counts"].flatten().tolist() == lengths
    assert (scene["E"] == torch.eye(4)).all()
    print(f"ladder {depths}: flagged share {_flag_share(act):.4%}")
    assert _flag_share(act) < FLAG_CAP
    for f, r in enumerate(act):
        if lengths[f] >= 65:
            assert _reach(r) >= 0.5, f"frame {f} (n = {lengths[f]}): the blend saturates before the back of the list"


@pytest.mark.parametrize("F,start", rc.LADDER_SUBSETS)
@pytest.mark.parametrize("depths", rc.DEPTHS)
def test_ladder_subsets_hold_the_long_lists(depths, F, start):
    """The launches of 1, 6 and 95 frames: the lists above 2048 are inside, and the product reference of the launch
    stays under the flagged-pixel cap."""
    _, act, prod = rc.ladder_case(depths)
    assert max(r["instances"] for r in rc.pick(act, start, F)) == 2600
    assert F < 6 or {513, 1000, 2047, 2048, 2049} <= {r["instances"] for r in rc.pick(act, start, F)}
    assert _flag_share(rc.pick(prod, start, F)) < FLAG_CAP


@pytest.mark.parametrize("depths", rc.DEPTHS)
def test_ladder_depth_patterns(depths):
    """What decides the sort's branch: the depth words of a frame's live Gaussians."""
    scene, _, _ = rc.ladder_case(depths)
    for f, n in enumerate(rc.ladder_lengths()):
        z = scene["xyz"][f, :, 2]
        live = z[z > 0]
        assert len(live) == n and (z[z <= 0] == -1).all()
        if n == 0:
            continue
        top = int(torch.unique(live, return_counts=True)[1].max())
        if depths == "equal":
            assert top == n and float(live[0]) == rc.Z_TIE
        elif depths == "clustered":
            assert top >= 0.7 * n
            # equal bit patterns share a bucket whatever the scale: the wave sorts' limit is 16 keys, sort_big's 32
            assert top > 16 or n < 24
            assert top > 32 or n < 46
        else:
            # one binade: the key's depth word is linear in z, and neighbours of a linspace are (3.0 - 2.2) / (n - 1)
            # apart, so a bucket of width range / (B - 1) holds at most ceil(n / (B - 1)) + 1 keys
            assert top == 1 and live.min() >= 2.0 and live.max() < 4.0
            for buckets, limit in ((256, 16), (512, 16), (2048, 32)):  # a form of B buckets sorts up to B keys
                if n <= buckets:
                    assert -(-n // (buckets - 1)) + 1 <= limit


@pytest.mark.parametrize("depths", ["clustered", "equal"])
def test_ladder_order_of_ties_is_visible(depths):
    scene, act, _ = rc.ladder_case(depths)
    flipped = rc.oracle_activated(rc.reverse_ties(scene))
    lengths = rc.ladder_lengths()
    for f in range(len(rc.LADDER)):  # one cycle: the later frames repeat the classes
        if lengths[f] < 63:
            continue
        covered = act[f]["alpha"] > 0
        moved = (np.abs(flipped[f]["color"] - act[f]["color"]).max(axis=0) > TOL)[covered].mean()
        assert moved >= 0.05, f"frame {f} (n = {lengths[f]}): reversed ties move {moved:.1%} of the covered pixels"
        assert flipped[f]["instances"] == act[f]["instances"]


@pytest.mark.parametrize("depths", rc.DEPTHS)
def test_product_reference_is_the_activated_oracle_clamped(depths):
    """render_batch on the raw records and the oracle on activated() are the same frames: raw() and activated() are
    two forms of one scene, so the product launch and the anchored configuration are compared with the same images.
    (To 1e-6, not bit for bit: torch's exp rounds an element differently in a vector lane and in the scalar tail, and
    render_batch activates frame by frame, activated() the whole scene at once.)"""
    scene, act, prod = rc.ladder_case(depths)
    for a, p in zip(act, prod):
        assert np.abs(np.clip(a["color"], 0, 1) - p["color"]).max() <= 1e-6
        assert np.abs(a["alpha"] - p["alpha"]).max() <= 1e-6
    assert rc.raw(scene).shape == (rc.LADDER_F, rc.LADDER_N, 16)


def test_raw_records_have_the_renderers_layout():
    """raw() packs what Renderer.unpack_gaussians views (xyz | opacity | rot | scale | color)."""
    from oracle import rasterizer as orc

    scene = rc.ladder_scene("spread", F=2, lengths=[5, 70], N=80)
    rec = rc.raw(scene)
    layout = {"xyz": (0, 3), "opacity": (3, 4), "rot": (4, 8), "scale": (8, 11), "color": (12, 15)}
    for k, (a, b) in layout.items():
        assert torch.equal(rec[..., a:b], scene[k])
    assert (rec[..., 11] == 0).all() and (rec[..., 15] == 0).all()
    assert rc.SCALE_BIAS == orc.SCALE_BIAS and orc.OPACITY_BIAS == 0.0
    act = rc.activated(scene)
    assert float(act["scale"].max()) < 0.1, "a footprint hit the activation's scale cap"
    assert float(scene["color"].min()) < 0 and float(scene["color"].max()) > 1, "the colour clamp is not exercised"


def test_mixed_scene_lists():
    scene, act, _ = rc.mixed_case()
    assert scene["xyz"].shape == (97, 1500, 3) and (scene["H"], scene["W"]) == (32, 48)
    assert torch.equal(rc.tile_lists(scene), scene["counts"])  # every Gaussian enters the one tile it was built for
    assert [r["instances"] for r in act] == scene["counts"].sum(1).tolist()
    assert _flag_share(act) < FLAG_CAP
    classes = set(scene["counts"].flatten().tolist())
    assert classes >= set(rc.MIXED_LENGTHS)
    # short, bucket-sorted, wave-bitonic and block-sorted lists inside single frames
    per_frame = [(row.min().item(), row.max().item()) for row in scene["counts"]]
    assert sum(lo <= 64 and hi > 512 for lo, hi in per_frame) >= 20


@pytest.mark.parametrize("depths", rc.DEPTHS)
def test_train_scene_puts_the_short_lists_behind_the_waves(depths):
    """A small train (lead 3): the leading frames are one frame repeated, and behind them every queue (frame % 8) meets
    every length sort_prefetched takes at least twice, all in lower (later) buckets than the leading frames."""
    lead = 3
    scene = rc.train_scene(depths, lead)
    lengths = rc.train_lengths(lead)
    nlead = scene["lead"]
    assert nlead == 8 * lead and scene["xyz"].shape[0] == len(lengths) == nlead + 208
    assert all(torch.equal(scene["xyz"][f], scene["xyz"][0]) for f in range(nlead))
    ref = rc.oracle_activated(rc.take(scene, nlead - 1, 209))
    assert [r["instances"] for r in ref] == lengths[nlead - 1:]
    assert _flag_share(ref) < FLAG_CAP
    for q in range(rc.QUEUES):
        mine = [n for f, n in enumerate(lengths) if f >= nlead and f % rc.QUEUES == q]
        assert all(mine.count(n) == 2 for n in rc.PREP_LADDER)
    assert max(rc.PREP_LADDER) <= 256 < rc.TRAIN_FILL <= 512
    assert rc.train_waves(256) == 512
