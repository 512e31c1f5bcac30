"""The CPU restatements of tests/project_grid_cases.py (what tests/test_project_grid_gpu.py holds the kernels to): the
fp32 restatements lie within the derived bounds of the fp64 models, the forward agrees with the oracle's
image_feature + points_projection, and every case still has the edges it was chosen for.  No HIP library is loaded."""
import numpy as np
import pytest
import torch

import project_grid_cases as pc
import stage1_splat_cases as sc
from oracle import triplane_net as o_tn


@pytest.mark.parametrize("key", pc.CASES, ids=pc.case_id)
def test_fp32_restatements_lie_within_the_bounds_of_the_fp64_models(key):
    c = pc.case(key)
    got = pc.forward_fp32(c["rgb"], c["grid"], c["pixel_of"])
    want, bound = pc.forward_fp64(c["rgb"], c["grid"], c["pixel_of"])
    err = (got.double() - want).abs()
    print(f"{pc.case_id(key)} forward: worst error / bound {float((err / bound.clamp_min(1e-300))[..., 3:].max()):.3f}")
    assert bool((err <= bound).all())
    assert bool((got[c["pixel_of"] < 0] == 0).all()) and torch.equal(got[..., :3].double(), want[..., :3])

    grad, grad_rgb, reached = pc.backward_fp32(c["dout"], c["ids"], c["Gh"], c["Gw"])
    want, bound = pc.backward_fp64(c["dout"], c["ids"], c["Gh"], c["Gw"])
    err = (grad.double() - want).abs()
    print(f"{pc.case_id(key)} backward: worst error / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all())
    assert bool((grad[~reached] == 0).all()) and bool((want[~reached] == 0).all())
    ids = torch.from_numpy(c["ids"])
    assert bool((grad_rgb.permute(0, 2, 3, 1)[ids < 0] == 0).all())
    assert bool((grad_rgb.permute(0, 2, 3, 1)[ids >= 0] != 0).any())


def test_identity_scale_returns_the_node_itself():
    c = pc.case((pc.RANDOM, (50, 70), 125))
    got = pc.forward_fp32(c["rgb"], c["grid"], c["pixel_of"])
    B, H, W = c["ids"].shape
    nodes = c["grid"].permute(0, 3, 1, 2).contiguous()                              # [B,Cg,H,W]: one node per pixel
    assert torch.equal(got[..., 3:].contiguous(), sc.expected_features(nodes, c["pixel_of"]))


# the oracle's image_feature reads a square token grid: (scene, side, Cg)
ORACLE_CASES = ((pc.RANDOM, 4, 5), (pc.RANDOM, 1, 3), (pc.LONG, 8, 5), ("lattice", 4, 5), (pc.ONE, 2, 2))


@pytest.mark.parametrize("scene_key,side,Cg", ORACLE_CASES, ids=lambda v: str(v))
def test_forward_restatement_agrees_with_the_oracle(scene_key, side, Cg):
    """oracle.image_feature (an identity feature_reducer over tokens that are the grid's nodes, F.interpolate, cat RGB)
    followed by oracle.points_projection.  torch's CPU interpolate is not bit-equal to the restatement in general (it
    resizes one axis after the other with weights of its own); its arithmetic has the same operations on the same
    magnitudes, so it obeys the same bound against fp64 and the two fp32 results may differ by twice the bound."""
    scene = pc._scene(scene_key)
    H, W = scene["H"], scene["W"]
    B = scene["points"].shape[0]
    g = torch.Generator().manual_seed(side + Cg)
    rgb = torch.rand(B, 3, H, W, generator=g)
    grid = torch.randn(B, side, side, Cg, generator=g)
    p = {"feature_reducer.weight": torch.eye(Cg), "feature_reducer.bias": torch.zeros(Cg)}
    dense = o_tn.image_feature(p, "", rgb[:, None], grid.reshape(B, 1, side * side, Cg)).reshape(B, 3 + Cg, H, W)
    want = o_tn.points_projection(scene["points"], scene["w2c"], scene["K"], dense, scene["radius_px"])
    pixel_of = sc.project_fp32(scene["points"], scene["w2c"], scene["K"], H, W, scene["radius_px"])
    got = pc.forward_fp32(rgb, grid, pixel_of)
    bound = pc.forward_fp64(rgb, grid, pixel_of)[1]
    assert torch.equal((got != 0).any(-1), (want != 0).any(-1)) and torch.equal((got != 0).any(-1), pixel_of >= 0)
    assert torch.equal(got[..., :3], want[..., :3])
    err = (got - want).double().abs()
    print(f"{scene_key} side {side}: bit-equal {torch.equal(got, want)}, worst difference / (2 bound) "
          f"{float((err / (2 * bound).clamp_min(1e-300))[..., 3:].max()):.3f}")
    assert bool((err <= 2 * bound).all())


@pytest.mark.parametrize("key", pc.CASES, ids=pc.case_id)
def test_cases_still_have_their_edges(key):
    c = pc.case(key)
    missing = pc.EDGES[key[:2]] - c["edges"]
    assert not missing, missing
    assert bool((c["pixel_of"] >= 0).any())                                          # hit points in every case


def test_the_cases_cover_every_edge_between_them():
    have = set().union(*(pc.EDGES[key[:2]] for key in pc.CASES))
    assert have == {"missed points", "won but not claimed", "nodes out of reach"} | pc.ALL_BORDERS
    # a node that receives both equal-node corners of one pixel, as two terms: count them in one case
    c = pc.case(("lattice", (4, 5), 125))
    ay, ax = pc.axis_fp32(c["ids"].shape[1], 4), pc.axis_fp32(c["ids"].shape[2], 5)
    _, ys, xs = np.nonzero(c["ids"] >= 0)
    both = (ay[0][ys] == ay[1][ys]) & (ay[2][ys] > 0) & (ay[3][ys] > 0)
    assert both.any() and (ay[0][ys[both]] == 3).all()
    assert ((ax[0][xs] == ax[1][xs]) & (ax[2][xs] > 0)).any()
