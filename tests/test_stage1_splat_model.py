"""The CPU restatements of tests/stage1_splat_cases.py against the oracle, wherever the oracle is defined, the
preconditions of every case builder, and the projection rule on hand-built points whose pixels are written out here.
tests/test_stage1_splat_gpu.py holds the kernels of csrc/splat.hip to these restatements."""
import pytest
import torch

import stage1_splat_cases as sc
from oracle import triplane_net as o_tn


def bitwise(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("key", sc.CELL_CASES, ids=sc.cells_id)
def test_cell_restatements_agree_with_the_oracle(key):
    case = sc.cells_case(*key)                                         # building the case checks its preconditions
    feat, cell_of, cells, R = case["feat"], case["cell_of"], case["cells"], case["R"]
    index = {k: cell_of[:, p].long()[:, None, :] for p, k in enumerate(sc.PLANES)}
    assert bitwise(sc.pool_local_fp32(feat, cell_of, cells), o_tn.pool_local(index, feat, R))
    for p, k in enumerate(sc.PLANES):
        seq = sc.cell_mean_seq_fp32(feat, cell_of[:, p], cells)
        where, mean64, abs_sum, count = sc.cell_mean_fp64(feat, cell_of[:, p], cells)
        bound = sc.cell_mean_bound(abs_sum, count[where[:, 0], where[:, 1]])
        assert int(count.sum()) == feat.shape[0] * feat.shape[1] and len(where) == int((count > 0).sum())
        assert bool(((sc.at_cells(seq, where).double() - mean64).abs() <= bound).all())
        scatter = o_tn.scatter_mean(feat.permute(0, 2, 1), index[k], cells)
        assert bool(((sc.at_cells(scatter, where).double() - mean64).abs() <= bound).all())
        for planes in (seq, scatter):
            assert bool((planes.permute(0, 2, 1)[count == 0] == 0).all())


def test_the_sequential_mean_is_sequential():
    """1 + 2**-24 + 2**-24 in that order stays 1 in fp32 (each half-ulp addend rounds to even); any other order gives
    1 + 2**-23"""
    feat = torch.tensor([[[1.0], [2.0 ** -24], [5.0], [2.0 ** -24]]])
    cell_of = torch.tensor([[0, 0, 1, 0]])
    got = sc.cell_mean_seq_fp32(feat, cell_of, 3)
    assert got[0, 0].tolist() == [float(torch.tensor(1.0) / 3), 5.0, 0.0]
    other = sc.cell_mean_seq_fp32(feat.flip(1), cell_of.flip(1), 3)
    assert other[0, 0, 0] == (torch.tensor(1.0) + 2.0 ** -23) / 3


def _oracle_equals_restatement(scene, C=3):
    feat = sc.scene_features(scene, C)
    want = o_tn.points_projection(scene["points"], scene["w2c"], scene["K"], feat, scene["radius_px"])
    pixel_of = sc.project_fp32(scene["points"], scene["w2c"], scene["K"], scene["H"], scene["W"], scene["radius_px"])
    if "pixel_of" in scene:
        assert torch.equal(pixel_of, scene["pixel_of"])
    assert bitwise(sc.expected_features(feat, pixel_of), want)
    return pixel_of


@pytest.mark.parametrize("shape", sc.PROJECT_SCENES, ids=lambda s: "N{}-{}x{}-r{}".format(*s))
def test_project_restatement_equals_the_oracle_on_the_random_scenes(shape):
    _oracle_equals_restatement(sc.project_scene(*shape))


def test_project_restatement_equals_the_oracle_on_ties_and_near_the_camera_plane():
    _oracle_equals_restatement(sc.ties_scene())
    near = sc.near_plane_scene()
    _oracle_equals_restatement(near)
    _oracle_equals_restatement(near["base"])
    # u or v = +-inf is outside the oracle (it converts them to int); the restatement's rule there: no pixel
    over = sc.near_plane_scene(overflow=True)
    n = near["points"].shape[1]
    assert torch.equal(over["pixel_of"][:, :n], near["pixel_of"]) and bool((over["pixel_of"][:, n:] == -1).all())


# (y, x) of the pixel whose features each point of stage1_splat_cases.lattice_scene() receives, None: zeros
LATTICE_WANT = [(6, 8),      # 0: (u, v) = (8, 4.5), r = 2.5; (6, 9) is at distance^2 6.25 exactly: strict <
                None,        # 1: the same place at Z = 4, hidden
                (12, 20),    # 2: the lower id of two identical points
                None,        # 3: the higher id
                (1, 1),      # 4: (0, 0), the disc cut by the top-left corner
                (15, 23),    # 5: (24, 16), the bottom-right corner
                None,        # 6: (-5, -5), off screen
                (9, 13),     # 7: on the axis at Z = 1e-30, nearest of all
                None,        # 8: on the axis at Z = 2, hidden by 7
                None, None,  # 9, 10: |u| ~ 6e30
                (9, 0),      # 11: (-1, 8), cut by the left border
                (5, 23),     # 12: (25, 4), right
                (0, 17),     # 13: (16, -1), top
                (15, 5)]     # 14: (4, 17), bottom


def test_hand_built_lattice_points_take_the_pixels_written_here():
    scene = sc.lattice_scene()
    pixel_of = _oracle_equals_restatement(scene, C=2)
    want = [-1 if p is None else p[0] * sc.LATTICE_W + p[1] for p in LATTICE_WANT]
    assert pixel_of[0].tolist() == want
    # and straight from the oracle, not through the restatement
    feat = sc.scene_features(scene, 2)
    out = o_tn.points_projection(scene["points"], scene["w2c"], scene["K"], feat, scene["radius_px"])
    for n, p in enumerate(LATTICE_WANT):
        assert torch.equal(out[0, n], torch.zeros(2) if p is None else feat[0, :, p[0], p[1]]), n
    # the strict <: pixel (6, 9) is at distance^2 6.25 exactly of point 0 and nobody's
    ids = sc.rasterise_fp32(scene["points"], scene["w2c"], scene["K"], scene["H"], scene["W"], scene["radius_px"])[0]
    assert ids[0, 6, 8] == 0 and ids[0, 6, 9] == -1
