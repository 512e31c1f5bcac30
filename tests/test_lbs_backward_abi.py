"""Host-side argument checks of the LBS and gather backwards' C entry points (no kernel is launched: every call below is
refused before it reaches the device), and the host-built transposed tables."""
import ctypes

import numpy as np
import pytest

from abi_support import ERR_INVALID, ERR_WORKSPACE, FAKE, lib  # noqa: F401 (lib: fixture)

V, J, NC, KW = 100, 4, 5, 2


def _tables():
    from audio_motion_avatar_amd import _lib

    t = _lib.BodyTables()
    t.num_verts, t.num_joints, t.num_coeffs, t.skin_k = V, J, NC, KW
    for name in ("v_template", "blend", "j_template", "j_dirs", "parents", "skin_idx", "skin_w"):
        setattr(t, name, FAKE)
    t.blend_split = None
    return t


def _parts(joints=(1, J - 1), coeffs=(3, NC - 3)):
    from audio_motion_avatar_amd import _lib

    pp = _lib.PoseParts()
    pp.num_pose_parts, pp.num_coeff_parts = len(joints), len(coeffs)
    for q, n in enumerate(joints):
        pp.pose[q], pp.pose_joints[q], pp.pose_stride[q] = FAKE, n, 3 * n
    for q, n in enumerate(coeffs):
        pp.coeff[q], pp.coeff_count[q], pp.coeff_stride[q] = FAKE, n, n
    return pp


def _args(lib, F=3, scratch_bytes=None, tables=None, parts=None):
    from audio_motion_avatar_amd import _lib

    a = _lib.LbsBackwardArgs()
    a.num_frames = F
    a._keep = (tables or _tables(), parts or _parts())
    a.tables, a.parts = ctypes.pointer(a._keep[0]), ctypes.pointer(a._keep[1])
    for name in ("grad_vertices", "grad_full_pose", "grad_coeffs", "skin_offsets", "skin_verts", "skin_weights",
                 "scratch"):
        setattr(a, name, FAKE)
    a.scratch_bytes = scratch_bytes if scratch_bytes is not None else lib.amav_lbs_backward_bytes(
        max(F, 1), ctypes.byref(a._keep[0]))
    return a


def test_symbols_are_exported_and_bound(lib):
    from audio_motion_avatar_amd import _lib

    for name in ("amav_lbs_backward", "amav_lbs_backward_bytes", "amav_points_gather_backward"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES


def test_scratch_size_query(lib):
    t = _tables()
    assert lib.amav_lbs_backward_bytes(0, ctypes.byref(t)) == 0
    assert lib.amav_lbs_backward_bytes(2, None) == 0
    small = lib.amav_lbs_backward_bytes(2, ctypes.byref(t))
    # at least the recomputed posed vertices [F,V,3] and the posed-vertex gradient [32-frame pad, 32-vertex pad, 3]
    assert small >= 4 * (2 * V * 3 + 32 * 128 * 3)
    assert lib.amav_lbs_backward_bytes(100, ctypes.byref(t)) > small
    bad = _tables()
    bad.num_joints = 65
    assert lib.amav_lbs_backward_bytes(2, ctypes.byref(bad)) == 0


def test_lbs_backward_refusals_return_error_codes_without_a_launch(lib):
    assert lib.amav_lbs_backward(None, None) == ERR_INVALID
    assert b"args is NULL" in lib.amav_last_error()
    for F in (0, -4):
        assert lib.amav_lbs_backward(ctypes.byref(_args(lib, F=F)), None) == ERR_INVALID
    for name in ("tables", "parts", "grad_vertices", "grad_full_pose", "grad_coeffs", "skin_offsets", "skin_verts",
                 "skin_weights", "scratch"):
        a = _args(lib)
        setattr(a, name, None)
        assert lib.amav_lbs_backward(ctypes.byref(a), None) == ERR_INVALID, name
    a = _args(lib, scratch_bytes=1024)
    assert lib.amav_lbs_backward(ctypes.byref(a), None) == ERR_WORKSPACE
    assert b"scratch" in lib.amav_last_error()
    a = _args(lib)
    a.scratch = FAKE + 4
    assert lib.amav_lbs_backward(ctypes.byref(a), None) == ERR_INVALID
    assert b"aligned" in lib.amav_last_error()
    # parts that do not add up to the tables' joints / coefficients, or a bad part
    too_many = _parts()
    too_many.num_pose_parts = 9
    for parts in (_parts(joints=(1, J)), _parts(coeffs=(NC - 1,)), too_many):
        a = _args(lib, parts=parts)
        assert lib.amav_lbs_backward(ctypes.byref(a), None) == ERR_INVALID
    pp = _parts()
    pp.pose_stride[1] = 2
    assert lib.amav_lbs_backward(ctypes.byref(_args(lib, parts=pp)), None) == ERR_INVALID
    assert b"stride" in lib.amav_last_error()
    bad = _tables()
    bad.skin_k = J + 1
    assert lib.amav_lbs_backward(ctypes.byref(_args(lib, tables=bad, scratch_bytes=1 << 30)), None) == ERR_INVALID


def test_gather_backward_refusals_return_error_codes_without_a_launch(lib):
    f = lib.amav_points_gather_backward
    for F, Vv, N in ((0, 10, 5), (2, 0, 5), (2, 10, 0), (-1, 10, 5)):
        assert f(F, Vv, N, FAKE, FAKE, FAKE, FAKE, None) == ERR_INVALID
    assert f(2, 10, 5, None, FAKE, FAKE, FAKE, None) == ERR_INVALID
    assert f(2, 10, 5, FAKE, FAKE, FAKE, None, None) == ERR_INVALID
    assert f(2, 10, 5, FAKE, None, FAKE, FAKE, None) == ERR_INVALID
    assert b"gather table" in lib.amav_last_error()
    assert f(2, 10, 5, FAKE, FAKE, None, FAKE, None) == ERR_INVALID
    assert f(2, 10, 5, FAKE, FAKE + 2, FAKE, FAKE, None) == ERR_INVALID
    assert b"aligned" in lib.amav_last_error()


def test_gather_table_transpose():
    import torch

    from audio_motion_avatar_amd import ops
    from audio_motion_avatar_amd._lib import AmavError

    idx = torch.tensor([[3, 3, 3, 3], [0, 3, 1, 1], [4, 0, 4, 0]], dtype=torch.int32)
    off, ent = ops.points_gather_csr(idx, 6)
    assert off.tolist() == [0, 3, 5, 5, 10, 12, 12]  # vertices 2 and 5: no entries
    assert ent.tolist() == [1, 2, 2, 1, 1, 0, 0, 0, 0, 1, 2, 2]  # ascending point ids, once per slot
    with pytest.raises(AmavError, match="outside"):
        ops.points_gather_csr(torch.tensor([[0, 1, 2, 6]], dtype=torch.int32), 6)
    with pytest.raises(AmavError, match="outside"):
        ops.points_gather_csr(torch.tensor([[0, -1, 2, 3]], dtype=torch.int32), 6)


def test_skin_table_transpose():
    from audio_motion_avatar_amd.body_model import build_skin_transpose

    skin_idx = np.array([[0, 2], [1, 0], [2, 0], [0, 1]], np.int32)
    skin_w = np.array([[0.5, 0.5], [1.0, 0.0], [0.25, 0.75], [0.9, 0.1]], np.float32)
    off, verts, w = build_skin_transpose(skin_idx, skin_w, 4)
    assert off.tolist() == [0, 3, 5, 7, 7]  # joint 3: no vertices; the zero padding weight is left out
    assert verts.tolist() == [0, 2, 3, 1, 3, 0, 2]
    assert np.array_equal(w, np.array([0.5, 0.75, 0.9, 1.0, 0.1, 0.5, 0.25], np.float32))
