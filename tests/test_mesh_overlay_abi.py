"""Host-side contract of the mesh overlay (include/amav.h, amav_mesh_overlay): every call below is refused before a launch.
int64 faces are converted to int32 by ops.mesh_overlay; that needs a device, so test_mesh_overlay_gpu.py runs them."""
import ctypes

import pytest
import torch

from abi_support import ERR_INVALID, ERR_WORKSPACE, FAKE, lib  # noqa: F401 (lib: fixture)


def good_args(lib, F=2, V=10, T=12, H=50, W=70):
    from audio_motion_avatar_amd import _lib

    a = _lib.STRUCTS["amav_mesh_overlay_args"]()
    a.num_frames, a.num_verts, a.num_faces, a.height, a.width = F, V, T, H, W
    a.frame_channels, a.cull_backfaces, a.small_box = 3, 1, -1
    for name in ("vertices", "faces", "K", "E", "frames", "out_rgb", "workspace"):
        setattr(a, name, FAKE)
    a.znear = 0.05
    a.workspace_bytes = lib.amav_mesh_overlay_workspace_bytes(F, V, T, H, W)
    return a


def test_workspace_bytes(lib):
    q = lib.amav_mesh_overlay_workspace_bytes
    for bad in ((0, 10, 12, 50, 70), (2, 0, 12, 50, 70), (2, 10, 0, 50, 70), (2, 10, 12, 0, 70), (2, 10, 12, 50, 0),
                (-1, 10, 12, 50, 70), (2, 10, 12, 50, -70), (2, 10, 12, 16385, 70), (65536, 10, 12, 50, 70)):
        assert q(*bad) == 0, bad
    assert q(2, 10, 12, 50, 70) >= 8 * 2 * 50 * 70
    # keys + camera z and snapped coordinates + shade and list + counters, each slab rounded up to 256 bytes
    F, V, T, H, W = 48, 10475, 20908, 512, 512
    exact = 8 * F * H * W + 12 * F * V + 16 * F * T + 12 * F
    assert exact <= q(F, V, T, H, W) <= exact + 6 * 256


def test_refusals_name_their_reason(lib):
    call = lambda a: lib.amav_mesh_overlay(ctypes.byref(a), None)
    assert lib.amav_mesh_overlay(None, None) == ERR_INVALID and b"args is NULL" in lib.amav_last_error()
    a = good_args(lib)
    a.workspace_bytes -= 1
    assert call(a) == ERR_WORKSPACE and b"workspace" in lib.amav_last_error()
    for field in ("num_frames", "num_verts", "num_faces", "height", "width"):
        for value in (0, -3):
            a = good_args(lib)
            setattr(a, field, value)
            assert call(a) == ERR_INVALID and b"bad sizes" in lib.amav_last_error(), field
    for field in ("vertices", "faces", "K", "E", "out_rgb", "workspace"):
        a = good_args(lib)
        setattr(a, field, None)
        assert call(a) == ERR_INVALID and b"NULL pointer" in lib.amav_last_error(), field
    for field, value in (("vertices", FAKE + 2), ("out_face_index", FAKE + 1), ("transl", FAKE + 3), ("workspace", FAKE + 8)):
        a = good_args(lib)
        setattr(a, field, value)
        assert call(a) == ERR_INVALID and b"misaligned" in lib.amav_last_error(), field
    a = good_args(lib)
    a.frame_channels = 5
    assert call(a) == ERR_INVALID and b"frame_channels" in lib.amav_last_error()
    a = good_args(lib)
    a.znear = 0.0
    assert call(a) == ERR_INVALID and b"znear" in lib.amav_last_error()


def test_the_op_refuses_cpu_tensors_and_the_module_other_materials():
    from audio_motion_avatar_amd import AmavError, mesh_overlay, ops

    v, f = torch.zeros(1, 4, 3), torch.zeros(2, 3, dtype=torch.int32)
    K, E = torch.eye(3)[None], torch.eye(4)[None]
    with pytest.raises(AmavError, match="only runs on an MI355X"):
        ops.mesh_overlay(v, f, K, E, 8, 8)
    r = mesh_overlay.SimpleMeshRenderer(f.numpy(), 8, 8)
    for kwargs in ({"metallic": 0.5}, {"roughness": 0.4}, {"emissive": (1, 0, 0)}):
        with pytest.raises(NotImplementedError):
            r.render_mesh(v[0], torch.zeros(8, 8, 3), K[0], E[0], **kwargs)
