"""Host-side argument checks of amav_points_project_grid and amav_points_project_grid_backward: both are exported and
declared in include/amav.h, and every call below is refused before a kernel is launched."""

from abi_support import FAKE, HEADER, lib  # noqa: F401 (lib: fixture)

B, N, H, W, GH, GW, CG = 2, 300, 40, 56, 4, 5, 125
NAMES = ("amav_points_project_grid", "amav_points_project_grid_backward")


def test_symbols_are_exported_and_declared(lib):
    from audio_motion_avatar_amd import _lib

    with open(HEADER) as f:
        header = f.read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name + "(" in header and name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["amav_points_project_grid"][1]) == 17
    assert len(_lib.SIGNATURES["amav_points_project_grid_backward"][1]) == 13


def _forward(lib, **over):
    a = dict(B=B, N=N, H=H, W=W, Gh=GH, Gw=GW, Cg=CG, points=FAKE, w2c=FAKE, K=FAKE, rgb=FAKE, grid=FAKE, radius=2.5,
             out=FAKE, ws=FAKE, ws_bytes=1 << 40)
    a.update(over)
    return lib.amav_points_project_grid(a["B"], a["N"], a["H"], a["W"], a["Gh"], a["Gw"], a["Cg"], a["points"], a["w2c"],
                                        a["K"], a["rgb"], a["grid"], a["radius"], a["out"], a["ws"], a["ws_bytes"], None)


def _backward(lib, **over):
    a = dict(B=B, N=N, H=H, W=W, Gh=GH, Gw=GW, Cg=CG, dout=FAKE, ws=FAKE, ws_bytes=1 << 40, dgrid=FAKE, drgb=FAKE)
    a.update(over)
    return lib.amav_points_project_grid_backward(a["B"], a["N"], a["H"], a["W"], a["Gh"], a["Gw"], a["Cg"], a["dout"],
                                                 a["ws"], a["ws_bytes"], a["dgrid"], a["drgb"], None)


def test_forward_refusals(lib):
    for name in ("B", "N", "H", "W", "Gh", "Gw", "Cg"):
        for bad in (0, -1):
            assert _forward(lib, **{name: bad}) == -1 and b"bad sizes" in lib.amav_last_error(), (name, bad)
    assert _forward(lib, B=65536) == -1 and b"bad sizes" in lib.amav_last_error()
    for bad in (0.0, -1.0):
        assert _forward(lib, radius=bad) == -1 and b"bad sizes" in lib.amav_last_error()
    assert _forward(lib, H=1 << 16, W=1 << 15) == -1 and b"too large" in lib.amav_last_error()   # H * W = 2^31
    assert _forward(lib, H=50000, W=50000) == -1 and b"too large" in lib.amav_last_error()
    assert _forward(lib, Gh=1 << 16, Gw=1 << 15) == -1 and b"too large" in lib.amav_last_error()
    for name in ("points", "w2c", "K", "rgb", "grid", "out", "ws"):
        assert _forward(lib, **{name: None}) == -1 and b"NULL" in lib.amav_last_error(), name
    need = lib.amav_points_project_workspace_bytes(B, N, H, W)
    assert need >= B * (8 * H * W + 4 * N)
    assert _forward(lib, ws_bytes=need - 1) == -3 and b"workspace" in lib.amav_last_error()
    assert _forward(lib, ws_bytes=0) == -3 and b"workspace" in lib.amav_last_error()


def test_backward_refusals(lib):
    for name in ("B", "N", "H", "W", "Gh", "Gw", "Cg"):
        for bad in (0, -1):
            assert _backward(lib, **{name: bad}) == -1 and b"bad sizes" in lib.amav_last_error(), (name, bad)
    assert _backward(lib, B=65536) == -1 and b"bad sizes" in lib.amav_last_error()
    assert _backward(lib, H=1 << 16, W=1 << 15) == -1 and b"too large" in lib.amav_last_error()
    assert _backward(lib, H=50000, W=50000) == -1 and b"too large" in lib.amav_last_error()
    assert _backward(lib, Gh=1 << 16, Gw=1 << 15) == -1 and b"too large" in lib.amav_last_error()
    for name in ("dout", "dgrid"):
        assert _backward(lib, **{name: None}) == -1 and b"NULL" in lib.amav_last_error(), name
    # the backward reads the forward's z-buffer: a workspace smaller than the forward's is refused, NULL too
    need = lib.amav_points_project_workspace_bytes(B, N, H, W)
    assert _backward(lib, ws_bytes=need - 1) == -3 and b"workspace" in lib.amav_last_error()
    assert _backward(lib, ws=None) == -3 and b"workspace" in lib.amav_last_error()
    # (grad_rgb = NULL is not an error: it means "not wanted"; tests/test_project_grid_gpu.py runs it)
