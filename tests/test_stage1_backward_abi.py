"""Host-side argument checks of the stage-1 backwards' C entry points (amav_cell_max_backward, amav_cell_mean_backward,
amav_points_project_backward): every call below is refused before a kernel is launched."""

from abi_support import FAKE, lib  # noqa: F401 (lib: fixture)


B, N, C, CELLS, H, W = 2, 300, 48, 64, 40, 56


def test_symbols_exist(lib):
    for name in ("amav_cell_max_backward", "amav_cell_max_backward_workspace_bytes", "amav_cell_mean_backward",
                 "amav_points_project_backward"):
        assert hasattr(lib, name), name


def test_workspace_bytes(lib):
    f = lib.amav_cell_max_backward_workspace_bytes
    for bad in ((0, C, CELLS), (B, 0, CELLS), (B, C, 0), (-1, C, CELLS)):
        assert f(*bad) == 0, bad
    assert f(B, C, CELLS) >= B * 3 * CELLS * C * 8  # an int32 arg and an fp32 sum per (plane, cell, channel)


def _max(lib, **over):
    a = dict(B=B, N=N, C=C, cells=CELLS, feat=FAKE, order=FAKE, seg=FAKE, cell_of=FAKE, dout=FAKE, dfeat=FAKE, ws=FAKE,
             ws_bytes=1 << 40)
    a.update(over)
    return lib.amav_cell_max_backward(a["B"], a["N"], a["C"], a["cells"], a["feat"], a["order"], a["seg"], a["cell_of"],
                                      a["dout"], a["dfeat"], a["ws"], a["ws_bytes"], None)


def test_cell_max_backward_refusals(lib):
    for name in ("B", "N", "C", "cells"):
        for bad in (0, -1):
            assert _max(lib, **{name: bad}) == -1 and b"bad sizes" in lib.amav_last_error(), (name, bad)
    assert _max(lib, B=70000) == -1 and b"bad sizes" in lib.amav_last_error()
    for name in ("feat", "order", "seg", "cell_of", "dout", "dfeat"):
        assert _max(lib, **{name: None}) == -1 and b"NULL" in lib.amav_last_error(), name
    need = lib.amav_cell_max_backward_workspace_bytes(B, C, CELLS)
    assert _max(lib, ws_bytes=need - 1) == -3 and b"workspace" in lib.amav_last_error()
    assert _max(lib, ws=None) == -3 and b"workspace" in lib.amav_last_error()


def test_cell_mean_backward_refusals(lib):
    def call(**over):
        a = dict(B=B, N=N, C=C, cells=CELLS, order=FAKE, seg=FAKE, dplanes=FAKE, dfeat=FAKE)
        a.update(over)
        return lib.amav_cell_mean_backward(a["B"], a["N"], a["C"], a["cells"], a["order"], a["seg"], a["dplanes"],
                                           a["dfeat"], None)

    for name in ("B", "N", "C", "cells"):
        for bad in (0, -1):
            assert call(**{name: bad}) == -1 and b"bad sizes" in lib.amav_last_error(), (name, bad)
    assert call(B=70000) == -1 and b"bad sizes" in lib.amav_last_error()
    for name in ("order", "seg", "dplanes", "dfeat"):
        assert call(**{name: None}) == -1 and b"NULL" in lib.amav_last_error(), name


def test_points_project_backward_refusals(lib):
    def call(**over):
        a = dict(B=B, N=N, C=C, H=H, W=W, dout=FAKE, ws=FAKE, ws_bytes=1 << 40, dfeat=FAKE)
        a.update(over)
        return lib.amav_points_project_backward(a["B"], a["N"], a["C"], a["H"], a["W"], a["dout"], a["ws"],
                                                a["ws_bytes"], a["dfeat"], None)

    for name in ("B", "N", "C", "H", "W"):
        for bad in (0, -1):
            assert call(**{name: bad}) == -1 and b"bad sizes" in lib.amav_last_error(), (name, bad)
    assert call(B=70000) == -1 and b"bad sizes" in lib.amav_last_error()
    assert call(H=50000, W=50000) == -1 and b"too large" in lib.amav_last_error()
    for name in ("dout", "dfeat"):
        assert call(**{name: None}) == -1 and b"NULL" in lib.amav_last_error(), name
    # the backward reads the forward's z-buffer: a workspace smaller than the forward's is refused
    need = lib.amav_points_project_workspace_bytes(B, N, H, W)
    assert call(ws_bytes=need - 1) == -3 and b"workspace" in lib.amav_last_error()
    assert call(ws=None) == -3 and b"workspace" in lib.amav_last_error()
