"""Host-side argument checks of the window cutting entry points (csrc/tile_windows.hip).  No kernel is launched: every
call below is refused, or has nothing to do, before it reaches the device."""
import ctypes
import re

from abi_support import ERR_INVALID, FAKE, HEADER, lib  # noqa: F401 (lib: fixture)


def _cut(lib, F=2, C=3, h=9, w=13, x=FAKE, K=4, size=10, frame=FAKE, oy=FAKE, ox=FAKE, out=FAKE):
    return lib.amav_windows_cut(F, C, h, w, x, K, size, frame, oy, ox, out, None)


def _transpose(lib, F=2, C=3, h=9, w=13, K=4, size=10, gw=FAKE, step=4, off_y=-3, off_x=-3, A=3, B=4, table=FAKE, gx=FAKE):
    return lib.amav_windows_cut_backward(F, C, h, w, K, size, gw, step, off_y, off_x, A, B, table, gx, None)


def _refused(lib, rc, entry, word):
    assert rc == ERR_INVALID
    msg = lib.amav_last_error()
    assert entry in msg and word in msg, msg


def test_symbols_header_and_bindings_agree(lib):
    from audio_motion_avatar_amd import _lib, ops

    text = open(HEADER).read()
    assert re.search(r"int amav_windows_cut\(int \w+, int \w+, int \w+, int \w+, const float \*\w+_dev, int \w+, int \w+,\s+"
                     r"const int32_t \*\w+_dev, const int32_t \*\w+_dev, const int32_t \*\w+_dev, float \*\w+_dev,\s+"
                     r"void \*\w+\);", text)
    i, p = ctypes.c_int, ctypes.c_void_p
    assert _lib.SIGNATURES["amav_windows_cut"] == (i, [i, i, i, i, p, i, i, p, p, p, p, p])
    assert _lib.SIGNATURES["amav_windows_cut_backward"] == (i, [i, i, i, i, i, i, p, i, i, i, i, i, p, p, p])
    for name in ("amav_windows_cut", "amav_windows_cut_backward"):
        assert hasattr(lib, name)
    for name in ("windows_cut", "windows_cut_backward", "windows_cut_differentiable", "windows_lattice"):
        assert callable(getattr(ops, name))


def test_cut_refusals(lib):
    entry = b"amav_windows_cut"
    for kw in (dict(F=-1), dict(C=-2), dict(h=-1), dict(w=-9), dict(K=-1)):
        _refused(lib, _cut(lib, **kw), entry, b"negative count")
    for size in (0, -4):
        _refused(lib, _cut(lib, size=size), entry, b"size")
    _refused(lib, _cut(lib, h=70000, w=70000), entry, b"2^31")
    _refused(lib, _cut(lib, size=50000), entry, b"2^31")
    for name in ("x", "frame", "oy", "ox", "out"):
        _refused(lib, _cut(lib, **{name: None}), entry, b"NULL")
    # nothing to cut: no pointer is looked at, nothing is launched
    assert _cut(lib, K=0, frame=None, oy=None, ox=None, out=None) == 0
    assert _cut(lib, C=0, x=None, out=None) == 0


def test_transpose_refusals(lib):
    entry = b"amav_windows_cut_backward"
    for kw in (dict(F=-1), dict(C=-2), dict(h=-1), dict(w=-9), dict(K=-1), dict(A=-1), dict(B=-3)):
        _refused(lib, _transpose(lib, **kw), entry, b"negative count")
    for size in (0, -4):
        _refused(lib, _transpose(lib, size=size), entry, b"size")
    for step in (0, -16):
        _refused(lib, _transpose(lib, step=step), entry, b"step")
    _refused(lib, _transpose(lib, h=70000, w=70000), entry, b"2^31")
    _refused(lib, _transpose(lib, A=2 ** 20, step=2 ** 12), entry, b"int32 range")
    _refused(lib, _transpose(lib, off_y=-2 ** 31), entry, b"int32 range")
    _refused(lib, _transpose(lib, off_x=2 ** 31 - 5), entry, b"int32 range")
    for name in ("gw", "table", "gx"):
        _refused(lib, _transpose(lib, **{name: None}), entry, b"NULL")
    # an empty grad_x: nothing to write
    assert _transpose(lib, F=0, gx=None, table=None, gw=None, K=0) == 0
    assert _transpose(lib, h=0, gx=None) == 0
