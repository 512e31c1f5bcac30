"""C ABI of the point refiner's train-mode BatchNorm entries (csrc/cloud_norm.hip): declared in include/amav.h, bound by
the generated signatures, exported by the library, and refusing bad arguments before any launch."""
import ctypes

import pytest

ENTRIES = ("amav_bn_batch_stats_workspace_bytes", "amav_bn_batch_stats", "amav_bn_gelu_train_backward",
           "amav_cluster_max_raw", "amav_cluster_max_route")
FAKE = 1 << 20  # a 16-byte aligned non-NULL address that no accepted call may reach


def _lib():
    from audio_motion_avatar_amd import _lib

    return _lib


def test_entries_are_declared_and_bound():
    _lib_ = _lib()
    with open(_lib_.HEADER_PATH) as f:
        header = f.read()
    i, l, p, z = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t
    want = {
        "amav_bn_batch_stats_workspace_bytes": (z, [l, i]),
        "amav_bn_batch_stats": (i, [l, i, p, p, p, p, z, p]),
        "amav_bn_gelu_train_backward": (i, [l, i, p, p, p, p, p, p, p, p, p, p, z, p]),
        "amav_cluster_max_raw": (i, [l, i, p, p, p, p, p]),
        "amav_cluster_max_route": (i, [l, i, p, p, p, p, p, p]),
    }
    for name in ENTRIES:
        assert name + "(" in header, name
        assert _lib_.SIGNATURES[name] == want[name], name


def test_library_exports_the_entries():
    lib = _lib().lib()
    for name in ENTRIES:
        assert hasattr(lib, name), name


def test_workspace_query():
    lib = _lib().lib()
    up = lambda v: (v + 255) // 256 * 256
    for rows, C in ((2, 32), (64, 32), (65, 260), (4099, 512), (300_000, 32)):
        # chunks of 64 rows: the backward's [chunks + 1, 3, C] fp64 sums (the statistics' [chunks, 2, C] fp32 fit inside)
        assert lib.amav_bn_batch_stats_workspace_bytes(rows, C) == up(((rows + 63) // 64 + 1) * 3 * C * 8)
    for bad in ((1, 32), (0, 32), (-5, 32), (100, 0), (100, 30), (100, -4)):
        assert lib.amav_bn_batch_stats_workspace_bytes(*bad) == 0, bad


def _refused(lib, rc, entry, word):
    assert rc != 0
    msg = lib.amav_last_error()
    assert entry in msg and word in msg, msg


def test_bad_arguments_are_refused_before_any_launch():
    lib = _lib().lib()
    ws = 1 << 16

    def stats(rows=100, C=32, x=FAKE, mean=FAKE, var=FAKE, w=FAKE, wb=ws):
        return lib.amav_bn_batch_stats(rows, C, x, mean, var, w, wb, None)

    _refused(lib, stats(rows=1), b"amav_bn_batch_stats", b"at least 2 rows")
    _refused(lib, stats(rows=0), b"amav_bn_batch_stats", b"at least 2 rows")
    _refused(lib, stats(C=30), b"amav_bn_batch_stats", b"bad sizes")
    _refused(lib, stats(x=None), b"amav_bn_batch_stats", b"NULL")
    _refused(lib, stats(mean=FAKE + 4), b"amav_bn_batch_stats", b"aligned")
    _refused(lib, stats(w=None), b"amav_bn_batch_stats", b"workspace")
    _refused(lib, stats(wb=16), b"amav_bn_batch_stats", b"workspace")

    def back(rows=100, C=32, wb=ws, **k):
        a = dict(x=FAKE, mean=FAKE, rstd=FAKE, w=FAKE, b=FAKE, g=FAKE, dx=FAKE, dw=FAKE, db=FAKE, ws=FAKE)
        a.update(k)
        return lib.amav_bn_gelu_train_backward(rows, C, a["x"], a["mean"], a["rstd"], a["w"], a["b"], a["g"], a["dx"],
                                               a["dw"], a["db"], a["ws"], wb, None)

    _refused(lib, back(rows=1), b"amav_bn_gelu_train_backward", b"at least 2 rows")
    _refused(lib, back(C=6), b"amav_bn_gelu_train_backward", b"bad sizes")
    for name in ("x", "mean", "rstd", "w", "b", "g", "dx", "dw", "db"):
        _refused(lib, back(**{name: None}), b"amav_bn_gelu_train_backward", b"NULL")
        _refused(lib, back(**{name: FAKE + 4}), b"amav_bn_gelu_train_backward", b"aligned")
    _refused(lib, back(wb=16), b"amav_bn_gelu_train_backward", b"workspace")

    def raw(clusters=3, C=32, x=FAKE, members=FAKE, seg=FAKE, out=FAKE):
        return lib.amav_cluster_max_raw(clusters, C, x, members, seg, out, None)

    _refused(lib, raw(clusters=0), b"amav_cluster_max_raw", b"bad sizes")
    _refused(lib, raw(C=34), b"amav_cluster_max_raw", b"bad sizes")
    _refused(lib, raw(seg=None), b"amav_cluster_max_raw", b"NULL")
    _refused(lib, raw(out=FAKE + 8), b"amav_cluster_max_raw", b"aligned")

    def route(clusters=3, C=32, x=FAKE, members=FAKE, seg=FAKE, g=FAKE, dx=FAKE):
        return lib.amav_cluster_max_route(clusters, C, x, members, seg, g, dx, None)

    _refused(lib, route(clusters=-1), b"amav_cluster_max_route", b"bad sizes")
    _refused(lib, route(C=2), b"amav_cluster_max_route", b"bad sizes")
    _refused(lib, route(members=None), b"amav_cluster_max_route", b"NULL")
    _refused(lib, route(g=FAKE + 4), b"amav_cluster_max_route", b"aligned")
