"""Host-side argument checks of the row kernels' backward entry points (csrc/attention_rows_backward.hip).  No kernel is
launched: every call below is refused before it reaches the device."""
import ctypes

from abi_support import ERR_INVALID, ERR_WORKSPACE, FAKE, lib  # noqa: F401 (lib: fixture)

CHUNK = 16


def _colsum(lib, rows=40, cols=8, x=FAKE, stride=8, per_group=20, out=FAKE, ws=FAKE, ws_bytes=1 << 20):
    return lib.amav_rows_colsum(rows, cols, x, stride, per_group, out, ws, ws_bytes, None)


def _geglu(lib, rows=4, inner=16, proj=FAKE, stride=32, bias=None, dout=FAKE, dproj=FAKE, dstride=32):
    return lib.amav_geglu_backward(rows, inner, proj, stride, bias, dout, dproj, dstride, None)


def _ln(lib, rows=40, dim=512, h=FAKE, w=FAKE, dnorm=FAKE, dh_out=FAKE, dh=FAKE, dw=FAKE, db=FAKE, ws=FAKE, ws_bytes=1 << 20):
    return lib.amav_add_layernorm_backward(rows, dim, h, w, 1e-5, dnorm, dh_out, dh, dw, db, ws, ws_bytes, None)


def _refused(lib, rc, entry, word, code=ERR_INVALID):
    assert rc == code
    msg = lib.amav_last_error()
    assert entry in msg and word in msg, msg


def test_symbols_and_bindings_agree(lib):
    from audio_motion_avatar_amd import _lib, ops

    i, l, f, p, z = ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t
    assert _lib.SIGNATURES["amav_rows_colsum_workspace_bytes"] == (z, [l, i, l])
    assert _lib.SIGNATURES["amav_rows_colsum"] == (i, [l, i, p, l, l, p, p, z, p])
    assert _lib.SIGNATURES["amav_geglu_backward"] == (i, [l, i, p, l, p, p, p, l, p])
    assert _lib.SIGNATURES["amav_add_layernorm_backward_workspace_bytes"] == (z, [l, i])
    assert _lib.SIGNATURES["amav_add_layernorm_backward"] == (i, [l, i, p, p, f, p, p, p, p, p, p, z, p])
    for name in ("rows_colsum", "geglu_backward", "add_layernorm_backward", "geglu_differentiable",
                 "add_layernorm_differentiable"):
        assert callable(getattr(ops, name))
    assert ops.ROWS_CHUNK == CHUNK


def test_workspace_sizes_follow_the_documented_chunks(lib):
    up = lambda n: (n + 255) // 256 * 256
    chunks = lambda rows: (rows + CHUNK - 1) // CHUNK
    for rows, cols, per_group in ((1, 8, 1), (16, 8, 16), (17, 8, 17), (51, 256, 17), (6304, 4096, 6304), (6304, 512, 3152)):
        want = up((rows // per_group) * chunks(per_group) * cols * 4)
        assert lib.amav_rows_colsum_workspace_bytes(rows, cols, per_group) == want
    for bad in ((0, 8, 1), (8, 6, 8), (8, 0, 8), (9, 8, 2), (8, 8, 0)):
        assert lib.amav_rows_colsum_workspace_bytes(*bad) == 0
    for rows, dim in ((1, 256), (16, 512), (17, 768), (6304, 1024)):
        assert lib.amav_add_layernorm_backward_workspace_bytes(rows, dim) == up(chunks(rows) * 2 * dim * 4)
    for bad in ((0, 512), (4, 128), (4, 640)):
        assert lib.amav_add_layernorm_backward_workspace_bytes(*bad) == 0


def test_colsum_refusals(lib):
    entry = b"amav_rows_colsum"
    for kw in (dict(rows=0), dict(cols=6), dict(cols=0)):
        _refused(lib, _colsum(lib, **kw), entry, b"multiple of 4")
    for kw in (dict(per_group=0), dict(per_group=7)):
        _refused(lib, _colsum(lib, **kw), entry, b"rows_per_group")
    for name in ("x", "out"):
        _refused(lib, _colsum(lib, **{name: None}), entry, b"NULL")
    for stride in (4, 10):
        _refused(lib, _colsum(lib, stride=stride), entry, b"stride")
    _refused(lib, _colsum(lib, x=FAKE + 4), entry, b"aligned")
    _refused(lib, _colsum(lib, ws=None), entry, b"workspace", ERR_WORKSPACE)
    _refused(lib, _colsum(lib, ws_bytes=16), entry, b"workspace", ERR_WORKSPACE)


def test_geglu_backward_refusals(lib):
    entry = b"amav_geglu_backward"
    for kw in (dict(rows=0), dict(inner=0), dict(inner=6)):
        _refused(lib, _geglu(lib, **kw), entry, b"bad sizes")
    for name in ("proj", "dout", "dproj"):
        _refused(lib, _geglu(lib, **{name: None}), entry, b"NULL")
    for kw in (dict(stride=28), dict(stride=34), dict(dstride=16), dict(dstride=33)):
        _refused(lib, _geglu(lib, **kw), entry, b"stride")
    _refused(lib, _geglu(lib, bias=FAKE + 8), entry, b"aligned")


def test_add_layernorm_backward_refusals(lib):
    entry = b"amav_add_layernorm_backward"
    for kw in (dict(rows=0), dict(dim=128), dict(dim=640)):
        _refused(lib, _ln(lib, **kw), entry, b"dim must be")
    for name in ("h", "w", "dh", "dw", "db"):
        _refused(lib, _ln(lib, **{name: None}), entry, b"NULL")
    _refused(lib, _ln(lib, dnorm=FAKE + 4), entry, b"aligned")
    _refused(lib, _ln(lib, ws=None), entry, b"workspace", ERR_WORKSPACE)
    _refused(lib, _ln(lib, ws_bytes=40 * 2 * 512 * 4 // 16 - 1), entry, b"workspace", ERR_WORKSPACE)
