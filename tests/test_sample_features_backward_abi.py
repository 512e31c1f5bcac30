"""Host-side argument checks of the feature sampling backward's C entry points (no kernel is launched: every call
below is refused before it reaches the device)."""
import ctypes
import re

from abi_support import ERR_INVALID, ERR_WORKSPACE, FAKE, HEADER, lib  # noqa: F401 (lib: fixture)

ENTRY = b"amav_triplane_sample_features_backward"


def _args(lib, F=2, N=100, C=8, R=8, scratch_bytes=None):
    from audio_motion_avatar_amd import _lib

    a = _lib.TriplaneSampleBackwardArgs()
    a.num_frames, a.num_points, a.channels, a.resolution, a.radius = F, N, C, R, 1.4
    for name in ("planes", "points", "grad_out", "grad_planes", "grad_points", "scratch"):
        setattr(a, name, FAKE)
    # the renderer's view of a token slab [F,C,3R^2]
    a.planes_frame_stride, a.planes_plane_stride, a.planes_chan_stride = C * 3 * R * R, R * R, 3 * R * R
    a.grad_frame_stride, a.grad_plane_stride, a.grad_chan_stride = C * 3 * R * R, R * R, 3 * R * R
    a.scratch_bytes = scratch_bytes if scratch_bytes is not None else lib.amav_triplane_sample_features_backward_bytes(
        max(F, 1), max(N, 1), max(C, 1), max(R, 1))
    return a


def _refused(lib, a, code=ERR_INVALID, word=None):
    assert lib.amav_triplane_sample_features_backward(ctypes.byref(a), None) == code
    msg = lib.amav_last_error()
    assert ENTRY in msg, msg
    if word is not None:
        assert word in msg, msg


def test_symbols_are_exported_and_bound(lib):
    from audio_motion_avatar_amd import _lib, ops

    for name in ("amav_triplane_sample_features_backward", "amav_triplane_sample_features_backward_bytes"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert callable(ops.triplane_sample_features_differentiable) and callable(ops.triplane_sample_features_backward)


def test_header_and_bindings_agree():
    from audio_motion_avatar_amd import _lib

    text = open(HEADER).read()
    assert re.search(r"size_t amav_triplane_sample_features_backward_bytes\(int \w+, int \w+, int \w+, int \w+\);", text)
    assert re.search(r"int amav_triplane_sample_features_backward\(const amav_triplane_sample_backward_args \*\w+, "
                     r"void \*\w+\);", text)
    restype, argtypes = _lib.SIGNATURES["amav_triplane_sample_features_backward_bytes"]
    assert restype is ctypes.c_size_t and argtypes == [ctypes.c_int] * 4
    restype, argtypes = _lib.SIGNATURES["amav_triplane_sample_features_backward"]
    assert restype is ctypes.c_int and argtypes == [ctypes.POINTER(_lib.TriplaneSampleBackwardArgs), ctypes.c_void_p]


def test_scratch_size_query_is_monotone(lib):
    size = lib.amav_triplane_sample_features_backward_bytes
    for bad in ((0, 10, 8, 8), (2, 0, 8, 8), (2, 10, -1, 8), (2, 10, 8, 0)):
        assert size(*bad) == 0
    base = (2, 100, 8, 8)
    # the ordered points of the three planes: an id and four weights each
    assert size(*base) >= 2 * 3 * 100 * (4 + 16)
    for axis, values in ((0, (1, 2, 3, 8, 64)), (1, (1, 63, 64, 65, 100, 30000)), (2, (1, 8, 48, 64, 256, 1024)),
                         (3, (1, 7, 8, 32, 41, 42, 64, 128))):
        sizes = []
        for v in values:
            shape = list(base)
            shape[axis] = v
            sizes.append(size(*shape))
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes), (axis, sizes)
        if axis != 2:  # the channel count does not enter: the order of the points does not depend on it
            assert sizes[-1] > sizes[0], (axis, sizes)


def test_refusals_return_error_codes_without_a_launch(lib):
    assert lib.amav_triplane_sample_features_backward(None, None) == ERR_INVALID
    assert b"args is NULL" in lib.amav_last_error() and ENTRY in lib.amav_last_error()
    for kw in (dict(F=0), dict(N=0), dict(C=0), dict(R=0), dict(F=-3)):
        _refused(lib, _args(lib, **kw), word=b"bad sizes")
    _refused(lib, _args(lib, F=70000), word=b"exceeds grid")
    _refused(lib, _args(lib, R=5000), word=b"too large")
    for name in ("points", "grad_out"):
        a = _args(lib)
        setattr(a, name, None)
        _refused(lib, a, word=b"NULL")
    a = _args(lib)
    a.grad_planes = a.grad_points = None
    _refused(lib, a, word=b"NULL")
    a = _args(lib)
    a.planes = None  # wanted by grad_points
    _refused(lib, a, word=b"NULL")
    a = _args(lib)
    a.scratch = None  # wanted by grad_planes
    _refused(lib, a, word=b"scratch is NULL")
    for radius in (0.0, -1.0):
        a = _args(lib)
        a.radius = radius
        _refused(lib, a, word=b"radius")
    a = _args(lib)
    a.scratch = FAKE + 4
    _refused(lib, a, word=b"aligned")
    for name in ("grad_frame_stride", "grad_plane_stride", "grad_chan_stride"):
        a = _args(lib)
        setattr(a, name, 10)
        _refused(lib, a, word=b"strides")
    a = _args(lib)
    a.planes_chan_stride = -1
    _refused(lib, a, word=b"stride")
    _refused(lib, _args(lib, scratch_bytes=1024), code=ERR_WORKSPACE, word=b"scratch")
