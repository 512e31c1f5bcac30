"""Host-side argument checks of the triplane decode backward's C entry points (no kernel is launched: every call below
is refused before it reaches the device)."""
import ctypes

from abi_support import ERR_INVALID, ERR_WORKSPACE, FAKE, lib  # noqa: F401 (lib: fixture)


def _args(F=2, N=100, C=8, R=8, scratch_bytes=None, lib=None):
    from audio_motion_avatar_amd import _lib

    a = _lib.TriplaneDecodeBackwardArgs()
    a.num_frames, a.num_points, a.channels, a.resolution, a.radius = F, N, C, R, 1.4
    a.tokens, a.tokens_frame_stride = FAKE, C * 3 * R * R
    for name in ("head_w_plane", "head_w_point", "points", "proj", "grad_records", "grad_tokens", "grad_head_w_plane",
                 "grad_head_w_point", "grad_points", "grad_transl", "scratch"):
        setattr(a, name, FAKE)
    a.boxes = None
    a.scratch_bytes = scratch_bytes if scratch_bytes is not None else (
        lib.amav_triplane_decode_backward_bytes(max(F, 1), max(N, 1), max(C, 1), max(R, 1)) if lib else 0)
    return a


def test_symbols_are_exported_and_bound(lib):
    from audio_motion_avatar_amd import _lib

    for name in ("amav_triplane_decode_backward", "amav_triplane_decode_backward_bytes"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES


def test_scratch_size_query(lib):
    assert lib.amav_triplane_decode_backward_bytes(0, 10, 8, 8) == 0
    assert lib.amav_triplane_decode_backward_bytes(2, 0, 8, 8) == 0
    assert lib.amav_triplane_decode_backward_bytes(2, 10, -1, 8) == 0
    small = lib.amav_triplane_decode_backward_bytes(2, 100, 8, 8)
    # at least the record gradient after the epilogue [F,N,16] and the texel gradient [F,3,R,R,16]
    assert small >= 4 * (2 * 100 * 16 + 2 * 3 * 64 * 16)
    assert lib.amav_triplane_decode_backward_bytes(4, 100, 8, 8) > small


def test_refusals_return_error_codes_without_a_launch(lib):
    assert lib.amav_triplane_decode_backward(None, None) == ERR_INVALID
    assert b"args is NULL" in lib.amav_last_error()
    for kw in (dict(F=0), dict(N=0), dict(C=0), dict(R=0), dict(F=70000)):
        assert lib.amav_triplane_decode_backward(ctypes.byref(_args(**kw, lib=lib)), None) == ERR_INVALID
    a = _args(C=1025, lib=lib)
    assert lib.amav_triplane_decode_backward(ctypes.byref(a), None) == ERR_INVALID
    assert b"LDS" in lib.amav_last_error()
    for name in ("tokens", "head_w_plane", "head_w_point", "points", "proj", "grad_records", "grad_tokens",
                 "grad_head_w_plane", "grad_head_w_point", "scratch"):
        a = _args(lib=lib)
        setattr(a, name, None)
        assert lib.amav_triplane_decode_backward(ctypes.byref(a), None) == ERR_INVALID, name
    a = _args(lib=lib)
    a.proj = FAKE + 4
    assert lib.amav_triplane_decode_backward(ctypes.byref(a), None) == ERR_INVALID
    assert b"aligned" in lib.amav_last_error()
    a = _args(lib=lib)
    a.radius = 0.0
    assert lib.amav_triplane_decode_backward(ctypes.byref(a), None) == ERR_INVALID
    a = _args(lib=lib)
    a.tokens_frame_stride = 10
    assert lib.amav_triplane_decode_backward(ctypes.byref(a), None) == ERR_INVALID
    a = _args(scratch_bytes=1024, lib=lib)
    assert lib.amav_triplane_decode_backward(ctypes.byref(a), None) == ERR_WORKSPACE
    assert b"scratch" in lib.amav_last_error()
