"""Host-side refusals of the frame exchange's entry points (no kernel is launched: every call here fails its argument
checks first) and the wire size formula against tests/wire_model.py."""
import ctypes

from abi_support import ERR_INVALID, ERR_WORKSPACE, FAKE, lib  # noqa: F401 (lib: fixture)

import wire_model as wm


def test_wire_bytes_is_the_models_size_formula(lib):
    for F, H, W in list(wm.SIZES.values()) + [wm.EMIT_FUSED, wm.EMIT_FUSED_SMALL]:
        T = wm.geometry(H, W)[2]
        for cap in (0, 1, 7, F * T // 2, F * T):
            assert lib.amav_frames_wire_bytes(F, H, W, cap) == wm.wire_bytes(F, H, W, cap), (F, H, W, cap)
        assert lib.amav_frames_wire_bytes(F, H, W, F * T + 1) == 0      # a capacity above the tile count
        assert lib.amav_frames_wire_bytes(F, H, W, -1) == 0
    for F, H, W in ((0, 16, 16), (-1, 16, 16), (1, 0, 16), (1, 16, 0), (1, -16, 16), (1, 16, -16)):
        assert lib.amav_frames_wire_bytes(F, H, W, 0) == 0


def test_pack_refuses_a_wire_buffer_one_byte_short(lib):
    rgba = ctypes.cast(FAKE, ctypes.POINTER(ctypes.c_float))
    bg = (ctypes.c_float * 3)(1.0, 1.0, 1.0)
    for F, H, W in wm.SIZES.values():
        need = wm.wire_bytes(F, H, W, 5)
        assert lib.amav_frames_pack_tiles(F, H, W, rgba, bg, None, 5, FAKE, need - 1, None) == ERR_WORKSPACE
        msg = lib.amav_last_error().decode()
        assert str(need - 1) in msg and str(need) in msg, msg
    F, H, W = wm.SMALL
    assert lib.amav_frames_pack_tiles(F, H, W, rgba, bg, None, F * 9 + 1, FAKE, 1 << 30, None) == ERR_INVALID
    assert b"exceeds the tile count" in lib.amav_last_error()


def test_unpack_refuses_a_short_or_unaligned_stride(lib):
    for F, H, W in wm.SIZES.values():
        need = wm.wire_bytes(F, H, W, 5)
        for stride in (need - 16, need + 8):
            assert lib.amav_frames_unpack_tiles(2, F, H, W, 5, FAKE, stride, FAKE, FAKE, None) == ERR_INVALID
            assert f"wire stride {stride} does not hold a {need}-byte buffer".encode() in lib.amav_last_error()
    F, H, W = wm.WIDE
    need = wm.wire_bytes(F, H, W, 5)
    for stride in (need - 16, need + 8):
        assert lib.amav_frames_unpack_tiles_delta(2, F, H, W, 5, FAKE, stride, FAKE, FAKE, FAKE, None) == ERR_INVALID
        assert b"wire stride" in lib.amav_last_error()


def test_delta_unpack_refuses_ragged_widths_and_frames_beyond_its_lds_table(lib):
    for F, H, W in (wm.RAGGED4, wm.RAGGED1, (3, 50, 70)):
        need = wm.wire_bytes(F, H, W, 5)
        assert lib.amav_frames_unpack_tiles_delta(1, F, H, W, 5, FAKE, need, FAKE, FAKE, FAKE, None) == ERR_INVALID
        assert b"not a multiple of 16" in lib.amav_last_error()
    need = wm.wire_bytes(1, 2160, 3840, 5)
    assert lib.amav_frames_unpack_tiles_delta(1, 1, 2160, 3840, 5, FAKE, need, FAKE, FAKE, FAKE, None) == ERR_INVALID
    assert b"LDS table" in lib.amav_last_error()


def test_delta_unpack_supported_agrees_with_the_kernels_limit(lib):
    """Where ops.frames_delta_unpack_supported(H, W) is false the entry point refuses the size on the host, for the
    width or for its LDS table (valid pointers, no launch: the call is refused).  Where it is true the frame passes both
    limits: asked with a misaligned output pointer (the check after the width's, so nothing is launched) the call is
    refused for the alignment, and the tile table fits the 64 KiB the launch asks for; that these sizes then run is
    tests/test_frame_wire_gpu.py's part."""
    from audio_motion_avatar_amd import ops

    sizes = [(1296, 2304), (2160, 3840), (50, 70)] + [(H, W) for _, H, W in wm.SIZES.values()]
    want = {(1296, 2304): True, (2160, 3840): False, (50, 70): False, wm.WIDE[1:]: True, wm.TED[1:]: True,
            wm.RAGGED4[1:]: False, wm.RAGGED1[1:]: False, wm.SMALL[1:]: True}
    for H, W in sizes:
        need = wm.wire_bytes(1, H, W, 1)
        supported = ops.frames_delta_unpack_supported(H, W)
        assert supported == want[(H, W)], (H, W)
        out = FAKE + 4 if supported else FAKE
        assert lib.amav_frames_unpack_tiles_delta(1, 1, H, W, 1, FAKE, need, out, FAKE, FAKE, None) == ERR_INVALID
        msg = lib.amav_last_error()
        if supported:
            assert b"misaligned buffer" in msg and (wm.geometry(H, W)[2] + wm.DELTA_WAVES * 128) * 4 <= 64 * 1024
        else:
            assert b"not a multiple of 16" in msg or b"LDS table" in msg, msg
    # the limit itself: (T + 16 * 128) ints in 64 KiB
    assert ops.DELTA_UNPACK_MAX_TILES == 64 * 1024 // 4 - wm.DELTA_WAVES * 128 == 14336
    assert ops.frames_delta_unpack_supported(16, 16 * 14336) and not ops.frames_delta_unpack_supported(16, 16 * 14337)
