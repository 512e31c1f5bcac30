"""Host side of the PNG / inflate entry points: declared, exported and bound; struct offsets; the workspace queries on
accepted and rejected sizes; every refusal include/amav.h lists answers with its error code (no kernel is launched:
each call fails a check first)."""
import ctypes

import pytest

from abi_support import ERR_INVALID, ERR_WORKSPACE, FAKE, HEADER, lib  # noqa: F401 (lib: fixture)

RGB, L = 0, 1
U8, F32 = 0, 1
NAMES = ["amav_inflate_workspace_bytes", "amav_inflate", "amav_png_decode_workspace_bytes", "amav_png_decode"]


def test_symbols_are_declared_exported_and_bound(lib):
    from audio_motion_avatar_amd import _lib

    text = open(HEADER).read()
    for name in NAMES:
        assert name + "(" in text and hasattr(lib, name) and name in _lib.SIGNATURES
    d = _lib.DEFINES
    assert (d["AMAV_PNG_RGB"], d["AMAV_PNG_L"]) == (RGB, L)
    assert (d["AMAV_PNG_STATUS_INFLATE"], d["AMAV_PNG_STATUS_SIZE"], d["AMAV_PNG_STATUS_FILTER"]) == (1, 2, 4)
    restype, argtypes = _lib.SIGNATURES["amav_png_decode"]
    assert restype is ctypes.c_int and len(argtypes) == 14 and argtypes[-1] is ctypes.c_void_p
    assert argtypes[3] is ctypes.c_void_p and argtypes[4] is ctypes.c_int64 and argtypes[9] is ctypes.c_size_t
    restype, argtypes = _lib.SIGNATURES["amav_inflate"]
    assert restype is ctypes.c_int and len(argtypes) == 11 and argtypes[2] is ctypes.c_int64 and argtypes[5] is ctypes.c_int64
    assert _lib.SIGNATURES["amav_png_decode_workspace_bytes"][0] is ctypes.c_size_t
    assert _lib.SIGNATURES["amav_inflate_workspace_bytes"][0] is ctypes.c_size_t
    Frame = _lib.STRUCTS["amav_png_frame"]
    assert ctypes.sizeof(Frame) == 40 and Frame.zlib_end.offset == 8 and Frame.palette_at.offset == 16
    assert (Frame.color_type.offset, Frame.bit_depth.offset, Frame.palette_entries.offset, Frame.absent.offset) == (24, 28, 32, 36)
    Stream = _lib.STRUCTS["amav_inflate_stream"]
    assert ctypes.sizeof(Stream) == 40 and Stream.in_end.offset == 8 and Stream.out_begin.offset == 16
    assert Stream.out_capacity.offset == 24 and Stream.wrapper.offset == 32


def test_workspace_sizes(lib):
    for F, H, W in [(1, 1, 1), (1, 1, 7), (3, 9, 7), (2, 65, 13), (48, 512, 512), (1, 16384, 16384), (65535, 1, 1), (5, 130, 70)]:
        frame = -(-(H * (1 + 4 * W)) // 16) * 16  # 4 bytes per pixel and the filter bytes; frames start 16-byte aligned
        got = lib.amav_png_decode_workspace_bytes(F, H, W)
        assert F * frame <= got < F * frame + 256 and got % 256 == 0, (F, H, W)
    for N in (1, 70, 65535):
        assert 0 < lib.amav_inflate_workspace_bytes(N) <= 256


def test_workspace_queries_reject(lib):
    for F, H, W in ((0, 16, 16), (-1, 16, 16), (65536, 16, 16), (1, 0, 16), (1, 16, 0), (1, 16385, 16), (1, 16, 16385), (1, -3, 16)):
        assert lib.amav_png_decode_workspace_bytes(F, H, W) == 0, (F, H, W)
    for N in (0, -1, 65536):
        assert lib.amav_inflate_workspace_bytes(N) == 0


def decode(lib, F=2, H=48, W=64, stream=FAKE, stream_bytes=1000, records=FAKE, mode=RGB, layout=F32, out=FAKE, out_bytes=None,
           status=FAKE, ws=FAKE, ws_bytes=None):
    if out_bytes is None:
        out_bytes = max(F, 1) * max(H, 1) * max(W, 1) * 12
    if ws_bytes is None:
        ws_bytes = lib.amav_png_decode_workspace_bytes(F, H, W) or 1 << 20
    return lib.amav_png_decode(F, H, W, stream, stream_bytes, records, mode, layout, out, out_bytes, status, ws, ws_bytes, None)


def test_png_decode_refusals(lib):
    def refused(text, code=ERR_INVALID, **kw):
        assert decode(lib, **kw) == code, kw
        assert text.encode() in lib.amav_last_error(), (kw, lib.amav_last_error())

    for F in (0, -2, 65536):
        refused("outside 1..65535", F=F)
    for H, W in ((0, 16), (16, 0), (16385, 16), (16, 16385), (-1, 16)):
        refused("outside 1..16384", H=H, W=W)
    for mode in (-1, 2, 3):
        refused(f"unknown mode {mode}", mode=mode)
    for layout in (-1, 2, 444):
        refused(f"unknown layout {layout}", layout=layout)
    for missing in ("stream", "records", "status"):
        refused("NULL stream, records or status", **{missing: None})
    refused("negative stream_bytes", stream_bytes=-1)
    refused("misaligned records or status", records=FAKE + 4)
    refused("misaligned records or status", status=FAKE + 2)
    refused("NULL out", out=None)
    refused("misaligned out", out=FAKE + 2)
    assert decode(lib, layout=U8, out=FAKE + 1, stream=FAKE + 3, ws_bytes=0) == ERR_WORKSPACE  # bytes need no alignment
    for mode, layout, need in ((RGB, F32, 2 * 48 * 64 * 12), (RGB, U8, 2 * 48 * 64 * 3), (L, F32, 2 * 48 * 64 * 4), (L, U8, 2 * 48 * 64)):
        refused(f"output buffer {need - 1} < {need}", ERR_WORKSPACE, mode=mode, layout=layout, out_bytes=need - 1)
    need = lib.amav_png_decode_workspace_bytes(2, 48, 64)
    refused(f"workspace {need - 1} < {need}", ERR_WORKSPACE, ws_bytes=need - 1)
    refused(f"workspace 0 < {need}", ERR_WORKSPACE, ws=None)
    refused("not 16-byte aligned", ERR_WORKSPACE, ws=FAKE + 8)


def inflate(lib, N=3, stream=FAKE, stream_bytes=1000, records=FAKE, out=FAKE, out_bytes=1000, produced=FAKE, status=FAKE,
            ws=FAKE, ws_bytes=256):
    return lib.amav_inflate(N, stream, stream_bytes, records, out, out_bytes, produced, status, ws, ws_bytes, None)


def test_inflate_refusals(lib):
    def refused(text, code=ERR_INVALID, **kw):
        assert inflate(lib, **kw) == code, kw
        assert text.encode() in lib.amav_last_error(), (kw, lib.amav_last_error())

    for N in (0, -1, 65536):
        refused("outside 1..65535", N=N)
    for missing in ("stream", "records", "out", "produced", "status"):
        refused("NULL stream, records, out, produced or status", **{missing: None})
    refused("negative stream_bytes or out_bytes", stream_bytes=-1)
    refused("negative stream_bytes or out_bytes", out_bytes=-1)
    refused("misaligned records, produced or status", records=FAKE + 4)
    refused("misaligned records, produced or status", produced=FAKE + 4)
    refused("misaligned records, produced or status", status=FAKE + 2)
    assert inflate(lib, stream=FAKE + 3, out=FAKE + 5, ws_bytes=0) == ERR_WORKSPACE  # streams and outputs lie anywhere
    refused("workspace 255 < 256", ERR_WORKSPACE, ws_bytes=255)
    refused("workspace 0 < 256", ERR_WORKSPACE, ws=None)
    refused("not 16-byte aligned", ERR_WORKSPACE, ws=FAKE + 8)


def test_ops_refuse_on_the_host():
    """The tensor-level wrappers refuse CPU tensors and wrong arguments before they reach the library."""
    import torch

    import png_cases as pc

    from audio_motion_avatar_amd import AmavError, ops, png

    records, stream = png.frame_records([pc.pillow_files()[0][1]])
    assert (records.num_frames, records.height, records.width) == (1, 48, 64)
    with pytest.raises(AmavError, match="HIP device"):
        ops.png_decode(stream, records)
    with pytest.raises(AmavError, match="records must be an ops.PngRecords"):
        ops.png_decode(stream, records.table)
    with pytest.raises(AmavError, match="whole 40-byte records"):
        ops.PngRecords(records.table[:-1], 48, 64)
    with pytest.raises(AmavError, match="HIP device"):
        ops.inflate(stream, torch.zeros(1, 5, dtype=torch.int64))
    assert ops.PNG_MODES == {"rgb": 0, "l": 1}
    assert (ops.PNG_STATUS_INFLATE, ops.PNG_STATUS_SIZE, ops.PNG_STATUS_FILTER) == (1, 2, 4)
