"""Host side of the PNG encode / deflate entry points: declared, exported and bound; struct offsets and defines; the
workspace and bound queries on accepted and rejected sizes; every refusal include/amav.h lists answers with its error
code (no kernel is launched: each call fails a check first); the tensor-level wrappers refuse on the host."""
import ctypes

import pytest

from abi_support import ERR_INVALID, ERR_WORKSPACE, FAKE, HEADER, lib  # noqa: F401 (lib: fixture)

RGBA_F32, CHW_F32, RGB_U8, GREY_U8, GREY_F32 = range(5)
ADAPTIVE = 5
NAMES = ["amav_deflate_workspace_bytes", "amav_deflate", "amav_png_stream_bound", "amav_png_encode_workspace_bytes", "amav_png_encode"]
PIECE = 8192


def test_symbols_are_declared_exported_and_bound(lib):
    from audio_motion_avatar_amd import _lib

    text = open(HEADER).read()
    for name in NAMES:
        assert name + "(" in text and hasattr(lib, name) and name in _lib.SIGNATURES
    d = _lib.DEFINES
    assert d["AMAV_DEFLATE_PIECE"] == PIECE and PIECE <= 32768
    assert (d["AMAV_PNG_STATUS_SIZE"], d["AMAV_PNG_STATUS_TABLE"]) == (2, 8)
    assert [d["AMAV_PNG_IN_" + n] for n in ("RGBA_F32", "CHW_F32", "RGB_U8", "GREY_U8", "GREY_F32")] == [0, 1, 2, 3, 4]
    assert (d["AMAV_PNG_FILTER_ADAPTIVE"], d["AMAV_PNG_ROUND_NEAREST"], d["AMAV_PNG_ROUND_TRUNCATE"]) == (5, 0, 1)
    restype, argtypes = _lib.SIGNATURES["amav_png_encode"]
    assert restype is ctypes.c_int and len(argtypes) == 14 and argtypes[-1] is ctypes.c_void_p
    assert argtypes[3] is ctypes.c_void_p and argtypes[8] is ctypes.c_int64 and argtypes[12] is ctypes.c_size_t
    restype, argtypes = _lib.SIGNATURES["amav_deflate"]
    assert restype is ctypes.c_int and len(argtypes) == 11 and argtypes[2] is ctypes.c_int64 and argtypes[5] is ctypes.c_int64
    assert _lib.SIGNATURES["amav_png_stream_bound"][0] is ctypes.c_int64
    assert _lib.SIGNATURES["amav_png_encode_workspace_bytes"][0] is ctypes.c_size_t
    assert _lib.SIGNATURES["amav_deflate_workspace_bytes"][0] is ctypes.c_size_t
    Stream = _lib.STRUCTS["amav_deflate_stream"]
    assert ctypes.sizeof(Stream) == 40 and Stream.in_end.offset == 8 and Stream.out_begin.offset == 16
    assert Stream.out_capacity.offset == 24 and Stream.wrapper.offset == 32
    Inflate = _lib.STRUCTS["amav_inflate_stream"]  # the same five fields
    assert [f[0] for f in Stream._fields_] == [f[0] for f in Inflate._fields_]


def test_bound_and_workspace_sizes(lib):
    for F, H, W, layout in [(1, 1, 1, RGB_U8), (2, 3, 7, RGBA_F32), (3, 65, 13, GREY_U8), (2, 130, 70, CHW_F32), (1, 2, 12000, RGB_U8),
                            (48, 512, 512, RGBA_F32), (1, 16384, 16384, GREY_F32), (65535, 1, 1, RGB_U8)]:
        C = 1 if layout in (GREY_U8, GREY_F32) else 3
        raw = H * (1 + W * C)
        pieces = -(-raw // PIECE)
        assert lib.amav_png_stream_bound(F, H, W, layout) == F * (33 + 12 + 6 + raw + pieces * 17), (F, H, W)
        got = lib.amav_png_encode_workspace_bytes(F, H, W, layout)
        tables = F * 12 + F * pieces * 20  # frame sizes, Adler-32s; per piece: bytes, two sums, offset
        assert F * raw + tables <= got <= F * (raw + 16) + tables + 8 * 256, (F, H, W)
        assert got % 256 == 0
    for N, nbytes in ((1, 0), (3, 100000), (65535, 1 << 30)):
        pieces = nbytes // PIECE + N
        got = lib.amav_deflate_workspace_bytes(N, nbytes)
        assert pieces * 20 + N * 12 <= got <= pieces * 20 + N * 12 + 8 + 8 * 256


def test_queries_reject(lib):
    for F, H, W in ((0, 16, 16), (-1, 16, 16), (65536, 16, 16), (1, 0, 16), (1, 16, 0), (1, 16385, 16), (1, 16, 16385), (1, -3, 16)):
        assert lib.amav_png_encode_workspace_bytes(F, H, W, RGB_U8) == 0, (F, H, W)
        assert lib.amav_png_stream_bound(F, H, W, RGB_U8) == 0, (F, H, W)
    for layout in (-1, 5, 77):
        assert lib.amav_png_encode_workspace_bytes(2, 16, 16, layout) == 0
        assert lib.amav_png_stream_bound(2, 16, 16, layout) == 0
    for N, nbytes in ((0, 10), (-1, 10), (65536, 10), (1, -1)):
        assert lib.amav_deflate_workspace_bytes(N, nbytes) == 0


def encode(lib, F=2, H=48, W=64, frames=FAKE, layout=RGBA_F32, filter=ADAPTIVE, rounding=0, stream=FAKE, capacity=1 << 20,
           offsets=FAKE, status=FAKE, ws=FAKE, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.amav_png_encode_workspace_bytes(F, H, W, layout) or 1 << 20
    return lib.amav_png_encode(F, H, W, frames, layout, filter, rounding, stream, capacity, offsets, status, ws, ws_bytes, None)


def test_png_encode_refusals(lib):
    def refused(text, code=ERR_INVALID, **kw):
        assert encode(lib, **kw) == code, kw
        assert text.encode() in lib.amav_last_error(), (kw, lib.amav_last_error())

    for F in (0, -2, 65536):
        refused("outside 1..65535", F=F)
    for H, W in ((0, 16), (16, 0), (16385, 16), (16, 16385), (-1, 16)):
        refused("outside 1..16384", H=H, W=W)
    for layout in (-1, 5, 444):
        refused(f"unknown layout {layout}", layout=layout)
    for filter in (-1, 6, 99):
        refused(f"unknown filter {filter}", filter=filter)
    for rounding in (-1, 2):
        refused(f"unknown rounding {rounding}", rounding=rounding)
    for missing in ("frames", "stream", "offsets", "status"):
        refused("NULL frames, stream, frame_offsets or status", **{missing: None})
    refused("negative capacity", capacity=-1)
    refused("misaligned frames, frame_offsets or status", frames=FAKE + 2)
    refused("misaligned frames, frame_offsets or status", offsets=FAKE + 4)
    refused("misaligned frames, frame_offsets or status", status=FAKE + 2)
    assert encode(lib, layout=RGB_U8, frames=FAKE + 1, stream=FAKE + 3, ws_bytes=0) == ERR_WORKSPACE  # bytes need no alignment
    need = lib.amav_png_encode_workspace_bytes(2, 48, 64, RGBA_F32)
    refused(f"workspace {need - 1} < {need}", ERR_WORKSPACE, ws_bytes=need - 1)
    refused(f"workspace 0 < {need}", ERR_WORKSPACE, ws=None)
    refused("not 16-byte aligned", ERR_WORKSPACE, ws=FAKE + 8)


def deflate(lib, N=3, data=FAKE, nbytes=100000, records=FAKE, out=FAKE, out_bytes=1000, produced=FAKE, status=FAKE, ws=FAKE,
            ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.amav_deflate_workspace_bytes(N, nbytes) or 1 << 20
    return lib.amav_deflate(N, data, nbytes, records, out, out_bytes, produced, status, ws, ws_bytes, None)


def test_deflate_refusals(lib):
    def refused(text, code=ERR_INVALID, **kw):
        assert deflate(lib, **kw) == code, kw
        assert text.encode() in lib.amav_last_error(), (kw, lib.amav_last_error())

    for N in (0, -1, 65536):
        refused("outside 1..65535", N=N)
    for missing in ("data", "records", "out", "produced", "status"):
        refused("NULL input, records, out, produced or status", **{missing: None})
    refused("negative in_bytes or out_bytes", nbytes=-1)
    refused("negative in_bytes or out_bytes", out_bytes=-1)
    refused("misaligned records, produced or status", records=FAKE + 4)
    refused("misaligned records, produced or status", produced=FAKE + 4)
    refused("misaligned records, produced or status", status=FAKE + 2)
    need = lib.amav_deflate_workspace_bytes(3, 100000)
    assert deflate(lib, data=FAKE + 3, out=FAKE + 5, ws_bytes=0) == ERR_WORKSPACE  # inputs and outputs lie anywhere
    refused(f"workspace {need - 1} < {need}", ERR_WORKSPACE, ws_bytes=need - 1)
    refused(f"workspace 0 < {need}", ERR_WORKSPACE, ws=None)
    refused("not 16-byte aligned", ERR_WORKSPACE, ws=FAKE + 8)


def test_ops_refuse_on_the_host():
    import torch

    from audio_motion_avatar_amd import AmavError, ops

    with pytest.raises(AmavError, match="HIP device"):
        ops.png_encode(torch.zeros(1, 4, 4, 3, dtype=torch.uint8))
    with pytest.raises(AmavError, match="HIP device"):
        ops.deflate(torch.zeros(8, dtype=torch.uint8), torch.zeros(1, 5, dtype=torch.int64))
    assert ops.PNG_FILTERS == {"none": 0, "sub": 1, "up": 2, "average": 3, "paeth": 4, "adaptive": 5}
    assert ops.PNG_ROUNDINGS == {"nearest": 0, "truncate": 1}
    assert ops.DEFLATE_PIECE == PIECE and ops.deflate_bound(70000, True) == 70000 + 5 * 9 + 6
    assert ops.png_stream_bound(2, 3, 7) == 2 * (33 + 12 + 6 + 3 * 22 + 17)
