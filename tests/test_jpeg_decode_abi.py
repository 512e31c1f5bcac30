"""Host side of the JPEG decoder's entry points: declared, exported and bound; the workspace query on accepted and
rejected sizes; every refusal include/amav.h lists answers with its error code (no kernel is launched: each call fails
a check first)."""
import ctypes

import pytest

from abi_support import ERR_INVALID, ERR_WORKSPACE, FAKE, HEADER, lib  # noqa: F401 (lib: fixture)

import jpeg_model as jm

S420, S444, GRAY = 420, 444, 400
U8, F32 = 0, 1
NAMES = ["amav_jpeg_decode_workspace_bytes", "amav_jpeg_decode_levels", "amav_jpeg_decode"]


def test_symbols_are_declared_exported_and_bound(lib):
    from audio_motion_avatar_amd import _lib

    text = open(HEADER).read()
    for name in NAMES:
        assert name + "(" in text and hasattr(lib, name) and name in _lib.SIGNATURES
    d = _lib.DEFINES
    assert (d["AMAV_JPEG_GRAY"], d["AMAV_JPEG_HWC_U8"], d["AMAV_JPEG_CHW_F32"]) == (GRAY, U8, F32)
    assert (d["AMAV_JPEG_STATUS_MARKERS"], d["AMAV_JPEG_STATUS_ENTROPY"]) == (1, 2)
    restype, argtypes = _lib.SIGNATURES["amav_jpeg_decode"]
    assert restype is ctypes.c_int and len(argtypes) == 14 and argtypes[-1] is ctypes.c_void_p
    assert argtypes[5] is ctypes.c_int64 and argtypes[4] is ctypes.c_void_p and argtypes[6] is ctypes.c_void_p
    assert _lib.SIGNATURES["amav_jpeg_decode_workspace_bytes"][0] is ctypes.c_size_t
    Frame = _lib.STRUCTS["amav_jpeg_frame"]
    assert ctypes.sizeof(Frame) == 1128 and Frame.quant.offset == 24 and Frame.ac_values.offset == 24 + 192 + 3 * 48
    assert Frame.scan_end.offset == 8 and Frame.restart_interval.offset == 16


SIZES = [(1, 1, 1), (1, 8, 8), (3, 16, 16), (1, 17, 33), (2, 48, 64), (48, 512, 512), (1, 65535, 65535), (65535, 8, 8)]


@pytest.mark.parametrize("sampling", [S420, S444, GRAY])
def test_workspace_sizes(lib, sampling):
    for F, H, W in SIZES:
        if sampling == GRAY:
            mcu, bpm = 8, 1
            my, mx = -(-H // 8), -(-W // 8)
        else:
            mcu, my, mx, bpm = jm.geometry(H, W, str(sampling))
        mcus, blocks = my * mx, my * mx * bpm
        search = 16 * F * mcus + 4 * F  # interval starts and ends, intervals found
        levels_only = lib.amav_jpeg_decode_workspace_bytes(F, H, W, sampling, 1)
        assert search <= levels_only <= search + 3 * 256 and levels_only % 256 == 0
        planes = my * mcu * mx * mcu + (0 if sampling == GRAY else 2 * my * 8 * mx * 8)
        whole = lib.amav_jpeg_decode_workspace_bytes(F, H, W, sampling, 0)
        need = search + 128 * F * blocks + 4 * F * planes
        assert need <= whole <= need + 6 * 256 and whole % 256 == 0, (F, H, W)


def test_workspace_query_rejects(lib):
    fn = lib.amav_jpeg_decode_workspace_bytes
    for F, H, W in ((0, 16, 16), (-1, 16, 16), (65536, 16, 16), (1, 0, 16), (1, 16, 0), (1, 65536, 16), (1, 16, 65536), (1, -3, 16)):
        assert fn(F, H, W, S420, 0) == 0 and fn(F, H, W, GRAY, 1) == 0, (F, H, W)
    for sampling in (0, 1, 422, 411, 440):
        assert fn(1, 16, 16, sampling, 0) == 0
    assert fn(30, 65535, 65535, S444, 0) == 0 and fn(30, 65535, 65535, GRAY, 0) != 0  # more than 2^31 - 1 blocks


def decode(lib, F=2, H=48, W=64, sampling=S420, stream=FAKE, stream_bytes=1000, records=FAKE, layout=F32, out=FAKE,
           out_bytes=None, status=FAKE, ws=FAKE, ws_bytes=None):
    if out_bytes is None:
        out_bytes = max(F, 1) * max(H, 1) * max(W, 1) * 12
    if ws_bytes is None:
        ws_bytes = lib.amav_jpeg_decode_workspace_bytes(F, H, W, sampling, 0) or 1 << 20
    return lib.amav_jpeg_decode(F, H, W, sampling, stream, stream_bytes, records, layout, out, out_bytes, status, ws, ws_bytes,
                                None)


def decode_levels(lib, F=2, H=48, W=64, sampling=S420, stream=FAKE, stream_bytes=1000, records=FAKE, levels=FAKE,
                  levels_bytes=None, status=FAKE, ws=FAKE, ws_bytes=None):
    if levels_bytes is None:
        levels_bytes = 1 << 24
    if ws_bytes is None:
        ws_bytes = lib.amav_jpeg_decode_workspace_bytes(F, H, W, sampling, 1) or 1 << 20
    return lib.amav_jpeg_decode_levels(F, H, W, sampling, stream, stream_bytes, records, levels, levels_bytes, status, ws,
                                       ws_bytes, None)


@pytest.mark.parametrize("call", [decode, decode_levels])
def test_refusals_shared_by_both_entry_points(lib, call):
    def refused(text, code=ERR_INVALID, **kw):
        assert call(lib, **kw) == code, kw
        assert text.encode() in lib.amav_last_error(), (kw, lib.amav_last_error())

    for sampling in (0, 422, 411, 1):
        refused(f"unknown sampling {sampling}", sampling=sampling)
    for F, H, W in ((0, 16, 16), (-2, 16, 16), (65536, 16, 16), (1, 0, 16), (1, 16, 0), (1, 65536, 16), (1, 16, 65536)):
        refused("outside 1..65535", F=F, H=H, W=W)
    refused("exceed the decoder's limits", F=40, H=65535, W=65535, sampling=S444)
    for missing in ("stream", "records", "status"):
        refused("NULL stream, records or status", **{missing: None})
    refused("negative stream_bytes", stream_bytes=-1)
    refused("misaligned records or status", records=FAKE + 4)
    refused("misaligned records or status", status=FAKE + 2)
    assert call(lib, stream=FAKE + 3, ws_bytes=0) == ERR_WORKSPACE  # an unaligned stream is fine: it got as far as the workspace
    levels_only = call is decode_levels
    need = lib.amav_jpeg_decode_workspace_bytes(2, 48, 64, S420, int(levels_only))
    refused(f"workspace {need - 1} < {need}", ERR_WORKSPACE, ws_bytes=need - 1)
    refused(f"workspace 0 < {need}", ERR_WORKSPACE, ws=None)
    refused("not 16-byte aligned", ERR_WORKSPACE, ws=FAKE + 8)


def test_decode_refusals(lib):
    def refused(text, code=ERR_INVALID, **kw):
        assert decode(lib, **kw) == code, kw
        assert text.encode() in lib.amav_last_error(), (kw, lib.amav_last_error())

    for layout in (-1, 2, 444):
        refused(f"unknown layout {layout}", layout=layout)
    refused("NULL out", out=None)
    refused("misaligned out", out=FAKE + 2)
    assert decode(lib, layout=U8, out=FAKE + 1, ws_bytes=0) == ERR_WORKSPACE  # bytes need no alignment
    refused(f"output buffer {2 * 48 * 64 * 12 - 1} < {2 * 48 * 64 * 12}", ERR_WORKSPACE, out_bytes=2 * 48 * 64 * 12 - 1)
    refused(f"output buffer {2 * 48 * 64 * 3 - 1} < {2 * 48 * 64 * 3}", ERR_WORKSPACE, layout=U8, out_bytes=2 * 48 * 64 * 3 - 1)


def test_decode_levels_refusals(lib):
    blocks = 2 * 3 * 4 * 6
    assert decode_levels(lib, levels=None) == ERR_INVALID and b"NULL levels" in lib.amav_last_error()
    assert decode_levels(lib, levels=FAKE + 8) == ERR_INVALID and b"misaligned levels" in lib.amav_last_error()
    assert decode_levels(lib, levels_bytes=128 * blocks - 1) == ERR_WORKSPACE
    assert f"levels buffer {128 * blocks - 1} < {128 * blocks}".encode() in lib.amav_last_error()


def test_ops_refuse_on_the_host():
    """The tensor-level wrappers refuse CPU tensors and wrong arguments before they reach the library."""
    import torch

    from audio_motion_avatar_amd import AmavError, mjpeg, ops

    import jpeg_decode_cases as dc

    header = mjpeg.parse_jpeg(dc.jpeg("smooth_420_16x16_q50"))[0]
    records = mjpeg.frame_records([header], [0])
    stream = torch.frombuffer(bytearray(dc.jpeg("smooth_420_16x16_q50")), dtype=torch.uint8)
    with pytest.raises(AmavError, match="HIP device"):
        ops.jpeg_decode(stream, records)
    with pytest.raises(AmavError, match="HIP device"):
        ops.jpeg_decode_levels(stream, records)
    with pytest.raises(AmavError, match="records must be an ops.JpegRecords"):
        ops.jpeg_decode(stream, records.table)
    with pytest.raises(AmavError, match="whole 1128-byte records"):
        ops.JpegRecords(records.table[:-1], 16, 16, "420")
    with pytest.raises(AmavError, match="unknown sampling"):
        ops.JpegRecords(records.table, 16, 16, "422")
    assert ops.JPEG_SAMPLING == {"420": 420, "444": 444, "gray": 400} and ops.JPEG_LAYOUTS == {"hwc_u8": 0, "chw_f32": 1}
