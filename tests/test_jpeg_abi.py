"""Host side of the JPEG entry points: declared, exported and bound; the size queries on accepted and rejected sizes;
every refusal include/amav.h lists answers with its error code (no kernel is launched: each call fails a check first)."""
import ctypes

import pytest

from abi_support import ERR_INVALID, ERR_WORKSPACE, FAKE, HEADER, lib  # noqa: F401 (lib: fixture)

import jpeg_model as jm

S420, S444 = 420, 444
NAMES = ["amav_jpeg_num_blocks", "amav_jpeg_stream_bound", "amav_jpeg_workspace_bytes", "amav_jpeg_coefficients",
         "amav_jpeg_encode"]
BG = (ctypes.c_float * 3)(1.0, 1.0, 1.0)


def test_symbols_are_declared_exported_and_bound(lib):
    from audio_motion_avatar_amd import _lib

    text = open(HEADER).read()
    for name in NAMES:
        assert name + "(" in text and hasattr(lib, name) and name in _lib.SIGNATURES
    assert _lib.DEFINES["AMAV_JPEG_420"] == S420 and _lib.DEFINES["AMAV_JPEG_444"] == S444
    assert _lib.DEFINES["AMAV_JPEG_HINT_WORKSPACE"] == 3 * 64 * 2
    restype, argtypes = _lib.SIGNATURES["amav_jpeg_encode"]
    assert restype is ctypes.c_int and len(argtypes) == 17 and argtypes[-1] is ctypes.c_void_p
    assert argtypes[11] is ctypes.c_int64  # capacity
    assert _lib.SIGNATURES["amav_jpeg_stream_bound"][0] is ctypes.c_size_t


SIZES = [(1, 1, 1), (1, 8, 8), (3, 16, 16), (1, 17, 33), (2, 48, 64), (1, 160, 16), (48, 512, 512), (1, 65535, 65535)]


@pytest.mark.parametrize("subsampling", [S420, S444])
def test_block_counts_bound_and_workspace(lib, subsampling):
    name = str(subsampling)
    for F, H, W in SIZES:
        mcu, my, mx, bpm = jm.geometry(H, W, name)
        blocks = F * my * mx * bpm
        assert lib.amav_jpeg_num_blocks(F, H, W, subsampling) == blocks
        for rr in (0, 1, 2):
            intervals = -(-my // rr) if rr else 1
            bound = lib.amav_jpeg_stream_bound(F, H, W, subsampling, rr)
            # worst case of a block: 22 bits of DC and 63 x 26 bits of AC, every byte stuffed; per interval one byte of
            # padding (stuffed) and a marker; the header (at most 640 bytes) and EOI
            per_block = 2 * -(-(22 + 63 * 26) // 8)
            assert bound == F * (640 + per_block * (blocks // F) + 2 * intervals + 2 * intervals + 2), (F, H, W, rr)
            ws = lib.amav_jpeg_workspace_bytes(F, H, W, subsampling, rr)
            assert ws >= 128 * blocks + 16 * F * intervals + 384 and ws % 256 == 0
            assert ws <= 128 * blocks + 16 * F * intervals + 384 + 4 * 256
    # the header really is below the 640 the bound allows: SOI 2, APP0 18, DQT 2 x 69, SOF0 19, DHT 2 x (33 + 183), DRI 6, SOS 14
    assert 2 + 18 + 2 * 69 + 19 + 2 * (33 + 183) + 6 + 14 == 629 <= 640


def test_size_queries_reject(lib):
    for fn in (lib.amav_jpeg_stream_bound, lib.amav_jpeg_workspace_bytes):
        for F, H, W in ((0, 16, 16), (-1, 16, 16), (1, 0, 16), (1, 16, 0), (1, 65536, 16), (1, 16, 65536), (1, -3, 16)):
            assert fn(F, H, W, S420, 1) == 0, (F, H, W)
        assert fn(1, 16, 16, 422, 1) == 0 and fn(1, 16, 16, 0, 1) == 0     # unknown subsampling
        assert fn(1, 16, 16, S420, -1) == 0                                  # negative restart_rows
        assert fn(1, 1024, 65535, S420, 16) == 0 and fn(1, 1024, 65535, S420, 15) != 0  # DRI counts MCUs in 16 bits
        assert fn(40, 65535, 65535, S444, 1) == 0                           # more than 2^31 - 1 blocks
    assert lib.amav_jpeg_num_blocks(1, 0, 16, S420) == 0 and lib.amav_jpeg_num_blocks(1, 16, 16, 411) == 0


def encode(lib, F=2, H=48, W=64, frames=FAKE, rgba=1, quality=90, sub=S420, rr=1, hint=None, bg=None, out=FAKE,
           capacity=1 << 20, offsets=FAKE, status=FAKE, ws=FAKE, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.amav_jpeg_workspace_bytes(F, H, W, sub, rr) or 1 << 20
    return lib.amav_jpeg_encode(F, H, W, frames, rgba, quality, sub, rr, hint, bg, out, capacity, offsets, status, ws,
                                ws_bytes, None)


def coefficients(lib, F=2, H=48, W=64, frames=FAKE, rgba=1, quality=90, sub=S420, hint=None, bg=None, levels=FAKE,
                 levels_bytes=None, ws=None, ws_bytes=0):
    if levels_bytes is None:
        levels_bytes = 128 * (lib.amav_jpeg_num_blocks(F, H, W, sub) or 1)
    return lib.amav_jpeg_coefficients(F, H, W, frames, rgba, quality, sub, hint, bg, levels, levels_bytes, ws, ws_bytes, None)


@pytest.mark.parametrize("call", [encode, coefficients])
def test_refusals_shared_by_both_entry_points(lib, call):
    def refused(text, **kw):
        assert call(lib, **kw) == ERR_INVALID, kw
        assert text.encode() in lib.amav_last_error(), (kw, lib.amav_last_error())

    for q in (0, -5, 101):
        refused(f"quality {q} outside 1..100", quality=q)
    for sub in (0, 422, 411, 1):
        refused(f"unknown subsampling {sub}", sub=sub)
    for F, H, W in ((0, 16, 16), (1, 0, 16), (1, 16, 0), (1, 65536, 16), (1, 16, 65536), (-2, 16, 16)):
        refused("outside 1..65535", F=F, H=H, W=W)
    refused("exceed the encoder's limits", F=40, H=65535, W=65535, sub=S444)
    refused("NULL frames", frames=None)
    refused("misaligned frames", frames=FAKE + 4)
    refused("a tile hint needs the background colour", hint=FAKE, bg=None)


def test_encode_refusals(lib):
    def refused(code, text, **kw):
        assert encode(lib, **kw) == code, kw
        assert text.encode() in lib.amav_last_error(), (kw, lib.amav_last_error())

    refused(ERR_INVALID, "restart_rows -1 is negative", rr=-1)
    refused(ERR_INVALID, "exceed the encoder's limits", H=1024, W=65535, rr=16)
    for missing in ("out", "offsets", "status"):
        refused(ERR_INVALID, "NULL output pointer", **{missing: None})
    refused(ERR_INVALID, "negative capacity", capacity=-1)
    refused(ERR_INVALID, "misaligned frame_offsets or status", offsets=FAKE + 4)
    refused(ERR_INVALID, "misaligned frame_offsets or status", status=FAKE + 2)
    need = lib.amav_jpeg_workspace_bytes(2, 48, 64, S420, 1)
    refused(ERR_WORKSPACE, f"workspace {need - 1} < {need}", ws_bytes=need - 1)
    refused(ERR_WORKSPACE, f"workspace 0 < {need}", ws=None)
    refused(ERR_WORKSPACE, "not 16-byte aligned", ws=FAKE + 8)
    # the workspace depends on the restart interval (sizes and offsets per interval)
    assert lib.amav_jpeg_workspace_bytes(2, 4800, 64, S420, 1) > lib.amav_jpeg_workspace_bytes(2, 4800, 64, S420, 0)


def test_coefficients_refusals(lib):
    blocks = lib.amav_jpeg_num_blocks(2, 48, 64, S420)
    assert coefficients(lib, levels=None) == ERR_INVALID and b"NULL levels" in lib.amav_last_error()
    assert coefficients(lib, levels=FAKE + 8) == ERR_INVALID and b"misaligned levels" in lib.amav_last_error()
    assert coefficients(lib, levels_bytes=128 * blocks - 1) == ERR_WORKSPACE
    assert f"levels buffer {128 * blocks - 1} < {128 * blocks}".encode() in lib.amav_last_error()
    for ws, ws_bytes in ((None, 384), (FAKE, 383), (FAKE + 4, 384)):
        assert coefficients(lib, hint=FAKE, bg=BG, ws=ws, ws_bytes=ws_bytes) == ERR_WORKSPACE
        assert b"a tile hint needs a 16-byte aligned workspace of 384 bytes" in lib.amav_last_error()


def test_ops_refuse_on_the_host():
    """The tensor-level wrappers refuse CPU tensors and wrong layouts before they reach the library."""
    import torch

    from audio_motion_avatar_amd import AmavError, ops

    with pytest.raises(AmavError, match="HIP device"):
        ops.jpeg_encode(torch.zeros(1, 8, 8, 3, dtype=torch.uint8))
    with pytest.raises(AmavError, match="HIP device"):
        ops.jpeg_coefficients(torch.zeros(1, 8, 8, 4))
    assert ops.jpeg_stream_bound(1, 8, 8, "444", 0) == 640 + 416 * 3 + 4 + 2
    with pytest.raises(AmavError, match="bad sizes"):
        ops.jpeg_stream_bound(1, 0, 8)
    assert ops.JPEG_SUBSAMPLING == {"420": 420, "444": 444}
