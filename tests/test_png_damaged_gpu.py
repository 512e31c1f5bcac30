"""Damaged DEFLATE streams and PNG frames on the device: every stream of the CPU-pinned list (tests/png_cases.py;
tests/test_png_model.py shows that zlib rejects each and which status bit it carries, tests/test_png_inflate_host.py runs
each through the kernel's own code under AddressSanitizer on the CPU).  Each sits between two sound neighbours; asserted
are the status words, the neighbours' exact bytes, the bytes the model says were produced before the stop, and that the
guard bytes around every output and around the workspace are intact.  Kept in a file of its own so that it can be run
alone and last."""
import struct
import zlib

import numpy as np
import pytest
import torch

import png_cases as pc
import png_model as pm

pytestmark = pytest.mark.gpu

GUARD = 0xC3


def test_damaged_streams_between_sound_ones():
    from audio_motion_avatar_amd import ops

    sound = [c for c in pc.sound_streams() if c[0].startswith(("dynamic_", "stored_huffman"))]  # raw streams
    blob, rows, expect, at, out_at = bytearray(), [], [], 0, 0

    def add(stream, wrapper, cap, want, status):
        nonlocal at, out_at
        blob.extend(b"\x5f" * 3 + stream)
        at += 3
        out_at += 13
        rows.append([at, at + len(stream), out_at, cap, wrapper])
        expect.append((want, status))
        at += len(stream)
        out_at += cap

    for k, (name, stream, wrapper, cap, bit) in enumerate(pc.damaged_streams()):
        n, s, w = sound[k % len(sound)]
        add(s, w, len(zlib.decompress(s, -15)), zlib.decompress(s, -15), 0)
        cap = 400 if cap is None else cap
        want, status = pm.inflate(stream, wrapper, cap)
        assert status & bit
        add(stream, wrapper, cap, want, status)
    n, s, w = sound[0]
    add(s, w, len(zlib.decompress(s, -15)), zlib.decompress(s, -15), 0)
    out = torch.full((out_at + 16,), GUARD, dtype=torch.uint8, device="cuda")
    stream = torch.frombuffer(bytearray(bytes(blob) + b"\x5f" * 8), dtype=torch.uint8).cuda()
    out, produced, status = ops.inflate(stream, torch.tensor(rows, dtype=torch.int64), out=out)
    torch.cuda.synchronize()  # the call returned and the kernel ended
    out, produced, status = out.cpu().numpy(), produced.cpu().tolist(), status.cpu().tolist()
    written = np.zeros(out.shape[0], bool)
    for k, (row, (want, want_status)) in enumerate(zip(rows, expect)):
        assert status[k] == want_status and produced[k] == len(want), (k, status[k], want_status, produced[k], len(want))
        assert out[row[2]:row[2] + len(want)].tobytes() == want, k
        written[row[2]:row[2] + len(want)] = True
    assert (out[~written] == GUARD).all(), "bytes beyond what a stream produced, or outside its range, were written"


def test_damaged_frames_between_sound_ones():
    """Through amav_png_decode itself, with the output and the workspace carved out of guard-filled buffers."""
    from audio_motion_avatar_amd import _lib, png

    H, W = pc.DAMAGED_H, pc.DAMAGED_W
    cases = pc.damaged_frames()
    streams, expect = [], []
    for k, (name, z, bit) in enumerate(cases):
        good, rows = pc.sound_frame(100 + k)
        streams += [good, z]
        pixels, status = pm.decode(z, H, W, 0, 8, mode="l")
        expect += [(0, rows), (status, pixels)]
    good, rows = pc.sound_frame(99)
    streams.append(good)
    expect.append((0, rows))
    F = len(streams)
    table, body = bytearray(), bytearray(b"\x5f" * 5)
    for z in streams:
        table += struct.pack("<qqqiiii", len(body), len(body) + len(z), 0, 0, 8, 0, 0)
        body += z + b"\x5f" * 3
    dev = torch.frombuffer(bytearray(bytes(table) + bytes(body)), dtype=torch.uint8).cuda()
    lib = _lib.lib()
    ws_bytes = lib.amav_png_decode_workspace_bytes(F, H, W)
    pad = 256
    ws = torch.full((ws_bytes + 2 * pad,), GUARD, dtype=torch.uint8, device="cuda")
    out = torch.full((F * H * W + 2 * pad,), GUARD, dtype=torch.uint8, device="cuda")
    status = torch.full((F + 2,), -7, dtype=torch.int32, device="cuda")
    assert ws.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    rc = lib.amav_png_decode(F, H, W, dev.data_ptr() + len(table), len(body), dev.data_ptr(), 1, 0, out.data_ptr() + pad, F * H * W,
                             status.data_ptr() + 4, ws.data_ptr() + pad, ws_bytes, None)
    assert rc == 0, lib.amav_last_error()
    torch.cuda.synchronize()  # the call returned and the kernels ended
    ws, out, status = ws.cpu().numpy(), out.cpu().numpy(), status.cpu().tolist()
    assert status[0] == -7 and status[-1] == -7
    assert (ws[:pad] == GUARD).all() and (ws[-pad:] == GUARD).all(), "the workspace's guard bytes"
    assert (out[:pad] == GUARD).all() and (out[-pad:] == GUARD).all(), "the output's guard bytes"
    frames = out[pad:-pad].reshape(F, H, W)
    names = ["sound"] * F
    names[1::2] = [c[0] for c in cases]
    for k, (want_status, rows) in enumerate(expect):
        assert status[1 + k] == want_status, (names[k], status[1 + k], want_status)
        assert np.array_equal(frames[k], rows), names[k] if k % 2 else ("neighbour of", names[k - 1] if k else names[1])
    for (name, _, bit), got in zip(cases, status[2::2]):
        assert got & bit, (name, got)
    # and through png.load_clip: the error names the damaged frames and only them
    files = [pc.write_png(rows[..., None], 0, 8, (4, 3, 2, 1, 0)) for rows in (expect[0][1], expect[2][1])]
    short = pc.write_png(np.zeros((H, W, 1), np.uint8), 0, 8, raw_override=bytes((H - 1) * (1 + W)))
    with pytest.raises(png.PngError, match=r"damaged frames 1 \(size\)$"):
        png.load_clip([files[0], short, files[1]], mode="l")
