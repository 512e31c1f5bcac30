"""ops.png_encode: every file opens in Pillow (verify() checks the chunk CRCs, load() the Adler-32) and holds the expected
uint8 pixels, the IDAT payload inflates to exactly the scanlines of the NumPy filter model (so the per-row filter choice
is checked too), ops.png_decode reads the same stream back, no frame passes its share of amav_png_stream_bound, and a
capacity that is too small sets the status and leaves what lies behind it alone."""
import io
import struct
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

import png_encode_cases as ec

pytestmark = pytest.mark.gpu

RGB_SHAPES = [(1, 1, 1), (2, 3, 7), (2, 130, 70), (1, 2, 12000)]  # the last: a row longer than a piece
GREY_SHAPE = (3, 65, 13)
FILTERS = ["none", "sub", "up", "average", "paeth", "adaptive"]
FILTER_CODE = {"none": 0, "sub": 1, "up": 2, "average": 3, "paeth": 4, "adaptive": "adaptive"}


def make_input(layout, shape, seed):
    """(device tensor in `layout`, the fp32 / uint8 values as [F,H,W,C] on the host)"""
    F, H, W = shape
    rng = np.random.default_rng(seed)
    C = 1 if layout.startswith("grey") else 3
    if layout.endswith("u8"):
        values = rng.integers(0, 256, (F, H, W, C), dtype=np.uint8)
        values[:, :, : W // 2] //= 64  # a smooth half, so filters and matches have something to find
    else:
        values = ec.edge_values(rng, (F, H, W, C))
        values[:, : H // 2] = np.float32(0.25)
        values.reshape(-1)[:: 97] = np.float32("nan")
    if layout == "rgba_f32":
        host = np.concatenate([values, rng.random((F, H, W, 1), dtype=np.float32)], axis=-1)
    elif layout == "chw_f32":
        host = np.ascontiguousarray(values.transpose(0, 3, 1, 2))
    elif layout in ("grey_u8", "grey_f32"):
        host = values[..., 0]
    else:
        host = values
    return torch.from_numpy(np.ascontiguousarray(host)).cuda(), values


def split(stream, offsets):
    data, offsets = stream.cpu().numpy().tobytes(), offsets.tolist()
    assert offsets[0] == 0 and offsets[-1] == len(data)
    return [data[a:b] for a, b in zip(offsets[:-1], offsets[1:])]


def idat_payload(blob):
    at, parts, kinds = 8, [], []
    while at < len(blob):
        n, kind = struct.unpack(">I4s", blob[at:at + 8])
        assert zlib.crc32(blob[at + 4:at + 8 + n]) == struct.unpack(">I", blob[at + 8 + n:at + 12 + n])[0], kind
        kinds.append(kind)
        if kind == b"IDAT":
            parts.append(blob[at + 8:at + 8 + n])
        at += 12 + n
    assert kinds[0] == b"IHDR" and kinds[-1] == b"IEND" and set(kinds[1:-1]) == {b"IDAT"}
    return b"".join(parts)


def check(layout, shape, filter, rounding):
    from audio_motion_avatar_amd import _lib, ops, png

    frames, values = make_input(layout, shape, seed=len(layout) + 7 * sum(shape))
    want = values if values.dtype == np.uint8 else ec.to_levels(values, rounding)
    F, H, W = shape
    C = want.shape[-1]
    stream, offsets = ops.png_encode(frames, filter=filter, rounding=rounding)
    files = split(stream, offsets)
    bound = _lib.lib().amav_png_stream_bound(F, H, W, 3 if C == 1 else 2)
    for f, blob in enumerate(files):
        assert len(blob) <= bound // F
        Image.open(io.BytesIO(blob)).verify()
        im = Image.open(io.BytesIO(blob))
        im.load()
        assert im.mode == ("L" if C == 1 else "RGB") and im.size == (W, H)
        assert np.array_equal(np.asarray(im).reshape(H, W, C), want[f]), (layout, shape, filter, rounding, f)
        assert zlib.decompress(idat_payload(blob)) == ec.filter_rows(want[f], FILTER_CODE[filter]), (layout, shape, filter, f)
    back = png.load_clip(files, mode="l" if C == 1 else "rgb", device="cuda", layout="hwc_u8")
    assert np.array_equal(back.cpu().numpy().reshape(F, H, W, C), want)
    return frames, files


@pytest.mark.parametrize("shape", RGB_SHAPES)
@pytest.mark.parametrize("layout", ["rgba_f32", "chw_f32", "rgb_u8"])
def test_rgb_layouts_at_every_shape(layout, shape):
    check(layout, shape, "adaptive", "nearest")


@pytest.mark.parametrize("layout", ["grey_u8", "grey_f32"])
def test_grey_layouts(layout):
    check(layout, GREY_SHAPE, "adaptive", "nearest")
    check(layout, (1, 1, 1), "paeth", "truncate")


@pytest.mark.parametrize("rounding", ["nearest", "truncate"])
@pytest.mark.parametrize("filter", FILTERS)
def test_filters_and_roundings(filter, rounding):
    check("rgba_f32", (2, 130, 70), filter, rounding)
    check("grey_f32", GREY_SHAPE, filter, rounding)
    check("chw_f32", (2, 3, 7), filter, rounding)


def test_two_calls_give_the_same_bytes_and_a_small_capacity_is_respected():
    from audio_motion_avatar_amd import ops

    frames, files = check("rgb_u8", (2, 130, 70), "adaptive", "nearest")
    need = sum(len(b) for b in files)
    for capacity in (need - 1, len(files[0]) + 40, 20, 0):
        stream = torch.full((need + 64,), 0xC3, dtype=torch.uint8, device="cuda")
        offsets, status = ops.png_encode_into(frames, stream, capacity=capacity)
        flat = stream.cpu().numpy()
        assert offsets.cpu().tolist() == [0, len(files[0]), need]  # the sizes needed, whatever fits
        assert status.cpu().tolist() == [ops.PNG_STATUS_SIZE if len(files[0]) > capacity else 0, ops.PNG_STATUS_SIZE]
        assert (flat[capacity:] == 0xC3).all(), "a byte at or behind the capacity was written"
        assert flat[:capacity].tobytes() == b"".join(files)[:capacity]
    stream, offsets = ops.png_encode(frames, capacity=100)  # the retry at the bound
    assert stream.cpu().numpy().tobytes() == b"".join(files)


def test_flat_frame_is_matched_not_spelled_out():
    """One colour, filter `up`: the residual is all zeros.  A 258-byte match at distance 1 costs 13 bits in the fixed code,
    0.6 % of the bytes it covers; with the per-piece framing the file stays far below 3 % of the 196 608 raw bytes.  A
    matcher that silently emits literals cannot get under 12 % (one bit per byte)."""
    from audio_motion_avatar_amd import ops

    frame = torch.empty(1, 256, 256, 3, dtype=torch.uint8, device="cuda")
    frame[..., 0], frame[..., 1], frame[..., 2] = 200, 30, 90
    stream, offsets = ops.png_encode(frame, filter="up")
    blob = stream.cpu().numpy().tobytes()
    assert len(blob) < 0.03 * 196608, len(blob)
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(blob))), frame[0].cpu().numpy())
    assert zlib.decompress(idat_payload(blob))[256 * 3 + 1:] == bytes([2] + [0] * 768) * 255


def test_noise_frame_stays_within_the_stored_bound():
    from audio_motion_avatar_amd import _lib, ops

    noise = torch.from_numpy(np.random.default_rng(8).integers(0, 256, (1, 200, 300, 3), dtype=np.uint8)).cuda()
    stream, offsets = ops.png_encode(noise, filter="none")
    blob = stream.cpu().numpy().tobytes()
    raw = 200 * 901
    assert len(blob) <= 33 + 12 + 6 + raw + ec.pieces_of(raw) * 17 == _lib.lib().amav_png_stream_bound(1, 200, 300, 2)
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(blob))), noise[0].cpu().numpy())
