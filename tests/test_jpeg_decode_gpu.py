"""The HIP baseline JPEG decoder (csrc/jpeg_decode.hip through ops.jpeg_decode_levels / ops.jpeg_decode): levels bit for
bit against the project's encoder and against jpeg_model's scan decoder on libjpeg's files; pixels against the float64
model of tests/jpeg_decode_model.py and against libjpeg's recorded decode; damaged frames.

Pixels against the model.  include/amav.h states the chain (dequantise, separable IDCT, + 128, clamp, triangle filter,
colour conversion), each step in fp32.  jpeg_decode_model.reconstruct evaluates it in float64 and returns with every
sample a bound delta on what fp32 rounding can move it by, derived there step by step from the unit roundoff U = 2^-24:
a component sample 20 U S + 128 U with S = sum |basis| |coefficient| |basis| of its block (nine roundings per term and
pass, the second pass carrying the first one's error, one more for + 128); the triangle filter four roundings of values
<= 255 on top of the filtered bound; Cb - 128 and Cr - 128 one rounding of <= 128 each; the colour conversion four
roundings of values <= 255 + 128 (k_cb + k_cr) on top of e_Y + k_cb e_Cb + k_cr e_Cr.  On these inputs delta is at most
1.2e-3.  The decoder may differ from rint(model) only where the model lies within delta of a half-integer, then by one
level; inputs are admitted only if such samples are at most 1 % (MAX_UNDECIDED, a condition on the inputs, which
tests/test_jpeg_decode_model.py also checks for a float32 numpy evaluation of the model)."""
import functools

import numpy as np
import pytest
import torch

import jpeg_cases as jc
import jpeg_decode_cases as dc
import jpeg_decode_model as dm
import jpeg_model as jm

pytestmark = pytest.mark.gpu

MAX_UNDECIDED = 0.01
GUARD = 0xA5


def upload(blobs, gap=3):
    """Frames laid into one device byte buffer at odd offsets, `gap` bytes of 0xFF 0xD9 0xFF 0xD0 litter between them
    (markers outside a frame's scan range must not be seen) -> (stream tensor, offsets)."""
    litter = (b"\xff\xd9\xff\xd0" * (gap // 4 + 1))[:gap]
    buf, offsets = bytearray(litter), []
    for b in blobs:
        offsets.append(len(buf))
        buf += b + litter
    return torch.frombuffer(buf, dtype=torch.uint8).cuda(), offsets


def records_for(blobs, offsets):
    from audio_motion_avatar_amd import mjpeg

    return mjpeg.frame_records([mjpeg.parse_jpeg(b)[0] for b in blobs], offsets).to("cuda")


def decode_levels(blobs):
    from audio_motion_avatar_amd import ops

    stream, offsets = upload(blobs)
    levels, status = ops.jpeg_decode_levels(stream, records_for(blobs, offsets))
    return levels.cpu().numpy(), status.cpu().numpy()


def decode(blobs, layout="hwc_u8", **kw):
    from audio_motion_avatar_amd import ops

    stream, offsets = upload(blobs)
    out, status = ops.jpeg_decode(stream, records_for(blobs, offsets), layout=layout, **kw)
    return out.cpu().numpy(), status.cpu().numpy()


# ------------------------------------------------------------------------------------------------------- levels
SIZES = [(8, 8), (16, 16), (17, 9), (24, 40), (33, 50)]
QUALITIES = (1, 50, 100)


@pytest.mark.parametrize("restart_rows", [0, 1, 2])
@pytest.mark.parametrize("subsampling", ["444", "420"])
def test_levels_of_the_projects_own_streams_are_exact(subsampling, restart_rows):
    """jpeg_decode_levels(jpeg_encode(x)) == jpeg_coefficients(x), bit for bit: three frames of three qualities (three
    sets of quantisation tables) in one call, and the middle one alone."""
    from audio_motion_avatar_amd import ops

    for H, W in SIZES:
        frames = torch.from_numpy(jc.noise(3, H, W, seed=H * 100 + W)).cuda()
        blobs, want = [], []
        for f, q in enumerate(QUALITIES):
            stream, offsets = ops.jpeg_encode(frames[f:f + 1], quality=q, subsampling=subsampling, restart_rows=restart_rows)
            assert int(offsets[0]) == 0
            blobs.append(stream.cpu().numpy().tobytes())
            want.append(ops.jpeg_coefficients(frames[f:f + 1], quality=q, subsampling=subsampling).cpu().numpy()[0])
        got, status = decode_levels(blobs)
        assert got.dtype == np.int16 and got.shape == (3,) + want[0].shape and not status.any(), (H, W, status)
        for f in range(3):
            assert np.array_equal(got[f], want[f]), (H, W, QUALITIES[f])
        alone, status = decode_levels(blobs[1:2])
        assert np.array_equal(alone[0], want[1]) and not status.any(), (H, W)


def test_levels_of_libjpegs_files_are_the_scan_decoders():
    """Optimised (per-file) Huffman tables, restart rows 0 and 1, one component; and, on the CPU side, that the set
    reaches every branch of the scan: ZRL, blocks that end without EOB, stuffed bytes, AC category 10, DC category 10+,
    and more than eight RSTn so that the cycle wraps."""
    ds = [dc.decoded(n) for n in dc.NAMES]
    assert sum(d.zrl for d in ds) > 0 and sum(d.blocks_without_eob for d in ds) > 0 and sum(d.stuffed for d in ds) > 0
    assert max(d.max_ac_category for d in ds) >= 10 and max(len(d.rst) for d in ds) > 8
    assert any(dc.FILES[n]["optimize"] and dc.FILES[n]["restart_marker_rows"] == r for n in dc.NAMES for r in (0, 1))
    for name, d in zip(dc.NAMES, ds):
        got, status = decode_levels([dc.jpeg(name)])
        assert not status.any(), (name, status)
        assert got.shape == (1,) + d.levels.shape and np.array_equal(got[0], d.levels), name


# ------------------------------------------------------------------------------------------------------- pixels
def check_against_model(got, rgb, delta, what):
    worst, decided_but_different, undecided = dm.disagreement(got, rgb, delta)
    print(f"{what}: max |difference| {worst}, undecided {undecided:.5f}, delta <= {delta.max():.2e}")
    assert undecided <= MAX_UNDECIDED, what        # a condition on the input, not on the decoder
    assert worst <= 1 and decided_but_different == 0, (what, worst, decided_but_different)


@pytest.mark.parametrize("name", dc.NAMES)
def test_pixels_against_the_model_and_libjpeg(name):
    rgb, delta = dc.model(name)
    got, status = decode([dc.jpeg(name)])
    assert got.dtype == np.uint8 and got.shape == (1,) + rgb.shape and not status.any()
    check_against_model(got[0], rgb, delta, name)
    limit = dc.LIBJPEG_MAX[dc.FILES[name]["sampling"]] + 1  # the model's measured bound plus the model's own +-1
    assert np.abs(got[0].astype(np.int64) - dc.libjpeg_rgb(name).astype(np.int64)).max() <= limit
    planar, status = decode([dc.jpeg(name)], layout="chw_f32")
    assert planar.dtype == np.float32 and planar.shape == (1, 3) + rgb.shape[:2] and not status.any()
    want = (torch.from_numpy(got[0]).permute(2, 0, 1).float() / 255.0).numpy()
    assert np.array_equal(planar[0], want), "chw_f32 is exactly uint8 / 255"


@pytest.mark.parametrize("subsampling,H,W", [("420", 33, 50), ("444", 17, 33), ("420", 25, 17)])
def test_pixels_of_the_projects_own_streams(subsampling, H, W):
    """Odd sizes through the project's encoder: partial MCUs on both edges, the chroma plane's clamped last row and
    column.  Three frames in one call against the model of each, each equal to the frame decoded alone, twice."""
    from audio_motion_avatar_amd import ops

    frames = torch.from_numpy(np.stack([jc.disc(1, H, W)[0], jc.noise(1, H, W, seed=2)[0], jc.disc(3, H, W)[2]])).cuda()
    blobs = []
    for f, q in enumerate((95, 60, 30)):
        stream, _ = ops.jpeg_encode(frames[f:f + 1], quality=q, subsampling=subsampling, restart_rows=1)
        blobs.append(stream.cpu().numpy().tobytes())
    got, status = decode(blobs)
    again, _ = decode(blobs)
    assert not status.any() and np.array_equal(got, again), "two runs are bit-equal"
    for f, blob in enumerate(blobs):
        rgb, delta = dm.reconstruct(dm.decode(blob))
        check_against_model(got[f], rgb, delta, f"{subsampling} {H}x{W} frame {f}")
        alone, status = decode([blob])
        assert not status.any() and np.array_equal(alone[0], got[f]), "a frame of a batch equals the frame alone"


def test_a_frame_without_dht_equals_the_frame_with_its_tables():
    for name in ("smooth_420_17x9_q90_rr1", "hf_444_16x16_q90_rr1", "smooth_gray_16x16_q40"):
        data = dc.jpeg(name)
        bare = dc.strip_dht(data)
        assert len(bare) < len(data) - 150 and b"\xff\xc4" not in bare[:bare.index(b"\xff\xda")]
        full, s0 = decode([data])
        got, s1 = decode([bare])
        assert not s0.any() and not s1.any() and np.array_equal(full, got), name


# ------------------------------------------------------------------------------------------------------ damage
@functools.lru_cache(maxsize=None)
def damage_inputs():
    """Three 4:4:4 frames of 33 x 50 at quality 100, five restart intervals of one MCU row each, libjpeg's."""
    frames = jc.noise(3, 33, 50, seed=11)
    return [jc.pillow_jpeg(f, 100, "444", 1) for f in frames]


def rst_positions(blob):
    from audio_motion_avatar_amd import mjpeg

    begin = mjpeg.parse_jpeg(blob)[0].scan_begin
    return [i for i in range(begin, len(blob) - 1) if blob[i] == 0xFF and 0xD0 <= blob[i + 1] <= 0xD7]


def truncated(blob):
    cut = rst_positions(blob)
    return blob[:(cut[2] + cut[3]) // 2]  # inside the fourth interval


def missing_rst(blob):
    at = rst_positions(blob)[1]
    return blob[:at] + blob[at + 2:]


def corrupted_code(blob):
    """24 bytes in the middle of the third interval become FF 00 x 12: 96 one-bits, and no Huffman code is all ones, so
    wherever the symbol boundaries fall a code of sixteen ones is met."""
    cut = rst_positions(blob)
    at = (cut[1] + cut[2]) // 2 - 12
    assert cut[1] + 2 < at and at + 24 < cut[2]
    return blob[:at] + b"\xff\x00" * 12 + blob[at + 24:]


@pytest.mark.parametrize("damage,bits", [(truncated, 1), (missing_rst, 1), (corrupted_code, 2)])
def test_a_damaged_frame_between_two_good_ones(damage, bits):
    """The damaged frame's status carries the expected bit, its neighbours decode exactly as they do alone, the intervals
    of the damaged frame that lie before the damage too, and nothing outside the output tensor changes."""
    from audio_motion_avatar_amd import ops

    good = damage_inputs()
    blobs = [good[0], damage(good[1]), good[2]]
    clean, status = decode(good)
    assert not status.any()
    stream, offsets = upload(blobs, gap=5)
    records = records_for(blobs, offsets)
    guarded = torch.full((5, 33, 50, 3), GUARD, dtype=torch.uint8, device="cuda")
    flags = torch.full((5,), 77, dtype=torch.int32, device="cuda")
    out, st = ops.jpeg_decode(stream, records, layout="hwc_u8", out=guarded[1:4], status=flags[1:4])
    assert out.data_ptr() == guarded[1:4].data_ptr() and st.data_ptr() == flags[1:4].data_ptr()
    got, flags = guarded.cpu().numpy(), flags.cpu().numpy()
    assert (got[0] == GUARD).all() and (got[4] == GUARD).all() and flags[0] == 77 and flags[4] == 77
    assert flags[1] == 0 and flags[3] == 0 and flags[2] & bits, flags
    assert np.array_equal(got[1], clean[0]) and np.array_equal(got[3], clean[2])
    # 4:4:4: an interval is a band of 8 pixel rows that no other interval reaches into
    intact = {truncated: 24, missing_rst: 8, corrupted_code: 16}[damage]
    assert np.array_equal(got[2][:intact], clean[1][:intact])
    assert not np.array_equal(got[2], clean[1])
    if damage is corrupted_code:  # the intervals after the damaged one are whole again
        assert np.array_equal(got[2][24:], clean[1][24:])
    # the levels: zero from the block the damage is met in to the end of that interval (and beyond, where the
    # interval's start is not known)
    levels, st2 = ops.jpeg_decode_levels(stream, records)
    levels, whole = levels.cpu().numpy(), decode_levels(good)[0]
    assert np.array_equal(st2.cpu().numpy(), flags[1:4])
    assert np.array_equal(levels[0], whole[0]) and np.array_equal(levels[2], whole[2])
    per_row = 7 * 3  # blocks of one MCU row
    if damage is truncated:
        assert not levels[1][4 * per_row:].any() and np.array_equal(levels[1][:3 * per_row], whole[1][:3 * per_row])
    if damage is corrupted_code:
        assert not levels[1][3 * per_row - 3:3 * per_row].any(), "the end of the damaged interval is zero"
        assert np.array_equal(levels[1][3 * per_row:], whole[1][3 * per_row:])
    if damage is missing_rst:
        assert not levels[1][4 * per_row:].any(), "four markers: the fifth interval's start is not known"
