"""tests/png_model.py held to its oracles on the CPU: zlib.decompress on every sound stream, rejection by zlib and the
stated status bit on every damaged one, numpy.array(Image.open(...).convert(...)) on every PNG file.  The GPU tests then
hold the kernels to the same oracles and, for the damaged inputs, to this model."""
import zlib

import numpy as np
import pytest

import png_cases as pc
import png_model as pm

from audio_motion_avatar_amd import png


def test_inflate_equals_zlib_on_every_sound_stream():
    names = [n for n, _, _ in pc.sound_streams()]
    assert len(set(names)) == len(names)
    for name, stream, wrapper in pc.sound_streams():
        ref = zlib.decompress(stream, 15 if wrapper else -15)
        out, status = pm.inflate(stream, wrapper)
        assert status == 0 and out == ref, name


def test_the_hand_written_streams_are_what_they_claim():
    by_name = {n: s for n, s, _ in pc.sound_streams()}
    assert len(zlib.decompress(by_name["fixed_far_window"], -15)) == 33287
    assert zlib.decompress(by_name["stored_len0"], -15) == b"" and len(zlib.decompress(by_name["stored_65535"], -15)) == 65535
    spans = pc.match_spans(pc.ring_wrap_tokens())  # the wrap of the 32 KiB ring, from the token positions
    assert any(d0 < 32768 < d1 for d0, d1, _, _ in spans), "a destination straddles offset 32 768"
    assert any(s0 < 32768 < s1 and d0 >= 32768 for d0, d1, s0, s1 in spans), "a source straddles offset 32 768"
    assert any(d1 - d0 == 258 and d0 - s0 == 32748 for d0, d1, s0, s1 in spans)
    assert len(zlib.decompress(by_name["fixed_ring_wrap"], -15)) == spans[-1][1] == 33516
    info = {n: i for n, _, i in pc.dynamic_cases()}
    for symbol in (16, 17, 18):  # a repeat that starts inside HLIT and ends inside HDIST
        sent, _, hlit = info[f"dynamic_repeat{symbol}_crosses"]
        assert any(s == symbol and at < hlit < at + n for s, at, n in sent), symbol
    assert info["dynamic_15_bit_code_hclen19"][1] == 19 and max(pc.literals_15_bits()) == 15
    assert info["dynamic_hclen5"][1] == 5
    names = {n for n, _, _ in pc.sound_streams()}
    for strategy in ("fixed", "huffman", "rle", "default"):  # the whole product of the zlib cases is there
        for level in (1, 6, 9):
            for wrapper in ("raw", "zlib"):
                for data in ("one", "zeros300", "noise70k", "far70k"):
                    assert {f"zlib_{strategy}_l{level}_{wrapper}_{data}", f"zlib_{strategy}_l{level}_{wrapper}_{data}_flush"} <= names
    flushed = [s for n, s, _ in pc.sound_streams() if n.endswith("_flush")]
    assert len(flushed) == 96 and all(b"\x00\x00\xff\xff" in s for s in flushed)  # the empty stored block of a full flush


def test_every_damaged_stream_is_rejected_by_zlib_and_flagged():
    names = [c[0] for c in pc.damaged_streams()]
    for want in ("block_type_3", "len_nlen_mismatch", "oversubscribed_lengths", "repeat_without_predecessor", "repeat_overruns",
                 "length_symbol_286", "length_symbol_287", "distance_symbol_30", "distance_symbol_31", "first_symbol_is_a_match",
                 "distance_one_too_far", "zeros300_into_100", "bad_zlib_method", "fdict_set", "hclen4_all_zero"):
        assert want in names
    assert sum(n.startswith("cut_at_") for n in names) == 8
    for name, stream, wrapper, capacity, bit in pc.damaged_streams():
        assert pc.zlib_rejects(stream, wrapper, capacity), name
        out, status = pm.inflate(stream, wrapper, capacity)
        assert status & bit, (name, status)
        assert len(out) <= (400 if capacity is None else capacity), name


def test_damaged_frames_carry_their_bit():
    need = pc.DAMAGED_H * (1 + pc.DAMAGED_W)
    for name, stream, bit in pc.damaged_frames():
        _, status = pm.decode(stream, pc.DAMAGED_H, pc.DAMAGED_W, 0, 8)
        assert status & bit, (name, status)
        try:
            ok = len(zlib.decompress(stream)) == need and bit != pm.STATUS_FILTER
        except zlib.error:
            ok = False
        assert not ok, name
    stream, rows = pc.sound_frame(3)
    pixels, status = pm.decode(stream, pc.DAMAGED_H, pc.DAMAGED_W, 0, 8, mode="l")
    assert status == 0 and np.array_equal(pixels, rows)


@pytest.mark.filterwarnings("ignore:Palette images with Transparency")
@pytest.mark.parametrize("files", [pc.pillow_files, pc.png_files])
def test_png_decode_equals_pillow(files):
    for name, data in files():
        h = png.parse_png(data)
        need = h.height * (1 + pm.row_bytes(h.width, h.color_type, h.bit_depth))
        raw, status = pm.inflate(png.zlib_stream(data, h), 1, need)
        assert status == 0 and len(raw) == need, name
        rows, status = pm.unfilter(raw, h.height, h.width, h.color_type, h.bit_depth)
        assert status == 0
        for mode in ("rgb", "l"):
            got = pm.convert(rows, h.width, h.color_type, h.bit_depth, h.palette, mode)
            assert np.array_equal(got, pc.pillow_decode(data, mode)), (name, mode)


def test_the_case_list_covers_what_it_should():
    names = [n for n, _ in pc.png_files()]
    for H, W in pc.SIZES:
        for ct, depth in pc.KINDS:
            assert any(n.startswith(f"{H}x{W}_t{ct}d{depth}_") for n in names)
    for filters in ("0", "1", "2", "3", "4", "01234431"):
        for ct, depth in pc.KINDS:
            assert any(f"_t{ct}d{depth}_f{filters}_" in n for n in names)
    assert any(n.endswith("_idat1") for n in names) and any(n.endswith("_idat100") for n in names)


def test_conversion_rules():
    rows = np.array([[0b10110100]], np.uint8)
    assert pm.convert(rows, 8, 0, 1, mode="l").tolist() == [[255, 0, 255, 255, 0, 255, 0, 0]]
    assert pm.convert(rows, 4, 0, 2, mode="l").tolist() == [[170, 255, 85, 0]]
    assert pm.convert(rows, 2, 0, 4, mode="l").tolist() == [[11 * 17, 4 * 17]]
    palette = bytes([10, 20, 30, 200, 100, 50])
    assert pm.convert(np.array([[1, 0, 2]], np.uint8), 3, 3, 8, palette).tolist() == [[[200, 100, 50], [10, 20, 30], [0, 0, 0]]]
    assert pm.convert(np.array([[255, 0, 0, 9]], np.uint8), 1, 6, 8, mode="l").tolist() == [[(19595 * 255 + 0x8000) >> 16]]
    assert pm.convert(np.array([[7, 200]], np.uint8), 1, 4, 8).tolist() == [[[7, 7, 7]]]
