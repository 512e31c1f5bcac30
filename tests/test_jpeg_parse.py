"""mjpeg.parse_jpeg: the header record of Pillow's files against jpeg_model's independent parse, the Annex K default of a
file without DHT, every refusal, and the packed amav_jpeg_frame record."""
import ctypes
import io
import struct

import numpy as np
import pytest
from PIL import Image

import jpeg_cases as jc
import jpeg_decode_cases as dc
import jpeg_decode_model as dm
import jpeg_model as jm


def pillow(rgb, mode="RGB", **kw):
    buf = io.BytesIO()
    Image.fromarray(rgb).convert(mode).save(buf, "JPEG", **kw)
    return buf.getvalue()


def model_tables(d, c):
    """(quant in zigzag order, {(length, code): symbol} DC, AC) of component c as jpeg_model parsed them."""
    tq, td, ta = d.component_tables[c]
    return bytes(d.quant[tq][jm.ZIGZAG].astype(np.uint8)), d.huffman[0, td], d.huffman[1, ta]


def codes(counts, values):
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            table[length, code], code, k = values[k], code + 1, k + 1
        code <<= 1
    return table


def check_against_model(data, pos=0):
    from audio_motion_avatar_amd.mjpeg import parse_jpeg

    h, used = parse_jpeg(data, pos)
    d = dm.decode(data[pos:])
    assert used == d.consumed and (h.height, h.width) == (d.height, d.width)
    assert h.sampling == dm.sampling_name(d) and h.components == len(d.sampling)
    assert h.restart_interval == d.restart_interval and h.segments == d.segments and h.has_eoi and h.has_dht
    assert h.scan_end == used and data[pos + h.scan_begin - 14 + (2 * (3 - h.components)):][:2] == b"\xff\xda"
    for c in range(h.components):
        q, dct, act = model_tables(d, c)
        assert bytes(h.quant[c]) == q and codes(*h.dc[c]) == dct and codes(*h.ac[c]) == act
    return h, d


@pytest.mark.parametrize("name", dc.NAMES)
def test_fixture_headers(name):
    check_against_model(dc.jpeg(name))


def test_optimised_tables_restart_rows_comments_and_an_offset():
    rgb = jc.noise(1, 40, 24, seed=3)[0]
    data = pillow(rgb, quality=85, optimize=True, restart_marker_rows=1, subsampling=2, comment=b"made for a test",
                  exif=b"Exif\0\0MM\0*\0\0\0\x08\0\0")
    h, d = check_against_model(b"\x00\x01\x02" + data, pos=3)
    assert 0xFE in h.segments and 0xE1 in h.segments, "COM and APP1 are skipped, not refused"
    assert h.restart_interval == 2 and h.sampling == "420"  # one MCU row of a 24-pixel-wide 4:2:0 file
    from audio_motion_avatar_amd.mjpeg import ANNEX_K_HUFFMAN

    assert codes(*h.ac[0]) != codes(*ANNEX_K_HUFFMAN[1, 0]), "optimised tables are the file's own"
    gray, dg = check_against_model(pillow(rgb, "L", quality=60, restart_marker_rows=2))
    assert gray.sampling == "gray" and gray.components == 1 and gray.restart_interval == 2 * 3


def test_a_file_without_dht_takes_annex_k():
    from audio_motion_avatar_amd.mjpeg import ANNEX_K_HUFFMAN, parse_jpeg

    data = dc.jpeg("smooth_420_17x9_q90_rr1")  # not optimised: libjpeg wrote the Annex K tables out
    full, _ = parse_jpeg(data)
    bare, used = parse_jpeg(dc.strip_dht(data))
    assert 0xC4 in full.segments and 0xC4 not in bare.segments and not bare.has_dht and full.has_dht
    assert (bare.dc, bare.ac, bare.quant) == (full.dc, full.ac, full.quant)
    assert used == len(dc.strip_dht(data)) and full.scan_end - full.scan_begin == bare.scan_end - bare.scan_begin
    d = jm.decode(data)
    for (cls, tid), (counts, values) in ANNEX_K_HUFFMAN.items():
        assert codes(counts, values) == d.huffman[cls, tid]


def patch(data, marker, at, value):
    """`data` with byte `at` of the first `marker` segment's body replaced."""
    pos = data.index(bytes([0xFF, marker]))
    return data[:pos + 4 + at] + bytes([value]) + data[pos + 5 + at:]


def test_refusals_name_their_cause():
    from audio_motion_avatar_amd.mjpeg import JpegError, frame_records, parse_jpeg

    rgb = jc.noise(1, 16, 16, seed=1)[0]
    base = pillow(rgb, quality=80, subsampling=0)

    def refused(data, text):
        with pytest.raises(JpegError, match=text):
            parse_jpeg(data)

    refused(pillow(rgb, quality=80, progressive=True), r"progressive \(SOF2\)")
    sof = base.index(b"\xff\xc0")
    refused(base[:sof + 1] + b"\xc9" + base[sof + 2:], "arithmetic coding")
    refused(base[:sof + 1] + b"\xc1" + base[sof + 2:], "extended sequential")
    refused(patch(base, 0xC0, 0, 12), "12 bit samples")
    refused(pillow(rgb, quality=80, subsampling=1), r"2x1 1x1 1x1 \(4:2:2 and others\)")
    refused(patch(base, 0xC0, 7, 0x12), r"1x2 1x1 1x1 \(4:2:2 and others\)")
    refused(pillow(rgb, "CMYK", quality=80), "CMYK")
    sos = base.index(b"\xff\xda")
    one_of_three = base[:sos] + b"\xff\xda" + struct.pack(">HB", 8, 1) + base[sos + 5:sos + 7] + b"\x00\x3f\x00" + base[sos + 14:]
    refused(one_of_three, "several scans are not supported")
    refused(patch(base, 0xDA, 7, 5), "spectral selection")
    refused(patch(base, 0xDB, 0, 0x10), "16-bit quantisation tables")
    refused(base[2:], "no SOI")
    refused(base[:sos + 4], "overruns the data")
    refused(patch(base, 0xC0, 8, 3), "quantisation table 3 is not defined")
    a, b = parse_jpeg(base)[0], parse_jpeg(pillow(jc.noise(1, 16, 24, seed=1)[0], quality=80, subsampling=0))[0]
    with pytest.raises(JpegError, match="frames of unequal geometry in one call: frame 1 is 24x16 444"):
        frame_records([a, b], [0, 1000])
    with pytest.raises(JpegError, match="unequal geometry"):
        frame_records([a, parse_jpeg(pillow(rgb, quality=80, subsampling=2))[0]], [0, 1000])


def test_truncated_file_parses_and_says_so():
    from audio_motion_avatar_amd.mjpeg import parse_jpeg

    data = dc.jpeg("smooth_420_48x40_q75_rr1")
    h, used = parse_jpeg(data[:-40])
    assert not h.has_eoi and used == len(data) - 40 == h.scan_end


def test_packed_record_is_the_headers_struct():
    from audio_motion_avatar_amd import _lib
    from audio_motion_avatar_amd.mjpeg import JPEG_RECORD_BYTES, frame_records, parse_jpeg

    Frame = _lib.STRUCTS["amav_jpeg_frame"]
    assert ctypes.sizeof(Frame) == JPEG_RECORD_BYTES == 1128
    names = ["smooth_420_48x40_q75_rr1", "smooth_420_48x40_q75_rr1"]
    headers = [parse_jpeg(dc.jpeg(n))[0] for n in names]
    records = frame_records(headers, [0, 5000])
    assert (records.num_frames, records.height, records.width, records.sampling) == (2, 48, 40, "420")
    raw = bytes(records.table.numpy())
    for i, (h, off) in enumerate(zip(headers, (0, 5000))):
        r = Frame.from_buffer_copy(raw, i * JPEG_RECORD_BYTES)
        assert (r.scan_begin, r.scan_end, r.restart_interval) == (off + h.scan_begin, off + h.scan_end, 3)
        for c in range(3):
            assert bytes(r.quant[64 * c:64 * c + 64]) == bytes(h.quant[c])
            assert bytes(r.dc_counts[16 * c:16 * c + 16]) == bytes(h.dc[c][0])
            assert bytes(r.dc_values[16 * c:16 * c + 16]).rstrip(b"\0") == bytes(h.dc[c][1]).rstrip(b"\0")
            assert bytes(r.ac_counts[16 * c:16 * c + 16]) == bytes(h.ac[c][0])
            assert bytes(r.ac_values[256 * c:256 * c + len(h.ac[c][1])]) == bytes(h.ac[c][1])
            assert not any(r.ac_values[256 * c + len(h.ac[c][1]):256 * c + 256])
        assert r.reserved == 0
    # a grey frame fills the first component's rows; the other two stay zero
    grey = parse_jpeg(pillow(jc.noise(1, 40, 24, seed=3)[0], "L", quality=60, restart_marker_rows=2))[0]
    r = Frame.from_buffer_copy(bytes(frame_records([grey], [7]).table.numpy()))
    assert (r.scan_begin, r.scan_end, r.restart_interval, r.reserved) == (7 + grey.scan_begin, 7 + grey.scan_end, 6, 0)
    assert bytes(r.quant[:64]) == bytes(grey.quant[0]) and bytes(r.dc_counts[:16]) == bytes(grey.dc[0][0])
    assert bytes(r.dc_values[:len(grey.dc[0][1])]) == bytes(grey.dc[0][1]) and bytes(r.ac_counts[:16]) == bytes(grey.ac[0][0])
    assert bytes(r.ac_values[:len(grey.ac[0][1])]) == bytes(grey.ac[0][1])
    for field, n in ((r.quant, 64), (r.dc_counts, 16), (r.dc_values, 16), (r.ac_counts, 16), (r.ac_values, 256)):
        assert not any(field[n:])
