"""png.parse_png: what it accepts and every PngError it lists; PngDirReader's order; pack_clip's buffer layout."""
import ctypes
import struct
import zlib

import numpy as np
import pytest

import png_cases as pc

from audio_motion_avatar_amd import png


def chunks(data):
    out, at = [], 8
    while at < len(data):
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        out.append((kind, data[at + 8:at + 8 + n]))
        at += 12 + n
    return out


def build(parts, signature=png.SIGNATURE):
    return signature + b"".join(pc._chunk(k, b) for k, b in parts)


def ihdr(w=4, h=3, depth=8, ct=2, comp=0, filt=0, lace=0):
    return b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ct, comp, filt, lace)


IDAT = (b"IDAT", zlib.compress(bytes(3 * 13)))
IEND = (b"IEND", b"")


def test_accepts_and_reports():
    samples = pc.random_samples(np.random.default_rng(1), 9, 7, 3, 4)
    palette = bytes(range(48))
    data = pc.write_png(samples, 3, 4, (0, 1), idat=10, palette=palette, trns=b"\x00\x01",
                        extra=[(b"gAMA", struct.pack(">I", 45455)), (b"zzZz", b"unknown ancillary")])
    h = png.parse_png(data)
    assert (h.height, h.width, h.color_type, h.bit_depth, h.palette, h.palette_entries) == (9, 7, 3, 4, palette, 16)
    assert len(h.idat) > 1 and all(b - a <= 10 for a, b in h.idat)
    joined = png.zlib_stream(data, h)
    assert len(zlib.decompress(joined)) == 9 * (1 + 4)
    assert [data[a - 4:a] for a, _ in h.idat] == [b"IDAT"] * len(h.idat)
    # PLTE in a truecolour file is a suggestion: parsed over, not kept
    assert png.parse_png(build([ihdr(), (b"PLTE", bytes(6)), IDAT, IEND])).palette == b""
    assert png.parse_png(bytearray(build([ihdr(), IDAT, IEND]))).idat  # bytes-like is fine
    assert png.parse_png(build([ihdr(w=16384, h=1), IDAT, IEND])).width == 16384


@pytest.mark.parametrize("name,data,text", [
    ("signature", build([ihdr(), IDAT, IEND], b"\x89PNG\r\n\x1a\r"), "signature"),
    ("crc", build([ihdr(), IDAT, IEND])[:-1] + b"\x00", "CRC"),
    ("crc_in_idat", build([ihdr(), IDAT, IEND]).replace(IDAT[1][:4], b"\x78\x9c\x00\x00", 1), "CRC"),
    ("no_ihdr", build([IDAT, IEND]), "before IHDR"),
    ("ihdr_twice", build([ihdr(), ihdr(), IDAT, IEND]), "IHDR"),
    ("no_idat", build([ihdr(), IEND]), "no IDAT"),
    ("no_iend", build([ihdr(), IDAT]), "no IEND"),
    ("idat_split_by_text", build([ihdr(), IDAT, (b"tEXt", b"k\x00v"), IDAT, IEND]), "not consecutive"),
    ("plte_after_idat", build([ihdr(ct=3), IDAT, (b"PLTE", bytes(6)), IEND]), "PLTE"),
    ("type3_without_plte", build([ihdr(ct=3), IDAT, IEND]), "without PLTE"),
    ("interlaced", build([ihdr(lace=1), IDAT, IEND]), "interlaced"),
    ("depth16", build([ihdr(depth=16), IDAT, IEND]), "16"),
    ("rgb_depth4", build([ihdr(depth=4), IDAT, IEND]), "not a PNG combination"),
    ("palette_depth16", build([ihdr(ct=3, depth=16), IDAT, IEND]), "not a PNG combination"),
    ("colour_type_5", build([ihdr(ct=5), IDAT, IEND]), "not a PNG combination"),
    ("compression_1", build([ihdr(comp=1), IDAT, IEND]), "compression method 1"),
    ("filter_method_1", build([ihdr(filt=1), IDAT, IEND]), "filter method 1"),
    ("width_0", build([ihdr(w=0), IDAT, IEND]), "outside 1..16384"),
    ("height_0", build([ihdr(h=0), IDAT, IEND]), "outside 1..16384"),
    ("width_16385", build([ihdr(w=16385), IDAT, IEND]), "outside 1..16384"),
    ("height_16385", build([ihdr(h=16385), IDAT, IEND]), "outside 1..16384"),
    ("truncated", build([ihdr(), IDAT, IEND])[:40], "chunk"),
    ("unknown_critical", build([ihdr(), (b"ABCD", b""), IDAT, IEND]), "critical"),
])
def test_refusals(name, data, text):
    with pytest.raises(png.PngError, match=text):
        png.parse_png(data)


def test_dir_reader_orders_by_number(tmp_path):
    one = build([ihdr(), IDAT, IEND])
    for stem in ("00010", "2", "00001"):
        (tmp_path / f"{stem}.png").write_bytes(one + stem.encode())
    (tmp_path / "notes.txt").write_text("x")
    reader = png.PngDirReader(str(tmp_path))
    assert len(reader) == 3 and [reader.frame_bytes(i)[len(one):] for i in range(3)] == [b"00001", b"2", b"00010"]
    (tmp_path / "b.png").write_bytes(one + b"b")
    assert [png.PngDirReader(str(tmp_path)).frame_bytes(i)[len(one):] for i in range(4)] == [b"00001", b"00010", b"2", b"b"]
    (tmp_path / "empty").mkdir()
    with pytest.raises(ValueError, match="no PNG files"):
        png.PngDirReader(str(tmp_path / "empty"))


def test_pack_clip_layout():
    rng = np.random.default_rng(2)
    a = pc.write_png(pc.random_samples(rng, 5, 6, 3, 8), 3, 8, (1,), idat=7, palette=bytes(range(30)))
    b = pc.write_png(pc.random_samples(rng, 5, 6, 2, 8), 2, 8, (4,))
    host, table_bytes, H, W = png.pack_clip([a, None, b])
    assert (table_bytes, H, W) == (120, 5, 6) and png.PNG_RECORD_BYTES == 40
    body = bytes(host[table_bytes:].tolist())
    recs = [struct.unpack_from("<qqqiiii", bytes(host[:table_bytes].tolist()), 40 * i) for i in range(3)]
    assert recs[1][6] == 1 and recs[0][6] == 0 and recs[2][6] == 0
    z0, z1, pal, ct, depth, entries, _ = recs[0]
    assert (ct, depth, entries) == (3, 8, 10) and body[pal:pal + 30] == bytes(range(30))
    assert len(zlib.decompress(body[z0:z1])) == 5 * 7  # the IDAT payloads, joined
    assert len(zlib.decompress(body[recs[2][0]:recs[2][1]])) == 5 * 19 and recs[2][3:6] == (2, 8, 0)
    # the same bytes read back through the struct generated from include/amav.h: every field is the parsed header's
    from audio_motion_avatar_amd import _lib

    Frame = _lib.STRUCTS["amav_png_frame"]
    assert ctypes.sizeof(Frame) == png.PNG_RECORD_BYTES
    raw, at = bytes(host[:table_bytes].tolist()), 30  # the streams follow the one palette
    for i, (blob, h) in enumerate([(a, png.parse_png(a)), (None, None), (b, png.parse_png(b))]):
        r = Frame.from_buffer_copy(raw, i * png.PNG_RECORD_BYTES)
        fields = (r.zlib_begin, r.zlib_end, r.palette_at, r.color_type, r.bit_depth, r.palette_entries, r.absent)
        if h is None:
            assert fields == (0, 0, 0, 0, 8, 0, 1)
            continue
        size = sum(e - s for s, e in h.idat)
        assert fields == (at, at + size, 0 if i == 0 else 30, h.color_type, h.bit_depth, h.palette_entries, 0)
        assert body[at:at + size] == png.zlib_stream(blob, h)
        at += size
    with pytest.raises(png.PngError, match="unequal size"):
        png.pack_clip([a, pc.write_png(pc.random_samples(rng, 5, 7, 2, 8), 2, 8)])
    with pytest.raises(png.PngError, match="frame 1: bad PNG signature"):
        png.pack_clip([a, b"nonsense"])
    with pytest.raises(png.PngError, match="at least one"):
        png.pack_clip([None])
