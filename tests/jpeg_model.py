"""Baseline JPEG as include/amav.h states it for amav_jpeg_encode, restated independently of the product in float64
numpy, plus a pure-Python decoder of the scan that reports what it met on the way.  tests/test_jpeg_model.py pins both
against libjpeg (through Pillow); tests/test_jpeg_gpu.py holds the HIP encoder against them.

    quant_tables(quality)                     -> two [64] tables, natural order (T.81 Annex K scaled by libjpeg's rule)
    quotients(rgb, quality, subsampling)      -> float64 [F, blocks, 64]: coefficient / table entry before rounding,
                                                 blocks in MCU-interleaved scan order, coefficients in zigzag order
    levels(rgb, quality, subsampling)         -> rint of the above, int64
    decode(jpeg_bytes)                        -> Decoded: header fields, levels [blocks, 64], event counters
    reconstruct_444(decoded)                  -> float64 RGB [H, W, 3] of a 4:4:4 file (dequantise, float IDCT, colour)
"""
import dataclasses

import numpy as np

QUANT_BASE = np.array([
    [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87,
     80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92,
     95, 98, 112, 100, 103, 99],
    [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99,
     99, 99] + [99] * 32])


def _zigzag():
    order = sorted(((y, x) for y in range(8) for x in range(8)),
                   key=lambda p: (p[0] + p[1], p[0] if (p[0] + p[1]) % 2 else p[1]))
    return np.array([y * 8 + x for y, x in order])


ZIGZAG = _zigzag()  # ZIGZAG[k] = natural index of the k-th coefficient of the scan
DCT = np.array([[(np.sqrt(1 / 8) if u == 0 else 0.5) * np.cos((2 * x + 1) * u * np.pi / 16) for x in range(8)]
                for u in range(8)])  # orthonormal DCT-II: coefficients = DCT @ block @ DCT.T


def quant_tables(quality):
    assert 1 <= quality <= 100
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((QUANT_BASE * s + 50) // 100, 1, 255)


def ycc(rgb):
    """float64 [..., 3] 0..255 -> Y, Cb, Cr (JFIF, full range, not rounded)."""
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    return np.stack([0.299 * r + 0.587 * g + 0.114 * b, -0.168736 * r - 0.331264 * g + 0.5 * b + 128,
                     0.5 * r - 0.418688 * g - 0.081312 * b + 128], axis=-1)


def geometry(H, W, subsampling):
    mcu = 8 if subsampling == "444" else 16
    my, mx = -(-H // mcu), -(-W // mcu)
    return mcu, my, mx, (3 if subsampling == "444" else 6)


def _blocks(plane):
    """[F, 8a, 8b] -> [F, a, b, 8, 8]"""
    F, h, w = plane.shape
    return plane.reshape(F, h // 8, 8, w // 8, 8).transpose(0, 1, 3, 2, 4)


def quotients(rgb, quality, subsampling="420"):
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.ndim == 4 and rgb.shape[-1] == 3
    F, H, W, _ = rgb.shape
    mcu, my, mx, bpm = geometry(H, W, subsampling)
    # a partial MCU replicates the last column / row
    pix = np.pad(rgb.astype(np.float64), ((0, 0), (0, my * mcu - H), (0, mx * mcu - W), (0, 0)), mode="edge")
    planes = ycc(pix) - 128.0
    q = quant_tables(quality).astype(np.float64)

    def coded(plane, table):  # [F, a, b, 64 zigzag]
        c = np.einsum("ux,fabxy,vy->fabuv", DCT, _blocks(plane), DCT)  # u: vertical frequency
        return (c.reshape(c.shape[:3] + (64,)) / q[table])[..., ZIGZAG]

    y = coded(planes[..., 0], 0)
    if subsampling == "444":
        per_mcu = [y, coded(planes[..., 1], 1), coded(planes[..., 2], 1)]
        out = np.stack(per_mcu, axis=3)  # [F, my, mx, 3, 64]
    else:
        sub = planes[..., 1:].reshape(F, my * 8, 2, mx * 8, 2, 2).mean(axis=(2, 4))  # chroma: mean of each 2x2
        y = y.reshape(F, my, 2, mx, 2, 64).transpose(0, 1, 3, 2, 4, 5).reshape(F, my, mx, 4, 64)  # Y00 Y01 Y10 Y11
        out = np.concatenate([y, coded(sub[..., 0], 1)[:, :, :, None], coded(sub[..., 1], 1)[:, :, :, None]], axis=3)
    return out.reshape(F, my * mx * bpm, 64)


def levels(rgb, quality, subsampling="420"):
    return np.rint(quotients(rgb, quality, subsampling)).astype(np.int64)


def undecided(quot, delta):
    """Where the exact quotient is within `delta` of a rounding boundary (the level may go either way)."""
    return np.abs(np.abs(quot - np.floor(quot)) - 0.5) <= delta


# --------------------------------------------------------------------------------------------------------- decoder
@dataclasses.dataclass
class Decoded:
    height: int = 0
    width: int = 0
    sampling: tuple = ()            # ((h, v) of Y, Cb, Cr)
    quant: dict = dataclasses.field(default_factory=dict)     # table id -> [64] natural order
    huffman: dict = dataclasses.field(default_factory=dict)   # (class, id) -> {(length, code): symbol}
    component_tables: list = dataclasses.field(default_factory=list)  # per component: (quant id, dc id, ac id)
    restart_interval: int = 0       # MCUs, 0 = none
    segments: list = dataclasses.field(default_factory=list)  # marker bytes in order of appearance
    levels: np.ndarray = None       # [blocks, 64] zigzag, MCU-interleaved order
    consumed: int = 0               # bytes up to and including EOI
    stuffed: int = 0                # FF 00 pairs in the entropy-coded data
    zrl: int = 0
    blocks_without_eob: int = 0
    max_dc_category: int = 0
    max_ac_category: int = 0
    rst: list = dataclasses.field(default_factory=list)       # n of every RSTn, in order


class _Bits:
    def __init__(self, data):
        self.value, self.left = int.from_bytes(data, "big"), 8 * len(data)

    def take(self, n):
        assert n <= self.left, "entropy-coded segment ends inside a symbol"
        self.left -= n
        return (self.value >> self.left) & ((1 << n) - 1)

    def symbol(self, table):
        code = 0
        for length in range(1, 17):
            code = code << 1 | self.take(1)
            if (length, code) in table:
                return table[length, code]
        raise AssertionError("no Huffman code of up to 16 bits matches")


def _extend(bits, size):
    return bits if size == 0 or bits >> (size - 1) else bits - (1 << size) + 1


def decode(data):
    """One baseline JPEG file at the start of `data` -> Decoded.  Asserts the structure the encoder promises: SOF0,
    one interleaved scan, every interval padded with 1-bits to a byte and followed directly by its marker (no fill
    bytes), RSTn only where the restart interval puts them."""
    d = Decoded()
    assert data[:2] == b"\xff\xd8", "no SOI"
    pos, comps, scan = 2, [], None
    while scan is None:
        assert data[pos] == 0xFF and data[pos + 1] not in (0x00, 0xFF), f"marker expected at {pos}"
        marker, n = data[pos + 1], int.from_bytes(data[pos + 2:pos + 4], "big")
        body = data[pos + 4:pos + 2 + n]
        d.segments.append(marker)
        if marker == 0xDB:
            while body:
                assert body[0] >> 4 == 0, "16-bit quantisation table in a baseline file"
                table = np.zeros(64, dtype=np.int64)
                table[ZIGZAG] = np.frombuffer(body[1:65], dtype=np.uint8)
                d.quant[body[0] & 15], body = table, body[65:]
        elif marker == 0xC4:
            while body:
                counts, vals, table, code, k = body[1:17], body[17:], {}, 0, 0
                for length in range(1, 17):
                    for _ in range(counts[length - 1]):
                        table[length, code], code, k = vals[k], code + 1, k + 1
                    code <<= 1
                d.huffman[body[0] >> 4, body[0] & 15], body = table, body[17 + k:]
        elif marker == 0xC0:
            assert body[0] == 8 and body[5] == 3
            d.height, d.width = int.from_bytes(body[1:3], "big"), int.from_bytes(body[3:5], "big")
            comps = [(body[6 + 3 * i], body[7 + 3 * i] >> 4, body[7 + 3 * i] & 15, body[8 + 3 * i]) for i in range(3)]
            d.sampling = tuple((h, v) for _, h, v, _ in comps)
        elif marker == 0xDD:
            d.restart_interval = int.from_bytes(body[:2], "big")
        elif marker == 0xDA:
            assert body[0] == 3 and bytes(body[7:10]) == b"\x00\x3f\x00", "not one interleaved sequential scan"
            scan = [(body[1 + 2 * i], body[2 + 2 * i] >> 4, body[2 + 2 * i] & 15) for i in range(3)]
        else:
            assert 0xE0 <= marker <= 0xEF or marker == 0xFE, f"unexpected marker {marker:02x}"
        pos += 2 + n
    assert [c[0] for c in comps] == [s[0] for s in scan]
    d.component_tables = [(c[3], s[1], s[2]) for c, s in zip(comps, scan)]
    hmax, vmax = max(h for h, _ in d.sampling), max(v for _, v in d.sampling)
    assert d.sampling[1] == d.sampling[2] == (1, 1)
    mcus = -(-d.height // (8 * vmax)) * -(-d.width // (8 * hmax))
    # split the entropy-coded data at its markers, undoing the byte stuffing
    intervals, cur = [], bytearray()
    while True:
        b = data[pos]
        if b != 0xFF:
            cur.append(b)
            pos += 1
            continue
        nxt = data[pos + 1]
        pos += 2
        if nxt == 0x00:
            cur.append(0xFF)
            d.stuffed += 1
        elif 0xD0 <= nxt <= 0xD7:
            d.rst.append(nxt - 0xD0)
            intervals.append(bytes(cur))
            cur = bytearray()
        else:
            assert nxt == 0xD9, f"marker {nxt:02x} inside the scan (fill bytes and other markers are not expected)"
            intervals.append(bytes(cur))
            break
    d.consumed = pos
    per = d.restart_interval or mcus
    assert len(intervals) == -(-mcus // per), f"{len(intervals)} intervals for {mcus} MCUs of {per}"
    out, done = [], 0
    for seg in intervals:
        bits, pred = _Bits(seg), [0, 0, 0]
        for _ in range(min(per, mcus - done)):
            for c, (h, v) in enumerate(d.sampling):
                _, dc_id, ac_id = d.component_tables[c]
                for _ in range(h * v):
                    block = np.zeros(64, dtype=np.int64)
                    size = bits.symbol(d.huffman[0, dc_id])
                    d.max_dc_category = max(d.max_dc_category, size)
                    pred[c] += _extend(bits.take(size), size)
                    block[0], k, eob = pred[c], 1, False
                    while k < 64:
                        rs = bits.symbol(d.huffman[1, ac_id])
                        run, size = rs >> 4, rs & 15
                        if size == 0:
                            if run != 15:
                                assert run == 0, "EOBn in a sequential scan"
                                eob = True
                                break
                            d.zrl += 1
                            k += 16
                            continue
                        k += run
                        assert k < 64, "run beyond the block"
                        d.max_ac_category = max(d.max_ac_category, size)
                        block[k] = _extend(bits.take(size), size)
                        k += 1
                    d.blocks_without_eob += not eob
                    out.append(block)
        done += min(per, mcus - done)
        pad = bits.left
        assert pad < 8 and bits.take(pad) == (1 << pad) - 1, "interval is not padded with 1-bits to a byte"
    d.levels = np.stack(out)
    return d


def reconstruct_444(d):
    """float64 RGB [H, W, 3] (not rounded; the YCbCr samples clipped to 0..255, the RGB not) of a decoded 4:4:4 file."""
    assert d.sampling == ((1, 1), (1, 1), (1, 1))
    my, mx = -(-d.height // 8), -(-d.width // 8)
    lv = d.levels.reshape(my, mx, 3, 64)
    planes = []
    for c in range(3):
        coeff = np.zeros((my, mx, 64))
        coeff[..., ZIGZAG] = lv[:, :, c] * d.quant[d.component_tables[c][0]][ZIGZAG]
        pix = np.einsum("ux,abuv,vy->abxy", DCT, coeff.reshape(my, mx, 8, 8), DCT) + 128.0
        # a decoder's samples are 8 bit: libjpeg range-limits the IDCT output of every component before the colour
        # conversion, which matters wherever quantisation noise overshoots (up to 32 grey levels on noise at quality 50)
        planes.append(np.clip(pix.transpose(0, 2, 1, 3).reshape(my * 8, mx * 8)[:d.height, :d.width], 0.0, 255.0))
    y, cb, cr = planes[0], planes[1] - 128.0, planes[2] - 128.0
    return np.stack([y + 1.402 * cr, y - 0.344136 * cb - 0.714136 * cr, y + 1.772 * cb], axis=-1)
