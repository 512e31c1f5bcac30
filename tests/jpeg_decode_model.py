"""The pixel rules include/amav.h states for amav_jpeg_decode, restated in numpy (float64, or float32 to see what the
format costs) on top of jpeg_model's pure-Python scan decoder: 4:4:4, 4:2:0 and one component.
tests/test_jpeg_decode_model.py pins this model against libjpeg (through Pillow) on the fixtures of
tests/golden/jpeg_decode/; tests/test_jpeg_decode_gpu.py holds the HIP decoder against it.

    decode(jpeg_bytes)                 -> jpeg_model.Decoded (jpeg_model.decode, plus files of one component)
    sampling_name(decoded)             -> "444" | "420" | "gray"
    reconstruct(decoded, dtype)        -> (rgb [H, W, 3] not rounded, delta [H, W, 3]): the stated chain evaluated in
                                          `dtype`, and a bound on what evaluating it in fp32 can move each sample
    to_uint8(rgb)                      -> round to nearest, clamp to 0..255
"""
import numpy as np

import jpeg_model as jm

U = 2.0 ** -24  # unit roundoff of fp32


def _decode_gray(data):
    """jpeg_model.decode for a file of one component (its scan is not interleaved: one 8x8 block per MCU)."""
    d = jm.Decoded()
    assert data[:2] == b"\xff\xd8", "no SOI"
    pos, comp, scan = 2, None, None
    while scan is None:
        assert data[pos] == 0xFF and data[pos + 1] not in (0x00, 0xFF), f"marker expected at {pos}"
        marker, n = data[pos + 1], int.from_bytes(data[pos + 2:pos + 4], "big")
        body = data[pos + 4:pos + 2 + n]
        d.segments.append(marker)
        if marker == 0xDB:
            while body:
                assert body[0] >> 4 == 0
                table = np.zeros(64, dtype=np.int64)
                table[jm.ZIGZAG] = np.frombuffer(body[1:65], dtype=np.uint8)
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
            assert body[0] == 8 and body[5] == 1
            d.height, d.width = int.from_bytes(body[1:3], "big"), int.from_bytes(body[3:5], "big")
            comp = (body[6], body[8])
            d.sampling = ((1, 1),)
        elif marker == 0xDD:
            d.restart_interval = int.from_bytes(body[:2], "big")
        elif marker == 0xDA:
            assert body[0] == 1 and bytes(body[3:6]) == b"\x00\x3f\x00" and body[1] == comp[0]
            scan = (body[2] >> 4, body[2] & 15)
        else:
            assert 0xE0 <= marker <= 0xEF or marker == 0xFE, f"unexpected marker {marker:02x}"
        pos += 2 + n
    d.component_tables = [(comp[1], scan[0], scan[1])]
    mcus = -(-d.height // 8) * -(-d.width // 8)
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
            assert nxt == 0xD9
            intervals.append(bytes(cur))
            break
    d.consumed = pos
    per = d.restart_interval or mcus
    assert len(intervals) == -(-mcus // per)
    out, done = [], 0
    for seg in intervals:
        bits, pred = jm._Bits(seg), 0
        for _ in range(min(per, mcus - done)):
            block = np.zeros(64, dtype=np.int64)
            size = bits.symbol(d.huffman[0, scan[0]])
            d.max_dc_category = max(d.max_dc_category, size)
            pred += jm._extend(bits.take(size), size)
            block[0], k, eob = pred, 1, False
            while k < 64:
                rs = bits.symbol(d.huffman[1, scan[1]])
                run, size = rs >> 4, rs & 15
                if size == 0:
                    if run != 15:
                        assert run == 0
                        eob = True
                        break
                    d.zrl += 1
                    k += 16
                    continue
                k += run
                assert k < 64
                d.max_ac_category = max(d.max_ac_category, size)
                block[k] = jm._extend(bits.take(size), size)
                k += 1
            d.blocks_without_eob += not eob
            out.append(block)
        done += min(per, mcus - done)
    d.levels = np.stack(out)
    return d


def decode(data):
    data = bytes(data)
    at = data.index(b"\xff\xc0")
    return _decode_gray(data) if data[at + 9] == 1 else jm.decode(data)


def sampling_name(d):
    return {((1, 1),): "gray", ((1, 1),) * 3: "444", ((2, 2), (1, 1), (1, 1)): "420"}[tuple(d.sampling)]


def _component_planes(d, dtype):
    """Per component: (samples after dequantisation, IDCT, + 128 and the clamp to [0, 255], on whole blocks;
    the fp32 error bound of each sample).  4:2:0 luma blocks are put back in raster order."""
    name = sampling_name(d)
    mcu = 16 if name == "420" else 8
    my, mx = -(-d.height // mcu), -(-d.width // mcu)
    bpm = {"gray": 1, "444": 3, "420": 6}[name]
    lv = d.levels.reshape(my, mx, bpm, 64)
    basis, absbasis = jm.DCT.astype(dtype), np.abs(jm.DCT)
    out = []
    for c in range(len(d.sampling)):
        if name == "420" and c == 0:
            blocks = lv[:, :, :4].reshape(my, mx, 2, 2, 64).transpose(0, 2, 1, 3, 4).reshape(my * 2, mx * 2, 64)
        else:
            blocks = lv[:, :, (c + 3 if name == "420" else c)]
        by, bx = blocks.shape[:2]
        coeff = np.zeros((by, bx, 64))
        coeff[..., jm.ZIGZAG] = blocks * d.quant[d.component_tables[c][0]][jm.ZIGZAG]
        assert np.abs(coeff).max() < 2 ** 24, "level x table entry is exact in fp32"
        coeff = coeff.reshape(by, bx, 8, 8)
        # u: vertical frequency -> x: row; the vertical pass first, as the kernel has it
        cols = np.einsum("ux,abuv->abxv", basis, coeff.astype(dtype)).astype(dtype)
        pix = np.einsum("abxv,vy->abxy", cols, basis).astype(dtype) + dtype(128.0)
        pix = np.clip(pix, dtype(0.0), dtype(255.0))
        # every sample is a sum over |basis| |coefficient| |basis| = S of terms that each pass through at most 9 fp32
        # roundings per pass (the constant, the product, 7 additions in any order), and the second pass also carries the
        # first one's error: 18 U S, taken as 19 U S for the second-order terms; + 128 adds one rounding of at most S + 128
        S = np.einsum("ux,abuv,vy->abxy", absbasis, np.abs(coeff), absbasis)
        err = 19 * U * S + U * (S + 128.0)
        flat = lambda a: a.transpose(0, 2, 1, 3).reshape(by * 8, bx * 8)  # noqa: E731
        out.append((flat(pix), flat(err)))
    return out


def _triangle(plane, H, W, dtype):
    """[ceil(H/2), ceil(W/2)] -> [H, W]: 3/4 of the nearer sample + 1/4 of the farther, vertically then horizontally,
    neighbours clamped at the plane's edge."""
    y, x = np.arange(H), np.arange(W)
    cy, cx = y >> 1, x >> 1
    ny = np.clip(cy + np.where(y & 1, 1, -1), 0, plane.shape[0] - 1)
    nx = np.clip(cx + np.where(x & 1, 1, -1), 0, plane.shape[1] - 1)
    a, b = dtype(0.75), dtype(0.25)
    rows = (a * plane[cy] + b * plane[ny]).astype(dtype)
    return (a * rows[:, cx] + b * rows[:, nx]).astype(dtype)


def reconstruct(d, dtype=np.float64):
    """(rgb [H, W, 3] in `dtype`, not rounded and not clamped; delta [H, W, 3] float64).  delta bounds how far an fp32
    evaluation of the chain (in any order of additions, fused or not) can be from the exact value:
        component sample   e = 20 U S + 128 U                      (see _component_planes)
        4:2:0 chroma       e' = triangle(e) + 4 U 255              (weights exact; two stages of two roundings <= 255 U)
        Cb', Cr'           one rounding each: 128 U
        colour             e_Y + sum_c k_c (e'_c + 128 U) + 4 U (255 + 128 sum_c k_c): the constant k_c, the product
                           and the additions are at most four roundings of values bounded by 255 + 128 sum k_c."""
    dtype = np.dtype(dtype).type
    H, W, name = d.height, d.width, sampling_name(d)
    planes = _component_planes(d, dtype)
    Y, eY = planes[0][0][:H, :W], planes[0][1][:H, :W]
    if name == "gray":
        return np.stack([Y, Y, Y], axis=-1), np.stack([eY, eY, eY], axis=-1)
    chroma = []
    for pix, err in planes[1:]:
        if name == "420":
            h2, w2 = -(-H // 2), -(-W // 2)
            pix = _triangle(pix[:h2, :w2], H, W, dtype)
            err = _triangle(err[:h2, :w2], H, W, np.float64) + 4 * U * 255.0
        else:
            pix, err = pix[:H, :W], err[:H, :W]
        chroma.append(((pix - dtype(128.0)).astype(dtype), err + 128.0 * U))
    (cb, ecb), (cr, ecr) = chroma
    k = dtype
    rgb = np.stack([Y + k(1.402) * cr, Y - k(0.344136) * cb - k(0.714136) * cr, Y + k(1.772) * cb], axis=-1).astype(dtype)
    delta = np.stack([eY + kcb * ecb + kcr * ecr + 4 * U * (255.0 + 128.0 * (kcb + kcr))
                      for kcb, kcr in ((0.0, 1.402), (0.344136, 0.714136), (1.772, 0.0))], axis=-1)
    return rgb, delta


def to_uint8(rgb):
    return np.clip(np.rint(rgb.astype(np.float64)), 0, 255).astype(np.uint8)


def disagreement(got_u8, rgb, delta):
    """(largest |got - rint(model)|, samples that differ where the model is decided, share of undecided samples)."""
    rgb = rgb.astype(np.float64)
    want = to_uint8(rgb)
    diff = np.abs(got_u8.astype(np.int64) - want.astype(np.int64))
    open_ = jm.undecided(rgb, delta)
    return int(diff.max()), int(np.count_nonzero((diff > 0) & ~open_)), float(open_.mean())
