"""The independent statement of what csrc/png_decode.hip computes: an inflate written out from RFC 1951 (bit by bit, no
lookup tables, no call to zlib) that returns the status bits of include/amav.h under the same rules, the five PNG filter
reversals, and the conversion rules of PIL's convert("RGB") / convert("L").  Plain Python and NumPy."""
import numpy as np

STATUS_INFLATE, STATUS_SIZE, STATUS_FILTER = 1, 2, 4

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


class _Damaged(Exception):
    pass


class _Full(Exception):
    pass


class _Bits:
    def __init__(self, data):
        self.data, self.pos = data, 0  # pos in bits

    def bit(self):
        if self.pos >= 8 * len(self.data):
            raise _Damaged("input exhausted")
        b = (self.data[self.pos >> 3] >> (self.pos & 7)) & 1
        self.pos += 1
        return b

    def bits(self, n):  # a value: least significant bit first
        return sum(self.bit() << i for i in range(n))


def canonical(lengths):
    """Code lengths -> {(length, code): symbol} (RFC 1951 3.2.2), or None when the lengths are over-subscribed."""
    count = [0] * 16
    for n in lengths:
        count[n] += 1
    count[0], left = 0, 1
    for n in range(1, 16):
        left = 2 * left - count[n]
        if left < 0:
            return None
    code, next_code = 0, [0] * 16
    for n in range(1, 16):
        code = (code + count[n - 1]) << 1
        next_code[n] = code
    table = {}
    for sym, n in enumerate(lengths):
        if n:
            table[n, next_code[n]] = sym
            next_code[n] += 1
    return table


def _symbol(br, table):
    code = 0
    for n in range(1, 16):
        code = code << 1 | br.bit()  # Huffman codes: most significant bit first
        if (n, code) in table:
            return table[n, code]
    raise _Damaged("a code not in the set")


def inflate(data, wrapper=0, capacity=None):
    """(bytes produced, status) of one stream under the rules of include/amav.h (amav_inflate)."""
    data, out, status = bytes(data), bytearray(), 0

    def emit(chunk):
        if capacity is not None and len(out) + len(chunk) > capacity:
            raise _Full
        out.extend(chunk)

    try:
        if wrapper:
            if len(data) < 2:
                raise _Damaged("no zlib header")
            cmf, flg = data[0], data[1]
            if cmf & 15 != 8 or cmf >> 4 > 7 or (cmf << 8 | flg) % 31 or flg & 32:
                raise _Damaged("bad zlib header or FDICT")
            data = data[2:]
        br = _Bits(data)
        while True:
            last, kind = br.bit(), br.bits(2)
            if kind == 0:
                br.pos = (br.pos + 7) & ~7
                n, inverse = br.bits(16), br.bits(16)
                if n ^ 0xFFFF != inverse:
                    raise _Damaged("stored LEN != ~NLEN")
                at = br.pos >> 3
                if at + n > len(data):
                    raise _Damaged("input exhausted inside a stored block")
                for k in range(0, n, 1024):  # the kernel's chunks: what fits before the capacity stops it is the same
                    emit(data[at + k:at + min(n, k + 1024)])
                br.pos += 8 * n
            elif kind == 3:
                raise _Damaged("reserved block type")
            else:
                if kind == 1:
                    lit, dist = canonical(FIXED_LIT), canonical(FIXED_DIST)
                else:
                    hlit, hdist, hclen = br.bits(5) + 257, br.bits(5) + 1, br.bits(4) + 4
                    if hlit > 286 or hdist > 30:
                        raise _Damaged("too many length or distance codes")
                    cl = [0] * 19
                    for i in range(hclen):
                        cl[CL_ORDER[i]] = br.bits(3)
                    cl_table = canonical(cl)
                    if cl_table is None:
                        raise _Damaged("over-subscribed code-length code")
                    lengths = []
                    while len(lengths) < hlit + hdist:
                        sym = _symbol(br, cl_table)
                        if sym < 16:
                            lengths.append(sym)
                            continue
                        if sym == 16:
                            if not lengths:
                                raise _Damaged("repeat with nothing to repeat")
                            rep, value = 3 + br.bits(2), lengths[-1]
                        elif sym == 17:
                            rep, value = 3 + br.bits(3), 0
                        else:
                            rep, value = 11 + br.bits(7), 0
                        if len(lengths) + rep > hlit + hdist:
                            raise _Damaged("repeat past HLIT + HDIST")
                        lengths += [value] * rep
                    lit, dist = canonical(lengths[:hlit]), canonical(lengths[hlit:])
                    if lit is None or dist is None:
                        raise _Damaged("over-subscribed lengths")
                while True:
                    sym = _symbol(br, lit)
                    if sym < 256:
                        emit(bytes([sym]))
                    elif sym == 256:
                        break
                    else:
                        if sym >= 286:
                            raise _Damaged("length symbol 286 / 287")
                        n = LEN_BASE[sym - 257] + br.bits(LEN_EXTRA[sym - 257])
                        d = _symbol(br, dist)
                        if d >= 30:
                            raise _Damaged("distance symbol 30 / 31")
                        d = DIST_BASE[d] + br.bits(DIST_EXTRA[d])
                        if d > len(out):
                            raise _Damaged("distance before the start of the output")
                        emit(bytes(out[len(out) - d + i % d] for i in range(n)))
            if last:
                break
    except _Damaged:
        status |= STATUS_INFLATE
    except _Full:
        status |= STATUS_SIZE
    return bytes(out), status


# ------------------------------------------------------------------------------------------------------------- PNG
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}


def row_bytes(width, color_type, depth):
    return (width * CHANNELS[color_type] * depth + 7) // 8


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else (b if pb <= pc else c)


def unfilter(raw, height, width, color_type, depth):
    """The inflated bytes of a frame -> (uint8 [H, rowbytes] of unfiltered rows, status)."""
    rb = row_bytes(width, color_type, depth)
    bpp = max(1, CHANNELS[color_type] * depth // 8)
    rows, status = np.zeros((height, rb), np.uint8), 0
    raw = bytes(raw) + bytes(max(0, height * (1 + rb) - len(raw)))
    prev = [0] * rb
    for y in range(height):
        ft, line = raw[y * (1 + rb)], list(raw[y * (1 + rb) + 1:(y + 1) * (1 + rb)])
        if ft > 4:
            status, ft = status | STATUS_FILTER, 0
        for i in range(rb):
            a = line[i - bpp] if i >= bpp else 0
            b = prev[i]
            c = prev[i - bpp] if i >= bpp else 0
            p = (0, a, b, (a + b) >> 1, _paeth(a, b, c))[ft]
            line[i] = (line[i] + p) & 255
        rows[y] = prev = line
    return rows, status


def convert(rows, width, color_type, depth, palette=b"", mode="rgb"):
    """Unfiltered rows -> uint8 [H, W, 3] (mode "rgb") or [H, W] ("l") as PIL's convert gives them."""
    height = rows.shape[0]
    ch = CHANNELS[color_type]
    if depth < 8:
        bits = np.unpackbits(rows, axis=1)[:, :width * depth].reshape(height, width, depth)  # most significant bit first
        samples = (bits.astype(np.uint32) << np.arange(depth - 1, -1, -1, dtype=np.uint32)).sum(-1)[..., None]
    else:
        samples = rows[:, :width * ch].reshape(height, width, ch).astype(np.uint32)
    if color_type in (0, 4):
        grey = samples[..., 0] * (255 // ((1 << depth) - 1))
        return (grey if mode == "l" else np.repeat(grey[..., None], 3, -1)).astype(np.uint8)
    if color_type == 3:
        entries = len(palette) // 3
        table = np.zeros((256, 3), np.uint32)
        table[:entries] = np.frombuffer(bytes(palette[:3 * entries]), np.uint8).reshape(-1, 3)
        rgb = table[samples[..., 0]]  # an index at or beyond the palette: (0, 0, 0)
    else:
        rgb = samples[..., :3]
    if mode == "l":
        return ((19595 * rgb[..., 0] + 38470 * rgb[..., 1] + 7471 * rgb[..., 2] + 0x8000) >> 16).astype(np.uint8)
    return rgb.astype(np.uint8)


def decode(zlib_stream, height, width, color_type, depth, palette=b"", mode="rgb"):
    """One frame as amav_png_decode decodes it: (pixels, status)."""
    need = height * (1 + row_bytes(width, color_type, depth))
    raw, status = inflate(zlib_stream, wrapper=1, capacity=need)
    if len(raw) != need:
        status |= STATUS_SIZE
    if status:  # not unfiltered: the pixels are 0
        return np.zeros((height, width, 3) if mode == "rgb" else (height, width), np.uint8), status
    rows, filter_status = unfilter(raw, height, width, color_type, depth)
    return convert(rows, width, color_type, depth, palette, mode), status | filter_status
