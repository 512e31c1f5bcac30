"""Writers and case lists shared by the PNG / inflate tests: a bit writer, fixed- and dynamic-Huffman block writers (code
lengths in, RFC 1951 3.2.7 header out), a PNG writer that forces a filter type per row and splits IDAT at given sizes,
the sound DEFLATE streams and the damaged ones.  Everything is generated from seeds; zlib is used as a compressor and
as the oracle, never inside the writers' own blocks."""
import functools
import json
import os
import struct
import zlib

import numpy as np

import png_model as pm


# ------------------------------------------------------------------------------------------------------- writers
class BitWriter:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def bits(self, value, n):  # a value: least significant bit first
        self.acc |= (value & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, n):  # a Huffman code: most significant bit first
        for i in range(n - 1, -1, -1):
            self.bits((code >> i) & 1, 1)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def bytes(self):
        assert self.n == 0, "align() first"
        return bytes(self.out)


def codes_of(lengths):
    """Code lengths -> {symbol: (code, length)}, canonical (RFC 1951 3.2.2)."""
    table = pm.canonical(lengths)
    assert table is not None, "over-subscribed"
    return {sym: (code, n) for (n, code), sym in table.items()}


def match(length, distance):
    """(length symbol, extra value, distance symbol, extra value) the usual way: the last base not above the value."""
    ls = 28 if length == 258 else max(i for i in range(28) if pm.LEN_BASE[i] <= length)
    ds = max(i for i in range(30) if pm.DIST_BASE[i] <= distance)
    return ("m", 257 + ls, length - pm.LEN_BASE[ls], ds, distance - pm.DIST_BASE[ds])


def put_tokens(bw, tokens, lit, dist):
    """tokens: an int literal, ("m", length symbol, extra, distance symbol, extra), or ("s", symbol) for a bare
    literal/length symbol; then the end-of-block code."""
    for t in tokens:
        if isinstance(t, (int, np.integer)):
            bw.code(*lit[int(t)])
        elif t[0] == "s":
            bw.code(*lit[t[1]])
        else:
            _, ls, le, ds, de = t
            bw.code(*lit[ls])
            if ls - 257 < 29:
                bw.bits(le, pm.LEN_EXTRA[ls - 257])
            bw.code(*dist[ds])
            if ds < 30:
                bw.bits(de, pm.DIST_EXTRA[ds])
    bw.code(*lit[256])


FIXED_LIT, FIXED_DIST = codes_of(pm.FIXED_LIT), codes_of(pm.FIXED_DIST)


def fixed_block(bw, tokens, last=True):
    bw.bits(int(last), 1)
    bw.bits(1, 2)
    put_tokens(bw, tokens, FIXED_LIT, FIXED_DIST)


def stored_block(bw, payload, last=True, nlen=None):
    bw.bits(int(last), 1)
    bw.bits(0, 2)
    bw.align()
    bw.bits(len(payload), 16)
    bw.bits(len(payload) ^ 0xFFFF if nlen is None else nlen, 16)
    bw.out += payload


def _complete_lengths(k):
    """k >= 2 code lengths that fill the code space exactly."""
    top = max(1, (k - 1).bit_length())
    short = (1 << top) - k
    return [top - 1] * short + [top] * (k - short)


def dynamic_header(bw, lit_lengths, dist_lengths, last=True, ops=None, hclen=None):
    """BTYPE 2 header for the given code lengths.  ops: the code-length symbols to send as (symbol, extra value) pairs;
    default: a greedy run-length coding of the joined lengths, whose runs cross from HLIT into HDIST where the values
    allow.  Returns the (symbol, first index, count) list that was sent."""
    joined = list(lit_lengths) + list(dist_lengths)
    if ops is None:
        ops, i = [], 0
        while i < len(joined):
            v, run = joined[i], 1
            while i + run < len(joined) and joined[i + run] == v:
                run += 1
            if v == 0 and run >= 3:
                n = min(run, 138)
                ops.append((18, n - 11) if n >= 11 else (17, n - 3))
                i += n
            elif v and run >= 4:
                ops.append((v, 0))
                n = min(run - 1, 6)
                ops.append((16, n - 3))
                i += 1 + n
            else:
                ops.append((v, 0))
                i += 1
    used = sorted({s for s, _ in ops} | {0, 18})  # at least two symbols, so that the code is complete
    cl = [0] * 19
    for s, n in zip(used, _complete_lengths(len(used))):
        cl[s] = n
    sent_cl = max(i for i in range(19) if cl[pm.CL_ORDER[i]]) + 1 if hclen is None else hclen
    sent_cl = max(4, sent_cl)
    bw.bits(int(last), 1)
    bw.bits(2, 2)
    bw.bits(len(lit_lengths) - 257, 5)
    bw.bits(len(dist_lengths) - 1, 5)
    bw.bits(sent_cl - 4, 4)
    for i in range(sent_cl):
        bw.bits(cl[pm.CL_ORDER[i]], 3)
    cl_codes = codes_of(cl)
    sent, at = [], 0
    for s, e in ops:
        bw.code(*cl_codes[s])
        n = 1
        if s == 16:
            bw.bits(e, 2)
            n = 3 + e
        elif s == 17:
            bw.bits(e, 3)
            n = 3 + e
        elif s == 18:
            bw.bits(e, 7)
            n = 11 + e
        sent.append((s, at, n))
        at += n
    return sent, sent_cl


def dynamic_block(bw, tokens, lit_lengths, dist_lengths, last=True, **kw):
    info = dynamic_header(bw, lit_lengths, dist_lengths, last, **kw)
    put_tokens(bw, tokens, codes_of(lit_lengths), codes_of(dist_lengths) if any(dist_lengths) else {})
    return info


def finish(bw):
    bw.align()
    return bw.bytes()


def _chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body))


def filter_rows(rows, filters, bpp):
    """uint8 [H, rowbytes] -> the filtered byte string with filters[y % len(filters)] forced on row y."""
    H, rb = rows.shape
    out, prev = bytearray(), np.zeros(rb, np.int32)
    for y in range(H):
        ft, cur = filters[y % len(filters)], rows[y].astype(np.int32)
        left = np.concatenate([np.zeros(bpp, np.int32), cur[:-bpp]]) if rb > bpp else np.zeros(rb, np.int32)
        upleft = np.concatenate([np.zeros(bpp, np.int32), prev[:-bpp]]) if rb > bpp else np.zeros(rb, np.int32)
        if ft == 0:
            pred = np.zeros(rb, np.int32)
        elif ft == 1:
            pred = left
        elif ft == 2:
            pred = prev
        elif ft == 3:
            pred = (left + prev) >> 1
        else:
            p = left + prev - upleft
            pa, pb, pc = abs(p - left), abs(p - prev), abs(p - upleft)
            pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, prev, upleft))
        out.append(ft)
        out += ((cur - pred) & 255).astype(np.uint8).tobytes()
        prev = cur
    return bytes(out)


def pack_rows(samples, depth):
    """uint8 [H, W, channels] samples (< 2^depth) -> uint8 [H, rowbytes], most significant bits first."""
    H, W, ch = samples.shape
    if depth == 8:
        return samples.reshape(H, W * ch).copy()
    bits = ((samples.reshape(H, W)[..., None] >> np.arange(depth - 1, -1, -1)) & 1).astype(np.uint8).reshape(H, W * depth)
    return np.packbits(bits, axis=1)


def write_png(samples, color_type, depth, filters=(0,), idat=None, palette=None, trns=None, level=6, extra=(),
              raw_override=None):
    """A PNG file of `samples` (uint8 [H, W, channels of the colour type]).  filters: forced per row, cyclically.
    idat: payload bytes per IDAT chunk (None: one chunk).  raw_override: filtered bytes to compress instead."""
    H, W, _ = samples.shape
    rows = pack_rows(samples, depth)
    bpp = max(1, pm.CHANNELS[color_type] * depth // 8)
    raw = filter_rows(rows, filters, bpp) if raw_override is None else raw_override
    z = zlib.compress(raw, level)
    out = pm_signature() + _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, depth, color_type, 0, 0, 0))
    for kind, body in extra:
        out += _chunk(kind, body)
    if palette is not None:
        out += _chunk(b"PLTE", bytes(palette))
    if trns is not None:
        out += _chunk(b"tRNS", bytes(trns))
    step = len(z) if idat is None else idat
    for at in range(0, len(z), max(1, step)):
        out += _chunk(b"IDAT", z[at:at + step])
    return out + _chunk(b"IEND", b"")


def pm_signature():
    return b"\x89PNG\r\n\x1a\n"


def random_samples(rng, H, W, color_type, depth):
    ch = pm.CHANNELS[color_type]
    if depth == 8 and H * W >= 64:  # smooth + noise, so that the filters see structure
        yy, xx = np.mgrid[0:H, 0:W]
        base = (3 * xx + 5 * yy)[..., None] + 40 * np.arange(ch)
        return ((base + rng.integers(0, 24, (H, W, ch))) & 255).astype(np.uint8)
    return rng.integers(0, 1 << depth, (H, W, ch)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------- sound streams
def _rng(seed):
    return np.random.default_rng(seed)


def _data_sets():
    rng = _rng(11)
    noise = rng.integers(0, 16, 70000).astype(np.uint8).tobytes()
    block = rng.integers(0, 256, 20000).astype(np.uint8).tobytes()
    far = (block + block + block + block)[:70000]  # repeats 20 000 bytes apart
    return {"one": b"\x5a", "zeros300": bytes(300), "noise70k": noise, "far70k": far}


def _compress(data, level, strategy, wbits, flush_at=None):
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, 9, strategy)
    if flush_at is None:
        return c.compress(data) + c.flush()
    return c.compress(data[:flush_at]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(data[flush_at:]) + c.flush()


def literals_15_bits():
    """Code lengths 1, 2, ... 14, 15, 15 over sixteen symbols (fifteen literals and the end-of-block): a complete code
    with two codes of the maximum length; the end-of-block takes one of the 15-bit codes."""
    lit = [0] * 257
    for i, s in enumerate(list(range(65, 80)) + [256]):
        lit[s] = min(i + 1, 15)
    return lit


def ring_wrap_tokens():
    """32 700 literals, then: a match whose destination 32 700..32 900 straddles output offset 32 768 (where the 32 KiB
    ring wraps); a match at 32 900 whose source 32 600..32 858 straddles it; a match of distance 32 748 at 33 158, whose
    destination bytes fall on the ring slots of source bytes 20 places on; a short-period match after the wrap."""
    return _rng(8).integers(0, 256, 32700).tolist() + [match(200, 150), match(258, 300), match(258, 32768 - 20), match(100, 140)]


def match_spans(tokens):
    """[(destination begin, end, source begin, end)] of the matches of `tokens`, in output offsets; the source range is
    what is read: min(length, distance) bytes from the distance back."""
    spans, at = [], 0
    for t in tokens:
        if isinstance(t, (int, np.integer)):
            at += 1
            continue
        length = pm.LEN_BASE[t[1] - 257] + t[2]
        distance = pm.DIST_BASE[t[3]] + t[4]
        spans.append((at, at + length, at - distance, at - distance + min(length, distance)))
        at += length
    return spans


@functools.lru_cache(maxsize=None)
def sound_streams():
    """[(name, stream, wrapper)]: every stream here decodes with zlib, which is the oracle."""
    cases = []
    # stored blocks
    bw = BitWriter()
    stored_block(bw, b"")
    cases.append(("stored_len0", finish(bw), 0))
    rng = _rng(5)
    for n in (1, 65535):
        bw = BitWriter()
        stored_block(bw, rng.integers(0, 256, n).astype(np.uint8).tobytes())
        cases.append((f"stored_{n}", finish(bw), 0))
    bw = BitWriter()
    stored_block(bw, b"first stored block", last=False)
    fixed_block(bw, list(b"abc") + [match(5, 3)], last=False)  # ends off a byte boundary
    stored_block(bw, b"second stored block")
    cases.append(("stored_huffman_stored", finish(bw), 0))
    # zlib's own output
    strategies = {"fixed": zlib.Z_FIXED, "huffman": zlib.Z_HUFFMAN_ONLY, "rle": zlib.Z_RLE, "default": zlib.Z_DEFAULT_STRATEGY}
    data = _data_sets()
    for s in strategies:  # the whole product: strategy x level x wrapper x data set, each plain and with a full flush
        for level in (1, 6, 9):
            for wbits in (-15, 15):
                for dname, d in data.items():
                    for flush_at in (None, len(d) // 2):
                        name = f"zlib_{s}_l{level}_{'raw' if wbits < 0 else 'zlib'}_{dname}{'_flush' if flush_at is not None else ''}"
                        cases.append((name, _compress(d, level, strategies[s], wbits, flush_at), int(wbits > 0)))
    # hand-written fixed-Huffman streams
    lits = _rng(6).integers(0, 256, 32768).tolist()
    bw = BitWriter()
    fixed_block(bw, lits + [match(258, 32768), match(258, 1), match(3, 32768)])
    cases.append(("fixed_far_window", finish(bw), 0))
    tokens = _rng(7).integers(0, 256, 32768).tolist()
    for i in range(29):  # every length code at its smallest and largest extra value
        for e in {0, (1 << pm.LEN_EXTRA[i]) - 1}:
            tokens.append(("m", 257 + i, e, 6, 1))
    for d in range(30):  # every distance code likewise
        for e in {0, (1 << pm.DIST_EXTRA[d]) - 1}:
            tokens.append(("m", 257 + 4, 0, d, e))
    bw = BitWriter()
    fixed_block(bw, tokens)
    cases.append(("fixed_every_code", finish(bw), 0))
    bw = BitWriter()
    fixed_block(bw, ring_wrap_tokens())
    cases.append(("fixed_ring_wrap", finish(bw), 0))
    # hand-written dynamic blocks
    cases.extend((n, s, 0) for n, s, _ in dynamic_cases())
    return cases


@functools.lru_cache(maxsize=None)
def dynamic_cases():
    """[(name, stream, header info)] of the hand-written dynamic blocks; info = (ops sent, HCLEN sent, HLIT)."""
    out = []
    # repeat code 16 across the boundary: fourteen 4-bit and four 5-bit literal/length codes, the last three symbols of
    # HLIT 4 bits long, then sixteen 4-bit distance codes
    lit = [0] * 260
    for s in list(range(97, 107)) + [256, 257, 258, 259]:
        lit[s] = 4
    for s in (48, 49, 50, 51):
        lit[s] = 5
    bw = BitWriter()
    info = dynamic_block(bw, list(b"abcdefghij0123") + [("m", 257, 0, 3, 0), ("m", 259, 0, 5, 1)] * 3, lit, [4] * 16)
    out.append(("dynamic_repeat16_crosses", finish(bw), info + (260,)))
    # repeat code 17 across it: two zero lengths end HLIT, two begin HDIST
    lit = [0] * 259
    lit[120], lit[256] = 1, 1
    bw = BitWriter()
    info = dynamic_block(bw, [120] * 9, lit, [0, 0, 1, 1])
    out.append(("dynamic_repeat17_crosses", finish(bw), info + (259,)))
    # repeat code 18 across it: HLIT 286 with 28 zero lengths at its end, six zero distance lengths, two codes of 1 bit
    lit = [0] * 286
    lit[65], lit[66], lit[256], lit[257] = 2, 2, 2, 2
    bw = BitWriter()
    info = dynamic_block(bw, [65, 66] * 6 + [("m", 257, 0, 6, 0), ("m", 257, 0, 7, 1)], lit, [0] * 6 + [1, 1])
    out.append(("dynamic_repeat18_crosses", finish(bw), info + (286,)))
    # a single distance code of length 1
    lit = [0] * 258
    lit[65], lit[66], lit[256], lit[257] = 2, 2, 2, 2
    bw = BitWriter()
    info = dynamic_block(bw, [65, 66, ("m", 257, 0, 0, 0), 66, ("m", 257, 0, 0, 0)], lit, [1])
    out.append(("dynamic_single_distance_code", finish(bw), info + (258,)))
    # no distance codes: literals only, one zero-length distance code
    lit = [0] * 257
    lit[65], lit[66], lit[67], lit[256] = 2, 2, 2, 2
    bw = BitWriter()
    info = dynamic_block(bw, [65, 66, 67, 67, 66, 65], lit, [0])
    out.append(("dynamic_no_distance_codes", finish(bw), info + (257,)))
    # a 15-bit literal/length code; code-length symbol 15 is the last of the transmission order: HCLEN 19
    bw = BitWriter()
    info = dynamic_block(bw, list(range(65, 80)) * 3, literals_15_bits(), [0])
    out.append(("dynamic_15_bit_code_hclen19", finish(bw), info + (257,)))
    # 255 literals and the end-of-block, 8 bits each: only code-length symbols 0, 8 and repeats are used: HCLEN 5, the
    # smallest that can describe a literal/length code at all (HCLEN 4 sends 16, 17, 18 and 0: every length is zero)
    lit = [8] * 255 + [0, 8]
    bw = BitWriter()
    info = dynamic_block(bw, list(range(255)) + [7, 7, 7], lit, [0])
    out.append(("dynamic_hclen5", finish(bw), info + (257,)))
    return out


# ----------------------------------------------------------------------------------------------- damaged streams
def cut_stream():
    """A 200-byte raw stream: a stored block, then a dynamic block, 400 bytes out.  The stored payload is sized so that
    the whole comes to 200 bytes."""
    rng = _rng(21)
    tail = (rng.integers(0, 7, 300) * 9).astype(np.uint8).tobytes()
    c = zlib.compressobj(9, zlib.DEFLATED, -15)
    huff = c.compress(tail) + c.flush()
    assert huff[0] & 6 == 4, "the second block must be dynamic"
    n = 200 - 5 - len(huff)
    assert 40 <= n <= 100, n
    bw = BitWriter()
    stored_block(bw, rng.integers(0, 256, n).astype(np.uint8).tobytes(), last=False)
    stream = finish(bw) + huff
    assert len(stream) == 200
    return stream, n


CUTS = (1, 3, 30, None, None, 150, 198, 199)  # None: filled in from the stored length (inside the dynamic header)


@functools.lru_cache(maxsize=None)
def damaged_streams():
    """[(name, raw-or-zlib stream, wrapper, capacity or None, the status bit it must raise)].  Each is rejected by
    zlib.decompress (an exception, or for the capacity case more bytes than fit).  None of them makes more than 400
    bytes before it is stopped."""
    I, S = pm.STATUS_INFLATE, pm.STATUS_SIZE
    out = []
    bw = BitWriter()
    fixed_block(bw, list(b"fine so far"), last=False)
    bw.bits(1, 1)
    bw.bits(3, 2)
    bw.bits(0, 13)
    out.append(("block_type_3", finish(bw), 0, None, I))
    bw = BitWriter()
    stored_block(bw, b"twelve bytes", nlen=12 ^ 0xFFFE)
    out.append(("len_nlen_mismatch", finish(bw), 0, None, I))

    def header_only(lit, dist, ops=None, tail_bits=64):
        bw = BitWriter()
        dynamic_header(bw, lit, dist, ops=ops)
        bw.bits(0, tail_bits)
        return finish(bw)

    lit = [0] * 257
    lit[65], lit[66], lit[67], lit[256] = 1, 1, 2, 2  # 1/2 + 1/2 + 1/4 + 1/4
    out.append(("oversubscribed_lengths", header_only(lit, [0]), 0, None, I))
    out.append(("repeat_without_predecessor", header_only([0] * 257, [0], ops=[(16, 0)] + [(0, 0)] * 255), 0, None, I))
    out.append(("repeat_overruns", header_only([0] * 257, [0], ops=[(8, 0)] + [(18, 127)] + [(18, 127)]), 0, None, I))
    # HCLEN 4: the code-length code has 16, 17, 18 and 0 only, so every length is zero and nothing can be decoded
    out.append(("hclen4_all_zero", _hclen4(), 0, None, I))
    for sym in (286, 287):
        bw = BitWriter()
        fixed_block(bw, [65, 66, ("s", sym), 67])
        out.append((f"length_symbol_{sym}", finish(bw), 0, None, I))
    for d in (30, 31):
        bw = BitWriter()
        fixed_block(bw, [65, 66, 67, ("m", 257, 0, d, 0), 68])
        out.append((f"distance_symbol_{d}", finish(bw), 0, None, I))
    bw = BitWriter()
    fixed_block(bw, [match(3, 1), 65])
    out.append(("first_symbol_is_a_match", finish(bw), 0, None, I))
    bw = BitWriter()
    fixed_block(bw, list(b"0123456789") + [match(4, 11)])
    out.append(("distance_one_too_far", finish(bw), 0, None, I))
    stream, n = cut_stream()
    cuts = list(CUTS)
    cuts[3], cuts[4] = 5 + n + 2, 5 + n + 12  # the dynamic header starts at byte 5 + n
    for at in cuts:
        out.append((f"cut_at_{at}", stream[:at], 0, None, I))
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    out.append(("zeros300_into_100", c.compress(bytes(300)) + c.flush(), 0, 100, S))
    good = zlib.compress(b"a sound stream under a bad header")
    out.append(("bad_zlib_method", bytes([0x79, 0x9C]) + good[2:], 1, None, I))
    out.append(("bad_zlib_check", bytes([0x78, 0x9D]) + good[2:], 1, None, I))
    out.append(("fdict_set", bytes([0x78, 0xBB]) + good[2:], 1, None, I))
    return out


def _hclen4():
    bw = BitWriter()
    bw.bits(1, 1)
    bw.bits(2, 2)
    bw.bits(0, 5)
    bw.bits(0, 5)
    bw.bits(0, 4)  # HCLEN 4
    for n in (0, 0, 1, 1):  # lengths of 16, 17, 18, 0
        bw.bits(n, 3)
    bw.code(1, 1)  # 18 (symbol 0 has code 0): 138 zeros
    bw.bits(127, 7)
    bw.code(1, 1)  # 18: 120 zeros -> 258 lengths
    bw.bits(109, 7)
    bw.bits(0, 64)
    return finish(bw)


def zlib_rejects(stream, wrapper, capacity):
    try:
        data = zlib.decompress(stream, 15 if wrapper else -15)
    except zlib.error:
        return True
    return capacity is not None and len(data) > capacity


# --------------------------------------------------------------------------------------------------- PNG frames
SIZES = [(1, 1), (1, 7), (9, 7), (65, 13), (3, 300), (130, 70)]
KINDS = [(0, 1), (0, 2), (0, 4), (0, 8), (2, 8), (3, 1), (3, 2), (3, 4), (3, 8), (4, 8), (6, 8)]
FILTER_SETS = [(0,), (1,), (2,), (3,), (4,), (0, 1, 2, 3, 4, 4, 3, 1)]


def make_palette(rng, depth):
    entries = 1 << depth
    return rng.integers(0, 256, 3 * entries).astype(np.uint8).tobytes()


@functools.lru_cache(maxsize=None)
def png_files():
    """[(name, file bytes)]: every size with every colour type / depth under a rotating filter set and IDAT split, and
    every filter set and split on every colour type at (9, 7) and (65, 13)."""
    rng, files, k = _rng(31), [], 0
    for H, W in SIZES:
        for ct, depth in KINDS:
            sets = FILTER_SETS if (H, W) in ((9, 7), (65, 13)) else [FILTER_SETS[k % len(FILTER_SETS)]]
            for filters in sets:
                k += 1
                samples = random_samples(rng, H, W, ct, depth)
                palette = make_palette(rng, depth) if ct == 3 else None
                trns = (bytes(rng.integers(0, 256, 3).tolist()) if ct == 3 else None)
                idat = (None, 100, 1)[k % 3]
                name = f"{H}x{W}_t{ct}d{depth}_f{''.join(map(str, filters))}_idat{idat}"
                files.append((name, write_png(samples, ct, depth, filters, idat, palette, trns, level=(1, 6, 9)[k % 3])))
    return files


def pillow_decode(data, mode):
    import io

    from PIL import Image

    return np.array(Image.open(io.BytesIO(data)).convert({"rgb": "RGB", "l": "L"}[mode]))


@functools.lru_cache(maxsize=None)
def pillow_files():
    """Files written by Pillow itself: a 64 x 48 gradient-plus-noise image and a binary mask as "1", "L" and "P", each
    at the default settings and with optimize=True."""
    import io

    from PIL import Image

    rng = _rng(41)
    yy, xx = np.mgrid[0:48, 0:64]
    rgb = ((np.stack([4 * xx, 5 * yy, 2 * (xx + yy)], -1) + rng.integers(0, 16, (48, 64, 3))) & 255).astype(np.uint8)
    mask = (((xx - 30) ** 2 + (yy - 20) ** 2) < 300).astype(np.uint8) * 255
    images = {"rgb": Image.fromarray(rgb), "mask_1": Image.fromarray(mask).convert("1"), "mask_L": Image.fromarray(mask),
              "mask_P": Image.fromarray(mask).convert("P")}
    files = []
    for name, im in images.items():
        for optimize in (False, True):
            buf = io.BytesIO()
            im.save(buf, "PNG", optimize=optimize)
            files.append((f"pillow_{name}{'_opt' if optimize else ''}", buf.getvalue()))
    return files


DAMAGED_H, DAMAGED_W = 16, 24  # grey, 8 bits: 16 x (1 + 24) = 400 bytes per frame


@functools.lru_cache(maxsize=None)
def damaged_frames():
    """[(name, zlib stream of a 16 x 24 grey frame, the status bit it must raise)]: every damaged stream above under a
    zlib header, and the PNG-level cases: a stream one row short, one three times too long, a filter byte 5."""
    frames = []
    for name, stream, wrapper, capacity, bit in damaged_streams():
        if capacity is not None:
            continue  # the capacity case is taken again below, at the frame's own size
        frames.append((name, stream if wrapper else b"\x78\x9c" + stream, bit))
    rng = _rng(51)
    rows = rng.integers(0, 256, (DAMAGED_H, DAMAGED_W)).astype(np.uint8)
    raw = filter_rows(rows, (0, 1, 2, 3, 4), 1)
    frames.append(("one_row_short", zlib.compress(raw[:-(1 + DAMAGED_W)]), pm.STATUS_SIZE))
    frames.append(("too_many_bytes", zlib.compress(bytes(3 * len(raw))), pm.STATUS_SIZE))
    bad = bytearray(raw)
    bad[3 * (1 + DAMAGED_W)] = 5
    frames.append(("filter_byte_5", zlib.compress(bytes(bad)), pm.STATUS_FILTER))
    return frames


def sound_frame(seed):
    """(zlib stream, pixels) of a sound 16 x 24 grey frame."""
    rows = _rng(seed).integers(0, 256, (DAMAGED_H, DAMAGED_W)).astype(np.uint8)
    return zlib.compress(filter_rows(rows, (4, 3, 2, 1, 0), 1)), rows


def write_dataset(root, count, H=6, W=8, pad_ratio=0.25, missing_masks=(), ratios=None, ids=None):
    """A directory laid out like the reference's dataset: imgs_png/ (RGB), samurai_seg/ (grey masks; none for the frames
    in missing_masks), smplx_params/ (JSON with the reference's keys; ratios: pad_ratio per frame, None = key left out)."""
    rng = np.random.default_rng(9)
    for folder in ("imgs_png", "samurai_seg", "smplx_params"):
        os.makedirs(os.path.join(root, folder), exist_ok=True)
    for k, i in enumerate(ids or range(count)):
        with open(os.path.join(root, "imgs_png", f"{i:05d}.png"), "wb") as fh:
            fh.write(write_png(random_samples(rng, H, W, 2, 8), 2, 8, (4,)))
        if i not in missing_masks:
            with open(os.path.join(root, "samurai_seg", f"{i:05d}.png"), "wb") as fh:
                fh.write(write_png((random_samples(rng, H, W, 0, 8) > 100).astype(np.uint8) * 255, 0, 8, (1,)))
        params = {"betas": rng.normal(size=10).tolist(), "trans": [0.1 * i, 0.2, 0.3], "root_pose": [0.01 * i, 0, 0],
                  "body_pose": rng.normal(size=(21, 3)).tolist(), "lhand_pose": rng.normal(size=(15, 3)).tolist(),
                  "rhand_pose": rng.normal(size=(15, 3)).tolist(), "jaw_pose": [0, 0, 0.5], "leye_pose": [0, 0, 0],
                  "reye_pose": [0, 0, 0], "focal": [1000.0 + i, 1100.0], "princpt": [W / 2, H / 2]}
        ratio = pad_ratio if ratios is None else ratios[k]
        if ratio is not None:
            params["pad_ratio"] = ratio
        with open(os.path.join(root, "smplx_params", f"{i:05d}.json"), "w") as fh:
            json.dump(params, fh)
