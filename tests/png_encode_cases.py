"""Inputs shared by the tests of the PNG / deflate encoder: the byte strings the deflate side is held to, the host program
(tools/png_deflate_host.cpp) that runs the device's code on the CPU, and the frames and NumPy restatements of the
frame-level tests."""
import os
import shutil
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIECE = 8192  # AMAV_DEFLATE_PIECE
STATUS_SIZE = 2
STORED, FIXED, DYNAMIC, ANY = 1, 2, 4, 7
NO_MATCH = 8  # the host program's switch: every byte a literal, so the histogram that is coded is the input's own


def pieces_of(n):
    return max(1, -(-n // PIECE))


def stored_bound(n, wrapper):
    """input + 5 bytes per piece + wrapper"""
    return n + 5 * pieces_of(n) + (6 if wrapper else 0)


def fibonacci(count):
    fib = [1, 1]
    while len(fib) < count:
        fib.append(fib[-1] + fib[-2])
    return fib[:count]


def fibonacci_piece():
    """Byte frequencies that follow the Fibonacci numbers as far as a piece has room: 17 symbols, 1 2 3 5 ... 2584, 6763
    bytes.  Coded without matching (NO_MATCH), the end-of-block symbol's 1 completes the sequence 1 1 2 3 ... and the
    unlimited Huffman tree over the 18 is 17 deep.  Under LZ77 the frequent symbols vanish into matches and the tree
    stays shallow: as one of deflate_cases() this is only another input."""
    counts = fibonacci(18)[1:]
    assert sum(counts) <= PIECE
    data = np.concatenate([np.full(c, 7 + 11 * i, np.uint8) for i, c in enumerate(counts)])
    return np.random.default_rng(20).permutation(data).tobytes()


def geometric_lengths_piece():
    """One piece over 255 byte values, 2^(L - 3) of them with probability 2^-L for L = 3 .. 10, the values shuffled so that
    equal code lengths are seldom neighbours.  Coded without matching, its literal code has about 2^(L - 3) codes of
    length L, so the code-length code sees frequencies near 1 2 4 ... 128 and its unlimited tree is deeper than 7."""
    rng = np.random.default_rng(7)
    values = rng.permutation(256)[:255].astype(np.uint8)
    counts, at = np.zeros(255, np.int64), 0
    for L in range(3, 11):
        counts[at:at + 2 ** (L - 3)] = PIECE >> L
        at += 2 ** (L - 3)
    data = np.repeat(values, counts)
    assert len(data) <= PIECE
    return rng.permutation(data).tobytes()


def huffman_depth(freqs):
    """The deepest leaf of an (unlimited) Huffman tree over the non-zero frequencies."""
    import heapq

    heap = [(f, 0) for f in freqs if f]
    heapq.heapify(heap)
    if len(heap) < 2:
        return len(heap)
    while len(heap) > 1:
        (fa, da), (fb, db) = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (fa + fb, max(da, db) + 1))
    return heap[0][1]


def kraft(lengths):
    from fractions import Fraction

    return sum(Fraction(1, 2 ** n) for n in lengths if n)


def dynamic_header(raw):
    """The first block of a raw DEFLATE stream, which must be dynamic: (code-length code lengths [19], how often each
    code-length symbol is sent, literal/length lengths, distance lengths)."""
    import png_model as pm

    br = pm._Bits(raw)
    br.bit()
    assert br.bits(2) == 2
    hlit, hdist, hclen = br.bits(5) + 257, br.bits(5) + 1, br.bits(4) + 4
    cl = [0] * 19
    for i in range(hclen):
        cl[pm.CL_ORDER[i]] = br.bits(3)
    table, sent, lengths = pm.canonical(cl), [0] * 19, []
    while len(lengths) < hlit + hdist:
        sym = pm._symbol(br, table)
        sent[sym] += 1
        if sym < 16:
            lengths.append(sym)
        elif sym == 16:
            lengths += [lengths[-1]] * (3 + br.bits(2))
        else:
            lengths += [0] * (3 + br.bits(3) if sym == 17 else 11 + br.bits(7))
    assert len(lengths) == hlit + hdist
    return cl, sent, lengths[:hlit], lengths[hlit:]


def run_lengths(program, tmp_path, cases):
    """The host program's --lengths: [(frequencies, limit)] -> [code lengths]"""
    src, dst = str(tmp_path / "lengths_in.bin"), str(tmp_path / "lengths_out.bin")
    with open(src, "wb") as fh:
        fh.write(struct.pack("<i", len(cases)))
        for freqs, limit in cases:
            fh.write(struct.pack(f"<ii{len(freqs)}I", len(freqs), limit, *freqs))
    done = subprocess.run([program, "--lengths", src, dst], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-4000:]
    blob, out, at = open(dst, "rb").read(), [], 0
    for freqs, _ in cases:
        out.append(list(blob[at:at + len(freqs)]))
        at += len(freqs)
    assert at == len(blob)
    return out


def deflate_cases():
    """[(name, bytes)]"""
    rng = np.random.default_rng(1951)
    text = rng.choice(np.frombuffer(b"acgt", np.uint8), 3 * PIECE).tobytes()
    block = rng.integers(0, 256, 5000, dtype=np.uint8).tobytes()  # shorter than a piece, so its repeats are in reach
    distinct = bytes(range(256))  # 256 different literals, no 3-byte string twice
    runs = b"".join(bytes([v]) * 19 for v in rng.permutation(256).astype(np.uint8)[:200].tolist())  # matches at distance 1 only
    return [
        ("empty", b""),
        ("one_byte", b"\x41"),
        ("two_bytes", b"\x00\xff"),
        ("equal_259", b"\x37" * 259),
        ("zeros_100000", bytes(100000)),
        ("random_70000", rng.integers(0, 256, 70000, dtype=np.uint8).tobytes()),
        ("text_acgt", text),
        ("piece_exact", rng.integers(0, 4, PIECE, dtype=np.uint8).tobytes()),
        ("piece_minus_1", rng.integers(0, 4, PIECE - 1, dtype=np.uint8).tobytes()),
        ("piece_plus_1", rng.integers(0, 4, PIECE + 1, dtype=np.uint8).tobytes()),
        ("random_block_repeated", (block * 3)[:PIECE + PIECE // 2]),
        ("fibonacci_17", fibonacci_piece()),
        ("geometric_lengths", geometric_lengths_piece()),
        ("distinct_256", distinct),
        ("distance_1_only", runs),
    ]


_program = None


def host_program(tmp_path_factory):
    """tools/png_deflate_host.cpp under AddressSanitizer and UBSan: a program of its own, nothing preloaded."""
    global _program
    if _program is None:
        compiler = next((c for c in ("g++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++")
                         if shutil.which(c)), None)
        assert compiler, "no host C++ compiler found"
        exe = str(tmp_path_factory.mktemp("deflate_host") / "png_deflate_host")
        subprocess.run([compiler, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tools", "png_deflate_host.cpp"), "-o", exe], check=True)
        _program = exe
    return _program


def run_host(program, tmp_path, streams):
    """streams: [(bytes, wrapper, modes, capacity)] -> [(status, needed, written bytes)]"""
    src, dst = str(tmp_path / "deflate_in.bin"), str(tmp_path / "deflate_out.bin")
    with open(src, "wb") as fh:
        fh.write(struct.pack("<i", len(streams)))
        for data, wrapper, modes, capacity in streams:
            fh.write(struct.pack("<iiqq", wrapper, modes, capacity, len(data)) + data)
    done = subprocess.run([program, src, dst], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-4000:]
    out, at, blob = [], 0, open(dst, "rb").read()
    for _ in streams:
        status, needed, written = struct.unpack_from("<iqq", blob, at)
        out.append((status, needed, blob[at + 20:at + 20 + written]))
        at += 20 + written
    assert at == len(blob)
    return out


def block_types(raw):
    """The BTYPE of every block of a raw DEFLATE stream made of byte-aligned pieces is not needed: only the first."""
    return (raw[0] >> 1) & 3


# ------------------------------------------------------------------------------------------------------------ frames
def to_levels(x, rounding="nearest"):
    """fp32 -> uint8 as include/amav.h states it: nearest = save_image's mul(255).add_(0.5).clamp_(0, 255) truncated, each
    step rounded to fp32; truncate = frames_to_rgb8's clamp to [0, 1], x 255, truncated; NaN -> 0."""
    x = np.asarray(x, np.float32)
    if rounding == "nearest":
        v = np.clip((x * np.float32(255.0)).astype(np.float32) + np.float32(0.5), np.float32(0), np.float32(255))
    else:
        v = (np.clip(x, np.float32(0), np.float32(1)) * np.float32(255.0)).astype(np.float32)
    return np.where(np.isnan(v), np.float32(0), v).astype(np.uint8)


def edge_values(rng, shape):
    """fp32 in and around [0, 1]: below 0, above 1, and one ulp either side of the points where `nearest` steps,
    (k + 0.5) / 255 as the issue writes them: k / 255 + 0.5 / 255."""
    x = rng.random(shape, dtype=np.float32) * np.float32(1.4) - np.float32(0.2)
    flat = x.reshape(-1)
    k = rng.integers(0, 255, flat.size).astype(np.float32)
    edge = k / np.float32(255) + np.float32(0.5) / np.float32(255)
    pick = rng.integers(0, 4, flat.size)
    flat[pick == 1] = np.nextafter(edge, np.float32(-1))[pick == 1]
    flat[pick == 2] = np.nextafter(edge, np.float32(2))[pick == 2]
    flat[pick == 3] = edge[pick == 3]
    return x


def filter_rows(img, which):
    """uint8 [H, W, C] -> the filtered scanlines (filter byte + row) of PNG filter `which` (0..4) or "adaptive": per row
    the filter with the smallest sum of absolute signed residuals, the lowest number on ties."""
    H, W, C = img.shape
    rows = img.reshape(H, W * C).astype(np.int32)
    out = bytearray()
    prev = np.zeros(W * C, np.int32)
    for y in range(H):
        cur = rows[y]
        left = np.concatenate([np.zeros(C, np.int32), cur[:-C]]) if W * C > C else np.zeros(W * C, np.int32)
        upleft = np.concatenate([np.zeros(C, np.int32), prev[:-C]]) if W * C > C else np.zeros(W * C, np.int32)
        p = left + prev - upleft
        pa, pb, pc = abs(p - left), abs(p - prev), abs(p - upleft)
        paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, prev, upleft))
        cands = [cur, cur - left, cur - prev, cur - (left + prev) // 2, cur - paeth]
        cands = [(c & 255).astype(np.uint8) for c in cands]
        if which == "adaptive":
            costs = [int(np.abs(c.view(np.int8).astype(np.int32)).sum()) for c in cands]
            ft = int(np.argmin(costs))
        else:
            ft = int(which)
        out += bytes([ft]) + cands[ft].tobytes()
        prev = cur
    return bytes(out)
