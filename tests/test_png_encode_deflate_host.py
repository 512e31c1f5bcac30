"""The device deflate's own code (csrc/png_deflate_core.h) on the CPU: tools/png_deflate_host.cpp is built with
-fsanitize=address,undefined (a program of its own, nothing preloaded) and every case of png_encode_cases.deflate_cases()
goes through it, raw and zlib-wrapped.  zlib.decompress must return the input (which also proves the Adler-32), the
sanitizers must stay silent, no stream may pass the stored-block bound, and a capacity one byte short must give SIZE
without a write at or behind it (the program checks its guard bytes and AddressSanitizer the exact-size block).  LZ77
hides a skewed byte histogram from the coder, so the code-length limiter is driven separately: whole pieces coded
without matching (the program's mode bit 8) and build_lengths alone on chosen histograms (its --lengths)."""
import zlib

import pytest

import png_encode_cases as ec


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return ec.host_program(tmp_path_factory)


@pytest.fixture(scope="module")
def encoded(program, tmp_path_factory):
    """{(name, wrapper): (status, needed, bytes)} at a capacity of the stored bound"""
    cases = ec.deflate_cases()
    streams = [(data, w, ec.ANY, ec.stored_bound(len(data), w)) for _, data in cases for w in (0, 1)]
    got = ec.run_host(program, tmp_path_factory.mktemp("all"), streams)
    return {(name, w): got[2 * i + w] for i, (name, _) in enumerate(cases) for w in (0, 1)}


@pytest.mark.parametrize("wrapper", [0, 1])
def test_every_case_inflates_to_its_input_within_the_stored_bound(encoded, wrapper):
    for name, data in ec.deflate_cases():
        status, needed, out = encoded[name, wrapper]
        assert status == 0 and needed == len(out), name
        assert len(out) <= ec.stored_bound(len(data), wrapper), (name, len(out))
        assert zlib.decompress(out, 15 if wrapper else -15) == data, name


def test_random_bytes_come_out_stored(encoded):
    data = dict(ec.deflate_cases())["random_70000"]
    _, _, out = encoded["random_70000", 0]
    assert len(out) == ec.stored_bound(len(data), 0)
    at = 0
    for k in range(ec.pieces_of(len(data))):  # every piece: a stored block of its bytes
        n = min(ec.PIECE, len(data) - k * ec.PIECE)
        assert out[at] == (1 if k == ec.pieces_of(len(data)) - 1 else 0)
        assert int.from_bytes(out[at + 1:at + 3], "little") == n
        at += 5 + n
    assert at == len(out)


def test_dynamic_codes_win_on_a_four_letter_text(program, tmp_path, encoded):
    data = dict(ec.deflate_cases())["text_acgt"]
    _, _, out = encoded["text_acgt", 0]
    (status, needed, fixed), = ec.run_host(program, tmp_path, [(data, 0, ec.FIXED, 2 * len(data))])
    assert status == 0 and zlib.decompress(fixed, -15) == data
    assert ec.block_types(fixed) == 1 and ec.block_types(out) == 2
    assert len(out) < len(fixed) and len(out) < 0.5 * len(data), (len(out), len(fixed))


def test_a_repeated_random_block_is_matched_at_a_long_distance(encoded):
    """5000 random bytes repeated: the first piece holds 3192 bytes that lie 5000 back, the second nothing twice."""
    data = dict(ec.deflate_cases())["random_block_repeated"]
    out = encoded["random_block_repeated", 0][2]
    assert ec.block_types(out) != 0 and len(out) < len(data) - 2500, len(out)


@pytest.mark.parametrize("wrapper", [0, 1])
def test_the_length_limiters_act_inside_real_streams(program, tmp_path, wrapper):
    """Without matching the coded histogram is the input's own.  The Fibonacci piece needs a literal tree 17 deep: it must
    come out 15 deep with a Kraft sum of exactly one.  The geometric piece makes the code-length code's frequencies run
    1 2 4 ...: its tree, 8 deep unlimited, must come out 7 deep and complete.  zlib must take both streams."""
    pieces = {"fibonacci": ec.fibonacci_piece(), "geometric": ec.geometric_lengths_piece()}
    got = ec.run_host(program, tmp_path, [(d, wrapper, ec.DYNAMIC | ec.NO_MATCH, 2 * len(d)) for d in pieces.values()])
    seen = {}
    for (name, data), (status, needed, out) in zip(pieces.items(), got):
        assert status == 0 and zlib.decompress(out, 15 if wrapper else -15) == data, name
        cl, sent, lit, dist = ec.dynamic_header(out[2:] if wrapper else out)
        hist = [data.count(v) for v in range(256)] + [1]
        assert [n != 0 for n in lit[:257]] == [f != 0 for f in hist], name  # every byte a literal, and the end of block
        assert ec.kraft(lit) == 1 and ec.kraft(cl) == 1 and max(lit) <= 15 and max(cl) <= 7, name
        assert sum(dist) == 1  # no match: one distance code of one bit
        seen[name] = (ec.huffman_depth(hist), max(lit), ec.huffman_depth(sent), max(cl))
    assert seen["fibonacci"][:2] == (17, 15), seen   # deeper than 15 unlimited, 15 as sent
    assert seen["geometric"][2:] == (8, 7), seen     # deeper than 7 unlimited, 7 as sent


def huffman_cost(freqs):
    import heapq

    heap, cost = sorted(f for f in freqs if f), 0
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        cost += a + b
        heapq.heappush(heap, a + b)
    return cost


def test_build_lengths_on_chosen_histograms(program, tmp_path):
    """build_lengths alone (the program's --lengths): Fibonacci frequencies that force the 15-bit and the 7-bit repair,
    and 300 seeded skewed histograms at both limits.  Always: no length above the limit, zero exactly where the frequency
    is zero, a Kraft sum of exactly one (one used symbol: one bit), no rarer symbol with a shorter code; optimal
    (Huffman's cost) wherever the unlimited tree fits the limit."""
    import numpy as np

    rng = np.random.default_rng(77)
    cases = [(ec.fibonacci(30), 15), (ec.fibonacci(19), 7), (ec.fibonacci(40)[::-1], 15), ([0, 5, 0], 15), ([0] * 19, 7),
             ([3, 0, 0, 9], 7), ([1] * 286, 15), ([1] * 19, 7)]
    for k in range(300):
        n, limit = (19, 7) if k % 2 else (int(rng.integers(2, 287)), 15)
        freqs = np.floor(np.exp(rng.uniform(0, rng.uniform(2, 20), n))).astype(np.int64)
        freqs[rng.random(n) < rng.uniform(0, 0.6)] = 0
        cases.append((np.minimum(freqs, 50_000_000).tolist(), limit))
    got = ec.run_lengths(program, tmp_path, cases)
    repaired = {7: 0, 15: 0}
    for (freqs, limit), lens in zip(cases, got):
        used = [(f, n) for f, n in zip(freqs, lens) if f]
        assert all((n == 0) == (f == 0) for f, n in zip(freqs, lens)) and max(lens) <= limit, (freqs, lens)
        if len(used) == 1:
            assert used[0][1] == 1
        elif used:
            assert ec.kraft(lens) == 1, (freqs, lens)
            by_freq = sorted(used)
            assert all(a[1] >= b[1] for a, b in zip(by_freq, by_freq[1:]) if a[0] < b[0]), (freqs, lens)
            if ec.huffman_depth(freqs) <= limit:
                assert sum(f * n for f, n in used) == huffman_cost(freqs), (freqs, lens)
            else:
                repaired[limit] += 1
                assert max(lens) == limit
    assert repaired[7] >= 20 and repaired[15] >= 20, repaired  # the repair is what most of these cases are for


def test_zeros_are_matched(encoded):
    assert len(encoded["zeros_100000", 0][2]) < 0.01 * 100000
    assert len(encoded["equal_259", 0][2]) <= 12


@pytest.mark.parametrize("modes", [ec.STORED, ec.FIXED, ec.DYNAMIC])
def test_every_case_under_each_forced_coding(program, tmp_path, modes):
    """Each coding forced on every input, dynamic also on the pieces that would not choose it: no match at all (one
    distance code of one bit that is never sent) and one used distance code.  (The length limiter is not reached this
    way: the two limiter tests of this file drive it.)"""
    cases = ec.deflate_cases()
    got = ec.run_host(program, tmp_path, [(data, 1, modes, 2 * len(data) + 600 * ec.pieces_of(len(data))) for _, data in cases])
    for (name, data), (status, needed, out) in zip(cases, got):
        assert status == 0 and zlib.decompress(out) == data, name
        want = {ec.STORED: 0, ec.FIXED: 1, ec.DYNAMIC: 2}[modes]
        if modes != ec.DYNAMIC or len(data) >= 2:  # a piece with fewer than two symbols cannot carry a dynamic block
            assert ec.block_types(out[2:]) == want, name


def test_capacity_is_never_passed(program, tmp_path, encoded):
    streams, names = [], []
    for name, data in ec.deflate_cases():
        for w in (0, 1):
            needed = encoded[name, w][1]
            streams += [(data, w, ec.ANY, needed - 1), (data, w, ec.ANY, needed // 2), (data, w, ec.ANY, 0)]
            names += [(name, w)] * 3
    got = ec.run_host(program, tmp_path, streams)
    for key, (data, w, _, cap), (status, needed, out) in zip(names, streams, got):
        assert status == ec.STATUS_SIZE and needed == encoded[key][1], key  # the size it needs
        assert out == encoded[key][2][:cap], key                           # what fits is the stream's start
