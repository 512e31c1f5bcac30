"""ops.deflate against the host build of the same code (tools/png_deflate_host.cpp): the same bytes for every case of
png_encode_cases.deflate_cases(), raw and zlib-wrapped, the same again on a second run, ops.inflate and zlib give the
input back, no stream passes the stored bound, and a capacity one byte short sets SIZE, reports the size needed and
leaves the guard bytes behind it alone."""
import zlib

import numpy as np
import pytest
import torch

import png_encode_cases as ec

pytestmark = pytest.mark.gpu

GUARD, LITTER = 0xC3, 0x5F


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """[(name, data, wrapper, host bytes)]"""
    program = ec.host_program(tmp_path_factory)
    cases = [(name, data, w) for name, data in ec.deflate_cases() for w in (0, 1)]
    got = ec.run_host(program, tmp_path_factory.mktemp("parity"), [(d, w, ec.ANY, ec.stored_bound(len(d), w)) for _, d, w in cases])
    assert all(s == 0 for s, _, _ in got)
    return [(name, d, w, out) for (name, d, w), (_, _, out) in zip(cases, got)]


def lay_out(host, capacity_of):
    blob, rows, at, out_at = bytearray(), [], 0, 0
    for k, (_, data, w, ref) in enumerate(host):
        pad = 1 + (3 * k) % 7  # inputs at odd offsets, litter in between
        blob += bytes([LITTER]) * pad + data
        at += pad
        out_at += 5 + (7 * k) % 16  # outputs at every alignment
        cap = capacity_of(data, w, ref)
        rows.append([at, at + len(data), out_at, cap, w])
        at += len(data)
        out_at += cap
    blob += bytes([LITTER]) * 9
    return torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda(), torch.tensor(rows, dtype=torch.int64), out_at + 11


def run(host, capacity_of):
    from audio_motion_avatar_amd import ops

    data, records, out_bytes = lay_out(host, capacity_of)
    out = torch.full((out_bytes,), GUARD, dtype=torch.uint8, device="cuda")
    out, produced, status = ops.deflate(data, records, out=out)
    return data, records, out, produced.cpu().tolist(), status.cpu().tolist()


def test_device_bytes_equal_the_host_build_and_inflate_back(host):
    from audio_motion_avatar_amd import ops

    data, records, out, produced, status = run(host, lambda d, w, ref: ec.stored_bound(len(d), w))
    flat = out.cpu().numpy()
    covered = np.zeros(flat.size, bool)
    for (name, d, w, ref), row, n, s in zip(host, records.tolist(), produced, status):
        assert s == 0 and n == len(ref) <= ec.stored_bound(len(d), w), (name, w, s, n, len(ref))
        got = flat[row[2]:row[2] + n].tobytes()
        assert got == ref, (name, w)
        assert zlib.decompress(got, 15 if w else -15) == d, (name, w)
        covered[row[2]:row[2] + n] = True
    assert (flat[~covered] == GUARD).all(), "a byte outside every stream's produced range was written"
    again = run(host, lambda d, w, ref: ec.stored_bound(len(d), w))[2]
    assert torch.equal(out, again), "two calls, the same bytes"
    # back through the device's own inflate
    rows, at = [], 0
    for row, n, (_, d, w, _) in zip(records.tolist(), produced, host):
        rows.append([row[2], row[2] + n, at, len(d), w])
        at += len(d) + 3
    back, made, st = ops.inflate(out, torch.tensor(rows, dtype=torch.int64))
    back = back.cpu().numpy()
    for (name, d, w, _), row, n, s in zip(host, rows, made.cpu().tolist(), st.cpu().tolist()):
        assert s == 0 and n == len(d) and back[row[2]:row[2] + n].tobytes() == d, (name, w)


def test_capacity_one_byte_short(host):
    data, records, out, produced, status = run(host, lambda d, w, ref: len(ref) - 1)
    flat = out.cpu().numpy()
    covered = np.zeros(flat.size, bool)
    for (name, d, w, ref), row, n, s in zip(host, records.tolist(), produced, status):
        assert s == ec.STATUS_SIZE and n == len(ref), (name, w, s, n)  # the size it needs
        assert flat[row[2]:row[2] + row[3]].tobytes() == ref[:row[3]], (name, w)
        covered[row[2]:row[2] + row[3]] = True
    assert (flat[~covered] == GUARD).all(), "a byte at or behind a capacity was written"


def test_overlapping_ranges_beyond_the_piece_table_are_flagged():
    from audio_motion_avatar_amd import ops

    n = 3 * ec.PIECE
    data = torch.zeros(n, dtype=torch.uint8, device="cuda")
    rows = [[0, n, k * 100, 100, 0] for k in range(6)]  # 18 pieces; the table holds 3 + 6
    out = torch.full((700,), GUARD, dtype=torch.uint8, device="cuda")
    out, produced, status = ops.deflate(data, torch.tensor(rows, dtype=torch.int64), out=out)
    assert status.cpu().tolist() == [0, 0, 0, ops.PNG_STATUS_TABLE, ops.PNG_STATUS_TABLE, ops.PNG_STATUS_TABLE]
    produced, flat = produced.cpu().tolist(), out.cpu().numpy()
    for k in range(3):
        assert zlib.decompress(flat[100 * k:100 * k + produced[k]].tobytes(), -15) == bytes(n)
    assert produced[3:] == [0, 0, 0] and (flat[300:] == GUARD).all()
