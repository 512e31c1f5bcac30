"""ops.inflate against zlib.decompress, bit for bit: stored blocks, zlib's own output under every strategy, hand-written
fixed- and dynamic-Huffman streams (tests/png_cases.py lists them).  The streams lie at odd offsets with litter between
them, every output sits between guard bytes that must survive, and the whole list also goes as batches of 70 streams."""
import zlib

import numpy as np
import pytest
import torch

import png_cases as pc

pytestmark = pytest.mark.gpu

GUARD, LITTER = 0xC3, 0x5F


def lay_out(cases, capacities=None):
    """[(name, stream, wrapper)] -> (stream bytes, records int64 [N,5], out buffer of guards, expected outputs)."""
    blob, rows, want, at, out_at = bytearray(), [], [], 0, 0
    for k, (name, stream, wrapper) in enumerate(cases):
        ref = zlib.decompress(stream, 15 if wrapper else -15)
        pad = 1 + (3 * k) % 7  # odd offsets, litter in between
        blob += bytes([LITTER]) * pad + stream
        at += pad
        out_at += 5 + (7 * k) % 16  # outputs at every alignment
        cap = len(ref) if capacities is None else capacities[k]
        rows.append([at, at + len(stream), out_at, cap, wrapper])
        want.append(ref)
        at += len(stream)
        out_at += cap
    blob += bytes([LITTER]) * 9
    return bytes(blob), torch.tensor(rows, dtype=torch.int64), out_at + 11, want


def run(cases):
    from audio_motion_avatar_amd import ops

    blob, records, out_bytes, want = lay_out(cases)
    stream = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
    out = torch.full((out_bytes,), GUARD, dtype=torch.uint8, device="cuda")
    out, produced, status = ops.inflate(stream, records, out=out)
    out, produced, status = out.cpu().numpy(), produced.cpu().tolist(), status.cpu().tolist()
    covered = np.zeros(out_bytes, bool)
    for (name, _, _), row, ref, n, s in zip(cases, records.tolist(), want, produced, status):
        assert s == 0 and n == len(ref), (name, s, n, len(ref))
        assert out[row[2]:row[2] + n].tobytes() == ref, name
        covered[row[2]:row[2] + row[3]] = True
    assert (out[~covered] == GUARD).all(), "a byte outside every stream's range was written"
    return out


def test_every_sound_stream_in_batches_of_70():
    cases = list(pc.sound_streams())
    assert len(cases) > 200
    first = run(cases[:70])  # more streams than one per-CU slot pattern would show
    for at in range(70, len(cases), 70):
        run(cases[at:at + 70])
    assert np.array_equal(first, run(cases[:70])), "two calls, the same bytes"


@pytest.mark.parametrize("name", ["stored_len0", "stored_1", "fixed_far_window", "fixed_ring_wrap", "dynamic_15_bit_code_hclen19"])
def test_one_stream_calls(name):
    run([c for c in pc.sound_streams() if c[0] == name])


def test_a_mixed_batch_of_70():
    cases = list(pc.sound_streams())
    order = np.random.default_rng(3).permutation(len(cases))[:70]
    run([cases[i] for i in order])


def test_default_output_buffer_and_device_records():
    from audio_motion_avatar_amd import ops

    cases = [c for c in pc.sound_streams() if c[0].startswith("dynamic_")]
    blob, records, _, want = lay_out(cases)
    stream = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
    out, produced, status = ops.inflate(stream, records.cuda())
    assert status.tolist() == [0] * len(cases)
    for row, ref in zip(records.tolist(), want):
        assert out[row[2]:row[2] + len(ref)].cpu().numpy().tobytes() == ref
