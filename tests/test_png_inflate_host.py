"""The device inflate's own code (csrc/png_inflate_core.h) on the CPU: tools/png_inflate_host.cpp is built with
-fsanitize=address,undefined and every sound and every damaged stream goes through it.  Sound streams must give zlib's
bytes, damaged ones the status and the bytes of tests/png_model.py, and the sanitizers must stay silent: this is where
the bounds rules of the kernel (no read at or past in_end, no write past the capacity) are checked before a GPU run."""
import os
import shutil
import struct
import subprocess
import zlib

import pytest

import png_cases as pc
import png_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    compiler = next((c for c in ("g++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++")
                     if shutil.which(c)), None)
    assert compiler, "no host C++ compiler found"
    exe = str(tmp_path_factory.mktemp("inflate_host") / "png_inflate_host")
    subprocess.run([compiler, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "png_inflate_host.cpp"), "-o", exe], check=True)
    return exe


def run(program, tmp_path, streams):
    """streams: [(bytes, wrapper, capacity)] -> [(status, produced bytes)]"""
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as fh:
        fh.write(struct.pack("<i", len(streams)))
        for data, wrapper, capacity in streams:
            fh.write(struct.pack("<iqq", wrapper, capacity, len(data)) + data)
    done = subprocess.run([program, src, dst], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-4000:]
    out, at, blob = [], 0, open(dst, "rb").read()
    for _ in streams:
        status, n = struct.unpack_from("<iq", blob, at)
        out.append((status, blob[at + 12:at + 12 + n]))
        at += 12 + n
    assert at == len(blob)
    return out


def test_sound_streams_equal_zlib(program, tmp_path):
    cases = pc.sound_streams()
    want = [zlib.decompress(s, 15 if w else -15) for _, s, w in cases]
    got = run(program, tmp_path, [(s, w, len(ref)) for (_, s, w), ref in zip(cases, want)])
    for (name, _, _), ref, (status, data) in zip(cases, want, got):
        assert status == 0 and data == ref, name


def test_capacity_is_never_passed(program, tmp_path):
    """Every sound stream again with room for one byte less than it makes, and for half: SIZE, and only whole symbols."""
    cases = [(n, s, w) for n, s, w in pc.sound_streams() if len(zlib.decompress(s, 15 if w else -15)) > 0]
    streams = []
    for _, s, w in cases:
        n = len(zlib.decompress(s, 15 if w else -15))
        streams += [(s, w, n - 1), (s, w, n // 2)]
    got = run(program, tmp_path, streams)
    for k, (status, data) in enumerate(got):
        _, s, w = cases[k // 2]
        ref = zlib.decompress(s, 15 if w else -15)
        assert status == pm.STATUS_SIZE and len(data) <= streams[k][2] and ref.startswith(data), cases[k // 2][0]


def test_damaged_streams_equal_the_model(program, tmp_path):
    cases = pc.damaged_streams()
    got = run(program, tmp_path, [(s, w, 400 if cap is None else cap) for _, s, w, cap, _ in cases])
    for (name, s, w, cap, bit), (status, data) in zip(cases, got):
        want, want_status = pm.inflate(s, w, 400 if cap is None else cap)
        assert status & bit and status == want_status and data == want, name


def test_damaged_frames_equal_the_model(program, tmp_path):
    need = pc.DAMAGED_H * (1 + pc.DAMAGED_W)
    cases = pc.damaged_frames()
    got = run(program, tmp_path, [(s, 1, need) for _, s, _ in cases])
    for (name, s, bit), (status, data) in zip(cases, got):
        want, want_status = pm.inflate(s, 1, need)
        assert status == want_status and data == want, name
