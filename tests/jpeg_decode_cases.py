"""The fixtures of tests/golden/jpeg_decode/ (tests/golden/make_jpeg_decode_golden.py writes them) and what the decoder
tests derive from them once: the model's decode of every file, its float64 reconstruction and fp32 bound."""
import functools
import json
import os

import numpy as np

import jpeg_decode_model as dm

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_decode")
with open(os.path.join(DIR, "manifest.json")) as _fh:
    FILES = json.load(_fh)["files"]
NAMES = sorted(FILES)

# model against libjpeg's decode (integer IDCT, rounded chroma), measured over the fixtures by
# tests/test_jpeg_decode_model.py; the GPU test allows one level more
LIBJPEG_MAX = {"444": 2, "gray": 1, "420": 3}


@functools.lru_cache(maxsize=None)
def jpeg(name):
    with open(os.path.join(DIR, name + ".jpg"), "rb") as fh:
        return fh.read()


@functools.lru_cache(maxsize=None)
def libjpeg_rgb(name):
    with np.load(os.path.join(DIR, "libjpeg_rgb.npz")) as recorded:
        out = recorded[name]
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def decoded(name):
    return dm.decode(jpeg(name))


@functools.lru_cache(maxsize=None)
def model(name):
    """(rgb float64 [H, W, 3] not rounded, delta [H, W, 3])"""
    rgb, delta = dm.reconstruct(decoded(name))
    rgb.setflags(write=False), delta.setflags(write=False)
    return rgb, delta


def strip_dht(data):
    """The file without its DHT segments: what MJPG-in-AVI writers leave out (the Annex K tables are implied)."""
    out, pos = bytearray(data[:2]), 2
    while True:
        marker, n = data[pos + 1], int.from_bytes(data[pos + 2:pos + 4], "big")
        if marker != 0xC4:
            out += data[pos:pos + 2 + n]
        pos += 2 + n
        if marker == 0xDA:
            return bytes(out) + data[pos:]
