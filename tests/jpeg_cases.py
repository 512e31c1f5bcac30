"""Inputs of tests/test_jpeg_gpu.py, made on the CPU from seeds: uint8 RGB frames [F, H, W, 3] and libjpeg's own encoding
of them (through Pillow, same quality / sampling / restart interval, standard Huffman tables), which is the reference
encoder of those tests."""
import functools
import io

import numpy as np
from PIL import Image

import jpeg_model as jm


def white(F, H, W):
    return np.full((F, H, W, 3), 255, dtype=np.uint8)


def noise(F, H, W, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (F, H, W, 3), dtype=np.uint8)


def checkerboard(F, H, W):
    """+- full range: bands of 16 rows alternate between a per-pixel checkerboard (an AC coefficient of category 10 at
    quality 100) and 8x8 blocks that flip between 0 and 255 (DC differences of category 11); frame f shifts the phase."""
    y, x = np.mgrid[0:H, 0:W]
    out = np.empty((F, H, W, 3), dtype=np.uint8)
    for f in range(F):
        pixel = (x + y + f) & 1
        block = ((x >> 3) + (y >> 3) + f) & 1
        out[f] = (np.where((y >> 4) & 1, block, pixel) * 255)[..., None]
    return out


def high_frequency(F, H, W):
    """Every 8x8 block holds one coefficient only, the last of the zigzag scan: (7, 7), amplitude 40 grey levels around
    mid-grey, so a block is DC, three ZRL, one symbol, and no EOB."""
    t = np.cos((2 * np.arange(8) + 1) * 7 * np.pi / 16)
    tile = 128 + 40 * np.outer(t, t) / (t[0] * t[0])
    img = np.tile(tile, (-(-H // 8), -(-W // 8)))[:H, :W]
    return np.repeat(np.rint(img).astype(np.uint8)[None, :, :, None], 3, axis=3).repeat(F, axis=0)


def disc(F, H, W):
    """A coloured, shaded disc on white that moves from frame to frame: the rendered-frame case (mostly background)."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.full((F, H, W, 3), 255, dtype=np.uint8)
    for f in range(F):
        cy, cx, r = H * (0.45 + 0.05 * f), W * (0.4 + 0.08 * f), 0.3 * min(H, W)
        d = np.sqrt((y - cy) ** 2 + (x - cx) ** 2) / r
        shade = np.clip(1.0 - 0.6 * d, 0.0, 1.0)
        colour = np.stack([200 * shade + 30, 90 * shade + 60 * np.sin(x / 3.0) ** 2, 40 + 150 * (1 - shade)], axis=-1)
        out[f][d < 1] = np.clip(colour, 0, 255).astype(np.uint8)[d < 1]
    return out


CONTENTS = {"white": white, "noise": noise, "checkerboard": checkerboard, "high_frequency": high_frequency, "disc": disc}

# name: (content, F, H, W, quality, subsampling, restart_rows)
CASES = {
    "white_1x1": ("white", 1, 1, 1, 90, "420", 1),
    "white_8x8": ("white", 1, 8, 8, 90, "420", 1),
    "noise_16x16_f3": ("noise", 3, 16, 16, 100, "420", 1),
    "noise_17x33": ("noise", 1, 17, 33, 100, "420", 1),
    "noise_17x33_444": ("noise", 1, 17, 33, 100, "444", 1),
    "noise_48x64_q50_rr2": ("noise", 1, 48, 64, 50, "420", 2),
    "noise_48x64_q8_444": ("noise", 1, 48, 64, 8, "444", 0),
    "noise_64x64_444_rr0": ("noise", 1, 64, 64, 90, "444", 0),  # 192 blocks: the entropy coder's rounds of 64, exactly
    "checkerboard_160x16": ("checkerboard", 1, 160, 16, 100, "420", 1),
    "checkerboard_80x8_444": ("checkerboard", 1, 80, 8, 100, "444", 1),
    "high_frequency_16x16_444": ("high_frequency", 1, 16, 16, 90, "444", 1),
    "high_frequency_17x33": ("high_frequency", 1, 17, 33, 90, "420", 1),
    "disc_48x64_rr0_f3": ("disc", 3, 48, 64, 90, "420", 0),
    "disc_48x64_444_rr2": ("disc", 1, 48, 64, 75, "444", 2),
    "disc_17x33_f3": ("disc", 3, 17, 33, 90, "420", 1),
}
COUNTER_CASES = [n for n, c in CASES.items() if c[0] in ("noise", "checkerboard")]


@functools.lru_cache(maxsize=None)
def frames(name):
    content, F, H, W = CASES[name][:4]
    out = CONTENTS[content](F, H, W)
    out.setflags(write=False)
    return out


def pillow_jpeg(rgb, quality, subsampling, restart_rows):
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, "JPEG", quality=quality, subsampling={"444": 0, "420": 2}[subsampling], optimize=False,
                              restart_marker_rows=restart_rows)
    return buf.getvalue()


@functools.lru_cache(maxsize=None)
def libjpeg_streams(name):
    """libjpeg's encoding of every frame of the case."""
    _, _, _, _, quality, subsampling, restart_rows = CASES[name]
    return tuple(pillow_jpeg(f, quality, subsampling, restart_rows) for f in frames(name))


@functools.lru_cache(maxsize=None)
def model_quotients(name):
    _, _, _, _, quality, subsampling, _ = CASES[name]
    out = jm.quotients(frames(name), quality, subsampling)
    out.setflags(write=False)
    return out


def events(decoded):
    """The scan events a stream exercises, as the set the counter test compares."""
    d = decoded
    return {k for k, hit in (("stuffed", d.stuffed > 0), ("zrl", d.zrl > 0), ("no_eob", d.blocks_without_eob > 0),
                             ("ac10", d.max_ac_category >= 10), ("dc10", d.max_dc_category >= 10)) if hit}


def psnr(a, b):
    mse = np.mean((np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) ** 2)
    return 99.0 if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)


def pillow_decode(jpeg):
    return np.asarray(Image.open(io.BytesIO(jpeg)).convert("RGB"))
