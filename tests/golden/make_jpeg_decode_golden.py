"""Writes tests/golden/jpeg_decode/: small baseline JPEG files encoded by libjpeg through Pillow, and beside them the
RGB libjpeg decodes each to (libjpeg_rgb.npz: NAME -> uint8 [H, W, 3]), so that the tests that compare against libjpeg's
decode do not depend on the Pillow build of the machine they run on.  manifest.json lists how each file was made.

    python tests/golden/make_jpeg_decode_golden.py
"""
import io
import json
import os

import numpy as np
from PIL import Image

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "jpeg_decode")


def smooth(H, W, seed):
    """Smooth colour gradients plus noise of a few grey levels: what a rendered or filmed frame looks like to the codec."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    base = np.stack([128 + 100 * np.sin(x / 9.0 + seed) * np.cos(y / 7.0), 40 + 180 * x / max(W - 1, 1) + 20 * np.sin(y / 3.0),
                     230 - 200 * y / max(H - 1, 1) + 15 * np.cos(x / 2.0)], axis=-1)
    return np.clip(base + rng.normal(0.0, 6.0, base.shape), 0, 255).astype(np.uint8)


def noise(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def checker(H, W, seed):
    """Bands of 16 rows: a per-pixel checkerboard (AC category 10 at quality 100), then 8x8 blocks flipping 0 / 255."""
    y, x = np.mgrid[0:H, 0:W]
    pixel, block = (x + y + seed) & 1, ((x >> 3) + (y >> 3) + seed) & 1
    return np.repeat((np.where((y >> 4) & 1, block, pixel) * 255).astype(np.uint8)[..., None], 3, axis=2)


def high_frequency(H, W, seed):
    """One coefficient per block, the last of the zigzag scan: DC, three ZRL, one symbol, no EOB."""
    t = np.cos((2 * np.arange(8) + 1) * 7 * np.pi / 16)
    img = np.tile(128 + 40 * np.outer(t, t) / (t[0] * t[0]), (-(-H // 8), -(-W // 8)))[:H, :W]
    return np.repeat(np.rint(img).astype(np.uint8)[..., None], 3, axis=2)


CONTENT = {"smooth": smooth, "noise": noise, "checker": checker, "hf": high_frequency}
# name: (content, H, W, mode, quality, restart_marker_rows, optimize)
FILES = {
    "smooth_444_17x9_q30": ("smooth", 17, 9, "444", 30, 0, False),
    "smooth_444_33x50_q75_rr1_opt": ("smooth", 33, 50, "444", 75, 1, True),
    "smooth_444_24x40_q100": ("smooth", 24, 40, "444", 100, 0, False),
    "smooth_420_16x16_q50": ("smooth", 16, 16, "420", 50, 0, False),
    "smooth_420_17x9_q90_rr1": ("smooth", 17, 9, "420", 90, 1, False),
    "smooth_420_33x50_q30_opt": ("smooth", 33, 50, "420", 30, 0, True),
    "smooth_420_24x40_q100_rr1_opt": ("smooth", 24, 40, "420", 100, 1, True),
    "smooth_420_48x40_q75_rr1": ("smooth", 48, 40, "420", 75, 1, False),
    "smooth_gray_33x50_q75_rr1_opt": ("smooth", 33, 50, "gray", 75, 1, True),
    "smooth_gray_16x16_q40": ("smooth", 16, 16, "gray", 40, 0, False),
    "checker_420_160x16_q100_rr1_opt": ("checker", 160, 16, "420", 100, 1, True),
    "noise_444_17x33_q100_opt": ("noise", 17, 33, "444", 100, 0, True),
    "noise_420_33x17_q95_rr1": ("noise", 33, 17, "420", 95, 1, False),
    "hf_444_16x16_q90_rr1": ("hf", 16, 16, "444", 90, 1, False),
}


def main():
    os.makedirs(OUT, exist_ok=True)
    manifest, recorded = {}, {}
    for seed, (name, (content, H, W, mode, quality, rows, optimize)) in enumerate(FILES.items()):
        rgb = CONTENT[content](H, W, seed)
        image = Image.fromarray(rgb).convert("L") if mode == "gray" else Image.fromarray(rgb)
        buf = io.BytesIO()
        kw = {} if mode == "gray" else {"subsampling": {"444": 0, "420": 2}[mode]}
        image.save(buf, "JPEG", quality=quality, optimize=optimize, restart_marker_rows=rows, **kw)
        data = buf.getvalue()
        with open(os.path.join(OUT, name + ".jpg"), "wb") as fh:
            fh.write(data)
        recorded[name] = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        manifest[name] = {"content": content, "height": H, "width": W, "sampling": mode, "quality": quality,
                          "restart_marker_rows": rows, "optimize": optimize, "bytes": len(data)}
    np.savez_compressed(os.path.join(OUT, "libjpeg_rgb.npz"), **recorded)
    import PIL

    manifest = {"pillow": PIL.__version__, "files": manifest}
    with open(os.path.join(OUT, "manifest.json"), "w") as fh:
        json.dump(manifest, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
