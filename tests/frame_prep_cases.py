"""Inputs of the frame-preparation tests: frames and masks from integer formulas of (frame, y, x, channel), no RNG, so
tests/golden/make_frame_prep_golden.py and the tests build identical inputs without storing them.

Each case: H, W, pad_ratio, frames uint8 [F,H,W,3], masks uint8 [F,H,W] or None (the mask file is missing: all ones)."""
import os

import numpy as np

H, W = 96, 72          # the small cases: no multiple of a tile, odd padded sizes with pad_ratio 0.1
BIG_H, BIG_W = 1100, 1300
REF_SIDE = 1024        # the reference hard-codes it (src/datasets/dataset_speech_vid.py:246-252)
EDGE = (0, 1, 511, 512, 1022, 1023)
STRIDE = 41


def frames(n, h=H, w=W, first=0):
    f, y, x, c = np.ogrid[first:first + n, 0:h, 0:w, 0:3]
    return ((f * 37 + y * 7 + x * 13 + c * 71 + (y * x) % 29 * 5) % 256).astype(np.uint8)


def blob(cy=55, cx=30, ry=20, rx=14, h=H, w=W):
    y, x = np.ogrid[0:h, 0:w]
    return (((y - cy) ** 2 * rx * rx + (x - cx) ** 2 * ry * ry <= ry * ry * rx * rx) * 255).astype(np.uint8)


def rect(y0, y1, x0, x1, h=H, w=W, value=255):
    m = np.zeros((h, w), np.uint8)
    m[y0:y1 + 1, x0:x1 + 1] = value
    return m


def dots(points, h=H, w=W):
    m = np.zeros((h, w), np.uint8)
    for y, x in points:
        m[y, x] = 255
    return m


def graded():
    """values 1..254 inside a rectangle: the composite is not just 0 / 1"""
    y, x = np.ogrid[0:H, 0:W]
    return np.where((y >= 20) & (y <= 70) & (x >= 10) & (x <= 60), 1 + (y * 5 + x * 3) % 254, 0).astype(np.uint8)


def case(name):
    small = dict(H=H, W=W, pad_ratio=0.0)
    if name == "a_blob":
        return dict(small, frames=frames(1), masks=blob()[None])
    if name == "b_top_right":  # both clamps act, the crop is 37 x 32
        return dict(small, frames=frames(1, first=1), masks=rect(0, 30, 50, W - 1)[None])
    if name == "c_empty":
        return dict(small, frames=frames(1, first=2), masks=np.zeros((1, H, W), np.uint8))
    if name == "d_no_mask":
        return dict(small, frames=frames(1, first=3), masks=None)
    if name == "e_padded":
        return dict(small, pad_ratio=0.1, frames=frames(1, first=4), masks=blob()[None])
    if name == "f_dots":  # one pixel: max_size 1; two pixels: max_size 5
        return dict(small, frames=frames(2, first=5), masks=np.stack([dots([(10, 20)]), dots([(10, 20), (13, 24)])]))
    if name == "g_big":  # max_size > 1024: the resize shrinks
        return dict(H=BIG_H, W=BIG_W, pad_ratio=0.0, frames=frames(1, BIG_H, BIG_W, first=7),
                    masks=rect(20, 1080, 30, 1270, BIG_H, BIG_W)[None])
    if name == "h_graded":
        return dict(small, frames=frames(1, first=8), masks=graded()[None])
    raise KeyError(name)


CASES = ("a_blob", "b_top_right", "c_empty", "d_no_mask", "e_padded", "f_dots", "g_big", "h_graded")
SMALL_IMAGES = tuple(n for n in CASES if n != "g_big")  # whose `images` the fixture holds whole


def nine_frames():
    """Nine 96 x 72 frames with nine different masks: no two frames share a box."""
    masks = [blob(), rect(0, 30, 50, W - 1), np.zeros((H, W), np.uint8), dots([(10, 20)]), dots([(10, 20), (13, 24)]),
             graded(), blob(30, 40, 12, 25), blob(80, 12, 30, 9), rect(95, 95, 0, W - 1)]
    return dict(H=H, W=W, pad_ratio=0.0, frames=frames(9, first=20), masks=np.stack(masks))


def golden_positions(side=REF_SIDE):
    """bool [side, side]: where the fixture stores `cropped_images` (rows and columns EDGE in full, every STRIDE-th of
    the rest in row-major order)."""
    keep = (np.arange(side * side) % STRIDE == 0).reshape(side, side)
    keep[list(EDGE), :] = True
    keep[:, list(EDGE)] = True
    return keep


def load_golden():
    """{"<case>/images", "<case>/cropped"}: what the reference returned (tests/golden/make_frame_prep_golden.py)"""
    out = {}
    for name in ("ref_frame_prep.npz", "ref_frame_prep_more.npz"):
        with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name)) as z:
            out.update({k: z[k] for k in z.files if not k.startswith("_")})
    return out
