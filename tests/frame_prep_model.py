"""NumPy model of amav_frames_prepare (include/amav.h): the box arithmetic in Python ints, the composite and the bilinear
in fp32 with one rounding per operator exactly as the header states them, and the bilinear once more in float64 from the
same fp32 weights and taps (what the kernel's fp32 result is measured against)."""
import numpy as np

f32 = np.float32


def padded_size(h, w, pad_ratio):
    hp, wp = int(h * (1 + pad_ratio)), int(w * (1 + pad_ratio))  # pad_image, in doubles
    return hp, wp, (hp - h) // 2, (wp - w) // 2


def box(mask, h, w, hp, wp):
    """(y_min, y_max, x_min, x_max, max_size) of one frame; mask: [h,w] array or None (all ones)."""
    if mask is None:
        ys, xs = np.arange(h), np.arange(w)
    else:
        ys, xs = np.flatnonzero((mask != 0).any(axis=1)), np.flatnonzero((mask != 0).any(axis=0))
    if len(ys) == 0:
        y0, y1, x0, x1 = 0, hp - 1, 0, wp - 1
    else:
        y0, y1, x0, x1 = int(ys[0]), int(ys[-1]), int(xs[0]), int(xs[-1])
        py, px = (y1 - y0) // 5, (x1 - x0) // 5
        y0, y1, x0, x1 = max(0, y0 - py), min(h - 1, y1 + py), max(0, x0 - px), min(w - 1, x1 + px)
        half, cy, cx = max(y1 - y0, x1 - x0) // 2, (y0 + y1) // 2, (x0 + x1) // 2
        y0, y1, x0, x1 = max(0, cy - half), min(h - 1, cy + half), max(0, cx - half), min(w - 1, cx + half)
    return y0, y1, x0, x1, max(y1 - y0, x1 - x0) + 1


def to_unit(a):
    """uint8 -> byte / 255 in fp32 (a true division); fp32 stays"""
    return a if a.dtype == np.float32 else a.astype(f32) / f32(255.0)


def images(frame, mask, pad_ratio):
    """frame: uint8 [h,w,3] or fp32 [3,h,w]; mask: uint8 / fp32 [h,w] or None -> fp32 [3,hp,wp]"""
    img = to_unit(frame.transpose(2, 0, 1) if frame.dtype == np.uint8 else frame)
    _, h, w = img.shape
    m = np.ones((h, w), f32) if mask is None else to_unit(mask)
    hp, wp, oy, ox = padded_size(h, w, pad_ratio)
    out = np.ones((3, hp, wp), f32)
    out[:, oy:oy + h, ox:ox + w] = img * m + (f32(1.0) - m)
    return out


def square(padded, b):
    y0, y1, x0, x1, side = b
    crop = padded[:, y0:y1 + 1, x0:x1 + 1]
    h, w = crop.shape[1:]
    top, left = (side - h) // 2, (side - w) // 2
    out = np.ones((3, side, side), f32)
    out[:, top:top + h, left:left + w] = crop
    return out


def _axis(side, s):
    scale = f32(side - 1) / f32(s - 1) if s > 1 else f32(0.0)
    src = scale * np.arange(s, dtype=f32)
    i0 = src.astype(np.int32)
    w1 = src - i0.astype(f32)
    return i0, np.minimum(i0 + 1, side - 1), f32(1.0) - w1, w1


def cropped(padded, b, s, wide=False):
    """bilinear, align_corners=True, of the squared crop: fp32 [3,s,s] (wide: float64 from the same weights and taps)"""
    sq = square(padded, b)
    i0, i1, a0, a1 = _axis(b[4], s)
    if wide:
        sq, a0, a1 = sq.astype(np.float64), a0.astype(np.float64), a1.astype(np.float64)
    top, bottom = sq[:, i0], sq[:, i1]
    w0, w1, h0, h1 = a0[None, None, :], a1[None, None, :], a0[None, :, None], a1[None, :, None]
    return h0 * (w0 * top[:, :, i0] + w1 * top[:, :, i1]) + h1 * (w0 * bottom[:, :, i0] + w1 * bottom[:, :, i1])


def prepare(case, s, wide=False, normalize=None):
    """A whole case of frame_prep_cases: (images list, cropped [F,3,s,s], boxes int32 [F,5])"""
    out_i, out_c, out_b = [], [], []
    for f in range(case["frames"].shape[0]):
        mask = None if case["masks"] is None else case["masks"][f]
        img = images(case["frames"][f], mask, case["pad_ratio"])
        h, w = (case["frames"].shape[1:3] if case["frames"].dtype == np.uint8 else case["frames"].shape[2:4])
        b = box(mask, h, w, img.shape[1], img.shape[2])
        c = cropped(img, b, s, wide)
        if normalize is not None:
            mean, std = (np.asarray(v, c.dtype)[:, None, None] for v in normalize)
            c = (c - mean) / std
        out_i.append(img), out_c.append(c), out_b.append(b)
    return out_i, np.stack(out_c), np.asarray(out_b, np.int32)
