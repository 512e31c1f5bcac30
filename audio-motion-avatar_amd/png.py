"""PNG clip input: the host side.  Chunk parsing only (struct + zlib.crc32; no Pillow, nothing is inflated here): the
frames of the reference's dataset (imgs_png/%05d.png, samurai_seg/%05d.png) are parsed, each frame's IDAT payloads are
joined into one zlib stream, and records, palettes and streams go up in one copy to one ops.png_decode call.

Not covered: interlaced (Adam7) and 16-bit files, which parse_png refuses; the Adler-32 of the zlib stream, which the
device does not verify (a chunk's CRC is checked here).

PNG clip output (below): save_clip, save_image, save_comparison and write_dataset_clip hand device tensors to
ops.png_encode and write the files it returns; conversion, filtering, deflate and the CRCs happen on the device."""
import ctypes
import os
import struct
import zlib

from . import _lib, clip_io

SIGNATURE = b"\x89PNG\r\n\x1a\n"
MAX_SIDE = 16384
ALLOWED_DEPTHS = {0: (1, 2, 4, 8, 16), 2: (8, 16), 3: (1, 2, 4, 8), 4: (8, 16), 6: (8, 16)}  # the standard's pairs
PngFrame = _lib.STRUCTS["amav_png_frame"]
PNG_RECORD_BYTES = ctypes.sizeof(PngFrame)


class PngError(ValueError):
    """The file is not a PNG this decoder takes (or the device flagged its stream)."""


class PngHeader:
    """What the decoder needs of one file: geometry, the PLTE bytes and where the IDAT payloads lie (byte ranges of the
    file, in file order)."""

    def __init__(self, height, width, color_type, bit_depth, palette, idat):
        self.height, self.width, self.color_type, self.bit_depth = height, width, color_type, bit_depth
        self.palette, self.idat = palette, idat

    @property
    def palette_entries(self):
        return len(self.palette) // 3


def parse_png(data):
    """bytes of one PNG file -> PngHeader.  Ancillary chunks (gAMA, tRNS, tEXt, unknown ones) are skipped, as PIL's
    convert("RGB") / convert("L") ignore them.  Raises PngError for what the module docstring and README list."""
    data = bytes(data) if not isinstance(data, (bytes, bytearray, memoryview)) else data
    if bytes(data[:8]) != SIGNATURE:
        raise PngError("bad PNG signature")
    at, header, palette, idat, idat_closed, ended = 8, None, b"", [], False, False
    while at < len(data):
        if at + 12 > len(data):
            raise PngError(f"truncated chunk at byte {at}")
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        if at + 12 + n > len(data):
            raise PngError(f"chunk {kind!r} at byte {at} runs past the end of the file")
        body = data[at + 8:at + 8 + n]
        if zlib.crc32(data[at + 4:at + 8 + n]) != struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0]:
            raise PngError(f"chunk {kind!r} at byte {at}: CRC mismatch")
        if header is None and kind != b"IHDR":
            raise PngError(f"{kind!r} before IHDR")
        if kind == b"IHDR":
            if header is not None or n != 13:
                raise PngError("misplaced or malformed IHDR")
            width, height, depth, color_type, compression, filter_method, interlace = struct.unpack(">IIBBBBB", body)
            if color_type not in ALLOWED_DEPTHS or depth not in ALLOWED_DEPTHS[color_type]:
                raise PngError(f"colour type {color_type} with bit depth {depth} is not a PNG combination")
            if depth == 16:
                raise PngError("bit depth 16 is not covered")
            if compression != 0 or filter_method != 0:
                raise PngError(f"compression method {compression} / filter method {filter_method} (only 0 / 0 exist)")
            if interlace != 0:
                raise PngError("interlaced (Adam7) files are not covered" if interlace == 1 else f"interlace method {interlace}")
            if not (1 <= width <= MAX_SIDE and 1 <= height <= MAX_SIDE):
                raise PngError(f"size {width}x{height} outside 1..{MAX_SIDE}")
            header = (height, width, color_type, depth)
        elif kind == b"PLTE":
            if idat or palette or n % 3 or not 3 <= n <= 768:
                raise PngError("misplaced or malformed PLTE")
            palette = bytes(body)
        elif kind == b"IDAT":
            if idat_closed:
                raise PngError("IDAT chunks are not consecutive")
            idat.append((at + 8, at + 8 + n))
        elif kind == b"IEND":
            ended = True
            break
        elif not kind[0] & 0x20:
            raise PngError(f"unknown critical chunk {kind!r}")
        if idat and kind != b"IDAT":
            idat_closed = True
        at += 12 + n
    if header is None:
        raise PngError("no IHDR")
    if not idat:
        raise PngError("no IDAT")
    if not ended:
        raise PngError("no IEND")
    if header[2] == 3 and not palette:
        raise PngError("colour type 3 without PLTE")
    return PngHeader(*header, palette if header[2] == 3 else b"", idat)  # elsewhere PLTE is a suggestion, not the pixels


def zlib_stream(data, header):
    """The file's IDAT payloads joined: one zlib stream."""
    return b"".join(bytes(data[a:b]) for a, b in header.idat)


class PngDirReader(clip_io.Reader):
    """A directory of per-frame PNG files.  With the dataset's all-digit stems (00000.png ...) in the order of
    int(stem), otherwise every *.png in name order.  Same shape as mjpeg.DirReader."""

    def __init__(self, path):
        names = sorted(n for n in os.listdir(path) if n.lower().endswith(".png"))
        if not names:
            raise ValueError(f"{path}: no PNG files")
        if all(os.path.splitext(n)[0].isdigit() for n in names):
            names.sort(key=lambda n: int(os.path.splitext(n)[0]))
        self._frames = [os.path.join(path, n) for n in names]
        self.height = self.width = None

    def frame_bytes(self, i):
        with open(self._frames[i], "rb") as fh:
            return fh.read()


class _Blobs(clip_io.Reader):
    """File contents the caller already holds (None = an absent frame), as a reader."""

    def __init__(self, blobs):
        self._frames = blobs

    def frame_bytes(self, i):
        return self._frames[i]


def pack_clip(blobs):
    """PNG files (bytes; None = an absent frame, all 255) -> (host uint8 tensor, table_bytes, height, width): the
    amav_png_frame records first, then the palettes, then each frame's IDAT payloads joined into one zlib stream; a
    record's offsets count from the end of the table (the `stream` of ops.png_decode is buffer[table_bytes:])."""
    import torch

    headers = []
    for i, blob in enumerate(blobs):
        try:
            headers.append(None if blob is None else parse_png(blob))
        except PngError as e:
            raise PngError(f"frame {i}: {e}") from None
    present = [h for h in headers if h is not None]
    if not present:
        raise PngError("pack_clip: at least one frame must be present")
    H, W = present[0].height, present[0].width
    for i, h in enumerate(headers):
        if h is not None and (h.height, h.width) != (H, W):
            raise PngError(f"frames of unequal size in one call: frame {i} is {h.width}x{h.height}, the first is {W}x{H}")
    parts, at, table = [], 0, bytearray()
    palette_at = []
    for h in headers:
        palette_at.append(at)
        if h is not None and h.palette:
            parts.append(h.palette)
            at += len(h.palette)
    for h, blob, pal in zip(headers, blobs, palette_at):
        if h is None:
            table += bytes(PngFrame(bit_depth=8, absent=1))
            continue
        begin = at
        for a, b in h.idat:
            parts.append(bytes(blob[a:b]))
            at += b - a
        table += bytes(PngFrame(zlib_begin=begin, zlib_end=at, palette_at=pal, color_type=h.color_type, bit_depth=h.bit_depth,
                                palette_entries=h.palette_entries))
    host = torch.frombuffer(bytearray(bytes(table) + b"".join(parts)) or bytearray(1), dtype=torch.uint8)
    return host, len(table), H, W


def frame_records(blobs):
    """PNG files -> (ops.PngRecords on the host, the stream bytes as a host uint8 tensor)."""
    from .ops import PngRecords

    host, table_bytes, H, W = pack_clip(blobs)
    return PngRecords(host[:table_bytes], H, W), host[table_bytes:]


def status_text(s):
    from . import ops

    names = [(ops.PNG_STATUS_INFLATE, "inflate"), (ops.PNG_STATUS_SIZE, "size"), (ops.PNG_STATUS_FILTER, "filter")]
    return "+".join(name for bit, name in names if s & bit)


def load_clip(path, frames=None, mode="rgb", device="cuda", layout="chw_f32", check=True):
    """A directory of PNG files (or an open reader, or a list of file contents in which None is an absent frame) ->
    device tensor: mode "rgb": fp32 [F,3,H,W] in [0, 1] (layout "chw_f32") or uint8 [F,H,W,3] ("hwc_u8"); mode "l":
    fp32 [F,1,H,W] or uint8 [F,H,W].  `frames`: indices (default: all).  The files are parsed on the host, one buffer
    goes up in one copy and one ops.png_decode call decodes it.  check=True reads the status words back once and raises
    PngError naming the frames the decoder flagged; check=False returns (tensor, status on the device) without
    synchronising."""
    from . import ops

    picked, blobs = clip_io.read_frames(_Blobs(path) if isinstance(path, (list, tuple)) else path, frames, PngDirReader)
    try:
        host, table_bytes, H, W = pack_clip(blobs)
    except PngError as e:
        raise PngError(f"load_clip: {e}") from None
    out, status = clip_io.decode_uploaded(host, table_bytes, device, lambda stream, table: ops.png_decode(
        stream, ops.PngRecords(table, H, W), mode=mode, layout=layout))
    if not check:
        return out, status
    clip_io.raise_damaged(PngError, picked, status, status_text)
    return out


# ---------------------------------------------------------------------------------------------------------- output
SAVE_CHUNK = 64  # frames per ops.png_encode call: bounds the encoder's workspace for long clips


def save_clip(directory, frames, pattern="%05d.png", start=0, filter="adaptive", rounding="nearest"):
    """Frames on the device (any layout ops.png_encode takes) -> one PNG file per frame, directory/pattern % (start + i).
    One encode call per SAVE_CHUNK frames, one download of its stream (not of the frames), one file write per frame.
    Returns the paths."""
    from . import ops

    os.makedirs(directory, exist_ok=True)
    paths = []
    for at in range(0, frames.shape[0], SAVE_CHUNK):
        stream, offsets = ops.png_encode(frames[at:at + SAVE_CHUNK].contiguous(), filter=filter, rounding=rounding)
        data, offsets = stream.cpu().numpy().tobytes(), offsets.tolist()
        for i in range(len(offsets) - 1):
            paths.append(os.path.join(directory, pattern % (start + at + i)))
            with open(paths[-1], "wb") as fh:
                fh.write(data[offsets[i]:offsets[i + 1]])
    return paths


def normalize_range(tensor):
    """torchvision.utils.make_grid(normalize=True) for one image: clamp to its own (min, max), then
    (x - min) / max(max - min, 1e-5).  Everything stays on the tensor's device."""
    import torch

    x = tensor.to(torch.float32)
    low, high = x.min(), x.max()
    return (x.clamp(min=low, max=high) - low) / (high - low).clamp(min=1e-5)


def _one_image(tensor, who):
    """[H,W], [1,H,W] -> grey [1,H,W]; [3,H,W] -> [1,3,H,W] (what save_image makes of a single image)."""
    if tensor.dim() == 4 and tensor.shape[0] == 1:
        tensor = tensor[0]
    if tensor.dim() == 2:
        tensor = tensor[None]
    if tensor.dim() != 3 or tensor.shape[0] not in (1, 3):
        raise ValueError(f"{who}: need one image [3,H,W], [1,H,W] or [H,W], got {tuple(tensor.shape)}")
    return tensor if tensor.shape[0] == 1 else tensor[None]


def save_image(tensor, path, normalize=False):
    """torchvision.utils.save_image(tensor, path, normalize=normalize) for a single fp32 image on the device: the
    optional min / max normalisation (on the device), then x * 255 + 0.5 clamped and truncated (the encoder's `nearest`
    rule), written as one PNG.  A one-channel image is written as greyscale (torchvision repeats it to RGB; the pixels
    read back with convert("RGB") are the same)."""
    import torch

    from . import ops

    image = _one_image(tensor, "save_image")
    if normalize:
        image = normalize_range(image)
    stream, _ = ops.png_encode(image.to(torch.float32).contiguous(), rounding="nearest")
    with open(path, "wb") as fh:
        fh.write(stream.cpu().numpy().tobytes())


def comparison_sheet(rendered, real):
    """The sheet of lightning_model_wrapper.py:536-570 / :610-638: rendered [T,H,W,3] and real [T,3,H,W] -> [3, T H, 2 W]:
    row t is rendered_t | real_t, the rows stacked downwards."""
    import torch

    rendered = rendered.permute(0, 3, 1, 2).to(torch.float32)
    rows = torch.cat([rendered, real.to(torch.float32)], dim=3)           # [T,3,H,2W]
    return rows.permute(1, 0, 2, 3).reshape(3, rows.shape[0] * rows.shape[2], rows.shape[3])


def save_comparison(path, rendered, real, normalize=True):
    """Write the rendered | real comparison sheet as one PNG: composed on the device with torch operators, normalised as
    save_image(..., normalize=True) does, encoded as one frame."""
    save_image(comparison_sheet(rendered, real), path, normalize=normalize)


def write_dataset_clip(root_dir, frames, masks=None, start=0):
    """Fill root_dir/imgs_png/%05d.png (frames: uint8 [F,H,W,3] or fp32 in any layout ops.png_encode takes) and
    root_dir/samurai_seg/%05d.png (masks: uint8 / fp32 [F,H,W], optional) from frame id `start`, the layout
    clip_data.load_dataset_clip and PngDirReader read back."""
    paths = save_clip(os.path.join(root_dir, "imgs_png"), frames, start=start)
    if masks is not None:
        if masks.dim() == 4 and masks.shape[1] == 1:
            masks = masks[:, 0]
        paths += save_clip(os.path.join(root_dir, "samurai_seg"), masks, start=start)
    return paths
