"""The frame exchange's tile-sparse wire format (include/amav.h, "Tile-sparse form of the same exchange") in plain NumPy:
an independent, byte-exact statement of what csrc/frames.hip and the rasterizer's direct emission write and read.  No
torch device use and no HIP library: tests/test_wire_model.py checks it against itself on the CPU,
tests/test_frame_wire_gpu.py checks the kernels against it.  Every comparison is an equality.

  wire = int32 header[16] {magic, count, cap, F, T, H, W, background 0x00BBGGRR, 0 x 8}
       | int32 frame_counts[F]          stored tiles of every frame
       | int32 offsets[F * T]           slot of every tile in the payload, -1 = background tile
       | padding to a multiple of 16 bytes
       | uint8 payload[cap][16 * 16 * 3]  a tile = 16 rows x 16 pixels x RGB; pixels outside the image hold background
       | padding to a multiple of 16 bytes
`count` and `frame_counts` are the UNCAPPED totals and the slots of the pack are the exclusive running index in
(frame, tile) order, also uncapped: a reader ignores slots >= cap (the tile reads as background) and raises its status
when count > cap.  Padding and unused slots are unspecified (to_bytes fills them with 0xA5 so a reader that touches them
is caught); a writer may hand out the slots in any order (the rasterizer does), readers go through `offsets`.
"""
import numpy as np

MAGIC = 0x414D4156
HEADER_INTS = 16
TILE = 16
TILE_BYTES = TILE * TILE * 3
FILL = 0xA5
SCAN_ROUND = 1024    # tile_scan_kernel scans a frame's flags in rounds of this many tiles
BALLOT = 64          # tile_unpack_delta_kernel compacts a tile row in rounds of this many tile columns
DELTA_WAVES = 16     # ... with this many waves per frame, wave w walking tile rows w, w + 16, ...
BAND_BLOCKS = 4      # tile_unpack_rows_kernel launches min(gy, 4) blocks per frame

# (F, H, W) of the GPU cases; tests/test_wire_model.py asserts the property each one is named for
WIDE = (3, 520, 1040)     # gx 65, gy 33, T 2145: 3 scan rounds (last partial), 2nd ballot round of one column, 33 rows > 2 x 16 waves, 8-row bottom band, band + delta kernels
TED = (2, 1296, 2304)     # the reference's own frame: 12 scan rounds, 3 ballot rounds, 54.8 KB delta LDS table
RAGGED4 = (2, 200, 1300)  # W % 16 != 0, W % 4 == 0: general unpack kernel with word stores, T = 1066 > 1024
RAGGED1 = (2, 200, 1301)  # W % 4 != 0: general unpack kernel with byte stores
SMALL = (2, 40, 48)       # gy 3 < the band kernel's 4 blocks per frame, 8-row bottom band
SIZES = dict(WIDE=WIDE, TED=TED, RAGGED4=RAGGED4, RAGGED1=RAGGED1, SMALL=SMALL)
# rasterizer emission (F, H, W): bin_kernel hands ceil(T / 1024) tiles to every thread
EMIT_FUSED = (96, 272, 1040)  # fused per-frame binning block (F >= 96) with T = 1105: 2 tiles per thread
EMIT_FUSED_SMALL = (96, 64, 96)  # fused binning block, T = 24: most threads own no tile


def geometry(H, W):
    """(gx, gy, T): tile columns, tile rows, tiles per frame."""
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    return gx, gy, gx * gy


def quant8(x):
    """fp32 -> uint8 as (frame * 255).astype(uint8) after a clamp to [0, 1]; NaN reads as 0 (fmaxf(NaN, 0) = 0)."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        c = np.where(np.isnan(x), np.float32(0), x)
        c = np.minimum(np.maximum(c, np.float32(0)), np.float32(1))
        return (c * np.float32(255)).astype(np.uint8)


def bg_word(bg3):
    r, g, b = (int(v) for v in quant8(np.asarray(bg3, dtype=np.float32)))
    return r | (g << 8) | (b << 16)


def bg_bytes(bgw):
    return np.array([bgw & 255, (bgw >> 8) & 255, (bgw >> 16) & 255], dtype=np.uint8)


def tiles_of(rgb8, bgw):
    """uint8 [F, H, W, 3] -> [F, gy, gx, 16, 16, 3]; out-of-image pixels read as background."""
    F, H, W, _ = rgb8.shape
    gx, gy, _ = geometry(H, W)
    full = np.empty((F, gy * TILE, gx * TILE, 3), dtype=np.uint8)
    full[...] = bg_bytes(bgw)
    full[:, :H, :W] = rgb8
    return np.ascontiguousarray(full.reshape(F, gy, TILE, gx, TILE, 3).transpose(0, 1, 3, 2, 4, 5))


def untile(tiles, H, W):
    """[F, gy, gx, 16, 16, 3] -> [F, H, W, 3] (cropped to the image)."""
    F, gy, gx = tiles.shape[:3]
    return np.ascontiguousarray(tiles.transpose(0, 1, 3, 2, 4, 5).reshape(F, gy * TILE, gx * TILE, 3)[:, :H, :W])


def pack(rgba, bg, cap, hint=None):
    """fp32 RGBA [F, H, W, 4] -> dict(header int32[16], frame_counts int32[F], offsets int32[F*T],
    payload uint8[min(count, cap), 768]).  A tile is stored when any quantised byte differs from the background bytes,
    or, with a hint (int [F*T]), when its hint is non-zero."""
    rgba = np.asarray(rgba, dtype=np.float32)
    F, H, W, _ = rgba.shape
    gx, gy, T = geometry(H, W)
    bgw = bg_word(bg)
    tiles = tiles_of(quant8(rgba[..., :3]), bgw).reshape(F * T, TILE_BYTES)
    if hint is None:
        flags = (tiles.reshape(F * T, TILE * TILE, 3) != bg_bytes(bgw)).any(axis=(1, 2))
    else:
        flags = np.asarray(hint).reshape(F * T) != 0
    slots = np.cumsum(flags, dtype=np.int64) - flags            # exclusive running index, uncapped
    count = int(flags.sum())
    header = np.zeros(HEADER_INTS, dtype=np.int32)
    header[:8] = np.array([MAGIC, count, cap, F, T, H, W, bgw], dtype=np.int64).astype(np.int32)
    return dict(header=header, frame_counts=flags.reshape(F, T).sum(axis=1).astype(np.int32),
                offsets=np.where(flags, slots, -1).astype(np.int32), payload=tiles[flags][:min(count, cap)].copy())


def recap(packed, cap):
    """The same clip packed with another capacity (what pack(..., cap) returns, without quantising again)."""
    header = packed["header"].copy()
    header[2] = cap
    assert packed["payload"].shape[0] >= min(int(header[1]), cap)
    return dict(header=header, frame_counts=packed["frame_counts"].copy(), offsets=packed["offsets"].copy(),
                payload=packed["payload"][:min(int(header[1]), cap)].copy())


def permute_slots(packed, cap, seed, fill=FILL):
    """The stored tiles scattered over all `cap` slots in a random order (slots >= cap stay dropped): another valid
    wire of the same frames, the form a writer that hands out slots in completion order produces.  Unused slots hold
    `fill`."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(cap).astype(np.int32)
    off = packed["offsets"]
    kept = (off >= 0) & (off < cap)
    new_off = off.copy()
    new_off[kept] = perm[off[kept]]
    payload = np.full((cap, TILE_BYTES), fill, dtype=np.uint8)
    n = packed["payload"].shape[0]
    payload[perm[:n]] = packed["payload"]
    return dict(header=packed["header"].copy(), frame_counts=packed["frame_counts"].copy(), offsets=new_off,
                payload=payload)


def ceil16(n):
    return (n + 15) // 16 * 16


def payload_at(F, T):
    return ceil16((HEADER_INTS + F + F * T) * 4)


def wire_bytes(F, H, W, cap):
    return ceil16(payload_at(F, geometry(H, W)[2]) + cap * TILE_BYTES)


def to_bytes(packed, F, T, cap, stride=None, fill=FILL):
    """The wire buffer as bytes (uint8 [stride or total]); padding and unused slots hold `fill`."""
    at = payload_at(F, T)
    total = ceil16(at + cap * TILE_BYTES)
    buf = np.full(total if stride is None else stride, fill, dtype=np.uint8)
    assert buf.size >= total and packed["frame_counts"].size == F and packed["offsets"].size == F * T
    ints = np.concatenate([packed["header"], packed["frame_counts"], packed["offsets"]]).astype(np.int32)
    buf[:ints.size * 4] = ints.view(np.uint8)
    n = packed["payload"].shape[0]
    assert n <= cap
    buf[at:at + n * TILE_BYTES] = packed["payload"].reshape(-1)
    return buf


def from_bytes(buf, F, T, cap):
    """Views of a wire buffer's parts; payload is all `cap` slots."""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    ints = buf[:(HEADER_INTS + F + F * T) * 4].view(np.int32)
    at = payload_at(F, T)
    return dict(header=ints[:HEADER_INTS], frame_counts=ints[HEADER_INTS:HEADER_INTS + F],
                offsets=ints[HEADER_INTS + F:], payload=buf[at:at + cap * TILE_BYTES].reshape(cap, TILE_BYTES))


def _unpack_one(buf, F, H, W, cap):
    gx, gy, T = geometry(H, W)
    p = from_bytes(buf, F, T, cap)
    bgw = int(p["header"][7]) & 0x00FFFFFF
    tiles = np.empty((F * T, TILE * TILE, 3), dtype=np.uint8)
    tiles[...] = bg_bytes(bgw)
    off = p["offsets"]
    stored = (off >= 0) & (off < cap)
    tiles[stored] = p["payload"][off[stored]].reshape(-1, TILE * TILE, 3)
    bad = int(p["header"][0]) != MAGIC or int(p["header"][1]) > cap
    return untile(tiles.reshape(F, gy, gx, TILE, TILE, 3), H, W), stored.reshape(F, gy, gx), bgw, bad


def unpack(buffers, F, H, W, cap):
    """Gathered wire buffers -> (dense uint8 [nb*F, H, W, 3], status).  A slot in [0, cap) gives the payload tile
    cropped to the image, anything else that buffer's own background; status 1 = a bad magic or a truncated sender."""
    outs, status = [], 0
    for buf in buffers:
        dense, _, _, bad = _unpack_one(buf, F, H, W, cap)
        outs.append(dense)
        status |= int(bad)
    return np.concatenate(outs), status


def unpack_delta(buffers, F, H, W, cap, out, state):
    """The differential unpack into a reused `out` (uint8 [nb*F, H, W, 3]) with its `state` (int32 [nb*F*T]), both
    updated in place: a stored tile writes the payload and sets the state to -1; a tile that is not stored and whose
    state is not this buffer's background word writes background and sets the state to it; every other tile is left
    alone.  Returns the status."""
    gx, gy, T = geometry(H, W)
    st = state.reshape(len(buffers), F, gy, gx)
    status = 0
    for b, buf in enumerate(buffers):
        dense, stored, bgw, bad = _unpack_one(buf, F, H, W, cap)
        status |= int(bad)
        clear = ~stored & (st[b] != bgw)
        write = np.repeat(np.repeat(stored | clear, TILE, axis=1), TILE, axis=2)[:, :H, :W]
        view = out[b * F:(b + 1) * F]
        view[write] = dense[write]
        st[b][stored] = -1
        st[b][clear] = bgw
    return status


def frames(F, H, W, bg, rects, seed, near=()):
    """Deterministic synthetic fp32 RGBA [F, H, W, 4]: background everywhere (alpha 0), uniform-random RGB (alpha 1) in
    every (frame, y0, y1, x0, x1) of `rects`, background + 1e-4 in every rectangle of `near`.  No random value
    quantises to the byte to_bytes() fills unused space with, so a leak of the fill is visible in the output."""
    rng = np.random.default_rng(seed)
    x = np.empty((F, H, W, 4), dtype=np.float32)
    x[..., :3] = np.asarray(bg, dtype=np.float32)
    x[..., 3] = 0
    for f, y0, y1, x0, x1 in rects:
        v = rng.random((y1 - y0, x1 - x0, 3), dtype=np.float32)
        v[quant8(v) == FILL] = 0
        x[f, y0:y1, x0:x1, :3] = v
        x[f, y0:y1, x0:x1, 3] = 1
    for f, y0, y1, x0, x1 in near:
        x[f, y0:y1, x0:x1, :3] = np.asarray(bg, dtype=np.float32) + np.float32(1e-4)
    return x


def tile_rect(f, ty, tx, H, W, inset=0):
    """(frame, y0, y1, x0, x1) of tile (ty, tx), shrunk by `inset` pixels on every side and cropped to the image."""
    y0, x0 = ty * TILE + inset, tx * TILE + inset
    y1, x1 = min(H, (ty + 1) * TILE - inset), min(W, (tx + 1) * TILE - inset)
    assert y0 < y1 and x0 < x1
    return (f, y0, y1, x0, x1)


def scene(name, variant=0):
    """(rects, near) of the test clip `variant` of a named size.
      0: frame 0 pure background (frame 1 for F = 3, between two drawn frames); tiles in column 0, column gx - 1, the
         bottom tile row, on both sides of tile index 1023 / 1024 and of tile column 63 / 64 where the size has them,
         one block of several tiles, and (near) one tile a tenth of a quantisation step off the background
      1: every frame drawn (the scan's carry across frames is non-zero), the same kinds of tiles at other places, so
         tiles of column 64 and of the bottom band appear and disappear between the two
      2: two tiles only (the well-behaved neighbour of a truncated sender)"""
    F, H, W = SIZES[name]
    gx, gy, T = geometry(H, W)
    R = lambda f, ty, tx, inset=0: tile_rect(f, ty, tx, H, W, inset)
    last = F - 1
    if variant == 2:
        return [R(last, 0, gx - 1, 2), R(0, gy - 1, 0)], []
    rects, near = [], []
    drawn = [f for f in range(F) if variant == 1 or f != (1 if F == 3 else 0)]
    shift = variant  # moves every tile of variant 1 away from variant 0's
    for i, f in enumerate(drawn):
        rects += [R(f, (1 + shift + i) % gy, 0, 3), R(f, (2 * shift + i) % gy, gx - 1, 1),
                  R(f, gy - 1, (gx // 2 + 5 * shift + i) % gx), R(f, gy - 1, gx - 1 - shift)]
        if T > SCAN_ROUND:
            for t in (SCAN_ROUND - 1, SCAN_ROUND) if variant == 0 else (SCAN_ROUND - 2, SCAN_ROUND + 1):
                rects.append(R(f, t // gx, t % gx, 2))
        if gx > BALLOT:
            row = (2 + 3 * shift + i) % gy
            rects += [R(f, row, BALLOT - 1), R(f, row, BALLOT, 4), R(f, (row + DELTA_WAVES) % gy, BALLOT)]
        if gx > 2 * BALLOT:
            rects += [R(f, (4 + shift) % gy, 2 * BALLOT - 1, 1), R(f, (4 + shift) % gy, 2 * BALLOT), R(f, gy - 1, gx - 2)]
        # a block of several tiles with ragged edges
        y0, x0 = min(H - 2, 20 + 16 * shift), min(W - 2, 23 + 48 * shift)
        rects.append((f, y0, min(H, y0 + 37), x0, min(W, x0 + 45)))
    if name in ("WIDE", "TED"):
        near.append(R(drawn[-1], 6, 7))
    return rects, near
