"""tests/wire_model.py against itself (CPU only): the NumPy statement of the exchange's wire format round-trips, its
named sizes reach the kernel branches they are named for, its quantisation is the documented truncation, and its
differential unpack follows the rule of include/amav.h on a hand-written sequence."""
import numpy as np
import pytest

import wire_model as wm

BGS = [(1.0, 1.0, 1.0), (0.25, 0.5, 0.75)]


@pytest.mark.parametrize("name", list(wm.SIZES))
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_round_trip(name, variant):
    F, H, W = wm.SIZES[name]
    gx, gy, T = wm.geometry(H, W)
    bg = BGS[variant % 2]
    rects, near = wm.scene(name, variant)
    x = wm.frames(F, H, W, bg, rects, seed=variant, near=near)
    want = wm.quant8(x[..., :3])
    m = wm.pack(x, bg, F * T)
    count = int(m["header"][1])
    assert 0 < count == int(m["frame_counts"].sum()) < F * T
    for cap, seed in ((count, None), (count + 7, 3), (F * T, 4)):
        p = wm.recap(m, cap) if seed is None else wm.permute_slots(wm.recap(m, cap), cap, seed)
        buf = wm.to_bytes(p, F, T, cap, stride=wm.wire_bytes(F, H, W, cap) + 32)
        assert buf.size % 16 == 0 and wm.from_bytes(buf, F, T, cap)["payload"].shape == (cap, 768)
        out, status = wm.unpack([buf], F, H, W, cap)
        assert status == 0 and np.array_equal(out, want)
        assert not (out == wm.FILL).any()


@pytest.mark.parametrize("name", list(wm.SIZES))
def test_scenes_hold_the_tiles_the_gpu_cases_rely_on(name):
    F, H, W = wm.SIZES[name]
    gx, gy, T = wm.geometry(H, W)
    bg = BGS[1]
    rects, near = wm.scene(name, 0)
    m = wm.pack(wm.frames(F, H, W, bg, rects, seed=0, near=near), bg, F * T)
    stored = (m["offsets"] >= 0).reshape(F, gy, gx)
    assert (m["frame_counts"] == 0).sum() == 1                      # one frame of pure background
    assert stored[:, :, 0].any() and stored[:, :, gx - 1].any() and stored[:, gy - 1].any()
    flat = stored.reshape(F, T)
    if T > wm.SCAN_ROUND:
        assert (flat[:, wm.SCAN_ROUND - 1] & flat[:, wm.SCAN_ROUND]).any()
    if name in ("WIDE", "TED"):
        assert (stored[:, :, wm.BALLOT - 1] & stored[:, :, wm.BALLOT]).any()
        (f, y0, y1, x0, x1), = near
        assert not stored[f, y0 // 16, x0 // 16], "a tile less than a quantisation step off the background is stored"
        x = wm.frames(F, H, W, bg, rects, seed=0, near=near)
        assert (x[f, y0:y1, x0:x1, :3] != np.asarray(bg, dtype=np.float32)).all()
    # the second clip draws every frame, and tiles of column 64 and of the bottom band come and go between the two
    rects1, near1 = wm.scene(name, 1)
    m1 = wm.pack(wm.frames(F, H, W, bg, rects1, seed=1, near=near1), bg, F * T)
    s1 = (m1["offsets"] >= 0).reshape(F, gy, gx)
    assert (m1["frame_counts"] > 0).all()
    if name in ("WIDE", "TED"):  # the sizes of the delta sequence
        assert (stored[:, gy - 1] & ~s1[:, gy - 1]).any() and (~stored[:, gy - 1] & s1[:, gy - 1]).any()
        assert (stored[:, :, 64] & ~s1[:, :, 64]).any() and (~stored[:, :, 64] & s1[:, :, 64]).any()
    m2 = wm.pack(wm.frames(F, H, W, bg, wm.scene(name, 2)[0], seed=2), bg, F * T)
    assert int(m2["header"][1]) == 2 <= int(m["header"][1]) // 2


def test_geometry_of_the_named_sizes():
    """Each size still reaches the branch it is named for."""
    geo = {n: wm.geometry(H, W) for n, (F, H, W) in wm.SIZES.items()}
    rounds = lambda T: -(-T // wm.SCAN_ROUND)
    assert wm.WIDE == (3, 520, 1040) and geo["WIDE"] == (65, 33, 2145)
    assert rounds(2145) == 3 and 2145 % wm.SCAN_ROUND == 97           # three scan rounds, the last partial
    assert 65 - wm.BALLOT == 1                                        # the second ballot round holds one tile column
    assert 33 > 2 * wm.DELTA_WAVES                                    # a wave of the delta kernel walks three tile rows
    assert 520 % 16 == 8 and 1040 % 16 == 0                           # 8-row bottom band, band + delta kernels
    assert wm.TED == (2, 1296, 2304) and geo["TED"] == (144, 81, 11664)
    assert rounds(11664) == 12 and -(-144 // wm.BALLOT) == 3 and 1296 % 16 == 0 and 2304 % 16 == 0
    assert 48 * 1024 < (11664 + wm.DELTA_WAVES * 128) * 4 <= 64 * 1024  # the delta kernel's LDS table: 54.8 KB
    assert wm.RAGGED4 == (2, 200, 1300) and geo["RAGGED4"] == (82, 13, 1066)
    assert 1300 % 16 != 0 and 1300 % 4 == 0 and 200 % 16 == 8 and 1066 > wm.SCAN_ROUND
    assert wm.RAGGED1 == (2, 200, 1301) and geo["RAGGED1"] == (82, 13, 1066) and 1301 % 4 != 0
    assert wm.SMALL == (2, 40, 48) and geo["SMALL"] == (3, 3, 9)
    assert 3 < wm.BAND_BLOCKS and 40 % 16 == 8 and 48 % 16 == 0
    # rasterizer emission: tiles per binning thread, frame count of the fused binning block
    per = lambda H, W: -(-wm.geometry(H, W)[2] // 1024)
    assert per(*wm.WIDE[1:]) == 3 and wm.WIDE[0] < 96
    assert wm.EMIT_FUSED[0] >= 96 and wm.geometry(*wm.EMIT_FUSED[1:])[2] == 1105 and per(*wm.EMIT_FUSED[1:]) == 2
    assert wm.EMIT_FUSED_SMALL[0] >= 96 and per(*wm.EMIT_FUSED_SMALL[1:]) == 1
    for n, (F, H, W) in wm.SIZES.items():
        T = geo[n][2]
        assert wm.payload_at(F, T) % 16 == 0 and wm.payload_at(F, T) - (16 + F + F * T) * 4 in range(16)
        assert wm.wire_bytes(F, H, W, 5) == wm.ceil16(wm.payload_at(F, T) + 5 * 768)


def quant_table():
    k = np.arange(256)
    exact = (k / 255).astype(np.float32)
    return k, exact, np.nextafter(exact, np.float32(-1)), np.nextafter(exact, np.float32(2))


def test_quantisation_table():
    k, exact, below, above = quant_table()
    assert np.array_equal(wm.quant8(exact), k)
    assert np.array_equal(wm.quant8(below)[1:], k[1:] - 1) and wm.quant8(below)[0] == 0
    assert np.array_equal(wm.quant8(above)[:255], k[:255]) and wm.quant8(above)[255] == 255
    special = np.array([-0.0, -1, 1, 1 + 2.0 ** -23, 2, 255, np.inf, -np.inf, np.nan], dtype=np.float32)
    assert wm.quant8(special).tolist() == [0, 0, 255, 255, 255, 255, 255, 0, 0]
    assert wm.bg_word((0.25, 0.5, 0.75)) == 63 | (127 << 8) | (191 << 16) and wm.bg_word((1, 1, 1)) == 0x00FFFFFF
    assert wm.bg_word((np.nan, -3.0, 7.0)) == 0x00FF0000


def test_delta_rule_on_a_hand_written_sequence():
    """2 x 2 tiles, one frame, two buffers: tiles appear, disappear, the background changes, one sender is truncated.
    After every step the reused buffer equals a full unpack and the state is what the rule says."""
    F, H, W = 1, 32, 32
    T, nb = 4, 2
    white, other = (1.0, 1.0, 1.0), (0.25, 0.5, 0.75)
    ww, wo = wm.bg_word(white), wm.bg_word(other)
    tile = lambda t: wm.tile_rect(0, t // 2, t % 2, H, W)

    def wires(tiles_a, tiles_b, bg, cap, seed):
        bufs = []
        for i, ts in enumerate((tiles_a, tiles_b)):
            x = wm.frames(F, H, W, bg, [tile(t) for t in ts], seed=seed + i)
            bufs.append(wm.to_bytes(wm.pack(x, bg, cap), F, T, cap))
        return bufs

    out = np.random.default_rng(0).integers(0, 255, (nb * F, H, W, 3), dtype=np.uint8)
    state = np.full(nb * F * T, -1, dtype=np.int32)
    steps = [  # tiles of buffer 0, of buffer 1, background, capacity, expected state, expected status
        ((0, 3), (1,), white, 4, [-1, ww, ww, -1, ww, -1, ww, ww], 0),
        ((0, 3), (1,), white, 4, [-1, ww, ww, -1, ww, -1, ww, ww], 0),     # unchanged: only stored tiles are written
        ((1,), (), white, 4, [ww, -1, ww, ww, ww, ww, ww, ww], 0),         # tiles 0 and 3 disappear, tile 1 appears
        ((1,), (), other, 4, [wo, -1, wo, wo, wo, wo, wo, wo], 0),         # every background tile is cleared again
        ((0, 3), (1,), white, 4, [-1, ww, ww, -1, ww, -1, ww, ww], 0),
        ((0, 1, 3), (1,), white, 1, [-1, ww, ww, ww, ww, -1, ww, ww], 1),  # cap 1: buffer 0 keeps only its first tile
    ]
    for i, (ta, tb, bg, cap, want_state, want_status) in enumerate(steps):
        bufs = wires(ta, tb, bg, cap, seed=10 * i)
        want, st_full = wm.unpack(bufs, F, H, W, cap)
        before = out.copy()
        if i == 1:
            out[0, 16:32, 0:16] = 7      # tile 2 of buffer 0: background, holds this background already
        status = wm.unpack_delta(bufs, F, H, W, cap, out, state)
        if i == 1:
            assert (out[0, 16:32, 0:16] == 7).all(), "an unchanged background tile was rewritten"
            out[0, 16:32, 0:16] = before[0, 16:32, 0:16]
        assert np.array_equal(out, want), f"step {i}"
        assert state.tolist() == want_state, f"step {i}"
        assert status == want_status == st_full, f"step {i}"
    # the truncated step really dropped tiles 1 and 3 of buffer 0: they read as background
    assert (out[0, 0:16, 16:32] == 255).all() and (out[0, 16:32, 16:32] == 255).all()
