"""The frame exchange's wire kernels (csrc/frames.hip, the wire emission of csrc/rasterizer.hip) against the byte-exact
NumPy model of the format in tests/wire_model.py, at the sizes that take the branches 512 x 512 frames never reach:
several scan rounds per frame, tile rows wider than one ballot, the delta kernel's 54.8 KB LDS table, partial bottom
bands, the general unpack kernel's word and byte stores past 1024 tiles, several tiles per binning thread.  Every
comparison is an equality of bytes on the host; nothing is checked through the project's own pack / unpack pair."""
import functools

import numpy as np
import pytest
import torch

import wire_model as wm
from helpers import random_scene

pytestmark = pytest.mark.gpu

BGS = [(1.0, 1.0, 1.0), (0.25, 0.5, 0.75)]
PACK_CASES = {"white-clip0": (0, 0), "colour-clip0": (1, 0), "colour-clip1": (1, 1)}  # (background, clip variant)
NAMES = list(wm.SIZES)
DELTA_NAMES = ["WIDE", "TED", "SMALL"]  # the delta kernel takes widths that are multiples of 16 only
UNPACK_FORMS = [(n, False) for n in NAMES] + [(n, True) for n in DELTA_NAMES]
UNPACK_IDS = [f"{n}-{'delta' if d else 'full'}" for n, d in UNPACK_FORMS]


@functools.lru_cache(maxsize=None)
def clip(name, variant, bgi):
    """(fp32 frames, the model's pack of them at full capacity) of a named size; computed once, never modified."""
    F, H, W = wm.SIZES[name]
    rects, near = wm.scene(name, variant)
    x = wm.frames(F, H, W, BGS[bgi], rects, seed=17 * variant + bgi, near=near)
    m = wm.pack(x, BGS[bgi], F * wm.geometry(H, W)[2])
    x.setflags(write=False)
    return x, m


def host(t):
    return t.detach().cpu().numpy()


def device(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()  # a copy: the cached clips are read-only


def assert_wire_equals(got, want, n_payload, what):
    for key in ("header", "frame_counts", "offsets"):
        assert np.array_equal(got[key], want[key]), f"{what}: {key}"
    assert np.array_equal(got["payload"][:n_payload], want["payload"][:n_payload]), f"{what}: payload"


# ---------------------------------------------------------------------------------------------------------- pack
@pytest.mark.parametrize("case", list(PACK_CASES))
@pytest.mark.parametrize("name", NAMES)
def test_pack_equals_the_model(name, case):
    from audio_motion_avatar_amd import ops

    bgi, variant = PACK_CASES[case]
    bg = BGS[bgi]
    F, H, W = wm.SIZES[name]
    T = wm.geometry(H, W)[2]
    x_host, m = clip(name, variant, bgi)
    x = device(x_host)
    count = int(m["header"][1])
    assert 4 <= count < F * T
    # capacity 0 only counts
    got = wm.from_bytes(host(ops.frames_pack_tiles(x, 0, bg)), F, T, 0)
    assert_wire_equals(got, wm.recap(m, 0), 0, "cap 0")
    assert ops.frames_wire_count(ops.frames_pack_tiles(x, 0, bg)) == (count, 0)
    for cap in (count, count + 7, F * T):
        wire = ops.frames_pack_tiles(x, cap, bg)
        assert wire.numel() == wm.wire_bytes(F, H, W, cap)
        assert_wire_equals(wm.from_bytes(host(wire), F, T, cap), wm.recap(m, cap), count, f"cap {cap}")
    # a truncated pack: the header says so, the offsets are the uncapped ones, the first `cap` tiles are there
    cap = count // 2
    got = wm.from_bytes(host(ops.frames_pack_tiles(x, cap, bg)), F, T, cap)
    assert int(got["header"][1]) == count > int(got["header"][2]) == cap
    assert_wire_equals(got, wm.recap(m, cap), cap, "truncated")


@pytest.mark.parametrize("name", NAMES)
def test_pack_with_a_tile_hint_equals_the_model(name):
    """The hint is a strict superset of the tiles that differ: the extra tiles are stored and hold background bytes."""
    from audio_motion_avatar_amd import ops

    bg = BGS[1]
    F, H, W = wm.SIZES[name]
    T = wm.geometry(H, W)[2]
    x_host, m = clip(name, 1, 1)
    flagged = m["offsets"] >= 0
    hint = np.where(flagged, 1 + np.arange(F * T) % 5, 0).astype(np.int32)
    hint[::7] = np.where(hint[::7] == 0, -3, hint[::7])          # any non-zero value selects the tile
    assert (flagged <= (hint != 0)).all() and int((hint != 0).sum()) > int(flagged.sum())
    cap = int((hint != 0).sum())
    mh = wm.pack(x_host, bg, cap, hint)
    extra = mh["payload"][mh["offsets"][(hint != 0) & ~flagged]].reshape(-1, 256, 3)
    assert int(mh["header"][1]) == cap and (extra == wm.bg_bytes(wm.bg_word(bg))).all()
    wire = ops.frames_pack_tiles(device(x_host), cap, bg, tile_hint=device(hint))
    assert_wire_equals(wm.from_bytes(host(wire), F, T, cap), mh, cap, "hinted")


# -------------------------------------------------------------------------------------------------------- unpack
def model_wires(name, specs, cap, stride=None):
    """Model-built wire buffers [nb, stride] of clips (variant, background, permutation seed or None); clips of more
    than `cap` tiles are truncated senders."""
    F, H, W = wm.SIZES[name]
    T = wm.geometry(H, W)[2]
    bufs = []
    for variant, bgi, seed in specs:
        p = wm.recap(clip(name, variant, bgi)[1], cap)
        if seed is not None:
            p = wm.permute_slots(p, cap, seed)
        bufs.append(wm.to_bytes(p, F, T, cap, stride=stride))
    return np.stack(bufs)


def max_count(name, specs):
    return max(int(clip(name, v, b)[1]["header"][1]) for v, b, _ in specs)


@pytest.mark.parametrize("name", NAMES)
def test_unpack_of_device_packed_wires_equals_the_model(name):
    """Two buffers of different content and different backgrounds in rows of need + 32 bytes."""
    from audio_motion_avatar_amd import ops

    F, H, W = wm.SIZES[name]
    specs = [(0, 0, None), (1, 1, None)]
    cap = max_count(name, specs) + 3
    need = wm.wire_bytes(F, H, W, cap)
    wires = torch.full((2, need + 32), wm.FILL, dtype=torch.uint8, device="cuda")
    for b, (variant, bgi, _) in enumerate(specs):
        ops.frames_pack_tiles(device(clip(name, variant, bgi)[0]), cap, BGS[bgi], wire=wires[b])
    out, status = ops.frames_unpack_tiles(wires, 2, F, H, W, cap)
    want, want_status = wm.unpack(model_wires(name, specs, cap), F, H, W, cap)
    assert np.array_equal(host(out), want) and int(status.item()) == want_status == 0
    assert np.array_equal(want[:F], wm.quant8(clip(name, 0, 0)[0][..., :3]))


@pytest.mark.parametrize("name,delta", UNPACK_FORMS, ids=UNPACK_IDS)
def test_unpack_of_permuted_model_wires(name, delta):
    """Wires with the slots in random order over the whole capacity (the form the rasterizer emits), unused slots and
    padding filled with 0xA5, through the full unpack and through the delta form with a fresh state."""
    from audio_motion_avatar_amd import ops

    F, H, W = wm.SIZES[name]
    specs = [(0, 1, 5), (1, 0, 6)]
    cap = max_count(name, specs) + 7
    bufs = model_wires(name, specs, cap, stride=wm.wire_bytes(F, H, W, cap) + 32)
    want, _ = wm.unpack(bufs, F, H, W, cap)
    assert not (want == wm.FILL).any()
    out = torch.full((2 * F, H, W, 3), wm.FILL, dtype=torch.uint8, device="cuda")
    state = ops.frames_tile_state(2, F, H, W, "cuda") if delta else None
    _, status = ops.frames_unpack_tiles(device(bufs), 2, F, H, W, cap, out=out, state=state)
    got = host(out)
    assert not (got == wm.FILL).any(), "the unpack left bytes unwritten or read unused space"
    assert np.array_equal(got, want) and int(status.item()) == 0
    if delta:
        st = np.full(state.numel(), -1, dtype=np.int32)
        wm.unpack_delta(bufs, F, H, W, cap, np.zeros_like(want), st)
        assert np.array_equal(host(state), st)


@pytest.mark.parametrize("name,delta", UNPACK_FORMS, ids=UNPACK_IDS)
def test_unpack_reports_a_truncated_sender_and_a_wrong_magic(name, delta):
    from audio_motion_avatar_amd import ops

    F, H, W = wm.SIZES[name]
    T = wm.geometry(H, W)[2]
    specs = [(2, 0, 8), (0, 1, 9)]                     # buffer 1 sends half of its tiles
    cap = int(clip(name, 0, 1)[1]["header"][1]) // 2
    assert int(clip(name, 2, 0)[1]["header"][1]) <= cap < int(clip(name, 0, 1)[1]["header"][1])
    bufs = model_wires(name, specs, cap)
    want, want_status = wm.unpack(bufs, F, H, W, cap)
    assert want_status == 1
    full, _ = wm.unpack(model_wires(name, specs, F * T), F, H, W, F * T)
    assert not np.array_equal(want, full) and np.array_equal(want[:F], full[:F])  # dropped tiles read as background

    def run(b):
        out = torch.full((2 * F, H, W, 3), wm.FILL, dtype=torch.uint8, device="cuda")
        state = ops.frames_tile_state(2, F, H, W, "cuda") if delta else None
        _, status = ops.frames_unpack_tiles(device(b), 2, F, H, W, cap, out=out, state=state)
        return host(out), int(status.item())

    got, status = run(bufs)
    assert np.array_equal(got, want) and status == 1
    # a wrong magic in one buffer of two that are otherwise fine
    fine = model_wires(name, [(2, 0, 8), (2, 1, 9)], cap)
    want_fine, st = wm.unpack(fine, F, H, W, cap)
    got, status = run(fine)
    assert np.array_equal(got, want_fine) and status == st == 0
    bad = fine.copy()
    bad[1, 0] ^= 1
    assert wm.unpack(bad, F, H, W, cap)[1] == 1
    assert run(bad)[1] == 1


def test_unpack_into_a_4_byte_aligned_output_takes_the_general_kernel():
    """WIDE (W % 16 == 0) into an output that starts 4 bytes into its storage: not 16-byte aligned, so the general
    kernel runs with its word stores."""
    from audio_motion_avatar_amd import ops

    F, H, W = wm.WIDE
    specs = [(0, 1, 5), (1, 0, 6)]
    cap = max_count("WIDE", specs) + 7
    bufs = model_wires("WIDE", specs, cap)
    want, _ = wm.unpack(bufs, F, H, W, cap)
    n = want.size
    storage = torch.full((n + 32,), wm.FILL, dtype=torch.uint8, device="cuda")
    out = storage[4:4 + n].view(2 * F, H, W, 3)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    _, status = ops.frames_unpack_tiles(device(bufs), 2, F, H, W, cap, out=out)
    got = host(storage)
    assert np.array_equal(got[4:4 + n].reshape(want.shape), want) and int(status.item()) == 0
    assert (got[:4] == wm.FILL).all() and (got[4 + n:] == wm.FILL).all(), "bytes outside the output were written"


# ------------------------------------------------------------------------------------------------ delta sequence
@pytest.mark.parametrize("name", ["WIDE", "TED"])
def test_delta_sequence_equals_the_model(name):
    """A reused output buffer over six steps, device `out` and `state` compared with the model's after every step:
    fresh state over garbage; the same wires again (two poisoned background tiles, one in tile column 64 and one in the
    bottom band, must survive); tiles of column 64 and of the bottom band appear and disappear; the background changes;
    back to the first; a truncated sender."""
    from audio_motion_avatar_amd import ops

    F, H, W = wm.SIZES[name]
    gx, gy, T = wm.geometry(H, W)
    nb = 2
    full = max_count(name, [(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0)]) + 7
    half = int(clip(name, 0, 0)[1]["header"][1]) // 2
    steps = [([(0, 0, 1), (1, 0, 2)], full), ([(0, 0, 1), (1, 0, 2)], full), ([(1, 0, 3), (0, 0, 4)], full),
             ([(1, 1, 3), (0, 1, 4)], full), ([(0, 0, 1), (1, 0, 2)], full), ([(0, 0, 5), (2, 0, 6)], half)]
    rng = np.random.default_rng(3)
    ref_out = rng.integers(0, 255, (nb * F, H, W, 3), dtype=np.uint8)
    ref_state = np.full(nb * F * T, -1, dtype=np.int32)
    out = device(ref_out)
    state = ops.frames_tile_state(nb, F, H, W, "cuda")
    # two tiles that are background in both buffers of steps 1 and 2
    stored0 = (clip(name, 0, 0)[1]["offsets"] >= 0).reshape(F, gy, gx)
    ty64 = int(np.flatnonzero(~stored0[0, :, 64])[-2])
    txb = int(np.flatnonzero(~stored0[0, gy - 1])[3])
    poison = [(slice(ty64 * 16, ty64 * 16 + 16), slice(64 * 16, 65 * 16)), (slice((gy - 1) * 16, H), slice(txb * 16, txb * 16 + 16))]
    for i, (specs, cap) in enumerate(steps):
        bufs = model_wires(name, specs, cap)
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        if i == 1:
            for ys, xs in poison:
                assert (ref_out[0, ys, xs] == 255).all()
                ref_out[0, ys, xs] = 7
                out[0, ys, xs] = 7
        ops.frames_unpack_tiles(device(bufs), nb, F, H, W, cap, out=out, status=status, state=state)
        want_status = wm.unpack_delta(bufs, F, H, W, cap, ref_out, ref_state)
        if i == 1:
            for ys, xs in poison:
                assert (ref_out[0, ys, xs] == 7).all()
        assert np.array_equal(host(out), ref_out), f"step {i}: out"
        assert np.array_equal(host(state), ref_state), f"step {i}: state"
        assert int(status.item()) == want_status == (1 if i == 5 else 0), f"step {i}: status"
        if i == 1:
            for ys, xs in poison:
                ref_out[0, ys, xs] = 255
                out[0, ys, xs] = 255
        assert np.array_equal(ref_out, wm.unpack(bufs, F, H, W, cap)[0]), f"step {i}: the model's two unpacks disagree"


# -------------------------------------------------------------------------------------------------- quantisation
def quant_values():
    k = np.arange(256)
    exact = (k / 255).astype(np.float32)
    special = np.array([-0.0, -1, 1, 1 + 2.0 ** -23, 2, 255, np.inf, -np.inf, np.nan], dtype=np.float32)
    return np.concatenate([exact, np.nextafter(exact, np.float32(-1)), np.nextafter(exact, np.float32(2)), special])


def test_to_rgb8_on_the_quantisation_table():
    """k / 255, the fp32 below and the fp32 above it for every k, and the values a clamp has to catch."""
    from audio_motion_avatar_amd import ops

    v = quant_values()
    n = 4 * 256 * 3
    x = np.empty((4, 256, 3, 4), dtype=np.float32)
    for c, step in enumerate((1, 5, 11, 13)):                     # steps coprime to len(v): every value in every channel
        x[..., c] = v[(np.arange(n) * step + 13 * c) % v.size].reshape(4, 256, 3)
    assert all(np.isin(v[~np.isnan(v)], x[..., c]).all() and np.isnan(x[..., c]).any() for c in range(3))
    got = host(ops.frames_to_rgb8(device(x)))
    assert np.array_equal(got, wm.quant8(x[..., :3]))


def test_pack_on_the_quantisation_table():
    """Tiles of the same values, with a background whose channels are themselves nextafter(k / 255, 0): whether a tile
    differs from the background is decided on the quantised bytes."""
    from audio_motion_avatar_amd import ops

    v = quant_values()
    F, H, W = 1, 48, 64
    T = wm.geometry(H, W)[2]
    bg = tuple(float(np.nextafter(np.float32(k / 255), np.float32(0))) for k in (64, 128, 200))
    assert wm.bg_word(bg) == 63 | (127 << 8) | (199 << 16)
    n = F * H * W
    x = np.empty((F, H, W, 4), dtype=np.float32)
    for c, step in enumerate((1, 5, 11, 13)):
        x[..., c] = v[(np.arange(n) * step + 13 * c) % v.size].reshape(F, H, W)
    x[0, 16:32, 16:32, :3] = np.asarray(bg, dtype=np.float32)                        # the background itself
    x[0, 16:32, 32:48, :3] = np.asarray([63 / 255, 127 / 255, 199 / 255], np.float32)  # other floats, the same bytes
    x[0, 32:48, 0:16, :3] = np.asarray(bg, dtype=np.float32)
    x[0, 40, 7, 1] = np.float32(128 / 255)                                           # one byte of one pixel differs
    m = wm.pack(x, bg, T)
    stored = (m["offsets"] >= 0).reshape(3, 4)
    assert not stored[1, 1] and not stored[1, 2] and stored[2, 0] and int(m["header"][1]) == T - 2
    wire = ops.frames_pack_tiles(device(x), T, bg)
    assert_wire_equals(wm.from_bytes(host(wire), F, T, T), m, T - 2, "table")
    out, status = ops.frames_unpack_tiles(wire[None], 1, F, H, W, T)
    assert np.array_equal(host(out), wm.quant8(x[..., :3])) and int(status.item()) == 0


# ------------------------------------------------------------------------------------------- rasterizer emission
EMIT_CASES = {
    # (F, H, W), Gaussians, spread, log_scale, background, seed
    "slice-3-per-thread": (wm.WIDE, 300, 0.35, -4.5, 1, 31),
    "fused-2-per-thread": (wm.EMIT_FUSED, 300, 0.35, -4.5, 0, 32),
    "fused-small": (wm.EMIT_FUSED_SMALL, 10, 0.3, -3.6, 1, 33),
}


@pytest.mark.parametrize("case", list(EMIT_CASES))
def test_rasterizer_emission_equals_the_model(case):
    """The wire buffer the rasterizer writes itself (slots handed out by its binning block, tiles written by its blend
    kernel) against the model's pack of the rendered frames with the rasterizer's tile counts as hint: same header,
    per-frame counts and stored tiles; the slots a permutation of 0 .. count - 1 in which every frame owns one
    contiguous range, ascending in tile order; every stored tile's bytes equal.
    Stored tiles per frame, measured on an MI355X (the test prints them): slice-3-per-thread 1015 .. 1053 of 2145
    (47 % .. 49 %), fused-2-per-thread 555 .. 755 of 1105 (50 % .. 68 %), fused-small 5 .. 15 of 24 (21 % .. 63 %)."""
    from audio_motion_avatar_amd import ops

    (F, H, W), N, spread, log_scale, bgi, seed = EMIT_CASES[case]
    bg = BGS[bgi]
    gx, gy, T = wm.geometry(H, W)
    sc = random_scene(seed, N, H, W, F, spread=spread, log_scale=log_scale)
    view, proj, tanfov, _ = ops.camera_from_intrinsics(sc["K"].cuda(), sc["E"].cuda(), H, W)
    cap = F * T
    wire = torch.full((wm.wire_bytes(F, H, W, cap),), wm.FILL, dtype=torch.uint8, device="cuda")
    c = lambda k: sc[k].cuda()
    out = ops.rasterize(c("xyz"), c("rot"), c("scale"), c("opacity"), c("color"), view, proj, tanfov, H, W, bg=bg,
                        clamp_output=True, wire=(wire, cap))
    assert not out["workspace"].status()[1]
    hint = host(out["workspace"].tile_counts())
    rgba = host(out["rgba"])
    per_frame = (hint.reshape(F, T) > 0).sum(axis=1)
    print(f"{case}: stored tiles per frame {per_frame.min()} .. {per_frame.max()} of {T} "
          f"({100 * per_frame.min() / T:.1f} % .. {100 * per_frame.max() / T:.1f} %)")
    assert (per_frame > 0.05 * T).all() and (per_frame < 0.95 * T).all()
    if T > 1024:
        assert (hint.reshape(F, T)[:, 1024:] > 0).any()
    m = wm.pack(rgba, bg, cap, hint)
    got = wm.from_bytes(host(wire), F, T, cap)
    count = int(m["header"][1])
    assert np.array_equal(got["header"][:8], m["header"][:8])
    assert np.array_equal(got["frame_counts"], m["frame_counts"])
    off, stored = got["offsets"], m["offsets"] >= 0
    assert np.array_equal(off >= 0, stored) and (off[~stored] == -1).all()
    assert np.array_equal(np.sort(off[stored]), np.arange(count))
    for f in range(F):
        s = off[f * T:(f + 1) * T]
        s = s[s >= 0]
        assert np.array_equal(s, s[0] + np.arange(s.size)), f"frame {f}: slots are not one ascending range"
    assert np.array_equal(got["payload"][off[stored]], m["payload"][m["offsets"][stored]])
    dense, status = ops.frames_unpack_tiles(wire[None], 1, F, H, W, cap)
    want, _ = wm.unpack([wm.to_bytes(m, F, T, cap)], F, H, W, cap)
    assert np.array_equal(host(dense), want) and int(status.item()) == 0
    assert np.array_equal(want, wm.quant8(rgba[..., :3]))
