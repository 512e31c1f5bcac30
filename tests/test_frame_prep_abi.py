"""Host side of amav_frames_prepare: declared, exported and bound; the workspace query; every refusal include/amav.h
lists answers with its error code (no kernel is launched: each call fails a check first); ops.prepare_frames and
clip_data refuse on the host what never reaches the library."""
import ctypes

import pytest

from abi_support import ERR_INVALID, ERR_WORKSPACE, FAKE, HEADER, lib  # noqa: F401 (lib: fixture)

NAMES = ["amav_frames_prepare_workspace_bytes", "amav_frames_prepare"]


def test_symbols_are_declared_exported_and_bound(lib):
    from audio_motion_avatar_amd import _lib

    text = open(HEADER).read()
    for name in NAMES:
        assert name + "(" in text and hasattr(lib, name) and name in _lib.SIGNATURES
    restype, argtypes = _lib.SIGNATURES["amav_frames_prepare"]
    assert restype is ctypes.c_int and len(argtypes) == 30 and argtypes[-1] is ctypes.c_void_p
    assert argtypes[3] is ctypes.c_void_p and argtypes[9] is ctypes.c_void_p, "frames and masks: device addresses"
    assert all(argtypes[i] is ctypes.c_int64 for i in (5, 6, 7, 8, 11, 12, 13)), "strides in elements, 64 bit"
    assert argtypes[19] == ctypes.POINTER(ctypes.c_float) and argtypes[20] == ctypes.POINTER(ctypes.c_float), "mean, std: host"
    assert all(argtypes[i] is ctypes.c_void_p for i in (21, 23, 25, 27)) and all(argtypes[i] is ctypes.c_size_t for i in (22, 24, 26, 28))
    assert _lib.SIGNATURES["amav_frames_prepare_workspace_bytes"][0] is ctypes.c_size_t


def test_workspace_query(lib):
    fn = lib.amav_frames_prepare_workspace_bytes
    for F in (1, 8, 9, 48, 16384):
        assert 16 * F <= fn(F) <= 16 * F + 256 and fn(F) % 256 == 0
    for F in (0, -1, 16385, 1 << 30):
        assert fn(F) == 0


def three(*v):
    return (ctypes.c_float * 3)(*v)


def prepare(lib, F=2, H=48, W=64, frames=FAKE, frames_f32=0, fs=None, masks=FAKE, masks_f32=0, ms=None, Hp=52, Wp=70, oy=2,
            ox=3, S=16, mean=None, std=None, images=FAKE, images_bytes=None, cropped=FAKE, cropped_bytes=None, boxes=FAKE,
            boxes_bytes=None, ws=FAKE, ws_bytes=None):
    fs = fs or (H * W * 3, 1, W * 3, 3)
    ms = ms or (H * W, W, 1)
    big = lambda n: n if n > 0 else 1  # noqa: E731
    images_bytes = 12 * big(F) * big(Hp) * big(Wp) if images_bytes is None else images_bytes
    cropped_bytes = 12 * big(F) * big(S) * big(S) if cropped_bytes is None else cropped_bytes
    boxes_bytes = 20 * big(F) if boxes_bytes is None else boxes_bytes
    ws_bytes = (lib.amav_frames_prepare_workspace_bytes(F) or 1 << 20) if ws_bytes is None else ws_bytes
    return lib.amav_frames_prepare(F, H, W, frames, frames_f32, *fs, masks, masks_f32, *ms, Hp, Wp, oy, ox, S, mean, std, images,
                                   images_bytes, cropped, cropped_bytes, boxes, boxes_bytes, ws, ws_bytes, None)


def test_refusals(lib):
    def refused(text, code=ERR_INVALID, **kw):
        assert prepare(lib, **kw) == code, kw
        assert text.encode() in lib.amav_last_error(), (kw, lib.amav_last_error())

    refused("NULL frames", frames=None)
    for F in (0, -3, 16385):
        refused(f"F={F} outside 1..16384", F=F)
    for H, W in ((0, 64), (48, 0), (-1, 64), (65536, 64), (48, 65536)):
        refused("outside 1..65535", H=H, W=W, Hp=max(H, 1), Wp=max(W, 1), oy=0, ox=0)
    refused("padded size 47 x 70", Hp=47, oy=0)  # Hp < H
    refused("padded size 52 x 63", Wp=63, ox=0)
    refused("padded size 65536 x 70", Hp=65536)
    for oy, ox in ((-1, 3), (5, 3), (2, -1), (2, 7)):
        refused(f"offsets ({oy}, {ox})", oy=oy, ox=ox)
    for S in (0, -1, 65536):
        refused(f"crop_side {S}", S=S)
    refused("flags are 0 or 1", frames_f32=2)
    refused("flags are 0 or 1", masks_f32=-1)
    refused("a stride inside a frame is negative", fs=(48 * 64 * 3, 1, -64 * 3, 3))
    refused("a stride inside a frame is negative", ms=(48 * 64, 64, -1))
    refused("spans 2^31 elements or more", fs=(1 << 40, 1, 1 << 26, 3))
    refused("spans 2^31 elements or more", ms=(1 << 40, 1 << 26, 1))
    assert prepare(lib, fs=(-(1 << 40), 1, 64 * 3, 3), ms=(-5, 64, 1), ws_bytes=0) == ERR_WORKSPACE  # the frame stride is free
    refused("mean and std come together", mean=three(0.5, 0.5, 0.5))
    refused("mean and std come together", std=three(0.5, 0.5, 0.5))
    for c in range(3):
        std = [0.2, 0.2, 0.2]
        std[c] = 0.0
        refused(f"std[{c}] is zero", mean=three(0.5, 0.5, 0.5), std=three(*std))
    refused("std[1] is zero or a value is NaN", mean=three(0.5, float("nan"), 0.5), std=three(1, 1, 1))
    refused("misaligned buffer", images=FAKE + 4)
    refused("misaligned buffer", cropped=FAKE + 8)
    refused("misaligned buffer", boxes=FAKE + 2)
    refused("misaligned buffer", frames=FAKE + 2, frames_f32=1)
    refused("misaligned buffer", masks=FAKE + 1, masks_f32=1)
    need = 12 * 2 * 52 * 70
    refused(f"images buffer {need - 4} < {need}", ERR_WORKSPACE, images_bytes=need - 4)  # one element short
    need = 12 * 2 * 16 * 16
    refused(f"cropped buffer {need - 4} < {need}", ERR_WORKSPACE, cropped_bytes=need - 4)
    refused("boxes buffer 36 < 40", ERR_WORKSPACE, boxes_bytes=36)
    need = lib.amav_frames_prepare_workspace_bytes(2)
    refused(f"workspace {need - 1} < {need}", ERR_WORKSPACE, ws_bytes=need - 1)
    refused(f"workspace 0 < {need}", ERR_WORKSPACE, ws=None)
    refused("workspace is not 16-byte aligned", ERR_WORKSPACE, ws=FAKE + 8)
    # bytes need no alignment, and a short buffer of an output that is not asked for is no error: the call gets as
    # far as the next check
    assert prepare(lib, frames=FAKE + 1, masks=FAKE + 3, ws_bytes=0) == ERR_WORKSPACE
    assert prepare(lib, images=None, images_bytes=0, ws_bytes=0) == ERR_WORKSPACE and b"workspace" in lib.amav_last_error()
    assert prepare(lib, cropped=None, cropped_bytes=0, boxes=None, boxes_bytes=0, images_bytes=0) == ERR_WORKSPACE
    assert b"images buffer" in lib.amav_last_error()


def test_ops_refuse_on_the_host():
    import torch

    from audio_motion_avatar_amd import AmavError, clip_data, ops

    frames = torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(AmavError, match="HIP device"):
        ops.prepare_frames(frames)
    with pytest.raises(AmavError, match="HIP device"):
        ops.prepare_frames(frames.permute(0, 3, 1, 2).float())
    assert ops.padded_size(96, 72, 0.1) == (105, 79, 4, 3) and ops.padded_size(512, 512, 0.0) == (512, 512, 0, 0)
    clip = {"images": torch.zeros(8, 3, 5, 4), "cropped_images": torch.zeros(8, 3, 6, 6), "boxes": torch.zeros(8, 5)}
    parts = clip_data.split_ref_target(clip)
    assert sorted(parts) == ["cropped_images", "ref_images", "target_video"]
    with pytest.raises(ValueError, match="shorter"):
        clip_data.split_ref_target({k: v[:5] for k, v in clip.items()})
