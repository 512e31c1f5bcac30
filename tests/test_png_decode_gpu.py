"""ops.png_decode against numpy.array(Image.open(...).convert(...)), bit for bit: every size, colour type, depth, forced
filter set and IDAT split of tests/png_cases.py, Pillow's own files, both modes and both layouts, mixed batches with an
absent record, png.load_clip / load_training_clip / load_dataset_clip on temporary directories."""
import os
import warnings

import numpy as np
import pytest
import torch

import png_cases as pc
import png_model as pm
from png_cases import write_dataset

pytestmark = pytest.mark.gpu

warnings.filterwarnings("ignore", message="Palette images with Transparency")


def decode(blobs, mode, layout):
    from audio_motion_avatar_amd import ops, png

    records, stream = png.frame_records(blobs)
    out, status = ops.png_decode(stream.cuda(), records.to("cuda"), mode=mode, layout=layout)
    return out.cpu(), status.cpu().tolist()


def as_u8(out, mode, layout):
    """Both layouts as uint8 [F,H,W,(3)]; the fp32 one must hold exactly uint8 / 255."""
    if layout == "hwc_u8":
        return out.numpy()
    u8 = (out * 255.0).round().to(torch.uint8)
    assert torch.equal(out, u8.float() / 255.0)
    u8 = u8.permute(0, 2, 3, 1).numpy()
    return u8 if mode == "rgb" else u8[..., 0]


def by_size(files):
    from audio_motion_avatar_amd import png

    groups = {}
    for name, data in files:
        h = png.parse_png(data)
        groups.setdefault((h.height, h.width), []).append((name, data))
    return groups


@pytest.mark.parametrize("mode", ["rgb", "l"])
@pytest.mark.parametrize("layout", ["hwc_u8", "chw_f32"])
def test_every_file_equals_pillow(mode, layout):
    groups = by_size(pc.png_files() + pc.pillow_files())
    assert set(pc.SIZES) <= set(groups)
    for (H, W), files in groups.items():  # one call per size: colour types, depths, filters and splits mixed in the batch
        out, status = decode([d for _, d in files], mode, layout)
        got = as_u8(out, mode, layout)
        for k, (name, data) in enumerate(files):
            assert status[k] == 0, (name, status[k])
            assert np.array_equal(got[k], pc.pillow_decode(data, mode)), (name, mode, layout)


def test_one_frame_calls_and_absent_records():
    files = dict(pc.png_files())
    name = next(n for n in files if n.startswith("130x70_t6d8"))
    out, status = decode([files[name]], "rgb", "hwc_u8")
    assert status == [0] and np.array_equal(out[0].numpy(), pc.pillow_decode(files[name], "rgb"))
    group = [d for n, d in pc.png_files() if n.startswith("65x13_")][::13][:5]  # five colour types
    blobs = [group[0], None, group[1], group[2], None, group[3], group[4]]
    for mode, layout in (("rgb", "hwc_u8"), ("l", "hwc_u8"), ("rgb", "chw_f32"), ("l", "chw_f32")):
        out, status = decode(blobs, mode, layout)
        got = as_u8(out, mode, layout)
        assert status == [0] * 7
        for k, b in enumerate(blobs):
            want = np.full(got[k].shape, 255, np.uint8) if b is None else pc.pillow_decode(b, mode)
            assert np.array_equal(got[k], want), (k, mode, layout)


@pytest.mark.parametrize("layout", ["hwc_u8", "chw_f32"])
def test_the_widest_row(layout):
    """W = 16 384, the largest the entry point takes: the unfilter kernel's carried row is then 4 W = 64 KiB of LDS, the
    most a launch can ask for.  One row and three (so that a row above exists), RGBA (16 384 units of 4 bytes), 1-bit
    grey (2048 units of 8 pixels) and an 8-bit palette."""
    rng = np.random.default_rng(7)
    for H in (1, 3):
        blobs = [pc.write_png(rng.integers(0, 256, (H, 16384, 4)).astype(np.uint8), 6, 8, (4, 3, 2)),
                 pc.write_png(rng.integers(0, 2, (H, 16384, 1)).astype(np.uint8), 0, 1, (1, 4, 3)),
                 pc.write_png(rng.integers(0, 256, (H, 16384, 1)).astype(np.uint8), 3, 8, (3, 2, 4), palette=pc.make_palette(rng, 8))]
        for mode in ("rgb", "l"):
            out, status = decode(blobs, mode, layout)
            got = as_u8(out, mode, layout)
            assert status == [0, 0, 0]
            for k, b in enumerate(blobs):
                assert np.array_equal(got[k], pc.pillow_decode(b, mode)), (H, k, mode)


def test_palette_index_beyond_the_palette_is_black():
    rng = np.random.default_rng(5)
    samples = rng.integers(0, 256, (9, 7, 1)).astype(np.uint8)
    palette = rng.integers(1, 256, 3 * 100).astype(np.uint8).tobytes()
    data = pc.write_png(samples, 3, 8, (4,), palette=palette)
    out, status = decode([data], "rgb", "hwc_u8")
    table = np.zeros((256, 3), np.uint8)
    table[:100] = np.frombuffer(palette, np.uint8).reshape(-1, 3)
    assert status == [0] and np.array_equal(out[0].numpy(), table[samples[..., 0]]) and (samples >= 100).any()


def test_two_calls_give_identical_bytes_and_out_is_used():
    from audio_motion_avatar_amd import ops, png

    blobs = [d for n, d in pc.png_files() if n.startswith("130x70_")]
    records, stream = png.frame_records(blobs)
    records, stream = records.to("cuda"), stream.cuda()
    a, sa = ops.png_decode(stream, records, layout="chw_f32")
    out, st = torch.empty_like(a), torch.empty_like(sa)
    b, sb = ops.png_decode(stream, records, layout="chw_f32", out=out, status=st)
    assert b is out and sb is st and torch.equal(a, b) and torch.equal(sa, sb) and not sa.any()


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("png_dataset"))
    write_dataset(root, 12, H=24, W=32, pad_ratio=0.25, missing_masks=(4,))
    return root


def pillow_clip(root, ids, mode, folder):
    import PIL.Image as Image

    frames = []
    for i in ids:
        path = os.path.join(root, folder, f"{i:05d}.png")
        if os.path.exists(path):
            frames.append(np.array(Image.open(path).convert(mode)))
        else:
            frames.append(np.full((24, 32), 255, np.uint8))
    return torch.from_numpy(np.stack(frames)).cuda()


def test_load_clip_and_load_training_clip(dataset, monkeypatch):
    from audio_motion_avatar_amd import clip_data, ops, png

    frames_dir, masks_dir = os.path.join(dataset, "imgs_png"), os.path.join(dataset, "samurai_seg")
    rgb = png.load_clip(frames_dir, frames=[0, 2, 6], layout="hwc_u8")
    assert torch.equal(rgb, pillow_clip(dataset, [0, 2, 6], "RGB", "imgs_png"))
    f32 = png.load_clip(frames_dir, frames=[0, 2, 6])
    assert torch.equal(f32.cpu(), rgb.cpu().permute(0, 3, 1, 2).float() / 255.0)  # an IEEE division, so on the host
    grey, status = png.load_clip(png.PngDirReader(masks_dir), frames=[1], mode="l", layout="hwc_u8", check=False)
    assert status.tolist() == [0] and torch.equal(grey, pillow_clip(dataset, [1], "L", "samurai_seg"))
    # masks_dir lacks 00004.png, so its positions are 0 1 2 3 5 ...: frames 0..3 line up with the images
    syncs = []
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **kw: syncs.append(1))
    clip = clip_data.load_training_clip(frames_dir, masks_dir, frames=range(0, 4), pad_ratio=0.25, crop_size=64)
    monkeypatch.undo()
    assert not syncs
    want = ops.prepare_frames(pillow_clip(dataset, range(4), "RGB", "imgs_png"), pillow_clip(dataset, range(4), "L", "samurai_seg"),
                              pad_ratio=0.25, crop_size=64)
    assert all(torch.equal(clip[k], w) for k, w in zip(("images", "cropped_images", "boxes"), want))


def test_load_dataset_clip_end_to_end(dataset):
    """32 x 24 frames, crop 64, the mask of frame 4 missing, pad_ratio 0.25 from the JSON: equal, bit for bit, to
    ops.prepare_frames fed with Pillow's decode of the same files."""
    from audio_motion_avatar_amd import clip_data, ops

    item = clip_data.load_dataset_clip(dataset, 0, clip_length=8, crop_size=64)
    ids = [0, 2, 4, 6, 8, 10, 10, 10]
    want = ops.prepare_frames(pillow_clip(dataset, ids, "RGB", "imgs_png"), pillow_clip(dataset, ids, "L", "samurai_seg"),
                              pad_ratio=0.25, crop_size=64)
    assert torch.equal(item["images"], want[0]) and torch.equal(item["cropped_images"], want[1])
    assert tuple(item["images"].shape) == (8, 3, 30, 40) and tuple(item["cropped_images"].shape) == (8, 3, 64, 64)
    assert item["batch_id"] == 0 and all(v.is_cuda for v in item["smplx_params"].values())
    assert tuple(item["camera"]["intrinsic"].shape) == (8, 3, 3) and tuple(item["camera"]["extrinsic"].shape) == (8, 4, 4)
    assert torch.equal(item["bg_color"], torch.ones(8, 3, device="cuda"))
    assert torch.equal(item["smplx_params"]["expression"], torch.zeros(8, 10, device="cuda"))
    assert float(item["smplx_params"]["focal"][3, 0]) == 1006.0


def test_load_clip_names_the_damaged_frame(dataset, tmp_path):
    from audio_motion_avatar_amd import png

    good = open(os.path.join(dataset, "imgs_png", "00000.png"), "rb").read()
    h = png.parse_png(good)
    rows = np.zeros((24, 32 * 3), np.uint8)
    raw = bytearray(pc.filter_rows(rows, (0,), 3))
    raw[5 * (1 + 96)] = 7  # a filter byte above 4
    bad = pc.write_png(np.zeros((24, 32, 3), np.uint8), 2, 8, raw_override=bytes(raw))
    assert (h.height, h.width) == (24, 32)
    with pytest.raises(png.PngError, match=r"damaged frames 1 \(filter\)"):
        png.load_clip([good, bad, good])
    out, status = png.load_clip([good, bad, good], check=False, layout="hwc_u8")
    assert status.tolist() == [0, pm.STATUS_FILTER, 0] and torch.equal(out[0], out[2])
