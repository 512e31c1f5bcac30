"""The file-level PNG writers: png.write_dataset_clip read back by clip_data.load_dataset_clip / png.load_clip bit for
bit, png.save_clip's naming and chunking, png.save_image and png.save_comparison against NumPy restatements read back with
Pillow, and the demo's FrameWriter(frames_format="png")."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

import png_encode_cases as ec
from png_cases import write_dataset

pytestmark = pytest.mark.gpu


def test_dataset_directory_round_trip(tmp_path):
    from audio_motion_avatar_amd import clip_data, ops, png

    root, count, H, W = str(tmp_path), 7, 6, 8
    write_dataset(root, count, H=H, W=W)  # the JSON files (and PNGs that are overwritten below)
    rng = np.random.default_rng(4)
    frames = torch.from_numpy(rng.integers(0, 256, (count, H, W, 3), dtype=np.uint8)).cuda()
    masks = torch.from_numpy((rng.integers(0, 3, (count, H, W)) > 0).astype(np.uint8) * 255).cuda()
    paths = png.write_dataset_clip(root, frames, masks)
    assert [os.path.relpath(p, root) for p in paths] == [f"imgs_png/{i:05d}.png" for i in range(count)] + \
        [f"samurai_seg/{i:05d}.png" for i in range(count)]
    assert torch.equal(png.load_clip(os.path.join(root, "imgs_png"), mode="rgb", layout="hwc_u8"), frames)
    assert torch.equal(png.load_clip(os.path.join(root, "samurai_seg"), mode="l", layout="hwc_u8"), masks)
    for i in (0, count - 1):
        assert np.array_equal(np.asarray(Image.open(paths[i])), frames[i].cpu().numpy())
        assert np.array_equal(np.asarray(Image.open(paths[count + i])), masks[i].cpu().numpy())
    item = clip_data.load_dataset_clip(root, 1, clip_length=3, crop_size=16)  # frames 1, 3, 5
    want = ops.prepare_frames(frames[1:6:2].contiguous(), masks[1:6:2].contiguous(), pad_ratio=0.25, crop_size=16)
    assert torch.equal(item["images"], want[0]) and torch.equal(item["cropped_images"], want[1])


def test_save_clip_names_chunks_and_layouts(tmp_path, monkeypatch):
    from audio_motion_avatar_amd import png

    monkeypatch.setattr(png, "SAVE_CHUNK", 3)  # 7 frames: calls of 3, 3 and 1
    x = ec.edge_values(np.random.default_rng(6), (7, 5, 9, 4))
    paths = png.save_clip(str(tmp_path / "out"), torch.from_numpy(x).cuda(), pattern="f%03d.png", start=10, filter="paeth")
    assert [os.path.basename(p) for p in paths] == [f"f{i:03d}.png" for i in range(10, 17)]
    for f, p in enumerate(paths):
        assert np.array_equal(np.asarray(Image.open(p)), ec.to_levels(x[f, ..., :3]))


def numpy_normalize(x):
    low, high = x.min(), x.max()
    return ((np.clip(x, low, high) - low) / np.maximum(high - low, np.float32(1e-5))).astype(np.float32)


@pytest.mark.parametrize("normalize", [False, True])
def test_save_image(tmp_path, normalize):
    from audio_motion_avatar_amd import png

    x = (np.random.default_rng(7).normal(0.4, 0.6, (3, 33, 21))).astype(np.float32)
    path = str(tmp_path / "image.png")
    png.save_image(torch.from_numpy(x).cuda(), path, normalize=normalize)
    want = ec.to_levels(numpy_normalize(x) if normalize else x).transpose(1, 2, 0)
    im = Image.open(path)
    assert im.mode == "RGB" and np.array_equal(np.asarray(im), want)
    png.save_image(torch.from_numpy(x[:1]).cuda(), path, normalize=normalize)  # one channel: greyscale
    want = ec.to_levels(numpy_normalize(x[:1]) if normalize else x[:1])[0]
    assert np.array_equal(np.asarray(Image.open(path).convert("RGB")), np.repeat(want[..., None], 3, axis=-1))


def test_save_comparison_sheet(tmp_path):
    from audio_motion_avatar_amd import png

    rng = np.random.default_rng(12)
    T, H, W = 3, 20, 14
    rendered = rng.random((T, H, W, 3), dtype=np.float32) * np.float32(1.2) - np.float32(0.1)
    real = rng.random((T, 3, H, W), dtype=np.float32)
    path = str(tmp_path / "sheet.png")
    png.save_comparison(path, torch.from_numpy(rendered).cuda(), torch.from_numpy(real).cuda())
    sheet = np.concatenate([np.concatenate([rendered[t], real[t].transpose(1, 2, 0)], axis=1) for t in range(T)], axis=0)
    assert sheet.shape == (T * H, 2 * W, 3)
    assert np.array_equal(np.asarray(Image.open(path)), ec.to_levels(numpy_normalize(sheet)))
    png.save_comparison(path, torch.from_numpy(rendered).cuda(), torch.from_numpy(real).cuda(), normalize=False)
    assert np.array_equal(np.asarray(Image.open(path)), ec.to_levels(sheet))


def test_frame_writer_png_frames(tmp_path):
    from audio_motion_avatar_amd.demo import FrameWriter

    H, W = 24, 40
    x = ec.edge_values(np.random.default_rng(13), (5, H, W, 3))
    frames_dir = str(tmp_path / "frames")
    with FrameWriter(str(tmp_path / "clip.rgb"), H, W, frames_dir=frames_dir, frames_format="png") as writer:
        writer.write(torch.from_numpy(x[:2]).cuda())
        writer.write(torch.from_numpy(x[2:]).cuda())
    assert sorted(os.listdir(frames_dir)) == [f"frame_{i:03d}.png" for i in range(5)]
    for i in range(5):
        assert np.array_equal(np.asarray(Image.open(os.path.join(frames_dir, f"frame_{i:03d}.png"))), ec.to_levels(x[i]))
    assert os.path.getsize(str(tmp_path / "clip.rgb")) == 5 * H * W * 3  # the raw target is written as before
    with pytest.raises(ValueError, match="jpg or png"):
        FrameWriter(str(tmp_path / "x.rgb"), H, W, frames_format="bmp")
