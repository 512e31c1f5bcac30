"""The JSON / camera half of clip_data.load_dataset_clip on a temporary directory laid out like the reference's dataset:
key map, shapes, dtypes, the repeat of the last frame, the missing-mask rule, the unequal-pad_ratio error.  The decode is
stubbed out, so no device is needed."""
import os

import pytest
import torch

import png_cases as pc
from png_cases import write_dataset

from audio_motion_avatar_amd import clip_data, png


def test_host_half(tmp_path):
    root = str(tmp_path)
    write_dataset(root, 11)
    ids, item = clip_data.dataset_clip_host(root, 2, clip_length=4)
    assert ids == [2, 4, 6, 8] and item["batch_id"] == 2 and item["pad_ratio"] == 0.25
    sp = item["smplx_params"]
    assert set(sp) == {"betas", "transl", "global_orient", "body_pose", "left_hand_pose", "right_hand_pose", "jaw_pose",
                       "leye_pose", "reye_pose", "pad_ratio", "focal", "princpt", "expression"}
    shapes = {"betas": (4, 10), "transl": (4, 3), "global_orient": (4, 3), "body_pose": (4, 21, 3), "left_hand_pose": (4, 15, 3),
              "right_hand_pose": (4, 15, 3), "jaw_pose": (4, 3), "leye_pose": (4, 3), "reye_pose": (4, 3), "pad_ratio": (4,),
              "focal": (4, 2), "princpt": (4, 2), "expression": (4, 10)}
    for k, shape in shapes.items():
        assert tuple(sp[k].shape) == shape and sp[k].dtype == torch.float32, k
    assert not sp["expression"].any() and torch.equal(sp["pad_ratio"], torch.full((4,), 0.25))
    assert torch.allclose(sp["transl"][:, 0], torch.tensor([0.2, 0.4, 0.6, 0.8]))
    assert torch.allclose(sp["global_orient"][:, 0], torch.tensor([0.02, 0.04, 0.06, 0.08]))
    K = item["camera"]["intrinsic"]
    assert K.shape == (4, 3, 3) and K.dtype == torch.float32
    want = torch.eye(3).repeat(4, 1, 1)
    want[:, 0, 0], want[:, 1, 1] = torch.tensor([1002.0, 1004.0, 1006.0, 1008.0]), 1100.0
    want[:, 0, 2], want[:, 1, 2] = 4.0, 3.0
    assert torch.equal(K, want)
    assert torch.equal(item["camera"]["extrinsic"], torch.eye(4).repeat(4, 1, 1))
    assert torch.equal(item["bg_color"], torch.ones(4, 3))


def test_last_frame_repeats_where_the_directory_ends(tmp_path):
    root = str(tmp_path)
    write_dataset(root, 7)
    ids, item = clip_data.dataset_clip_host(root, 3, clip_length=4)  # 3, 5, then nothing below 7
    assert ids == [3, 5, 5, 5]
    assert torch.allclose(item["smplx_params"]["transl"][:, 0], torch.tensor([0.3, 0.5, 0.5, 0.5]))
    assert clip_data.dataset_clip_host(root, 6, clip_length=8)[0] == [6] * 8
    with pytest.raises(IndexError):
        clip_data.dataset_clip_host(root, 7)


def test_frames_follow_the_numbers_of_the_files(tmp_path):
    root = str(tmp_path)
    write_dataset(root, 0, ids=[5, 7, 10, 11, 30])
    assert clip_data.dataset_clip_host(root, 1, clip_length=2)[0] == [7, 11]


def test_a_file_without_a_frame_number_is_named(tmp_path):
    root = str(tmp_path)
    write_dataset(root, 3)
    open(os.path.join(root, "imgs_png", "preview.png"), "wb").close()
    open(os.path.join(root, "imgs_png", "notes.txt"), "wb").close()  # not a .png: ignored
    with pytest.raises(ValueError, match=r"imgs_png/preview.png is not named by a frame number"):
        clip_data.dataset_clip_host(root, 0, clip_length=1)


def test_pad_ratio_defaults_and_must_agree(tmp_path):
    write_dataset(str(tmp_path / "a"), 4, ratios=[None] * 4)
    assert clip_data.dataset_clip_host(str(tmp_path / "a"), 0, clip_length=2)[1]["pad_ratio"] == 0.0
    write_dataset(str(tmp_path / "b"), 4, ratios=[0.25, 0.25, 0.5, 0.25])
    with pytest.raises(ValueError, match="pad_ratio differs"):
        clip_data.dataset_clip_host(str(tmp_path / "b"), 0, clip_length=2)
    assert clip_data.dataset_clip_host(str(tmp_path / "b"), 1, clip_length=2)[1]["pad_ratio"] == 0.25  # frames 1 and 3


def test_item_with_the_decode_stubbed(tmp_path, monkeypatch):
    """load_dataset_clip end to end on the host: png.load_clip and ops.prepare_frames replaced, so that what it hands to
    them (files in clip order, None for the missing mask, the JSON's pad_ratio, crop_size) is what is checked."""
    root = str(tmp_path)
    write_dataset(root, 6, missing_masks=(2,))
    calls = []

    def fake_load_clip(blobs, mode="rgb", device="cuda", layout="chw_f32", check=True, frames=None):
        calls.append((mode, layout, check, [None if b is None else png.parse_png(b).color_type for b in blobs]))
        shape = (len(blobs), 6, 8, 3) if mode == "rgb" else (len(blobs), 6, 8)
        return torch.zeros(shape, dtype=torch.uint8), torch.zeros(len(blobs), dtype=torch.int32)

    def fake_prepare(rgb, mask, pad_ratio=0.0, crop_size=1024):
        calls.append(("prepare", pad_ratio, crop_size, None if mask is None else tuple(mask.shape)))
        return torch.zeros(3, 3, 7, 10), torch.zeros(3, 3, crop_size, crop_size), torch.zeros(3, 5, dtype=torch.int32)

    monkeypatch.setattr(png, "load_clip", fake_load_clip)
    monkeypatch.setattr(clip_data.ops, "prepare_frames", fake_prepare)
    item = clip_data.load_dataset_clip(root, 0, clip_length=3, crop_size=16, device="cpu")
    assert calls == [("rgb", "hwc_u8", False, [2, 2, 2]), ("l", "hwc_u8", False, [0, None, 0]), ("prepare", 0.25, 16, (3, 6, 8))]
    assert set(item) == {"smplx_params", "images", "camera", "bg_color", "cropped_images", "batch_id"}
    assert item["images"].shape == (3, 3, 7, 10) and item["cropped_images"].shape == (3, 3, 16, 16) and item["batch_id"] == 0
    bare = str(tmp_path / "no_masks")
    write_dataset(bare, 4, missing_masks=range(4))
    calls.clear()
    clip_data.load_dataset_clip(bare, 0, clip_length=2, crop_size=16, device="cpu")
    assert calls[0][3] == [2, 2] and calls[1] == ("prepare", 0.25, 16, None)  # no mask file at all: masks=None, all ones
