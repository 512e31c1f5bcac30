"""The image half of the reference's training data on the device: a Motion-JPEG clip or a directory of PNG frames (and
its segmentation-mask clip) -> the tensors GaussianAudioDataset.__getitem__ calls `images` and `cropped_images`
(src/datasets/dataset_speech_vid.py:170-252) and collate_fn_speech's split of them into reference and target frames
(src/utils/data_utils.py:83-104); and load_dataset_clip, the whole item of __getitem__ but its audio feature, from a
directory laid out like the reference's dataset (imgs_png/, samurai_seg/, smplx_params/).

Two load_clip calls (bytes up, one ops.jpeg_decode or ops.png_decode each) and one ops.prepare_frames call; the decoder's
status words are read back once, at the end, which is the only host synchronisation."""
import json
import os

import torch

from . import mjpeg, ops, png


def _is_png_dir(path):
    """A directory that holds no .jpg / .jpeg but does hold .png files: the reference's imgs_png/ and samurai_seg/."""
    if not isinstance(path, (str, os.PathLike)) or not os.path.isdir(path):
        return False
    names = [n.lower() for n in os.listdir(path)]
    return not any(n.endswith((".jpg", ".jpeg")) for n in names) and any(n.endswith(".png") for n in names)


def _prepare(who, rgb, mask, status, is_png, picked, pad_ratio, crop_size):
    images, cropped, boxes = ops.prepare_frames(rgb, mask, pad_ratio=pad_ratio, crop_size=crop_size)
    flagged = status.cpu().tolist()  # the one read-back
    bad = [i for i, s in enumerate(flagged) if s]
    if bad:
        n = rgb.shape[0]
        raise (png.PngError if is_png else mjpeg.JpegError)(f"{who}: damaged " + ", ".join(
            f"{'mask' if i >= n else 'frame'} {i % n if picked is None else picked[i % n]}" for i in bad))
    return {"images": images, "cropped_images": cropped, "boxes": boxes}


def load_training_clip(frames_path, masks_path=None, frames=None, pad_ratio=0.0, crop_size=1024, device="cuda"):
    """{"images": fp32 [F,3,Hp,Wp], "cropped_images": fp32 [F,3,crop_size,crop_size], "boxes": int32 [F,5]} on `device`.

    frames_path / masks_path: anything mjpeg.load_clip reads (.avi, .mjpeg, a frames directory, an open reader), or a
    directory of PNG files (no .jpg in it: the reference's imgs_png/ and samurai_seg/), or a png.PngDirReader; the mask
    clip may be grey or colour (a JPEG clip's first channel is the mask; a PNG goes through convert("L")) and None means
    all ones, the reference's answer to a missing mask file.  `frames`: indices into both clips, e.g. range(i, i + 16, 2)
    for the reference's stride-2 clips of 8.  Raises mjpeg.JpegError (png.PngError when a PNG clip is involved) naming
    the frames the decoder flagged."""
    picked = None if frames is None else [int(i) for i in frames]
    frames_png = isinstance(frames_path, png.PngDirReader) or _is_png_dir(frames_path)
    masks_png = isinstance(masks_path, png.PngDirReader) or _is_png_dir(masks_path)
    if frames_png:
        rgb, status = png.load_clip(frames_path, frames=picked, mode="rgb", device=device, layout="hwc_u8", check=False)
    else:
        rgb, status = mjpeg.load_clip(frames_path, frames=picked, device=device, layout="hwc_u8", check=False)
    mask = None
    if masks_path is not None:
        if masks_png:
            mask, mask_status = png.load_clip(masks_path, frames=picked, mode="l", device=device, layout="hwc_u8", check=False)
            shape = tuple(mask.shape)
        else:
            grey, mask_status = mjpeg.load_clip(masks_path, frames=picked, device=device, layout="hwc_u8", check=False)
            mask, shape = grey[..., 0], tuple(grey.shape[:3])
        if shape != tuple(rgb.shape[:3]):
            raise ValueError(f"load_training_clip: mask clip {shape} does not match the frames {tuple(rgb.shape[:3])}")
        status = torch.cat([status, mask_status])
    return _prepare("load_training_clip", rgb, mask, status, frames_png or masks_png, picked, pad_ratio, crop_size)


# the reference's renaming of the JSON's keys (_load_smplx_params, src/datasets/dataset_speech_vid.py:119-141)
SMPLX_KEYS = {"betas": "betas", "trans": "transl", "root_pose": "global_orient", "body_pose": "body_pose",
              "lhand_pose": "left_hand_pose", "rhand_pose": "right_hand_pose", "jaw_pose": "jaw_pose", "leye_pose": "leye_pose",
              "reye_pose": "reye_pose", "focal": "focal", "princpt": "princpt"}


def dataset_clip_host(root_dir, index, clip_length=8):
    """The host half of load_dataset_clip, no device and no image decode: (frame ids, item).  Frame ids: the stems of
    imgs_png/*.png in the order of int(stem), taken at index, index + 2, ... below index + 2 * clip_length and the last
    one repeated up to clip_length where the directory ends early.  item: `smplx_params` (stacked fp32 tensors under
    the reference's keys, `expression` ten zeros, `pad_ratio` / `focal` / `princpt` kept), `camera` (`intrinsic`
    [F,3,3] from focal / princpt, `extrinsic` [F,4,4] identities), `bg_color` ones [F,3], `batch_id`, and `pad_ratio`,
    the clip's one value as a float (ValueError if the frames disagree: the reference's torch.stack of padded images of
    unequal size fails there too; ValueError also for a .png in imgs_png/ whose stem is not a number)."""
    index, clip_length = int(index), int(clip_length)
    names = [n for n in os.listdir(os.path.join(root_dir, "imgs_png")) if n.lower().endswith(".png")]
    stray = sorted(n for n in names if not n.split(".")[0].isdigit())
    if stray:  # the frame number names the mask and the JSON of a frame (the reference's int(frame_id) fails here too)
        raise ValueError(f"load_dataset_clip: imgs_png/{stray[0]} is not named by a frame number (%05d.png)")
    names.sort(key=lambda n: int(n.split(".")[0]))
    if clip_length < 1 or not 0 <= index < len(names):
        raise IndexError(f"load_dataset_clip: index {index} / clip_length {clip_length} with {len(names)} frames")
    ids = [int(names[i].split(".")[0]) for i in range(index, min(index + 2 * clip_length, len(names)), 2)]
    ids += [ids[-1]] * (clip_length - len(ids))
    per_frame, ratios = [], set()
    for frame_id in ids:
        with open(os.path.join(root_dir, "smplx_params", f"{frame_id:05d}.json")) as fh:
            raw = json.load(fh)
        params = {ours: torch.tensor(raw[theirs], dtype=torch.float32) for theirs, ours in SMPLX_KEYS.items()}
        ratios.add(float(raw.get("pad_ratio", 0.0)))  # the padding is computed from the double, as the reference does
        params["pad_ratio"] = torch.tensor(float(raw.get("pad_ratio", 0.0)), dtype=torch.float32)
        params["expression"] = torch.zeros(10)
        per_frame.append(params)
    if len(ratios) != 1:
        raise ValueError(f"load_dataset_clip: pad_ratio differs inside the clip ({sorted(ratios)}): its padded images cannot be stacked")
    smplx = {k: torch.stack([p[k] for p in per_frame]) for k in per_frame[0]}
    F = len(ids)
    intrinsic = torch.eye(3).repeat(F, 1, 1)
    intrinsic[:, 0, 0], intrinsic[:, 1, 1] = smplx["focal"][:, 0], smplx["focal"][:, 1]
    intrinsic[:, 0, 2], intrinsic[:, 1, 2] = smplx["princpt"][:, 0], smplx["princpt"][:, 1]
    item = {"smplx_params": smplx, "camera": {"intrinsic": intrinsic, "extrinsic": torch.eye(4).repeat(F, 1, 1)},
            "bg_color": torch.ones(F, 3), "batch_id": index, "pad_ratio": ratios.pop()}
    return ids, item


def load_dataset_clip(root_dir, index, clip_length=8, crop_size=1024, device="cuda"):
    """GaussianAudioDataset.__getitem__(index) (src/datasets/dataset_speech_vid.py:147-293) without `audio_feature`
    (audio_frontend.py owns it), from root_dir/imgs_png, root_dir/samurai_seg and root_dir/smplx_params: `images`,
    `cropped_images` (ops.prepare_frames of the PNG files decoded on the device; a missing mask file is all ones, per
    frame), `smplx_params`, `camera`, `bg_color` and `batch_id` as dataset_clip_host describes, every tensor on `device`.
    No Pillow and no host decode are on this path.  A missing image file raises FileNotFoundError (the reference
    substitutes a black 512 x 512 frame there)."""
    ids, item = dataset_clip_host(root_dir, index, clip_length)
    pad_ratio = item.pop("pad_ratio")

    def read(folder, frame_id, optional):
        path = os.path.join(root_dir, folder, f"{frame_id:05d}.png")
        if optional and not os.path.exists(path):
            return None
        with open(path, "rb") as fh:
            return fh.read()

    rgb, status = png.load_clip([read("imgs_png", i, False) for i in ids], mode="rgb", device=device, layout="hwc_u8", check=False)
    masks = [read("samurai_seg", i, True) for i in ids]
    mask = None
    if any(m is not None for m in masks):
        mask, mask_status = png.load_clip(masks, mode="l", device=device, layout="hwc_u8", check=False)
        if tuple(mask.shape) != tuple(rgb.shape[:3]):
            raise ValueError(f"load_dataset_clip: masks {tuple(mask.shape)} do not match the frames {tuple(rgb.shape[:3])}")
        status = torch.cat([status, mask_status])
    clip = _prepare("load_dataset_clip", rgb, mask, status, True, ids, pad_ratio, crop_size)
    to = lambda t: t.to(device)  # noqa: E731
    return {"smplx_params": {k: to(v) for k, v in item["smplx_params"].items()}, "images": clip["images"],
            "camera": {k: to(v) for k, v in item["camera"].items()}, "bg_color": to(item["bg_color"]),
            "cropped_images": clip["cropped_images"], "batch_id": item["batch_id"]}


def split_ref_target(clip, n_ref=2, n_target=6):
    """collate_fn_speech's slicing of one clip (views, no copies): the first n_ref frames are the reference, the last
    n_target the target; `cropped_images` is kept for the reference frames only."""
    n = clip["images"].shape[0]
    if n < max(n_ref, n_target):
        raise ValueError(f"split_ref_target: a clip of {n} frames is shorter than n_ref={n_ref} / n_target={n_target}")
    return {"ref_images": clip["images"][:n_ref], "target_video": clip["images"][n - n_target:],
            "cropped_images": clip["cropped_images"][:n_ref]}
