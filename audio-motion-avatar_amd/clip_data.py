"""The image half of the reference's training data on the device: a Motion-JPEG clip (and its segmentation-mask clip) ->
the tensors GaussianAudioDataset.__getitem__ calls `images` and `cropped_images` (src/datasets/dataset_speech_vid.py:170-252)
and collate_fn_speech's split of them into reference and target frames (src/utils/data_utils.py:83-104).

Two mjpeg.load_clip calls (bytes up, one ops.jpeg_decode each) and one ops.prepare_frames call; the decoder's status words
are read back once, at the end, which is the only host synchronisation."""
import torch

from . import mjpeg, ops


def load_training_clip(frames_path, masks_path=None, frames=None, pad_ratio=0.0, crop_size=1024, device="cuda"):
    """{"images": fp32 [F,3,Hp,Wp], "cropped_images": fp32 [F,3,crop_size,crop_size], "boxes": int32 [F,5]} on `device`.

    frames_path / masks_path: anything mjpeg.load_clip reads (.avi, .mjpeg, a frames directory, an open reader); the mask
    clip may be grey or colour (its first channel is the mask, as PIL's convert("L") of a grey PNG) and None means all
    ones, the reference's answer to a missing mask file.  `frames`: indices into both clips, e.g. range(i, i + 16, 2)
    for the reference's stride-2 clips of 8.  Raises mjpeg.JpegError naming the frames the decoder flagged."""
    picked = None if frames is None else [int(i) for i in frames]
    rgb, status = mjpeg.load_clip(frames_path, frames=picked, device=device, layout="hwc_u8", check=False)
    mask = None
    if masks_path is not None:
        grey, mask_status = mjpeg.load_clip(masks_path, frames=picked, device=device, layout="hwc_u8", check=False)
        if grey.shape != rgb.shape:
            raise ValueError(f"load_training_clip: mask clip {tuple(grey.shape)} does not match the frames {tuple(rgb.shape)}")
        mask, status = grey[..., 0], torch.cat([status, mask_status])
    images, cropped, boxes = ops.prepare_frames(rgb, mask, pad_ratio=pad_ratio, crop_size=crop_size)
    flagged = status.cpu().tolist()  # the one read-back
    bad = [i for i, s in enumerate(flagged) if s]
    if bad:
        n = rgb.shape[0]
        raise mjpeg.JpegError("load_training_clip: damaged " + ", ".join(
            f"{'mask' if i >= n else 'frame'} {i % n if picked is None else picked[i % n]}" for i in bad))
    return {"images": images, "cropped_images": cropped, "boxes": boxes}


def split_ref_target(clip, n_ref=2, n_target=6):
    """collate_fn_speech's slicing of one clip (views, no copies): the first n_ref frames are the reference, the last
    n_target the target; `cropped_images` is kept for the reference frames only."""
    n = clip["images"].shape[0]
    if n < max(n_ref, n_target):
        raise ValueError(f"split_ref_target: a clip of {n} frames is shorter than n_ref={n_ref} / n_target={n_target}")
    return {"ref_images": clip["images"][:n_ref], "target_video": clip["images"][n - n_target:],
            "cropped_images": clip["cropped_images"][:n_ref]}
