"""mjpeg.load_clip on the device: a clip written by AviWriter from the project's encoder comes back as the tensor the
decoder makes of its frames, by range and by index list, from an .avi, a bare .mjpeg and a frames directory; a damaged
frame raises with its index; the result feeds losses.image_losses as it is."""
import os

import numpy as np
import pytest
import torch

import jpeg_cases as jc
import jpeg_decode_model as dm

pytestmark = pytest.mark.gpu

H, W, F = 24, 40, 5


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    """(directory, the frames' JPEG bytes, the float64 model's uint8 decode of each)"""
    from audio_motion_avatar_amd import mjpeg, ops

    root = tmp_path_factory.mktemp("clip")
    frames = torch.from_numpy(jc.disc(F, H, W)).cuda()
    stream, offsets = ops.jpeg_encode(frames, quality=90, subsampling="420", restart_rows=1)
    data = stream.cpu().numpy().tobytes()
    jpegs = [data[int(a):int(b)] for a, b in zip(offsets[:-1], offsets[1:])]
    pcm = np.zeros(8000, dtype="<i2").tobytes()
    with mjpeg.AviWriter(str(root / "clip.avi"), H, W, 24.0, audio=(pcm, 1, 8000)) as w:
        for j in jpegs:
            w.write_frame(j)
    (root / "clip.mjpeg").write_bytes(b"".join(jpegs))
    os.makedirs(root / "frames")
    for i, j in enumerate(jpegs):
        (root / "frames" / f"frame_{i:03d}.jpg").write_bytes(j)
    models = [dm.reconstruct(dm.decode(j)) for j in jpegs]
    return root, jpegs, models


def test_round_trip_through_the_avi(clip):
    from audio_motion_avatar_amd import mjpeg

    root, jpegs, models = clip
    video = mjpeg.load_clip(str(root / "clip.avi"))
    assert video.is_cuda and video.dtype == torch.float32 and tuple(video.shape) == (F, 3, H, W)
    bytes8 = mjpeg.load_clip(str(root / "clip.avi"), layout="hwc_u8")
    assert bytes8.dtype == torch.uint8 and tuple(bytes8.shape) == (F, H, W, 3)
    # the dataset's `float() / 255.0` of an 8-bit decode, a true division (on the host: the device's division by a
    # scalar multiplies by its reciprocal, which is not the same number everywhere)
    assert torch.equal(video.cpu(), bytes8.cpu().permute(0, 3, 1, 2).float() / 255.0)
    got = bytes8.cpu().numpy()
    for f, (rgb, delta) in enumerate(models):
        worst, decided_but_different, undecided = dm.disagreement(got[f], rgb, delta)
        assert undecided <= 0.01 and worst <= 1 and decided_but_different == 0, (f, worst, decided_but_different, undecided)
    source = jc.disc(F, H, W)
    assert jc.psnr(got, source) > 25.0, "and it is the clip that was written"
    for other in ("clip.mjpeg", "frames"):
        assert torch.equal(mjpeg.load_clip(str(root / other), layout="hwc_u8"), bytes8), other


def test_frame_selection(clip):
    from audio_motion_avatar_amd import mjpeg

    root = clip[0]
    whole = mjpeg.load_clip(str(root / "clip.avi"))
    assert torch.equal(mjpeg.load_clip(str(root / "clip.avi"), frames=range(0, F, 2)), whole[0::2])
    assert torch.equal(mjpeg.load_clip(str(root / "clip.avi"), frames=[4, 1, 1]), whole[[4, 1, 1]])
    out, status = mjpeg.load_clip(str(root / "clip.mjpeg"), frames=[3], check=False)
    assert torch.equal(out, whole[3:4]) and status.is_cuda and status.dtype == torch.int32 and status.tolist() == [0]


def test_check_names_the_damaged_frame(clip, tmp_path):
    from audio_motion_avatar_amd import mjpeg

    root, jpegs, _ = clip
    begin = mjpeg.parse_jpeg(jpegs[2])[0].scan_begin
    rst = jpegs[2].index(b"\xff\xd0", begin)
    broken = jpegs[2][:rst] + jpegs[2][rst + 2:]  # the first restart marker is gone
    with mjpeg.AviWriter(str(tmp_path / "broken.avi"), H, W, 24.0) as w:
        for j in jpegs[:2] + [broken] + jpegs[3:]:
            w.write_frame(j)
    with pytest.raises(mjpeg.JpegError, match=r"damaged frames 2 \(markers"):
        mjpeg.load_clip(str(tmp_path / "broken.avi"))
    assert torch.equal(mjpeg.load_clip(str(tmp_path / "broken.avi"), frames=[0, 1, 3, 4]),
                       mjpeg.load_clip(str(root / "clip.avi"), frames=[0, 1, 3, 4]))
    out, status = mjpeg.load_clip(str(tmp_path / "broken.avi"), check=False)
    assert status.tolist()[:2] == [0, 0] and status.tolist()[3:] == [0, 0] and status.tolist()[2] & 1


def test_the_clip_is_a_training_target_as_it_is(clip):
    from audio_motion_avatar_amd import mjpeg
    from audio_motion_avatar_amd.losses import image_losses

    target = mjpeg.load_clip(str(clip[0] / "clip.avi"))[None].permute(0, 1, 3, 4, 2)  # [B, T, H, W, C], a view
    rendered = torch.from_numpy(jc.disc(F, H, W)).cuda().float().div(255.0)[None].requires_grad_()
    l1, ssim = image_losses(rendered, target)
    (l1 + (1 - ssim)).backward()
    l1, ssim = float(l1.detach()), float(ssim.detach())
    assert 0 < l1 < 0.1 and 0.5 < ssim < 1.0, (l1, ssim)
    assert rendered.grad is not None and torch.isfinite(rendered.grad).all()
