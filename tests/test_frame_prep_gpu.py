"""ops.prepare_frames (amav_frames_prepare) on the device against the NumPy model (tests/frame_prep_model.py) and against
what the reference's own dataset code returned (tests/golden/ref_frame_prep*.npz).

Tolerances.  `boxes` and `images` are exact.  `cropped` is compared with the model's float64 evaluation of the same fp32
weights and taps: the kernel rounds four products, two inner sums, two outer products and the last sum of values <= 1,
at most 2^-25 each and not all at full size (bound 3 x 2^-24); the test allows 6 x 2^-24.  Against the reference's fp32
result, which makes as many roundings of its own in another order, 12 x 2^-24.  A wrong tap is wrong by grey levels."""
import numpy as np
import pytest
import torch

import frame_prep_cases as fc
import frame_prep_model as fm

pytestmark = pytest.mark.gpu

TOL_MODEL, TOL_REF = 6 * 2.0 ** -24, 12 * 2.0 ** -24
_cache = {}


def golden():
    if "golden" not in _cache:
        _cache["golden"] = fc.load_golden()
    return _cache["golden"]


def model(name, side):
    """(images list, float64 cropped, boxes) of a case, computed once"""
    if (name, side) not in _cache:
        case = fc.nine_frames() if name == "nine" else fc.case(name)
        _cache[name, side] = fm.prepare(case, side, wide=True)
    return _cache[name, side]


def device_inputs(case):
    frames = torch.from_numpy(case["frames"]).cuda()
    masks = None if case["masks"] is None else torch.from_numpy(case["masks"]).cuda()
    return frames, masks


def run(case, side, **kw):
    from audio_motion_avatar_amd import ops

    frames, masks = device_inputs(case)
    return ops.prepare_frames(frames, masks, pad_ratio=case["pad_ratio"], crop_size=side, **kw)


@pytest.mark.parametrize("name", fc.CASES)
def test_cases_at_the_reference_size(name):
    case = fc.case(name)
    images, cropped, boxes = run(case, fc.REF_SIDE)
    want_images, want_cropped, want_boxes = model(name, fc.REF_SIDE)
    assert boxes.dtype == torch.int32 and np.array_equal(boxes.cpu().numpy(), want_boxes), (boxes.tolist(), want_boxes.tolist())
    got = images.cpu().numpy()
    assert got.dtype == np.float32 and np.array_equal(got, np.stack(want_images)), "images: the model, bit for bit"
    if name in fc.SMALL_IMAGES:
        assert np.array_equal(got, golden()[name + "/images"]), "images: the reference, bit for bit"
    got = cropped.cpu().numpy()
    assert got.shape == want_cropped.shape and got.dtype == np.float32
    worst = float(np.abs(got - want_cropped).max())
    ref = golden()[name + "/cropped"]
    worst_ref = float(np.abs(got[:, :, fc.golden_positions()].astype(np.float64) - ref).max())
    print(f"{name}: |kernel - float64 model| {worst * 2 ** 24:.2f} x 2^-24, |kernel - reference| {worst_ref * 2 ** 24:.2f} x 2^-24")
    assert worst <= TOL_MODEL
    assert worst_ref <= TOL_REF


@pytest.mark.parametrize("side", [64, 1])
@pytest.mark.parametrize("name", ["a_blob", "b_top_right", "f_dots"])
def test_small_outputs(name, side):
    """64: the four-wide store path, shrinking and enlarging; 1: the scalar path and scale = 0"""
    _, cropped, boxes = run(fc.case(name), side, images=False)
    _, want, want_boxes = model(name, side)
    assert np.array_equal(boxes.cpu().numpy(), want_boxes)
    assert float(np.abs(cropped.cpu().numpy() - want).max()) <= TOL_MODEL


def test_odd_output_side_takes_the_scalar_path():
    _, cropped, _ = run(fc.case("e_padded"), 37, images=False)
    assert float(np.abs(cropped.cpu().numpy() - model("e_padded", 37)[1]).max()) <= TOL_MODEL


def test_max_size_equal_to_the_output_is_the_square_image():
    case = fc.case("b_top_right")
    images, cropped, boxes = run(case, 37)
    assert boxes.tolist() == [[0, 36, 40, 71, 37]]
    assert np.array_equal(cropped.cpu().numpy()[0], fm.square(images.cpu().numpy()[0], tuple(boxes.tolist()[0])))


def test_layouts_and_views_give_the_same_bits():
    from audio_motion_avatar_amd import ops

    case = fc.nine_frames()
    frames, masks = device_inputs(case)
    base = ops.prepare_frames(frames, masks, crop_size=64)
    chw = (frames.cpu().permute(0, 3, 1, 2).float() / 255.0).contiguous().cuda()  # the decoder's fp32 layout: byte / 255
    mask_f = (masks.cpu().float() / 255.0).cuda()
    grey = masks[..., None].expand(-1, -1, -1, 3).contiguous()  # a decoded grey clip: R = G = B
    wide = torch.zeros(9, fc.H + 2, fc.W + 5, 3, dtype=torch.uint8, device="cuda")
    wide[:, 1:-1, 2:-3] = frames
    for other in (ops.prepare_frames(chw, masks, crop_size=64), ops.prepare_frames(frames, mask_f, crop_size=64),
                  ops.prepare_frames(chw, mask_f, crop_size=64), ops.prepare_frames(frames, grey[..., 0], crop_size=64),
                  ops.prepare_frames(wide[:, 1:-1, 2:-3], grey[..., 0], crop_size=64)):
        assert all(torch.equal(a, b) for a, b in zip(base, other))
    # every second frame of a longer clip: a frame stride that is no multiple of the frame size
    picked = ops.prepare_frames(frames[::2], masks[::2], crop_size=64)
    assert all(torch.equal(a[::2], b) for a, b in zip(base, picked))


def test_normalize_is_torchs_subtract_and_divide():
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    case = fc.case("h_graded")
    _, plain, _ = run(case, 64, images=False)
    _, normed, _ = run(case, 64, images=False, normalize=(mean, std))
    want = (plain.cpu() - torch.tensor(mean).view(1, 3, 1, 1)) / torch.tensor(std).view(1, 3, 1, 1)  # on the host: IEEE
    assert torch.equal(normed.cpu(), want)


def test_two_runs_are_bit_equal():
    case = fc.nine_frames()
    first = run(case, 128)
    for _ in range(3):
        assert all(torch.equal(a, b) for a, b in zip(first, run(case, 128)))


def test_skipped_outputs_are_not_touched():
    from audio_motion_avatar_amd import ops

    case = fc.case("e_padded")
    frames, masks = device_inputs(case)
    sentinel_i = torch.full((1, 3, 105, 79), -7.0, device="cuda")
    sentinel_c = torch.full((1, 3, 64, 64), -7.0, device="cuda")
    full = ops.prepare_frames(frames, masks, pad_ratio=0.1, crop_size=64)
    images, cropped, boxes = ops.prepare_frames(frames, masks, pad_ratio=0.1, crop_size=64, images=False, out_images=sentinel_i,
                                                out_cropped=sentinel_c)
    assert images is None and cropped is sentinel_c and bool((sentinel_i == -7.0).all())
    assert torch.equal(cropped, full[1]) and torch.equal(boxes, full[2])
    sentinel_c.fill_(-7.0)
    images, cropped, boxes = ops.prepare_frames(frames, masks, pad_ratio=0.1, crop_size=64, cropped=False, out_images=sentinel_i,
                                                out_cropped=sentinel_c)
    assert cropped is None and images is sentinel_i and bool((sentinel_c == -7.0).all())
    assert torch.equal(images, full[0]) and torch.equal(boxes, full[2])
    # through the C ABI with neither output: the boxes alone, and guard elements behind them stay
    from audio_motion_avatar_amd import _lib

    guard = torch.full((8,), -7, dtype=torch.int32, device="cuda")
    ws = torch.empty(_lib.lib().amav_frames_prepare_workspace_bytes(1), dtype=torch.uint8, device="cuda")
    ops._call("amav_frames_prepare", 1, fc.H, fc.W, frames.data_ptr(), 0, *frames.permute(0, 3, 1, 2).stride(), masks.data_ptr(), 0,
              *masks.stride(), 105, 79, 4, 3, 64, None, None, None, 0, None, 0, guard.data_ptr(), 20, ws.data_ptr(), ws.numel())
    assert guard.tolist() == full[2].tolist()[0] + [-7, -7, -7]


def test_capacity_one_element_short_is_refused():
    from audio_motion_avatar_amd import AmavError, _lib, ops

    case = fc.case("a_blob")
    frames, masks = device_inputs(case)
    ws = torch.empty(_lib.lib().amav_frames_prepare_workspace_bytes(1), dtype=torch.uint8, device="cuda")
    images = torch.full((3 * fc.H * fc.W,), -7.0, device="cuda")
    cropped = torch.full((3 * 64 * 64,), -7.0, device="cuda")
    boxes = torch.full((5,), -7, dtype=torch.int32, device="cuda")

    def call(images_bytes, cropped_bytes, boxes_bytes):
        ops._call("amav_frames_prepare", 1, fc.H, fc.W, frames.data_ptr(), 0, *frames.permute(0, 3, 1, 2).stride(),
                  masks.data_ptr(), 0, *masks.stride(), fc.H, fc.W, 0, 0, 64, None, None, images.data_ptr(), images_bytes,
                  cropped.data_ptr(), cropped_bytes, boxes.data_ptr(), boxes_bytes, ws.data_ptr(), ws.numel())

    full = (images.numel() * 4, cropped.numel() * 4, 20)
    for short in range(3):
        sizes = [n - 4 if i == short else n for i, n in enumerate(full)]
        with pytest.raises(AmavError, match="buffer"):
            call(*sizes)
    torch.cuda.synchronize()
    assert bool((images == -7.0).all()) and bool((cropped == -7.0).all()) and boxes.tolist() == [-7] * 5, "nothing was launched"
    call(*full)
    want = ops.prepare_frames(frames, masks, crop_size=64)
    assert torch.equal(images.view(1, 3, fc.H, fc.W), want[0]) and torch.equal(cropped.view(1, 3, 64, 64), want[1])
    assert boxes.tolist() == want[2].tolist()[0]


def test_one_frame_and_nine_frames_in_one_call():
    """Nine different masks in one call: the frames do not share a box, and each frame equals its own single-frame call."""
    from audio_motion_avatar_amd import ops

    case = fc.nine_frames()
    images, cropped, boxes = run(case, 64)
    want_images, want_cropped, want_boxes = model("nine", 64)
    assert np.array_equal(boxes.cpu().numpy(), want_boxes) and len({tuple(b) for b in want_boxes.tolist()}) == 9
    assert np.array_equal(images.cpu().numpy(), np.stack(want_images))
    assert float(np.abs(cropped.cpu().numpy() - want_cropped).max()) <= TOL_MODEL
    frames, masks = device_inputs(case)
    for f in (0, 4, 8):
        one = ops.prepare_frames(frames[f:f + 1], masks[f:f + 1], crop_size=64)
        assert all(torch.equal(a, b[f:f + 1]) for a, b in zip(one, (images, cropped, boxes)))


def test_autograd_inputs_are_refused():
    from audio_motion_avatar_amd import AmavError, ops

    frames = torch.rand(1, 3, 8, 8, device="cuda", requires_grad=True)
    with pytest.raises(AmavError, match="carries no autograd"):
        ops.prepare_frames(frames, crop_size=8)
    with torch.no_grad():
        images, cropped, boxes = ops.prepare_frames(frames, crop_size=8)
    assert torch.equal(images, frames.detach()) and boxes.tolist() == [[0, 6, 0, 6, 7]]
