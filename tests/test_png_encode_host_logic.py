"""Host logic of the PNG output path: save_image's normalisation against a NumPy restatement (and against torchvision
where it imports), the comparison sheet's layout, the shapes save_image takes.

Two tests here run no project code: test_nearest_rounding_is_the_torch_expression and
test_filter_model_round_trips_through_the_unfilter_model validate the reference models of png_encode_cases.py
(to_levels against the torch expression save_image evaluates, filter_rows against Pillow's unfilter) that the GPU tests
then hold the kernels to.  The project's own rounding and filters run on the device only and are checked there
(tests/test_png_encode_frames_gpu.py)."""
import numpy as np
import pytest
import torch

import png_encode_cases as ec


def numpy_normalize(x):
    x = np.asarray(x, np.float32)
    low, high = x.min(), x.max()
    return ((np.clip(x, low, high) - low) / np.maximum(high - low, np.float32(1e-5))).astype(np.float32)


def test_nearest_rounding_is_the_torch_expression():
    """Validates the reference model only (see the module docstring)."""
    x = ec.edge_values(np.random.default_rng(5), (3, 41, 67))
    x[0, 0, :4] = [np.inf, -np.inf, -0.0, 1.0]
    want = torch.from_numpy(x.copy()).mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8).numpy()
    assert np.array_equal(ec.to_levels(x, "nearest"), want)
    k = np.arange(256, dtype=np.float32)
    assert np.array_equal(ec.to_levels(k / np.float32(255), "nearest"), np.arange(256))  # decode(encode) is the identity
    assert np.array_equal(ec.to_levels(k / np.float32(255), "truncate"),
                          (np.clip(k / np.float32(255), 0, 1) * np.float32(255)).astype(np.uint8))
    assert ec.to_levels(np.float32("nan"), "nearest") == 0 and ec.to_levels(np.float32("nan"), "truncate") == 0


@pytest.mark.parametrize("case", ["spread", "flat", "negative"])
def test_normalisation_equals_the_numpy_restatement(case):
    from audio_motion_avatar_amd import png

    rng = np.random.default_rng(11)
    x = {"spread": rng.normal(0.3, 2.0, (3, 19, 23)), "flat": np.full((3, 5, 7), 0.25),
         "negative": -rng.random((1, 9, 4)) - 3}[case].astype(np.float32)
    got = png.normalize_range(torch.from_numpy(x)).numpy()
    assert np.array_equal(got, numpy_normalize(x))
    assert got.min() == 0 and (case == "flat" or got.max() == 1)
    try:
        from torchvision.utils import make_grid
    except ImportError:
        return
    grid = make_grid(torch.from_numpy(x)[None], normalize=True, padding=0).numpy()
    assert np.array_equal(np.broadcast_to(got, grid.shape), grid)


def test_comparison_sheet_layout():
    from audio_motion_avatar_amd import png

    rng = np.random.default_rng(2)
    T, H, W = 3, 5, 4
    rendered, real = rng.random((T, H, W, 3), dtype=np.float32), rng.random((T, 3, H, W), dtype=np.float32)
    sheet = png.comparison_sheet(torch.from_numpy(rendered), torch.from_numpy(real)).numpy()
    assert sheet.shape == (3, T * H, 2 * W)
    for t in range(T):
        assert np.array_equal(sheet[:, t * H:(t + 1) * H, :W], rendered[t].transpose(2, 0, 1))
        assert np.array_equal(sheet[:, t * H:(t + 1) * H, W:], real[t])


def test_one_image_shapes():
    from audio_motion_avatar_amd import png

    assert png._one_image(torch.zeros(3, 4, 5), "t").shape == (1, 3, 4, 5)
    assert png._one_image(torch.zeros(1, 4, 5), "t").shape == (1, 4, 5)
    assert png._one_image(torch.zeros(4, 5), "t").shape == (1, 4, 5)
    with pytest.raises(ValueError):
        png._one_image(torch.zeros(2, 4, 5), "t")


@pytest.mark.parametrize("which", [0, 1, 2, 3, 4, "adaptive"])
def test_filter_model_round_trips_through_the_unfilter_model(which):
    """The NumPy filter restatement the GPU tests hold the kernel to, undone by Pillow: validates the reference model only."""
    import io
    import struct
    import zlib

    from PIL import Image

    rng = np.random.default_rng(3)
    for shape in ((7, 5, 3), (4, 9, 1), (1, 1, 3)):
        img = rng.integers(0, 256, shape, dtype=np.uint8)
        H, W, C = shape

        def chunk(kind, body):
            return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body))

        blob = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2 if C == 3 else 0, 0, 0, 0)) + \
            chunk(b"IDAT", zlib.compress(ec.filter_rows(img, which))) + chunk(b"IEND", b"")
        back = np.asarray(Image.open(io.BytesIO(blob))).reshape(shape)
        assert np.array_equal(back, img)
