"""The NumPy model of the frame preparation (tests/frame_prep_model.py) against what the reference's own dataset code
returned for the same inputs (tests/golden/ref_frame_prep*.npz, written by tests/golden/make_frame_prep_golden.py):
`images` bit for bit, `cropped_images` within 12 x 2^-24 at every stored position (each side makes at most six roundings
of values <= 1; a wrong tap is an error of the order of a grey level, not of an ulp), the integer form of the 20 % box
padding, and known answers of the box arithmetic."""
import json
import os

import numpy as np
import pytest

import frame_prep_cases as fc
import frame_prep_model as fm

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
TOL = 12 * 2.0 ** -24


@pytest.fixture(scope="module")
def golden():
    return fc.load_golden()


def test_manifest_says_no_placeholder_was_used():
    m = json.load(open(os.path.join(GOLDEN, "ref_frame_prep_manifest.json")))
    assert m["placeholder_uses_during_run"] == 0
    assert [f["file"] for f in m["fixtures"]] == ["ref_frame_prep.npz", "ref_frame_prep_more.npz"]
    cases = {k: v for f in m["fixtures"] for k, v in f["meta"]["cases"].items()}
    assert sorted(cases) == sorted(fc.CASES)
    assert all(f["meta"]["positions"] == int(fc.golden_positions().sum()) for f in m["fixtures"])
    assert all(os.path.getsize(os.path.join(GOLDEN, f["file"])) < 1000000 for f in m["fixtures"])


@pytest.mark.parametrize("name", fc.CASES)
def test_model_against_the_reference(golden, name):
    case = fc.case(name)
    images, cropped, boxes = fm.prepare(case, fc.REF_SIDE)
    if name in fc.SMALL_IMAGES:
        ref = golden[name + "/images"]
        assert ref.dtype == np.float32 and ref.shape == np.stack(images).shape
        assert np.array_equal(ref, np.stack(images)), "images: bit for bit"
    ref = golden[name + "/cropped"]
    got = cropped[:, :, fc.golden_positions()]
    assert ref.shape == got.shape and got.dtype == np.float32
    worst = float(np.abs(ref.astype(np.float64) - got).max())
    print(f"{name}: boxes {boxes.tolist()} worst |model - reference| = {worst:.3e} ({worst * 2 ** 24:.2f} x 2^-24)")
    assert worst <= TOL
    wide = fm.prepare(case, fc.REF_SIDE, wide=True)[1][:, :, fc.golden_positions()]
    assert float(np.abs(ref - wide).max()) <= TOL


def test_fifth_is_the_reference_padding():
    h = np.arange(65536)
    assert np.array_equal((h * 0.2).astype(np.int64), h // 5)  # int(h * 0.2) in doubles, truncated
    assert all(int(v * 0.2) == v // 5 for v in (0, 1, 4, 5, 9, 10, 65534, 65535, 131071))


def test_box_known_answers():
    H, W = fc.H, fc.W
    b = fc.case("b_top_right")
    assert fm.box(b["masks"][0], H, W, H, W) == (0, 36, 40, 71, 37)  # both clamps: 37 x 32, not square
    assert fm.box(np.zeros((H, W), np.uint8), H, W, H, W) == (0, H - 1, 0, W - 1, H)
    assert fm.box(np.zeros((H, W), np.uint8), H, W, 105, 79) == (0, 104, 0, 78, 105)  # empty: the whole padded image
    f = fc.case("f_dots")
    assert fm.box(f["masks"][0], H, W, H, W) == (10, 10, 20, 20, 1)
    assert fm.box(f["masks"][1], H, W, H, W) == (9, 13, 20, 24, 5)
    # all ones: crop_size = 95, centre 47, 47 + 95 // 2 = 94: the reference's re-centring drops the last row
    assert fm.box(None, H, W, H, W) == (0, 94, 0, 71, 95)
    # two neighbours in a row: crop_size = 1, crop_size // 2 = 0, so the reference's box is a single pixel
    assert fm.box(fc.dots([(10, 20), (10, 21)]), H, W, H, W) == (10, 10, 20, 20, 1)
    assert fm.padded_size(96, 72, 0.1) == (105, 79, 4, 3) and fm.padded_size(512, 512, 0.1) == (563, 563, 25, 25)


def test_max_size_equal_to_the_output_is_the_square_image():
    case = fc.case("b_top_right")
    img = fm.images(case["frames"][0], case["masks"][0], 0.0)
    b = fm.box(case["masks"][0], fc.H, fc.W, fc.H, fc.W)
    assert np.array_equal(fm.cropped(img, b, b[4]), fm.square(img, b))
    assert fm.cropped(img, b, 1).shape == (3, 1, 1) and np.array_equal(fm.cropped(img, b, 1)[:, 0, 0], fm.square(img, b)[:, 0, 0])
