"""tests/jpeg_decode_model.py, the restatement of the decoder's pixel rules, against libjpeg's decode of the committed
fixtures (recorded beside them), and against its own evaluation in float32."""
import io

import numpy as np
import pytest

import jpeg_decode_cases as dc
import jpeg_decode_model as dm
import jpeg_model as jm

# Largest |rint(model) - libjpeg| per sampling and the share of samples beyond 1 level, over the fixtures.  libjpeg
# decodes with an integer IDCT and rounds the upsampled chroma; the model rounds once, at the end.
#                  bound    measured on the fixtures
MAX_LEVELS = {"444": 2,     # 2
              "420": 3,     # 2 (3 on 4e-6 of the samples of larger images)
              "gray": 1}    # 1
SHARE_ABOVE_1 = {"444": 0.0062,   # 0.0036 (smooth_444_33x50_q75_rr1_opt)
                 "420": 0.02,     # 0.0190 (noise_420_33x17_q95_rr1)
                 "gray": 0.0}     # 0
SHARE_ABOVE_2 = {"444": 0.0, "420": 4e-6, "gray": 0.0}  # 0 everywhere


def test_bounds_are_the_ones_the_gpu_test_builds_on():
    assert dc.LIBJPEG_MAX == MAX_LEVELS


@pytest.mark.parametrize("name", dc.NAMES)
def test_model_against_libjpeg(name):
    d = dc.decoded(name)
    sampling = dm.sampling_name(d)
    assert sampling == dc.FILES[name]["sampling"] and (d.height, d.width) == (dc.FILES[name]["height"], dc.FILES[name]["width"])
    rgb, _ = dc.model(name)
    diff = np.abs(dm.to_uint8(rgb).astype(np.int64) - dc.libjpeg_rgb(name).astype(np.int64))
    print(f"{name}: max {diff.max()}, above 1: {np.mean(diff > 1):.5f}, above 2: {np.mean(diff > 2):.6f}")
    assert diff.max() <= MAX_LEVELS[sampling]
    assert np.mean(diff > 1) <= SHARE_ABOVE_1[sampling]
    assert np.mean(diff > 2) <= SHARE_ABOVE_2[sampling]


@pytest.mark.parametrize("name", [n for n in dc.NAMES if dc.FILES[n]["sampling"] == "444"])
def test_444_is_jpeg_models_reconstruction(name):
    assert np.allclose(dc.model(name)[0], jm.reconstruct_444(dc.decoded(name)), rtol=0, atol=1e-9)


def test_recorded_decode_is_this_pillows():
    """libjpeg_rgb.npz holds libjpeg's decode; where this Pillow's libjpeg agrees (it need not), nothing drifted."""
    from PIL import Image

    same = [np.array_equal(np.asarray(Image.open(io.BytesIO(dc.jpeg(n))).convert("RGB")), dc.libjpeg_rgb(n)) for n in dc.NAMES]
    print(f"{sum(same)} of {len(same)} fixtures decode here as recorded")
    assert all(dc.libjpeg_rgb(n).shape == (dc.FILES[n]["height"], dc.FILES[n]["width"], 3) for n in dc.NAMES)


def test_chroma_rule_is_the_ceil_plane_triangle():
    """Replicating each chroma sample 2x2 is far off libjpeg (13..64 levels on the 4:2:0 fixtures, 18 here).  Filtering the
    block-padded plane instead of the ceil(H/2) x ceil(W/2) one differs in the last odd row / column only, and libjpeg's
    own files hide it (its encoder pads by replication, so the padding repeats the edge): here it must merely stay
    within the bound, the GPU test holds the kernel to the rule sample by sample."""
    name = "smooth_420_33x50_q30_opt"
    d, want = dc.decoded(name), dc.libjpeg_rgb(name).astype(np.int64)
    planes = dm._component_planes(d, np.float64)
    H, W = d.height, d.width

    def rgb_with(upsample):
        Y = planes[0][0][:H, :W]
        cb, cr = (upsample(p) - 128.0 for p, _ in planes[1:])
        return dm.to_uint8(np.stack([Y + 1.402 * cr, Y - 0.344136 * cb - 0.714136 * cr, Y + 1.772 * cb], axis=-1)).astype(np.int64)

    rule = rgb_with(lambda p: dm._triangle(p[:-(-H // 2), :-(-W // 2)], H, W, np.float64))
    padded = rgb_with(lambda p: dm._triangle(p, p.shape[0] * 2, p.shape[1] * 2, np.float64)[:H, :W])
    replicated = rgb_with(lambda p: p.repeat(2, axis=0).repeat(2, axis=1)[:H, :W])
    assert np.abs(rule - want).max() <= MAX_LEVELS["420"]
    assert np.abs(padded - want).max() <= MAX_LEVELS["420"] and np.abs(replicated - want).max() > 4 * MAX_LEVELS["420"]


@pytest.mark.parametrize("name", dc.NAMES)
def test_float32_evaluation_stays_inside_the_bound(name):
    """The condition the GPU test puts on its inputs: evaluated in float32, the model differs from its float64 rounding
    by at most 1, only where the float64 value is within delta of a half-integer, and such samples are at most 1 %."""
    d = dc.decoded(name)
    rgb, delta = dc.model(name)
    rgb32, _ = dm.reconstruct(d, np.float32)
    assert rgb32.dtype == np.float32
    assert np.abs(rgb32.astype(np.float64) - rgb).max() <= delta.max()
    assert np.all(np.abs(rgb32.astype(np.float64) - rgb) <= delta)
    worst, decided_but_different, undecided = dm.disagreement(dm.to_uint8(rgb32), rgb, delta)
    assert worst <= 1 and decided_but_different == 0 and undecided <= 0.01, (worst, decided_but_different, undecided)


def test_the_set_reaches_every_branch_of_the_scan():
    ds = [dc.decoded(n) for n in dc.NAMES]
    assert sum(d.zrl for d in ds) > 0 and sum(d.blocks_without_eob for d in ds) > 0 and sum(d.stuffed for d in ds) > 0
    assert max(d.max_ac_category for d in ds) >= 10 and max(d.max_dc_category for d in ds) >= 10
    assert max(len(d.rst) for d in ds) > 8, "the RSTn cycle wraps"
    assert {dm.sampling_name(d) for d in ds} == {"444", "420", "gray"}
