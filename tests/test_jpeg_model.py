"""jpeg_model.py against libjpeg (through Pillow): the model's tables are libjpeg's, its scan decoder reads libjpeg's
baseline files to the last byte, and what it decodes reconstructs to libjpeg's own decode."""
import io

import numpy as np
import pytest
from PIL import Image

import jpeg_cases as jc
import jpeg_model as jm


@pytest.mark.parametrize("quality", [1, 50, 90, 100])
def test_tables_are_libjpegs(quality):
    jpeg = jc.pillow_jpeg(jc.noise(1, 16, 16)[0], quality, "420", 1)
    im = Image.open(io.BytesIO(jpeg))
    tables = jm.quant_tables(quality)
    assert sorted(im.quantization) == [0, 1]
    for i in (0, 1):
        assert list(im.quantization[i]) == list(tables[i])
    assert tables.min() >= 1 and tables.max() <= 255
    if quality == 100:
        assert (tables == 1).all()
    if quality == 50:
        assert np.array_equal(tables, jm.QUANT_BASE)


def test_zigzag_is_the_standards():
    assert list(jm.ZIGZAG[:16]) == [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5]
    assert sorted(jm.ZIGZAG) == list(range(64)) and jm.ZIGZAG[63] == 63 and jm.ZIGZAG[62] == 62 and jm.ZIGZAG[61] == 55
    assert np.allclose(jm.DCT @ jm.DCT.T, np.eye(8), atol=1e-15)


PILLOW_FILES = [(name, sub) for name in ("noise_48x64_q50_rr2", "noise_17x33", "checkerboard_160x16", "disc_48x64_rr0_f3",
                                         "high_frequency_17x33", "white_1x1") for sub in ("420", "444")]


@pytest.mark.parametrize("name,subsampling", PILLOW_FILES)
def test_decoder_consumes_libjpegs_files(name, subsampling):
    """optimize=False, restart_marker_rows=1: every byte up to EOI, the header fields, RSTn in cyclic order."""
    _, _, H, W, quality, _, _ = jc.CASES[name]
    rgb = jc.frames(name)[0]
    jpeg = jc.pillow_jpeg(rgb, quality, subsampling, 1)
    d = jm.decode(jpeg)
    assert d.consumed == len(jpeg)
    assert (d.height, d.width) == (H, W)
    assert d.sampling == (((1, 1) if subsampling == "444" else (2, 2)), (1, 1), (1, 1))
    mcu, my, mx, bpm = jm.geometry(H, W, subsampling)
    assert d.restart_interval == mx and d.rst == [i % 8 for i in range(my - 1)]
    assert d.levels.shape == (my * mx * bpm, 64)
    tables = jm.quant_tables(quality)
    assert np.array_equal(d.quant[0], tables[0]) and np.array_equal(d.quant[1], tables[1])
    # and the same through Pillow's own view of the file
    im = Image.open(io.BytesIO(jpeg))
    assert list(im.quantization[0]) == list(d.quant[0])


@pytest.mark.parametrize("name", ["noise_48x64_q50_rr2", "noise_17x33", "checkerboard_80x8_444", "disc_48x64_444_rr2",
                                  "high_frequency_16x16_444", "noise_48x64_q8_444"])
def test_decoded_levels_reconstruct_to_libjpegs_decode(name):
    """4:4:4 files: dequantise, float IDCT, range-limit the samples as a decoder does, colour-convert: within 2 grey
    levels of libjpeg's integer IDCT and colour conversion (its documented accuracy)."""
    _, _, H, W, quality, _, _ = jc.CASES[name]
    jpeg = jc.pillow_jpeg(jc.frames(name)[0], quality, "444", 1)
    ours = np.clip(np.rint(jm.reconstruct_444(jm.decode(jpeg))), 0, 255)
    theirs = jc.pillow_decode(jpeg).astype(np.float64)
    assert ours.shape == theirs.shape == (H, W, 3)
    assert np.abs(ours - theirs).max() <= 2


@pytest.mark.parametrize("name", ["noise_48x64_q50_rr2", "disc_48x64_rr0_f3", "checkerboard_160x16"])
def test_model_levels_are_libjpegs_up_to_rounding(name):
    """Whole MCUs only (libjpeg fills blocks beyond the image differently): the float64 model and libjpeg's integer
    encoder agree on every level to within one, and on all but a few per cent."""
    _, _, H, W, quality, subsampling, _ = jc.CASES[name]
    assert H % 16 == 0 and W % 16 == 0
    want = jm.levels(jc.frames(name)[:1], quality, subsampling)[0]
    got = jm.decode(jc.libjpeg_streams(name)[0]).levels
    assert np.abs(want - got).max() <= 1 and np.mean(want != got) <= 0.05


def test_undecided_fraction_of_the_inputs():
    """The bound of test_jpeg_gpu.py's level check holds for its inputs by the model alone."""
    for name in jc.CASES:
        assert jm.undecided(jc.model_quotients(name), 0.01).mean() <= 0.05, name


def test_decoder_counts_what_the_streams_hold():
    """The events test_jpeg_gpu.py asks of the encoder are in libjpeg's streams of the same inputs."""
    seen = set()
    for name in jc.COUNTER_CASES:
        for s in jc.libjpeg_streams(name):
            seen |= jc.events(jm.decode(s))
    assert seen == {"stuffed", "zrl", "no_eob", "ac10", "dc10"}
    d = jm.decode(jc.libjpeg_streams("high_frequency_16x16_444")[0])
    assert d.zrl >= 3 and d.blocks_without_eob >= 1  # a block whose only coefficient is the scan's last
