"""Stage 1 with upsample_triplane, the parts that need no GPU: TriplaneDownsampler / ConvNeXtBlock (library path) and the
fp64 restatement of tests/downsampler_cases.py against the vectors produced by running the reference's own classes
(tests/golden/make_downsampler_golden.py -> ref_stage1_downsampler.npz, tier 1), the module's parameter names, the
refusals, and the host-side argument checks of the new entry points (no launch happens here).

Tolerance: the rule of tests/test_reference_golden.py for fp32 torch against fp32 torch on the same operators -- only the
summation order inside library kernels may differ: 2e-6 relative to the output scale (its close()).  The fp64
restatement differs from the fixture by the fixture's own fp32 rounding, which the same rule covers."""
import json
import os
from types import SimpleNamespace

import pytest
import torch

import downsampler_cases as dc
from abi_support import ERR_INVALID, ERR_WORKSPACE, FAKE, lib  # noqa: F401 (lib: fixture)
from helpers import ref_fixture, seeded_params
from test_reference_golden import close


def _module(meta):
    from audio_motion_avatar_amd.triplane_net import TriplaneDownsampler

    ds = TriplaneDownsampler(SimpleNamespace(**meta["cfg"])).eval()
    ds.load_state_dict(seeded_params(meta["params"], meta["param_prefix"]), strict=True)
    return ds


def test_manifest_says_no_placeholder_was_used():
    m = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "ref_downsampler_manifest.json")))
    assert m["placeholder_uses_during_run"] == 0
    assert {e["file"]: e["tier"] for e in m["fixtures"]} == {"ref_stage1_downsampler.npz": 1, "ref_stage1_upsampled.npz": 2}
    for e in m["fixtures"]:
        assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", e["file"])) < 1 << 20


def test_restatement_and_library_path_equal_the_reference_classes(monkeypatch):
    a, meta, tier = ref_fixture("stage1_downsampler")
    assert tier == 1 and meta["cfg"] == {"triplane_feature_dim": 64, "upsample_factor": 3}
    p = seeded_params(meta["params"], meta["param_prefix"])
    want = [dc.planes_of(a[k]) for k in ("after_block0", "after_block1", "y")]
    for got, w, what in zip(dc.downsampler(dc.to(p, torch.float64), "", dc.planes_of(a["x"]).double(), 3), want,
                            ("block 0", "block 1", "output")):
        close(got.float(), w, what=f"fp64 restatement, {what}")
    monkeypatch.setenv("AMAV_STAGE1_DOWNSAMPLER", "library")
    ds = _module(meta)
    with torch.no_grad():
        close(ds(a["x"]), a["y"], what="module, reference layout")
        close(ds(dc.planes_of(a["x"])), want[2], what="module, channels-last planes")
        x0 = a["x"][:, 0]
        close(ds.blocks[0](x0), a["after_block0"][:, 0], what="ConvNeXtBlock 0")
        close(ds.blocks[1](a["after_block0"][:, 1]), a["after_block1"][:, 1], what="ConvNeXtBlock 1")
    monkeypatch.delenv("AMAV_STAGE1_DOWNSAMPLER")
    with torch.no_grad():  # the default on a CPU tensor is the library path too: no device requirement
        assert torch.equal(ds(a["x"]), _module(meta)(a["x"]))


def test_state_dict_names_and_shapes_are_the_references():
    _, meta, _ = ref_fixture("stage1_downsampler")
    ds = _module(meta)
    assert {k: list(v.shape) for k, v in ds.state_dict().items()} == meta["params"]
    assert sorted(meta["params"]) == sorted(
        [f"blocks.{b}.{m}.{leaf}" for b in (0, 1) for m in ("dwconv", "norm", "pwconv1", "pwconv2")
         for leaf in ("weight", "bias")] + ["down.weight", "down.bias"])
    _, meta2, _ = ref_fixture("stage1_upsampled")
    assert all(("triplane_downsampler." + k) in meta2["params_encoder"] for k in meta["params"])


def test_gradients_reach_every_parameter_on_the_library_path():
    _, meta, _ = ref_fixture("stage1_downsampler")
    ds = _module(meta)
    x = dc.randn(3, 3, 6, 6, 64).requires_grad_(True)
    ds(x).square().sum().backward()
    assert all(p.grad is not None and bool(p.grad.any()) for p in ds.parameters()) and bool(x.grad.any())


def test_upsample_factor_below_two_is_refused():
    from audio_motion_avatar_amd import AmavError
    from audio_motion_avatar_amd.triplane_net import TriplaneDownsampler

    for factor in (1, 0):
        with pytest.raises(AmavError, match="upsample_factor"):
            TriplaneDownsampler(SimpleNamespace(triplane_feature_dim=64, upsample_factor=factor))
    assert TriplaneDownsampler(SimpleNamespace(triplane_feature_dim=64, upsample_factor=2)).scale == 2


def test_encoder_with_the_flag_constructs_on_the_cpu():
    from audio_motion_avatar_amd import AmavError
    from audio_motion_avatar_amd.config import Stage1Config
    from audio_motion_avatar_amd.smplx_decoder import SMPLXDecoder
    from audio_motion_avatar_amd.triplane_net import SMPLXTriplaneEncoder, TriplaneDownsampler

    cfg = Stage1Config(upsample_triplane=True, triplane_feature_dim=64, triplane_resolution=4, smplx_transformer_layers=1,
                       device="cpu")
    enc = SMPLXTriplaneEncoder(cfg, SMPLXDecoder(cfg))
    assert isinstance(enc.triplane_downsampler, TriplaneDownsampler)
    assert (enc.triplane_resolution, enc.cell_resolution) == (4, 12)
    names = [k for k in enc.state_dict() if k.startswith("triplane_downsampler.")]
    assert len(names) == 18 and "triplane_downsampler.blocks.1.pwconv2.bias" in names
    verts = torch.tensor([[[-1.4, -1.4, -1.4], [1.4, 1.4, 1.4], [0.0, 0.0, 0.0]]])
    assert enc.cell_indices(verts)[0].tolist() == [[0, 143, 6 + 12 * 6]] * 3          # cells of the 12 x 12 grid
    with pytest.raises(AmavError, match="upsample_factor"):
        SMPLXTriplaneEncoder(Stage1Config(upsample_triplane=True, upsample_factor=1, device="cpu"), None)
    flat = SMPLXTriplaneEncoder(Stage1Config(triplane_feature_dim=64, triplane_resolution=4, smplx_transformer_layers=1,
                                             device="cpu"), SMPLXDecoder(cfg))
    assert not hasattr(flat, "triplane_downsampler") and flat.cell_resolution == 4


def test_dwconv7_layernorm_entry_points_refuse_bad_arguments(lib):
    ok = (2, 9, 13, 64, FAKE, FAKE, FAKE, FAKE, FAKE, 1e-6, None, FAKE, None, 0, 0, None)
    bad = lambda i, v: ok[:i] + (v,) + ok[i + 1:]
    for args, msg in ((bad(3, 96), b"multiple of 64"), (bad(3, 576), b"multiple of 64"), (bad(3, 0), b"multiple of 64"),
                      (bad(0, 0), b"planes=0"), (bad(1, -1), b"height=-1"), (bad(4, None), b"NULL"), (bad(7, None), b"NULL"),
                      (bad(11, None), b"exactly one"), (bad(12, FAKE), b"exactly one"), (bad(11, FAKE + 4), b"aligned"),
                      (bad(9, -1.0), b"eps")):
        assert lib.amav_dwconv7_layernorm(*args) == ERR_INVALID and msg in lib.amav_last_error(), (args, lib.amav_last_error())
    split = ok[:11] + (None, FAKE, 7, 0, None)
    assert lib.amav_dwconv7_layernorm(*split) == ERR_INVALID and b"format" in lib.amav_last_error()
    assert lib.amav_dwconv7_layernorm_backward_workspace_bytes(2, 9, 13, 96) == 0
    assert lib.amav_dwconv7_layernorm_backward_workspace_bytes(0, 9, 13, 64) == 0
    need = lib.amav_dwconv7_layernorm_backward_workspace_bytes(2, 9, 13, 64)
    rows, tiles = 2 * 9 * 13, 2 * 2 * 2
    assert need >= 4 * 64 * (rows + 2 * ((rows + 15) // 16) + 50 * tiles)
    bwd = (2, 9, 13, 64) + (FAKE,) * 4 + (1e-6,) + (FAKE,) * 6
    assert lib.amav_dwconv7_layernorm_backward(*bwd, FAKE, need - 1, None) == ERR_WORKSPACE
    assert lib.amav_dwconv7_layernorm_backward(*bwd, None, need, None) == ERR_WORKSPACE
    assert lib.amav_dwconv7_layernorm_backward(*(bwd[:9] + (None,) + bwd[10:]), FAKE, need, None) == ERR_INVALID
    assert b"NULL" in lib.amav_last_error()
    assert lib.amav_dwconv7_layernorm_backward(*((2, 9, 13, 100) + bwd[4:]), FAKE, need, None) == ERR_INVALID


def test_gelu_and_patch_gather_entry_points_refuse_bad_arguments(lib):
    def refused(fn, args, message=None):
        assert fn(*args) == ERR_INVALID, args
        assert message is None or message in lib.amav_last_error(), (args, lib.amav_last_error())

    gelu, gelu_b = lib.amav_gelu_bias, lib.amav_gelu_bias_backward
    refused(gelu, (4, 6, FAKE, 8, None, FAKE, None, 0, 0, None), b"bad sizes")
    refused(gelu, (0, 8, FAKE, 8, None, FAKE, None, 0, 0, None))
    refused(gelu, (4, 12, FAKE, 12, None, None, FAKE, 0, 0, None))            # a split operand needs inner % 8
    refused(gelu, (4, 8, FAKE, 8, None, FAKE, FAKE, 0, 0, None), b"exactly one")
    refused(gelu, (4, 8, None, 8, None, FAKE, None, 0, 0, None))
    refused(gelu, (4, 8, FAKE, 6, None, FAKE, None, 0, 0, None), b"row stride")
    refused(gelu, (4, 8, FAKE, 8, None, None, FAKE, 1, 500, None), b"format")
    refused(gelu_b, (4, 8, FAKE, 8, None, None, FAKE, 8, None), b"NULL")
    refused(gelu_b, (4, 8, FAKE, 8, None, FAKE, FAKE, 4, None), b"row stride")
    refused(gelu_b, (4, 8, FAKE + 8, 8, None, FAKE, FAKE, 8, None), b"aligned")
    gather, gather_b = lib.amav_patch4_gather, lib.amav_patch4_gather_backward
    refused(gather, (3, 12, 12, 64, 1, FAKE, FAKE, None, 0, 0, None), b"stride")
    refused(gather, (3, 1, 12, 64, 3, FAKE, FAKE, None, 0, 0, None))
    refused(gather, (3, 12, 12, 6, 3, FAKE, FAKE, None, 0, 0, None))
    refused(gather, (3, 12, 12, 64, 3, None, FAKE, None, 0, 0, None))
    refused(gather, (3, 12, 12, 64, 3, FAKE, None, None, 0, 0, None), b"exactly one")
    refused(gather_b, (3, 12, 12, 64, 0, FAKE, FAKE, None))
    refused(gather_b, (3, 12, 12, 64, 3, None, FAKE, None), b"NULL")
    refused(gather_b, (0, 12, 12, 64, 3, FAKE, FAKE, None))


def test_wrappers_refuse_cpu_tensors():
    from audio_motion_avatar_amd import AmavError, ops

    x = torch.zeros(1, 5, 5, 64)
    with pytest.raises(AmavError, match="only runs on an MI355X"):
        ops.dwconv7_layernorm(x, torch.zeros(64, 1, 7, 7), *(torch.zeros(64),) * 3)
    with pytest.raises(AmavError, match="only runs on an MI355X"):
        ops.gelu_bias(torch.zeros(4, 8))
    with pytest.raises(AmavError, match="only runs on an MI355X"):
        ops.patch4_gather(x, 3)
    assert ops.patch4_out_size(12, 3) == 4 and ops.patch4_out_size(9, 2) == 4 and ops.patch4_out_size(13, 5) == 3
    assert ops.dwconv7_channels_ok(64) and ops.dwconv7_channels_ok(512) and not ops.dwconv7_channels_ok(32)
    assert not ops.dwconv7_channels_ok(96) and not ops.dwconv7_channels_ok(576)
