"""Host-side argument checks of the point refiner's backward entry points (csrc/cloud_backward.hip, and
amav_patch_attention_lse in csrc/cloud.hip): every call below is refused before a kernel is launched, so none of the fake
pointers is ever dereferenced.  Each case starts from arguments that are valid except for the one it names."""
import os

import pytest

from abi_support import ERR_WORKSPACE, FAKE, lib  # noqa: F401 (lib: fixture)


def _refused(lib, rc, *words, code=-1):
    msg = lib.amav_last_error()
    assert rc == code, (rc, msg)
    for w in words:
        assert w in msg, (w, msg)


def test_symbols_exist(lib):
    for name in ("amav_patch_attention_lse", "amav_patch_attention_backward", "amav_patch_attention_backward_workspace_bytes",
                 "amav_subm_pair_sum_csr", "amav_subm_pair_wgrad", "amav_subm_pair_wgrad_workspace_bytes",
                 "amav_cluster_max_backward", "amav_cluster_sum"):
        assert hasattr(lib, name), name


def test_workspace_error_code_is_the_headers():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "amav.h")).read()
    import re

    m = re.search(r"AMAV_ERR_WORKSPACE\s*\(?(-?\d+)", text)
    assert m and int(m.group(1)) == ERR_WORKSPACE


def test_patch_attention_lse_refusals(lib):
    def call(**over):
        a = dict(patches=10, max_patch=512, heads=4, D=64, qkv=FAKE, order=FAKE, desc=FAKE, out=FAKE, lse=FAKE)
        a.update(over)
        return lib.amav_patch_attention_lse(a["patches"], a["max_patch"], a["heads"], a["D"], a["qkv"], a["order"],
                                            a["desc"], a["out"], a["lse"], 0.125, None)

    for D in (128, 8, 48, 0):
        _refused(lib, call(D=D), b"amav_patch_attention_lse", b"head_dim %d" % D)
    for patches in (0, -1, 65536):
        _refused(lib, call(patches=patches), b"amav_patch_attention_lse", b"bad sizes")
    _refused(lib, call(heads=0), b"amav_patch_attention_lse", b"bad sizes")
    _refused(lib, call(max_patch=0), b"amav_patch_attention_lse", b"bad sizes")
    for name in ("qkv", "order", "desc", "out", "lse"):
        _refused(lib, call(**{name: None}), b"amav_patch_attention_lse", b"NULL")
    for name in ("qkv", "desc", "out"):
        _refused(lib, call(**{name: FAKE + 4}), b"amav_patch_attention_lse", b"aligned")
    _refused(lib, call(lse=FAKE + 2), b"amav_patch_attention_lse", b"aligned")


def test_patch_attention_backward_refusals(lib):
    ptrs = ("qkv", "order", "desc", "out", "lse", "dout", "dqkv")
    need = lib.amav_patch_attention_backward_workspace_bytes(5000, 4, 64)
    assert need >= 5000 * 4 * 4 + 5000 * 2 * 256 * 4 and need % 256 == 0

    def call(**over):
        a = dict(n=5000, patches=10, max_patch=512, heads=4, D=64, scale=0.125, ws=FAKE, ws_bytes=need,
                 **{p: FAKE for p in ptrs})
        a.update(over)
        return lib.amav_patch_attention_backward(a["n"], a["patches"], a["max_patch"], a["heads"], a["D"], a["qkv"],
                                                 a["order"], a["desc"], a["out"], a["lse"], a["dout"], a["dqkv"],
                                                 a["scale"], a["ws"], a["ws_bytes"], None)

    for D in (128, 8, 48, 0):
        _refused(lib, call(D=D), b"amav_patch_attention_backward", b"head_dim %d" % D)
        assert lib.amav_patch_attention_backward_workspace_bytes(5000, 4, D) == 0
    for n in (0, -1, 1 << 31):
        _refused(lib, call(n=n), b"amav_patch_attention_backward", b"bad sizes")
    assert lib.amav_patch_attention_backward_workspace_bytes(0, 4, 64) == 0
    assert lib.amav_patch_attention_backward_workspace_bytes(5000, 0, 64) == 0
    for patches in (0, -1, 65536):
        _refused(lib, call(patches=patches), b"amav_patch_attention_backward", b"bad sizes")
    _refused(lib, call(heads=0), b"amav_patch_attention_backward", b"bad sizes")
    _refused(lib, call(max_patch=0), b"amav_patch_attention_backward", b"bad sizes")
    for name in ptrs:
        _refused(lib, call(**{name: None}), b"amav_patch_attention_backward", b"NULL")
    for name in ("qkv", "desc", "out", "dout", "dqkv", "ws"):
        _refused(lib, call(**{name: FAKE + 4}), b"amav_patch_attention_backward", b"aligned")
    for scale in (float("nan"), float("inf")):
        _refused(lib, call(scale=scale), b"amav_patch_attention_backward", b"scale")
    _refused(lib, call(ws_bytes=need - 1), b"amav_patch_attention_backward", b"workspace", code=ERR_WORKSPACE)
    _refused(lib, call(ws=None), b"amav_patch_attention_backward", b"workspace", code=ERR_WORKSPACE)


def test_subm_pair_sum_csr_refusals(lib):
    def call(**over):
        a = dict(n=500, C=64, products=FAKE, lo=0, count=3000, start=FAKE, pairs=FAKE, acc=0, out=FAKE)
        a.update(over)
        return lib.amav_subm_pair_sum_csr(a["n"], a["C"], a["products"], a["lo"], a["count"], a["start"], a["pairs"],
                                          a["acc"], a["out"], None)

    for C in (6, 66, 0, -4):
        _refused(lib, call(C=C), b"amav_subm_pair_sum_csr", b"bad sizes")
    for n in (0, -1, 1 << 31):
        _refused(lib, call(n=n), b"amav_subm_pair_sum_csr", b"bad sizes")
    _refused(lib, call(lo=-1), b"amav_subm_pair_sum_csr", b"bad sizes")
    _refused(lib, call(count=0), b"amav_subm_pair_sum_csr", b"bad sizes")
    _refused(lib, call(lo=1 << 30, count=1 << 30), b"amav_subm_pair_sum_csr", b"bad sizes")
    for name in ("products", "start", "pairs", "out"):
        _refused(lib, call(**{name: None}), b"amav_subm_pair_sum_csr", b"NULL")
    for name in ("products", "out"):
        _refused(lib, call(**{name: FAKE + 4}), b"amav_subm_pair_sum_csr", b"aligned")


def test_subm_pair_wgrad_refusals(lib):
    ptrs = ("feat", "g", "src", "dst", "tap_start", "slice_start", "dw")
    need = lib.amav_subm_pair_wgrad_workspace_bytes(40, 64, 128)
    assert need == 40 * 64 * 128 * 4

    def call(**over):
        a = dict(pairs=3000, slices=40, chunk=128, taps=27, cin=64, cout=128, ws=FAKE, ws_bytes=need,
                 **{p: FAKE for p in ptrs})
        a.update(over)
        return lib.amav_subm_pair_wgrad(a["pairs"], a["slices"], a["chunk"], a["taps"], a["cin"], a["cout"], a["feat"],
                                        a["g"], a["src"], a["dst"], a["tap_start"], a["slice_start"], a["dw"], a["ws"],
                                        a["ws_bytes"], None)

    for cin in (48, 16, 0, -32):
        _refused(lib, call(cin=cin), b"amav_subm_pair_wgrad", b"multiples of 32")
        assert lib.amav_subm_pair_wgrad_workspace_bytes(40, cin, 128) == 0
    for cout in (48, 100, 0, -32):
        _refused(lib, call(cout=cout), b"amav_subm_pair_wgrad", b"multiples of 32")
        assert lib.amav_subm_pair_wgrad_workspace_bytes(40, 64, cout) == 0
    for pairs in (0, -1, 1 << 31):
        _refused(lib, call(pairs=pairs), b"amav_subm_pair_wgrad", b"bad sizes")
    _refused(lib, call(slices=0), b"amav_subm_pair_wgrad", b"bad sizes")
    assert lib.amav_subm_pair_wgrad_workspace_bytes(0, 64, 128) == 0
    _refused(lib, call(taps=0), b"amav_subm_pair_wgrad", b"bad sizes")
    for chunk in (0, -128, 64, 100, 130):
        _refused(lib, call(chunk=chunk), b"amav_subm_pair_wgrad", b"chunk=%d" % chunk)
    for name in ptrs:
        _refused(lib, call(**{name: None}), b"amav_subm_pair_wgrad", b"NULL")
    for name in ("feat", "g", "dw", "ws"):
        _refused(lib, call(**{name: FAKE + 4}), b"amav_subm_pair_wgrad", b"aligned")
    _refused(lib, call(ws_bytes=need - 1), b"amav_subm_pair_wgrad", b"workspace", code=ERR_WORKSPACE)
    _refused(lib, call(ws=None), b"amav_subm_pair_wgrad", b"workspace", code=ERR_WORKSPACE)


def test_cluster_max_backward_refusals(lib):
    ptrs = ("x", "members", "seg", "scale", "shift", "dout", "dx", "dz", "xmax")

    def call(**over):
        a = dict(clusters=37, C=512, **{p: FAKE for p in ptrs})
        a.update(over)
        return lib.amav_cluster_max_backward(a["clusters"], a["C"], a["x"], a["members"], a["seg"], a["scale"], a["shift"],
                                             a["dout"], a["dx"], a["dz"], a["xmax"], None)

    for C in (6, 514, 0, -4):
        _refused(lib, call(C=C), b"amav_cluster_max_backward", b"bad sizes")
    for clusters in (0, -1):
        _refused(lib, call(clusters=clusters), b"amav_cluster_max_backward", b"bad sizes")
    for name in ptrs:
        _refused(lib, call(**{name: None}), b"amav_cluster_max_backward", b"NULL")
    for name in ("x", "scale", "shift", "dout", "dx", "dz", "xmax"):
        _refused(lib, call(**{name: FAKE + 4}), b"amav_cluster_max_backward", b"aligned")


def test_cluster_sum_refusals(lib):
    def call(**over):
        a = dict(clusters=37, C=260, x=FAKE, members=FAKE, seg=FAKE, out=FAKE)
        a.update(over)
        return lib.amav_cluster_sum(a["clusters"], a["C"], a["x"], a["members"], a["seg"], a["out"], None)

    for C in (6, 514, 0, -4):
        _refused(lib, call(C=C), b"amav_cluster_sum", b"bad sizes")
    for clusters in (0, -1):
        _refused(lib, call(clusters=clusters), b"amav_cluster_sum", b"bad sizes")
    for name in ("x", "members", "seg", "out"):
        _refused(lib, call(**{name: None}), b"amav_cluster_sum", b"NULL")
    for name in ("x", "out"):
        _refused(lib, call(**{name: FAKE + 4}), b"amav_cluster_sum", b"aligned")


def test_differentiable_ops_refuse_cpu_tensors():
    """The autograd entry points check for HIP tensors like every other wrapper: nothing runs on the CPU."""
    import torch

    from audio_motion_avatar_amd import AmavError, ops

    x = torch.zeros(8, 96)
    idx = torch.zeros(8, dtype=torch.int64)
    with pytest.raises(AmavError, match="HIP"):
        ops.patch_attention_differentiable(x, idx, torch.zeros(1, 4, dtype=torch.int32), 2, 8)
    with pytest.raises(AmavError, match="HIP"):
        ops.cluster_max_differentiable(x, idx, torch.tensor([0, 8]), torch.ones(96), torch.zeros(96))
    with pytest.raises(AmavError, match="HIP"):
        ops.cluster_sum(x, idx, torch.tensor([0, 8]))
