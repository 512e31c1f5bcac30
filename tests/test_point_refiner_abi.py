"""Host-side argument checks of the point refiner's C entry points (csrc/cloud.hip): every call below is refused before
a kernel is launched, so none of the fake pointers is ever dereferenced.  Each case starts from arguments that are
valid except for the one it names."""

import pytest

from abi_support import FAKE, lib  # noqa: F401 (lib: fixture)


def _refused(lib, rc, *words):
    msg = lib.amav_last_error()
    assert rc == -1, (rc, msg)
    for w in words:
        assert w in msg, (w, msg)


def test_symbols_exist(lib):
    for name in ("amav_cloud_voxelize", "amav_cloud_codes", "amav_cloud_neighbors", "amav_subm_pair_gemm",
                 "amav_subm_pair_gemm_split", "amav_subm_pair_sum", "amav_patch_attention", "amav_cluster_max",
                 "amav_bn_gelu", "amav_unpool_merge", "amav_rows_norm"):
        assert hasattr(lib, name), name


def test_rows_norm_refusals(lib):
    ptrs = ("x", "base", "wa", "ba", "wb", "bb", "out_sum", "out_norm")

    def call(**over):
        a = dict(rows=100, C=256, eps=1e-5, **{p: FAKE for p in ptrs})
        a.update(over)
        return lib.amav_rows_norm(a["rows"], a["C"], a["x"], a["base"], a["wa"], a["ba"], a["wb"], a["bb"], a["eps"],
                                  a["out_sum"], a["out_norm"], None)

    for C in (48, 1024, 0, 16, 768):
        _refused(lib, call(C=C), b"amav_rows_norm", b"channels=%d" % C)
    for rows in (0, -1):
        _refused(lib, call(rows=rows), b"amav_rows_norm", b"rows=%d" % rows)
    _refused(lib, call(ba=None), b"amav_rows_norm", b"NULL")             # weight_a without bias_a
    _refused(lib, call(wa=None), b"amav_rows_norm", b"NULL")             # bias_a without weight_a
    for name in ("x", "base", "wb", "bb", "out_sum", "out_norm"):
        _refused(lib, call(**{name: None}), b"amav_rows_norm", b"NULL")
    for name in ptrs:
        _refused(lib, call(**{name: FAKE + 4}), b"amav_rows_norm", b"aligned")
    _refused(lib, call(wa=None, ba=None, x=FAKE + 4), b"amav_rows_norm", b"aligned")


def test_cluster_max_refusals(lib):
    def call(**over):
        a = dict(clusters=37, C=512, x=FAKE, members=FAKE, seg=FAKE, scale=FAKE, shift=FAKE, out=FAKE)
        a.update(over)
        return lib.amav_cluster_max(a["clusters"], a["C"], a["x"], a["members"], a["seg"], a["scale"], a["shift"],
                                    a["out"], None)

    for C in (6, 514, 0, -4):
        _refused(lib, call(C=C), b"amav_cluster_max", b"bad sizes")
    for clusters in (0, -1):
        _refused(lib, call(clusters=clusters), b"amav_cluster_max", b"bad sizes")
    for name in ("x", "members", "seg", "scale", "shift", "out"):
        _refused(lib, call(**{name: None}), b"amav_cluster_max", b"NULL")
    for name in ("x", "scale", "shift", "out"):
        _refused(lib, call(**{name: FAKE + 4}), b"amav_cluster_max", b"aligned")


def test_bn_gelu_refusals(lib):
    def call(**over):
        a = dict(rows=1001, C=36, x=FAKE, scale=FAKE, shift=FAKE, out=FAKE)
        a.update(over)
        return lib.amav_bn_gelu(a["rows"], a["C"], a["x"], a["scale"], a["shift"], a["out"], None)

    for C in (6, 38, 0, -4):
        _refused(lib, call(C=C), b"amav_bn_gelu", b"bad sizes")
    for rows in (0, -1):
        _refused(lib, call(rows=rows), b"amav_bn_gelu", b"bad sizes")
    for name in ("x", "scale", "shift", "out"):
        _refused(lib, call(**{name: None}), b"amav_bn_gelu", b"NULL")
        _refused(lib, call(**{name: FAKE + 4}), b"amav_bn_gelu", b"aligned")


def test_unpool_merge_refusals(lib):
    ptrs = ("x", "scale", "shift", "up", "cluster", "skip", "sum")

    def call(**over):
        a = dict(rows=1001, C=256, **{p: FAKE for p in ptrs})
        a.update(over)
        return lib.amav_unpool_merge(a["rows"], a["C"], a["x"], a["scale"], a["shift"], a["up"], a["cluster"], a["skip"],
                                     a["sum"], None)

    for C in (6, 258, 0, -4):
        _refused(lib, call(C=C), b"amav_unpool_merge", b"bad sizes")
    for rows in (0, -1):
        _refused(lib, call(rows=rows), b"amav_unpool_merge", b"bad sizes")
    for name in ptrs:
        _refused(lib, call(**{name: None}), b"amav_unpool_merge", b"NULL")
    for name in ("x", "scale", "shift", "up", "skip", "sum"):
        _refused(lib, call(**{name: FAKE + 4}), b"amav_unpool_merge", b"aligned")


def test_subm_pair_sum_refusals(lib):
    def call(**over):
        a = dict(n=500, taps=27, cout=64, products=FAKE, pair_of=FAKE, bias=FAKE, out=FAKE)
        a.update(over)
        return lib.amav_subm_pair_sum(a["n"], a["taps"], a["cout"], a["products"], a["pair_of"], a["bias"], a["out"],
                                      None)

    for cout in (6, 66, 0, -4):
        _refused(lib, call(cout=cout), b"amav_subm_pair_sum", b"bad sizes")
    _refused(lib, call(n=0), b"amav_subm_pair_sum", b"bad sizes")
    _refused(lib, call(taps=0), b"amav_subm_pair_sum", b"bad sizes")
    for name in ("products", "pair_of", "out"):
        _refused(lib, call(**{name: None}), b"amav_subm_pair_sum", b"NULL")
    for name in ("products", "bias", "out"):
        _refused(lib, call(**{name: FAKE + 4}), b"amav_subm_pair_sum", b"aligned")


def test_subm_pair_gemm_refusals(lib):
    def call(**over):
        a = dict(pairs=3000, tiles=40, taps=27, cin=64, cout=128, feat=FAKE, src=FAKE, tap_start=FAKE, tile_start=FAKE,
                 w=FAKE, products=FAKE)
        a.update(over)
        return lib.amav_subm_pair_gemm(a["pairs"], a["tiles"], a["taps"], a["cin"], a["cout"], a["feat"], a["src"],
                                       a["tap_start"], a["tile_start"], a["w"], a["products"], None)

    for cin in (48, 16, 0, -32):
        _refused(lib, call(cin=cin), b"amav_subm_pair_gemm", b"multiples of 32")
    for cout in (48, 100, 0, -32):
        _refused(lib, call(cout=cout), b"amav_subm_pair_gemm", b"multiples of 32")
    for pairs in (0, -1, 1 << 31):
        _refused(lib, call(pairs=pairs), b"amav_subm_pair_gemm", b"bad sizes")
    _refused(lib, call(tiles=0), b"amav_subm_pair_gemm", b"bad sizes")
    _refused(lib, call(taps=0), b"amav_subm_pair_gemm", b"bad sizes")
    for name in ("feat", "src", "tap_start", "tile_start", "w", "products"):
        _refused(lib, call(**{name: None}), b"amav_subm_pair_gemm", b"NULL")
    for name in ("feat", "w", "products"):
        _refused(lib, call(**{name: FAKE + 4}), b"amav_subm_pair_gemm", b"aligned")


def test_subm_pair_gemm_split_refusals(lib):
    def call(**over):
        a = dict(pairs=3000, tiles=40, taps=27, cin=64, cout=128, rows=500, feat=FAKE, src=FAKE, tap_start=FAKE,
                 tile_start=FAKE, ws=FAKE, scratch=FAKE, products=FAKE)
        a.update(over)
        return lib.amav_subm_pair_gemm_split(a["pairs"], a["tiles"], a["taps"], a["cin"], a["cout"], a["rows"],
                                             a["feat"], a["src"], a["tap_start"], a["tile_start"], a["ws"],
                                             a["scratch"], a["products"], None)

    for cin in (48, 16, 0):
        _refused(lib, call(cin=cin), b"amav_subm_pair_gemm_split", b"multiples of 32")
    for cout in (48, 100, 0):
        _refused(lib, call(cout=cout), b"amav_subm_pair_gemm_split", b"multiples of 32")
    for pairs in (0, -1, 1 << 31):
        _refused(lib, call(pairs=pairs), b"amav_subm_pair_gemm_split", b"bad sizes")
    _refused(lib, call(rows=0), b"amav_subm_pair_gemm_split", b"bad sizes")
    _refused(lib, call(tiles=0), b"amav_subm_pair_gemm_split", b"bad sizes")
    for name in ("feat", "src", "tap_start", "tile_start", "ws", "scratch", "products"):
        _refused(lib, call(**{name: None}), b"amav_subm_pair_gemm_split", b"NULL")
    for name in ("feat", "ws", "scratch", "products"):
        _refused(lib, call(**{name: FAKE + 4}), b"amav_subm_pair_gemm_split", b"aligned")


def test_patch_attention_refusals(lib):
    def call(**over):
        a = dict(patches=10, max_patch=512, heads=4, D=64, qkv=FAKE, order=FAKE, desc=FAKE, out=FAKE)
        a.update(over)
        return lib.amav_patch_attention(a["patches"], a["max_patch"], a["heads"], a["D"], a["qkv"], a["order"],
                                        a["desc"], a["out"], 0.125, None)

    for D in (128, 8, 48, 0):
        _refused(lib, call(D=D), b"amav_patch_attention", b"head_dim %d" % D)
    for patches in (0, -1, 65536):
        _refused(lib, call(patches=patches), b"amav_patch_attention", b"bad sizes")
    _refused(lib, call(heads=0), b"amav_patch_attention", b"bad sizes")
    _refused(lib, call(max_patch=0), b"amav_patch_attention", b"bad sizes")
    for name in ("qkv", "order", "desc", "out"):
        _refused(lib, call(**{name: None}), b"amav_patch_attention", b"NULL")
    for name in ("qkv", "desc", "out"):
        _refused(lib, call(**{name: FAKE + 4}), b"amav_patch_attention", b"aligned")


def test_serialisation_refusals(lib):
    def nbr(**over):
        a = dict(n=500, ksize=3)
        a.update(over)
        return lib.amav_cloud_neighbors(a["n"], a["ksize"], FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, None)

    for ksize in (4, 1, 7, 0):
        _refused(lib, nbr(ksize=ksize), b"amav_cloud_neighbors", b"ksize=%d" % ksize)
    _refused(lib, nbr(n=0), b"amav_cloud_neighbors", b"bad sizes")
    _refused(lib, lib.amav_cloud_neighbors(500, 3, FAKE, FAKE, FAKE, None, FAKE, FAKE, FAKE, None),
             b"amav_cloud_neighbors", b"NULL")

    def vox(**over):
        a = dict(n=500, clouds=2, res=100.0, points=FAKE)
        a.update(over)
        return lib.amav_cloud_voxelize(a["n"], a["clouds"], a["points"], FAKE, a["res"], FAKE, FAKE, FAKE, None)

    for clouds in (0, -1, 32768):
        _refused(lib, vox(clouds=clouds), b"amav_cloud_voxelize", b"clouds=%d" % clouds)
    _refused(lib, vox(n=0), b"amav_cloud_voxelize", b"bad sizes")
    for res in (0.0, -100.0, float("nan")):
        _refused(lib, vox(res=res), b"amav_cloud_voxelize", b"resolution")
    _refused(lib, vox(points=None), b"amav_cloud_voxelize", b"NULL")

    _refused(lib, lib.amav_cloud_codes(0, FAKE, FAKE, FAKE, FAKE, None), b"amav_cloud_codes", b"bad size")
    _refused(lib, lib.amav_cloud_codes(500, FAKE, None, FAKE, FAKE, None), b"amav_cloud_codes", b"NULL")


def test_rows_norm_refuses_two_eps():
    """The kernel takes one eps: a pair of LayerNorms with different eps is refused on the host, before any tensor is
    looked at (Block.forward then takes the library LayerNorm path)."""
    import torch

    from audio_motion_avatar_amd import AmavError, ops

    a, b = torch.nn.LayerNorm(64, eps=1e-3), torch.nn.LayerNorm(64)
    x = torch.zeros(8, 64)
    with pytest.raises(AmavError, match="eps"):
        ops.rows_norm(x, x, b, norm_a=a)
