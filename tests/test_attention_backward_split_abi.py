"""Host side of the attention backward on fp16 x 2 split products (amav_selfattn_backward_split,
amav_crossattn_backward_split): the header, the generated binding and the library agree, the size queries run on the
host alone, and every call below is refused before a kernel is launched."""
import ctypes

from abi_support import ERR_INVALID, ERR_WORKSPACE, FAKE, lib  # noqa: F401 (lib: fixture)

B, S, SQ, SK, H, D = 2, 100, 100, 130, 8, 64
HD = H * D
PAIRS = {"amav_selfattn_backward_split": "amav_selfattn_backward",
         "amav_selfattn_backward_split_workspace_bytes": "amav_selfattn_backward_workspace_bytes",
         "amav_crossattn_backward_split": "amav_crossattn_backward",
         "amav_crossattn_backward_split_workspace_bytes": "amav_crossattn_backward_workspace_bytes"}


def _self(lib, **over):
    a = dict(B=B, S=S, H=H, D=D, q=FAKE, k=FAKE, v=FAKE, rs=3 * HD, out=FAKE, out_rs=HD, lse=FAKE, dout=FAKE,
             dout_rs=HD, dqkv=FAKE, dqkv_rs=3 * HD, scale=0.125, ws=FAKE, ws_bytes=1 << 40)
    a.update(over)
    return lib.amav_selfattn_backward_split(a["B"], a["S"], a["H"], a["D"], a["q"], a["k"], a["v"], a["rs"], a["out"],
                                            a["out_rs"], a["lse"], a["dout"], a["dout_rs"], a["dqkv"], a["dqkv_rs"],
                                            a["scale"], a["ws"], a["ws_bytes"], None)


def _cross(lib, **over):
    a = dict(B=B, Sq=SQ, Sk=SK, H=H, D=D, q=FAKE, q_rs=HD, k=FAKE, v=FAKE, kv_rs=2 * HD, out=FAKE, out_rs=HD, lse=FAKE,
             dout=FAKE, dout_rs=HD, dq=FAKE, dq_rs=HD, dkv=FAKE, dkv_rs=2 * HD, scale=0.125, ws=FAKE, ws_bytes=1 << 40)
    a.update(over)
    return lib.amav_crossattn_backward_split(a["B"], a["Sq"], a["Sk"], a["H"], a["D"], a["q"], a["q_rs"], a["k"], a["v"],
                                             a["kv_rs"], a["out"], a["out_rs"], a["lse"], a["dout"], a["dout_rs"],
                                             a["dq"], a["dq_rs"], a["dkv"], a["dkv_rs"], a["scale"], a["ws"],
                                             a["ws_bytes"], None)


def _refused(lib, rc, code, *texts):
    return rc == code and all(t in lib.amav_last_error() for t in texts)


def test_symbols_are_declared_exported_and_bound(lib):
    from audio_motion_avatar_amd import _lib

    for name, exact in PAIRS.items():
        assert name in _lib.SIGNATURES, name      # declared in include/amav.h
        assert hasattr(lib, name), name           # exported by the library
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1], name
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[exact], name   # the arguments of the exact-fp32 entry point
    assert lib.amav_selfattn_backward_split_workspace_bytes.restype is ctypes.c_size_t


def test_size_queries(lib):
    f, g = lib.amav_selfattn_backward_split_workspace_bytes, lib.amav_crossattn_backward_split_workspace_bytes
    for bad in ((0, S, H, D), (B, 0, H, D), (B, S, 0, D), (-1, S, H, D), (B, S, H, 32), (B, S, H, 128)):
        assert f(*bad) == 0 and g(*bad) == 0, bad
    # one fp32 delta per (batch, head, query) and the header of the operand scales on top
    assert f(B, S, H, D) >= B * H * S * 4 + 6 * 4 and g(B, SQ, H, D) >= B * H * SQ * 4 + 6 * 4
    assert f(B, S, H, D) > lib.amav_selfattn_backward_workspace_bytes(B, S, H, D)
    assert g(B, SQ, H, D) > lib.amav_crossattn_backward_workspace_bytes(B, SQ, H, D)
    assert f(1, 6304, 8, 64) >= 8 * 6304 * 4 + 6 * 4


def test_selfattn_refusals(lib):
    name = b"amav_selfattn_backward_split"
    for size in ("B", "S", "H"):
        assert _refused(lib, _self(lib, **{size: 0}), ERR_INVALID, name, b"bad sizes"), size
    for dim in (16, 32, 128):
        assert _refused(lib, _self(lib, D=dim), ERR_INVALID, name, b"head_dim"), dim
    for arg in ("q", "k", "v", "out", "lse", "dout", "dqkv"):
        assert _refused(lib, _self(lib, **{arg: None}), ERR_INVALID, name, b"NULL"), arg
    for arg in ("q", "k", "v", "out", "dout", "dqkv"):
        assert _refused(lib, _self(lib, **{arg: FAKE + 4}), ERR_INVALID, name, b"aligned"), arg
    assert _refused(lib, _self(lib, lse=FAKE + 2), ERR_INVALID, name, b"aligned")
    for arg, stride in (("rs", HD - 4), ("out_rs", HD - 4), ("dout_rs", HD - 4), ("rs", 3 * HD + 2), ("out_rs", HD + 1),
                        ("dout_rs", HD + 2)):
        assert _refused(lib, _self(lib, **{arg: stride}), ERR_INVALID, name, b"row stride"), (arg, stride)
    for stride in (3 * HD - 4, 3 * HD + 2):
        assert _refused(lib, _self(lib, dqkv_rs=stride), ERR_INVALID, name, b"dqkv row stride"), stride
    for scale in (float("inf"), float("-inf"), float("nan")):
        assert _refused(lib, _self(lib, scale=scale), ERR_INVALID, name, b"scale"), scale
    big = 70000 * D
    assert _refused(lib, _self(lib, H=70000, rs=3 * big, out_rs=big, dout_rs=big, dqkv_rs=3 * big), ERR_INVALID, b"grid")
    need = lib.amav_selfattn_backward_split_workspace_bytes(B, S, H, D)
    assert _refused(lib, _self(lib, ws_bytes=need - 1), ERR_WORKSPACE, name, b"workspace")
    # the exact-fp32 backward's workspace (delta alone) is too small: the header has to fit as well
    assert _refused(lib, _self(lib, ws_bytes=lib.amav_selfattn_backward_workspace_bytes(B, S, H, D)), ERR_WORKSPACE,
                    b"workspace")
    assert _refused(lib, _self(lib, ws=None), ERR_WORKSPACE, name, b"workspace")


def test_crossattn_refusals(lib):
    name = b"amav_crossattn_backward_split"
    for size in ("B", "Sq", "Sk", "H"):
        assert _refused(lib, _cross(lib, **{size: 0}), ERR_INVALID, name, b"bad sizes"), size
    for dim in (16, 32, 128):
        assert _refused(lib, _cross(lib, D=dim), ERR_INVALID, name, b"head_dim"), dim
    for arg in ("q", "k", "v", "out", "lse", "dout", "dq", "dkv"):
        assert _refused(lib, _cross(lib, **{arg: None}), ERR_INVALID, name, b"NULL"), arg
    for arg in ("q", "k", "v", "out", "dout", "dq", "dkv"):
        assert _refused(lib, _cross(lib, **{arg: FAKE + 4}), ERR_INVALID, name, b"aligned"), arg
    assert _refused(lib, _cross(lib, lse=FAKE + 2), ERR_INVALID, name, b"aligned")
    for arg in ("q_rs", "kv_rs", "out_rs", "dout_rs", "dq_rs"):
        for stride in (HD - 4, 2 * HD + 2):
            assert _refused(lib, _cross(lib, **{arg: stride}), ERR_INVALID, name, b"row strides"), (arg, stride)
    for stride in (2 * HD - 4, 2 * HD + 2):
        assert _refused(lib, _cross(lib, dkv_rs=stride), ERR_INVALID, name, b"dkv row stride"), stride
    for scale in (float("inf"), float("nan")):
        assert _refused(lib, _cross(lib, scale=scale), ERR_INVALID, name, b"scale"), scale
    big = 70000 * D
    assert _refused(lib, _cross(lib, H=70000, q_rs=big, kv_rs=2 * big, out_rs=big, dout_rs=big, dq_rs=big,
                                dkv_rs=2 * big), ERR_INVALID, b"grid")
    need = lib.amav_crossattn_backward_split_workspace_bytes(B, SQ, H, D)
    assert _refused(lib, _cross(lib, ws_bytes=need - 1), ERR_WORKSPACE, name, b"workspace")
    assert _refused(lib, _cross(lib, ws=None), ERR_WORKSPACE, name, b"workspace")


def test_python_switch_refuses_unknown_arithmetics(monkeypatch):
    """ops._attn_backward_split: "f32" | "split", None follows AMAV_ATTN_BACKWARD per call (default f32)."""
    import pytest

    from audio_motion_avatar_amd import ops
    from audio_motion_avatar_amd._lib import AmavError

    monkeypatch.delenv("AMAV_ATTN_BACKWARD", raising=False)
    assert ops._attn_backward_split(None) is False and ops._attn_backward_split("f32") is False
    assert ops._attn_backward_split("split") is True
    monkeypatch.setenv("AMAV_ATTN_BACKWARD", "split")
    assert ops._attn_backward_split(None) is True and ops._attn_backward_split("f32") is False
    monkeypatch.setenv("AMAV_ATTN_BACKWARD", "f32")
    assert ops._attn_backward_split(None) is False and ops._attn_backward_split("split") is True
    for bad in ("", "fp16", "SPLIT", "1"):
        monkeypatch.setenv("AMAV_ATTN_BACKWARD", bad)
        with pytest.raises(AmavError, match="AMAV_ATTN_BACKWARD"):
            ops._attn_backward_split(None)
        with pytest.raises(AmavError, match="arithmetic"):
            ops._attn_backward_split(bad)
