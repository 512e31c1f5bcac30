"""Host-side argument checks of the self-attention backward's C entry points (amav_selfattn_forward_lse,
amav_selfattn_backward): every call below is refused before a kernel is launched."""

from abi_support import FAKE, lib  # noqa: F401 (lib: fixture)


B, S, H, D = 2, 100, 8, 64


def _bwd(lib, **over):
    a = dict(B=B, S=S, H=H, D=D, q=FAKE, k=FAKE, v=FAKE, rs=3 * H * D, out=FAKE, out_rs=H * D, lse=FAKE, dout=FAKE,
             dout_rs=H * D, dqkv=FAKE, dqkv_rs=3 * H * D, scale=0.125, ws=FAKE, ws_bytes=1 << 40)
    a.update(over)
    return lib.amav_selfattn_backward(a["B"], a["S"], a["H"], a["D"], a["q"], a["k"], a["v"], a["rs"], a["out"],
                                      a["out_rs"], a["lse"], a["dout"], a["dout_rs"], a["dqkv"], a["dqkv_rs"],
                                      a["scale"], a["ws"], a["ws_bytes"], None)


def test_symbols_exist(lib):
    for name in ("amav_selfattn_forward_lse", "amav_selfattn_backward", "amav_selfattn_backward_workspace_bytes"):
        assert hasattr(lib, name), name


def test_workspace_bytes(lib):
    f = lib.amav_selfattn_backward_workspace_bytes
    for bad in ((0, S, H, D), (B, 0, H, D), (B, S, 0, D), (-1, S, H, D), (B, S, H, 32), (B, S, H, 128)):
        assert f(*bad) == 0, bad
    assert f(B, S, H, D) >= B * H * S * 4  # one fp32 delta per (batch, head, query)
    assert f(1, 6304, 8, 64) >= 8 * 6304 * 4


def test_backward_refusals(lib):
    assert _bwd(lib, ws_bytes=1 << 40, ws=FAKE, B=0) == -1 and b"bad sizes" in lib.amav_last_error()
    assert _bwd(lib, S=0) == -1 and b"bad sizes" in lib.amav_last_error()
    assert _bwd(lib, H=0) == -1 and b"bad sizes" in lib.amav_last_error()
    assert _bwd(lib, D=32) == -1 and b"head_dim" in lib.amav_last_error()
    for name in ("q", "k", "v", "out", "lse", "dout", "dqkv"):
        assert _bwd(lib, **{name: None}) == -1 and b"NULL" in lib.amav_last_error(), name
    for name in ("q", "k", "v", "out", "dout", "dqkv"):
        assert _bwd(lib, **{name: FAKE + 4}) == -1 and b"aligned" in lib.amav_last_error(), name
    assert _bwd(lib, lse=FAKE + 2) == -1 and b"aligned" in lib.amav_last_error()
    for name, low in (("rs", H * D - 4), ("out_rs", H * D - 4), ("dout_rs", H * D - 4), ("rs", 3 * H * D + 2),
                      ("out_rs", H * D + 1), ("dout_rs", H * D + 2)):
        assert _bwd(lib, **{name: low}) == -1 and b"row stride" in lib.amav_last_error(), name
    assert _bwd(lib, dqkv_rs=3 * H * D - 4) == -1 and b"dqkv row stride" in lib.amav_last_error()
    assert _bwd(lib, dqkv_rs=3 * H * D + 2) == -1 and b"dqkv row stride" in lib.amav_last_error()
    assert _bwd(lib, scale=float("inf")) == -1 and b"scale" in lib.amav_last_error()
    big = 70000 * D
    assert _bwd(lib, H=70000, rs=3 * big, out_rs=big, dout_rs=big, dqkv_rs=3 * big) == -1
    assert b"grid" in lib.amav_last_error()
    need = lib.amav_selfattn_backward_workspace_bytes(B, S, H, D)
    assert _bwd(lib, ws_bytes=need - 1) == -3 and b"workspace" in lib.amav_last_error()
    assert _bwd(lib, ws=None) == -3 and b"workspace" in lib.amav_last_error()


def test_forward_lse_refusals(lib):
    f = lib.amav_selfattn_forward_lse
    ok = dict(q=FAKE, k=FAKE, v=FAKE, out=FAKE, lse=FAKE)

    def call(**over):
        a = dict(ok, B=B, S=S, H=H, D=D, rs=3 * H * D, ws=FAKE, ws_bytes=1 << 40)
        a.update(over)
        return f(a["B"], a["S"], a["H"], a["D"], a["q"], a["k"], a["v"], a["rs"], a["out"], H * D, 0.125, a["lse"],
                 a["ws"], a["ws_bytes"], None)

    assert call(lse=None) == -1 and b"NULL lse" in lib.amav_last_error()
    assert call(q=None) == -1 and b"NULL" in lib.amav_last_error()
    assert call(D=32) == -1 and b"head_dim" in lib.amav_last_error()
    assert call(q=FAKE + 4) == -1 and b"aligned" in lib.amav_last_error()
    assert call(rs=H * D - 4) == -1 and b"row strides" in lib.amav_last_error()
    assert call(ws_bytes=16) == -3 and b"workspace" in lib.amav_last_error()
    for variant in ("f32", "bf16"):
        assert lib.amav_set_option(b"attn", variant.encode()) == 0
        try:
            assert call() == -1 and b"fp16 x 2 kernel only" in lib.amav_last_error()
        finally:
            assert lib.amav_set_option(b"attn", b"default") == 0
