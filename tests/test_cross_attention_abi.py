"""Host-side argument checks of the cross-attention C entry points (amav_crossattn_*): every call below is refused
before a kernel is launched, and the size queries run on the host alone."""
from abi_support import ERR_INVALID, ERR_WORKSPACE, FAKE, lib  # noqa: F401 (lib: fixture)

B, SQ, SK, H, D = 2, 100, 130, 8, 64
HD = H * D
SYMBOLS = ("amav_crossattn_workspace_bytes", "amav_crossattn_key_split", "amav_crossattn_forward",
           "amav_crossattn_backward_workspace_bytes", "amav_crossattn_backward")


def _fwd(lib, **over):
    a = dict(B=B, Sq=SQ, Sk=SK, H=H, D=D, q=FAKE, q_rs=HD, k=FAKE, v=FAKE, kv_rs=2 * HD, out=FAKE, out_rs=HD, scale=0.125,
             lse=FAKE, ws=FAKE, ws_bytes=1 << 40)
    a.update(over)
    return lib.amav_crossattn_forward(a["B"], a["Sq"], a["Sk"], a["H"], a["D"], a["q"], a["q_rs"], a["k"], a["v"],
                                      a["kv_rs"], a["out"], a["out_rs"], a["scale"], a["lse"], a["ws"], a["ws_bytes"], None)


def _bwd(lib, **over):
    a = dict(B=B, Sq=SQ, Sk=SK, H=H, D=D, q=FAKE, q_rs=HD, k=FAKE, v=FAKE, kv_rs=2 * HD, out=FAKE, out_rs=HD, lse=FAKE,
             dout=FAKE, dout_rs=HD, dq=FAKE, dq_rs=HD, dkv=FAKE, dkv_rs=2 * HD, scale=0.125, ws=FAKE, ws_bytes=1 << 40)
    a.update(over)
    return lib.amav_crossattn_backward(a["B"], a["Sq"], a["Sk"], a["H"], a["D"], a["q"], a["q_rs"], a["k"], a["v"],
                                       a["kv_rs"], a["out"], a["out_rs"], a["lse"], a["dout"], a["dout_rs"], a["dq"],
                                       a["dq_rs"], a["dkv"], a["dkv_rs"], a["scale"], a["ws"], a["ws_bytes"], None)


def _refused(lib, rc, code, text):
    return rc == code and text in lib.amav_last_error()


def test_symbols_are_exported_and_bound(lib):
    from audio_motion_avatar_amd import _lib

    for name in SYMBOLS:
        assert name in _lib.SIGNATURES, name      # declared in include/amav.h
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1], name


def test_size_queries(lib):
    fwd, bwd, split = (lib.amav_crossattn_workspace_bytes, lib.amav_crossattn_backward_workspace_bytes,
                       lib.amav_crossattn_key_split)
    for bad in ((0, SQ, SK, H, D), (B, 0, SK, H, D), (B, SQ, 0, H, D), (B, SQ, SK, 0, D), (-1, SQ, SK, H, D),
                (B, SQ, SK, H, 32), (B, SQ, SK, H, 128)):
        assert fwd(*bad) == 0, bad
    for bad in ((0, SQ, H, D), (B, 0, H, D), (B, SQ, 0, D), (B, -3, H, D), (B, SQ, H, 32), (B, SQ, H, 128)):
        assert bwd(*bad) == 0, bad
    for bad in ((0, SQ, SK, H), (B, 0, SK, H), (B, SQ, 0, H), (B, SQ, SK, 0)):
        assert split(*bad) == 0, bad
    # the split K and V^T operands: two fp16 parts of [B, H, Sk (padded to 64 for V^T), 64]
    assert fwd(B, SQ, SK, H, D) >= 2 * 2 * B * H * D * (SK + 192)
    assert bwd(B, SQ, H, D) >= B * H * SQ * 4     # one fp32 delta per (batch, head, query)
    # plus the partial states of a split key sweep: 66 floats per (slice, batch, head, query)
    assert fwd(1, 5, 1030, 1, D) >= 2 * 5 * 66 * 4 + 2 * 2 * D * (1030 + 1088)


def test_key_split(lib):
    split = lib.amav_crossattn_key_split
    assert split(1, 128, 64, 1) == 1      # one key tile
    # one block of queries, 17 key tiles: two slices halve the sweep, three would leave fewer than 8 tiles per slice
    assert split(1, 5, 1030, 1) == 2
    assert split(1, 1030, 5, 1) == 1      # the roles are not swapped: one key tile, nine query blocks


def test_forward_refusals(lib):
    for size in ("B", "Sq", "Sk", "H"):
        assert _refused(lib, _fwd(lib, **{size: 0}), ERR_INVALID, b"bad sizes"), size
    assert _refused(lib, _fwd(lib, D=32), ERR_INVALID, b"head_dim")
    for name in ("q", "k", "v", "out"):
        assert _refused(lib, _fwd(lib, **{name: None}), ERR_INVALID, b"NULL"), name
        assert _refused(lib, _fwd(lib, **{name: FAKE + 4}), ERR_INVALID, b"aligned"), name
    assert _refused(lib, _fwd(lib, lse=FAKE + 2), ERR_INVALID, b"aligned")
    for name, stride in (("q_rs", HD - 4), ("kv_rs", HD - 4), ("out_rs", HD - 4), ("q_rs", HD + 2), ("kv_rs", 2 * HD + 1),
                         ("out_rs", HD + 2)):
        assert _refused(lib, _fwd(lib, **{name: stride}), ERR_INVALID, b"row strides"), (name, stride)
    for scale in (float("inf"), float("nan")):
        assert _refused(lib, _fwd(lib, scale=scale), ERR_INVALID, b"scale")
    big = 70000 * D
    assert _refused(lib, _fwd(lib, H=70000, q_rs=big, kv_rs=2 * big, out_rs=big), ERR_INVALID, b"grid")
    assert _refused(lib, _fwd(lib, B=70000), ERR_INVALID, b"grid")
    need = lib.amav_crossattn_workspace_bytes(B, SQ, SK, H, D)
    assert _refused(lib, _fwd(lib, ws_bytes=need - 1), ERR_WORKSPACE, b"workspace")
    assert _refused(lib, _fwd(lib, ws=None), ERR_WORKSPACE, b"workspace")
    assert _refused(lib, _fwd(lib, lse=None, ws_bytes=need - 1), ERR_WORKSPACE, b"workspace")   # lse is optional


def test_forward_ignores_the_attn_option(lib):
    """The cross entry point always runs fp16 x 2: under attn = bf16 | f32 it is refused for its workspace, as under
    the default, and not for the variant (amav_selfattn_forward_lse is)."""
    for variant in ("f32", "bf16"):
        assert lib.amav_set_option(b"attn", variant.encode()) == 0
        try:
            assert lib.amav_crossattn_workspace_bytes(B, SQ, SK, H, D) > 0
            assert _refused(lib, _fwd(lib, ws_bytes=16), ERR_WORKSPACE, b"workspace")
        finally:
            assert lib.amav_set_option(b"attn", b"default") == 0
    default = lib.amav_crossattn_workspace_bytes(B, SQ, SK, H, D)
    assert lib.amav_set_option(b"attn", b"f32") == 0
    try:
        assert lib.amav_crossattn_workspace_bytes(B, SQ, SK, H, D) == default
    finally:
        assert lib.amav_set_option(b"attn", b"default") == 0


def test_backward_refusals(lib):
    for size in ("B", "Sq", "Sk", "H"):
        assert _refused(lib, _bwd(lib, **{size: 0}), ERR_INVALID, b"bad sizes"), size
    assert _refused(lib, _bwd(lib, D=32), ERR_INVALID, b"head_dim")
    for name in ("q", "k", "v", "out", "lse", "dout", "dq", "dkv"):
        assert _refused(lib, _bwd(lib, **{name: None}), ERR_INVALID, b"NULL"), name
    for name in ("q", "k", "v", "out", "dout", "dq", "dkv"):
        assert _refused(lib, _bwd(lib, **{name: FAKE + 4}), ERR_INVALID, b"aligned"), name
    assert _refused(lib, _bwd(lib, lse=FAKE + 2), ERR_INVALID, b"aligned")
    for name in ("q_rs", "kv_rs", "out_rs", "dout_rs", "dq_rs"):
        for stride in (HD - 4, 2 * HD + 2):
            assert _refused(lib, _bwd(lib, **{name: stride}), ERR_INVALID, b"row strides"), (name, stride)
    for stride in (2 * HD - 4, 2 * HD + 2):
        assert _refused(lib, _bwd(lib, dkv_rs=stride), ERR_INVALID, b"dkv row stride"), stride
    assert _refused(lib, _bwd(lib, scale=float("inf")), ERR_INVALID, b"scale")
    big = 70000 * D
    assert _refused(lib, _bwd(lib, H=70000, q_rs=big, kv_rs=2 * big, out_rs=big, dout_rs=big, dq_rs=big, dkv_rs=2 * big),
                    ERR_INVALID, b"grid")
    need = lib.amav_crossattn_backward_workspace_bytes(B, SQ, H, D)
    assert _refused(lib, _bwd(lib, ws_bytes=need - 1), ERR_WORKSPACE, b"workspace")
    assert _refused(lib, _bwd(lib, ws=None), ERR_WORKSPACE, b"workspace")
