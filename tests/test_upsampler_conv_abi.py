"""Host-side argument checks of the triplane upsampler's 3x3 cell convolution (csrc/upsample_conv.hip): every call below
is refused before a kernel is launched, so none of the fake pointers is ever dereferenced.  Each case starts from
arguments that are valid except for the one it names."""
import ctypes

from abi_support import ERR_INVALID, ERR_WORKSPACE, FAKE, lib  # noqa: F401 (lib: fixture)

POINTERS = ("x_dev", "weights_split_dev", "in_scale_dev", "in_shift_dev", "origin_dev", "bias_dev", "residual_dev",
            "out_dev", "workspace_dev")


def _args(lib, **over):
    from audio_motion_avatar_amd import _lib

    a = _lib.Conv3x3Args()
    values = dict(cells=3, height=6, width=8, cin=64, cout=96, upsample_input=0, relu_out=0, extent=64,
                  weights_split_bytes=lib.amav_conv3x3_weights_split_bytes(64, 96),
                  workspace_bytes=lib.amav_conv3x3_workspace_bytes(), **{p: FAKE for p in POINTERS})
    values.update(over)
    for k, v in values.items():
        setattr(a, k, v)
    return a


def _refused(lib, rc, code, *words):
    msg = lib.amav_last_error()
    assert rc == code, (rc, msg)
    for w in (b"amav_conv3x3_cells",) + words:
        assert w in msg, (w, msg)


def test_struct_layout_and_symbols(lib):
    from audio_motion_avatar_amd import _lib

    S = _lib.Conv3x3Args
    assert S is _lib.STRUCTS["amav_conv3x3_args"]
    want = [("cells", 0, 8), ("height", 8, 4), ("width", 12, 4), ("cin", 16, 4), ("cout", 20, 4), ("upsample_input", 24, 4),
            ("relu_out", 28, 4), ("extent", 32, 4), ("x_dev", 40, 8), ("weights_split_dev", 48, 8),
            ("weights_split_bytes", 56, 8), ("in_scale_dev", 64, 8), ("in_shift_dev", 72, 8), ("origin_dev", 80, 8),
            ("bias_dev", 88, 8), ("residual_dev", 96, 8), ("out_dev", 104, 8), ("workspace_dev", 112, 8),
            ("workspace_bytes", 120, 8)]
    assert [(f, getattr(S, f).offset, getattr(S, f).size) for f, _ in S._fields_] == want
    assert ctypes.sizeof(S) == 128
    for name in ("amav_conv3x3_weights_split_bytes", "amav_conv3x3_workspace_bytes", "amav_conv3x3_prepare_weights_split",
                 "amav_conv3x3_cells"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name


def test_weights_split_bytes(lib):
    # 256-byte header + 9 taps x 64 x 96 weights x 2 parts x 2 bytes
    assert lib.amav_conv3x3_weights_split_bytes(64, 96) == 256 + 9 * 64 * 96 * 2 * 2 == 221440
    for cin, cout in ((48, 96), (64, 40), (0, 32), (32, 0), (-32, 32), (32, -64)):
        assert lib.amav_conv3x3_weights_split_bytes(cin, cout) == 0, (cin, cout)
    assert lib.amav_conv3x3_workspace_bytes() >= 16


def test_prepare_weights_refusals(lib):
    need = lib.amav_conv3x3_weights_split_bytes(64, 96)

    def call(cin=64, cout=96, w=FAKE, scale=None, out=FAKE, nbytes=need):
        return lib.amav_conv3x3_prepare_weights_split(cin, cout, w, scale, out, nbytes, None)

    for over in (dict(cin=48), dict(cout=40), dict(cin=0), dict(cout=-32)):
        assert call(**over) == ERR_INVALID and b"multiples of 32" in lib.amav_last_error()
    for over in (dict(w=None), dict(out=None), dict(out=FAKE + 16)):
        assert call(**over) == ERR_INVALID and b"NULL / misaligned" in lib.amav_last_error()
    assert call(nbytes=need - 1) == ERR_WORKSPACE and b"required %d" % need in lib.amav_last_error()


def test_cells_refusals(lib):
    def call(**over):
        return lib.amav_conv3x3_cells(ctypes.byref(_args(lib, **over)), None)

    assert lib.amav_conv3x3_cells(None, None) == ERR_INVALID and b"args is NULL" in lib.amav_last_error()
    for name in ("x_dev", "weights_split_dev", "out_dev"):                       # null required pointers
        _refused(lib, call(**{name: None}), ERR_INVALID, b"NULL")
    for over in (dict(cells=0), dict(cells=-2), dict(height=0), dict(width=-1)):  # non-positive sizes
        _refused(lib, call(**over), ERR_INVALID, b"bad sizes")
    for over in (dict(cin=48), dict(cin=0), dict(cout=80), dict(cout=-32)):       # channels
        _refused(lib, call(**over), ERR_INVALID, b"multiples of 32")
    for over in (dict(height=7), dict(width=9), dict(height=5, width=5)):         # odd sizes with upsample_input
        _refused(lib, call(upsample_input=1, **over), ERR_INVALID, b"even")
    _refused(lib, call(in_shift_dev=None), ERR_INVALID, b"come together")         # in_scale without in_shift
    _refused(lib, call(in_scale_dev=None), ERR_INVALID, b"come together")
    _refused(lib, call(extent=0), ERR_INVALID, b"extent")
    for name in ("x_dev", "in_scale_dev", "in_shift_dev", "weights_split_dev"):
        _refused(lib, call(**{name: FAKE + 4}), ERR_INVALID, b"aligned")
    need = lib.amav_conv3x3_workspace_bytes()                                     # workspace too small
    _refused(lib, call(workspace_bytes=need - 1), ERR_WORKSPACE, b"workspace")
    _refused(lib, call(workspace_bytes=0), ERR_WORKSPACE, b"workspace")
    _refused(lib, call(workspace_dev=None), ERR_WORKSPACE, b"workspace")
    _refused(lib, call(weights_split_bytes=lib.amav_conv3x3_weights_split_bytes(64, 96) - 1), ERR_WORKSPACE,
             b"weights_split")
    # the optional pointers may all be absent: then the first thing refused is something else
    _refused(lib, call(in_scale_dev=None, in_shift_dev=None, origin_dev=None, bias_dev=None, residual_dev=None, cells=0),
             ERR_INVALID, b"bad sizes")
