"""Host-side argument checks of the 3x3 cell convolution's backward (csrc/upsample_conv.hip,
amav_conv3x3_cells_backward and its companions): every call below is refused before a kernel is launched, so none of the
fake pointers is ever dereferenced, and every workspace query on rejected arguments returns 0.  Each case starts from
arguments that are valid except for the one it names."""
import ctypes

from abi_support import ERR_INVALID, ERR_WORKSPACE, FAKE, lib  # noqa: F401 (lib: fixture)

POINTERS = ("x_dev", "weights_split_t_dev", "in_scale_dev", "in_shift_dev", "origin_dev", "out_dev", "grad_out_dev",
            "grad_x_dev", "grad_weight_dev", "grad_bias_dev", "grad_in_scale_dev", "grad_in_shift_dev", "workspace_dev")


def _args(lib, **over):
    from audio_motion_avatar_amd import _lib

    a = _lib.Conv3x3BackwardArgs()
    values = dict(cells=3, height=6, width=8, cin=64, cout=96, upsample_input=0, relu_out=1, extent=64, wgrad_slices=0,
                  weights_split_t_bytes=lib.amav_conv3x3_weights_split_bytes(96, 64), **{p: FAKE for p in POINTERS})
    values.update(over)
    for k, v in values.items():
        setattr(a, k, v)
    if "workspace_bytes" not in over:
        a.workspace_bytes = lib.amav_conv3x3_backward_workspace_bytes(ctypes.byref(a), a.wgrad_slices)
    return a


def _refused(lib, code, *words, **over):
    """The call is refused with `code` and a message holding `words`; unless the workspace is what is wrong, the
    workspace query refuses the same arguments (0 bytes)."""
    a = _args(lib, **over)
    if code == ERR_INVALID:
        assert lib.amav_conv3x3_backward_workspace_bytes(ctypes.byref(a), a.wgrad_slices) == 0, over
    rc = lib.amav_conv3x3_cells_backward(ctypes.byref(a), None)
    msg = lib.amav_last_error()
    assert rc == code, (rc, msg, over)
    for w in (b"amav_conv3x3_cells_backward",) + words:
        assert w in msg, (w, msg)


def test_struct_layout_and_symbols(lib):
    from audio_motion_avatar_amd import _lib

    S = _lib.Conv3x3BackwardArgs
    assert S is _lib.STRUCTS["amav_conv3x3_backward_args"]
    want = [("cells", 0, 8), ("height", 8, 4), ("width", 12, 4), ("cin", 16, 4), ("cout", 20, 4), ("upsample_input", 24, 4),
            ("relu_out", 28, 4), ("extent", 32, 4), ("wgrad_slices", 36, 4), ("x_dev", 40, 8), ("weights_split_t_dev", 48, 8),
            ("weights_split_t_bytes", 56, 8), ("in_scale_dev", 64, 8), ("in_shift_dev", 72, 8), ("origin_dev", 80, 8),
            ("out_dev", 88, 8), ("grad_out_dev", 96, 8), ("grad_x_dev", 104, 8), ("grad_weight_dev", 112, 8),
            ("grad_bias_dev", 120, 8), ("grad_in_scale_dev", 128, 8), ("grad_in_shift_dev", 136, 8), ("workspace_dev", 144, 8),
            ("workspace_bytes", 152, 8)]
    assert [(f, getattr(S, f).offset, getattr(S, f).size) for f, _ in S._fields_] == want
    assert ctypes.sizeof(S) == 160
    for name in ("amav_conv3x3_prepare_weights_split_transposed", "amav_conv3x3_backward_workspace_bytes",
                 "amav_conv3x3_cells_backward"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name


def test_workspace_query(lib):
    def query(slices=0, **over):
        return lib.amav_conv3x3_backward_workspace_bytes(ctypes.byref(_args(lib, workspace_bytes=0, **over)), slices)

    full = query()
    assert full > 0 and full % 256 == 0
    # K H W = 144 texels = 3 tiles: the heuristic never cuts more slices than there are tiles
    slot = 9 * 64 * 96 * 4
    assert query(slices=1) == full - 2 * slot and query(slices=3) == full and query(slices=7) == full + 4 * slot
    # each gradient that is not asked for takes its share away; the weight gradient's slots are the largest
    assert query(grad_weight_dev=None) < full - 2 * slot
    assert query(grad_bias_dev=None) < full and query(grad_in_scale_dev=None, grad_in_shift_dev=None) < full
    # the plain convolution writes grad_x straight from the data gradient: no [K,H,W,Cin] buffer
    plain = dict(in_scale_dev=None, in_shift_dev=None, grad_in_scale_dev=None, grad_in_shift_dev=None, origin_dev=None)
    assert query(**plain) + 3 * 6 * 8 * 64 * 4 <= query(grad_in_scale_dev=None, grad_in_shift_dev=None)
    assert lib.amav_conv3x3_backward_workspace_bytes(None, 0) == 0
    for over in (dict(cin=48), dict(cout=0), dict(cells=0), dict(height=-1), dict(slices=-1), dict(slices=4097),
                 dict(upsample_input=1, height=7), dict(grad_out_dev=None), dict(extent=0)):
        assert query(**over) == 0, over


def test_prepare_weights_transposed_refusals(lib):
    need = lib.amav_conv3x3_weights_split_bytes(96, 64)

    def call(cin=64, cout=96, w=FAKE, out=FAKE, nbytes=need):
        return lib.amav_conv3x3_prepare_weights_split_transposed(cin, cout, w, out, nbytes, None)

    for over in (dict(cin=48), dict(cout=40), dict(cin=0), dict(cout=-32)):
        assert call(**over) == ERR_INVALID and b"multiples of 32" in lib.amav_last_error()
    for over in (dict(w=None), dict(out=None), dict(out=FAKE + 16)):
        assert call(**over) == ERR_INVALID and b"NULL / misaligned" in lib.amav_last_error()
    assert call(nbytes=need - 1) == ERR_WORKSPACE and b"required %d" % need in lib.amav_last_error()


def test_backward_refusals(lib):
    assert lib.amav_conv3x3_cells_backward(None, None) == ERR_INVALID and b"args is NULL" in lib.amav_last_error()
    for name in ("x_dev", "grad_out_dev"):                                        # null required pointers
        _refused(lib, ERR_INVALID, b"NULL", **{name: None})
    _refused(lib, ERR_INVALID, b"relu_out needs", out_dev=None)
    _refused(lib, ERR_INVALID, b"weights_split_t", weights_split_t_dev=None)
    for over in (dict(cells=0), dict(cells=-2), dict(height=0), dict(width=-1)):  # non-positive sizes
        _refused(lib, ERR_INVALID, b"bad sizes", **over)
    for over in (dict(cin=48), dict(cin=0), dict(cout=80), dict(cout=-32)):       # channels
        _refused(lib, ERR_INVALID, b"multiples of 32", **over)
    for over in (dict(height=7), dict(width=9), dict(height=5, width=5)):         # odd sizes with upsample_input
        _refused(lib, ERR_INVALID, b"even", upsample_input=1, **over)
    _refused(lib, ERR_INVALID, b"come together", in_shift_dev=None)
    _refused(lib, ERR_INVALID, b"come together", in_scale_dev=None)
    _refused(lib, ERR_INVALID, b"come together", grad_in_shift_dev=None)
    _refused(lib, ERR_INVALID, b"without a prologue", in_scale_dev=None, in_shift_dev=None)
    _refused(lib, ERR_INVALID, b"extent", extent=0)
    _refused(lib, ERR_INVALID, b"no gradient", grad_x_dev=None, grad_weight_dev=None, grad_bias_dev=None,
             grad_in_scale_dev=None, grad_in_shift_dev=None)
    for over in (dict(wgrad_slices=-1), dict(wgrad_slices=4097)):
        _refused(lib, ERR_INVALID, b"wgrad_slices", **over)
    for name in ("x_dev", "in_scale_dev", "in_shift_dev", "out_dev", "grad_out_dev", "grad_x_dev", "grad_weight_dev",
                 "grad_bias_dev", "grad_in_scale_dev", "grad_in_shift_dev", "weights_split_t_dev"):
        _refused(lib, ERR_INVALID, b"aligned", **{name: FAKE + 4})
    need = _args(lib).workspace_bytes                                             # workspace
    _refused(lib, ERR_WORKSPACE, b"workspace", workspace_bytes=need - 1)
    _refused(lib, ERR_WORKSPACE, b"workspace", workspace_bytes=0)
    _refused(lib, ERR_WORKSPACE, b"workspace", workspace_dev=None)
    _refused(lib, ERR_WORKSPACE, b"workspace", workspace_dev=FAKE + 16)
    _refused(lib, ERR_WORKSPACE, b"weights_split_t", weights_split_t_bytes=lib.amav_conv3x3_weights_split_bytes(96, 64) - 1)
    # forcing more slices than the query was asked for needs more workspace
    _refused(lib, ERR_WORKSPACE, b"workspace", wgrad_slices=5,
             workspace_bytes=lib.amav_conv3x3_backward_workspace_bytes(ctypes.byref(_args(lib)), 3))
    # without relu_out the saved output is not read: its absence is not what is refused
    _refused(lib, ERR_INVALID, b"bad sizes", relu_out=0, out_dev=None, cells=0)
