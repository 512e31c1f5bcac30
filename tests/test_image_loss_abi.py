"""Host side of the fused image loss (amav_image_loss_*): the header, the generated binding and the library agree, the
Python names exist, every refusal comes back before the device is touched and the empty problems return 0."""
import ctypes
import re

from abi_support import ERR_INVALID, ERR_WORKSPACE, FAKE, HEADER, lib  # noqa: F401 (lib: fixture)

SYMBOLS = ("amav_image_loss_workspace_bytes", "amav_image_loss_forward", "amav_image_loss_backward")
N, H, W, C = 2, 37, 41, 3
TILES = 3 * 3


def _views(ptr=FAKE):
    from audio_motion_avatar_amd import _lib

    return _lib.ImageView(ptr, H * W * C, W * C, C, 1), _lib.ImageView(ptr, H * W * C, W * C, C, 1)


def _fwd(lib, **over):
    from audio_motion_avatar_amd import _lib

    x, y = _views()
    a = dict(N=N, H=H, W=W, C=C, x=ctypes.byref(x), y=ctypes.byref(y), window=ctypes.byref(_lib.ImageLossWindow()),
             sums=FAKE, maps=FAKE, ws=FAKE, ws_bytes=1 << 30)
    a.update(over)
    return lib.amav_image_loss_forward(a["N"], a["H"], a["W"], a["C"], a["x"], a["y"], a["window"], a["sums"], a["maps"],
                                       a["ws"], a["ws_bytes"], None)


def _bwd(lib, **over):
    from audio_motion_avatar_amd import _lib

    x, y = _views()
    a = dict(N=N, H=H, W=W, C=C, x=ctypes.byref(x), y=ctypes.byref(y), window=ctypes.byref(_lib.ImageLossWindow()),
             maps=FAKE, g_l1=FAKE, g_ssim=FAKE, grad_x=FAKE)
    a.update(over)
    return lib.amav_image_loss_backward(a["N"], a["H"], a["W"], a["C"], a["x"], a["y"], a["window"], a["maps"],
                                        a["g_l1"], a["g_ssim"], a["grad_x"], None)


def _refused(lib, rc, code, *texts):
    message = lib.amav_last_error()
    return rc == code and all(t in message for t in texts)


def test_header_binding_and_library_agree(lib):
    from audio_motion_avatar_amd import _lib

    with open(HEADER) as f:
        text = f.read()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1], name      # an export of the library
    view = _lib.STRUCTS["amav_image_view"]
    assert [(n, t) for n, t in view._fields_] == [("ptr", ctypes.c_void_p)] + [
        (n, ctypes.c_int64) for n in ("image_stride", "row_stride", "pixel_stride", "channel_stride")]
    window = _lib.STRUCTS["amav_image_loss_window"]
    assert ctypes.sizeof(window) == 11 * 4 and window._fields_[0][0] == "taps"
    fwd = _lib.SIGNATURES["amav_image_loss_forward"][1]
    assert fwd[4] == fwd[5] == ctypes.POINTER(view) and fwd[6] == ctypes.POINTER(window)
    assert _lib.SIGNATURES["amav_image_loss_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 3)


def test_python_names_exist():
    from audio_motion_avatar_amd import losses, ops

    for name in ("image_loss_sums", "image_loss_backward", "image_loss_differentiable"):
        assert callable(getattr(ops, name)), name
    assert callable(losses.image_losses)
    assert ops.IMAGE_LOSS_WINDOW == 11


def test_the_window_is_the_one_create_window_multiplies(lib):
    import torch

    from audio_motion_avatar_amd import losses, ops

    taps = torch.tensor(list(ops._image_loss_window().taps))
    assert torch.equal(taps, losses.gaussian(11, 1.5).float())
    assert torch.equal(torch.outer(taps, taps), losses.create_window(11, 1)[0, 0])


def test_workspace_query(lib):
    q = lib.amav_image_loss_workspace_bytes
    assert q(N, H, W) == N * TILES * 2 * 4          # one pair of fp32 partial sums per 16 x 16 tile and image
    assert q(1, 16, 16) == 8 and q(1, 17, 16) == 16 and q(1, 1, 70) == 5 * 8
    for empty in ((0, H, W), (N, 0, W), (N, H, 0), (-1, H, W), (N, -2, W), (N, H, -3)):
        assert q(*empty) == 0, empty


def test_forward_refusals(lib):
    for size in ("N", "H", "W"):
        assert _refused(lib, _fwd(lib, **{size: -1}), ERR_INVALID, b"amav_image_loss_forward", b"negative"), size
    for channels in (0, 5, -1):
        assert _refused(lib, _fwd(lib, C=channels), ERR_INVALID, b"amav_image_loss_forward", b"channels"), channels
    assert _refused(lib, _fwd(lib, H=1 << 15, W=1 << 15, C=2), ERR_INVALID, b"amav_image_loss_forward", b"2^31 - 1")
    for name in ("x", "y", "window", "sums"):
        assert _refused(lib, _fwd(lib, **{name: None}), ERR_INVALID, b"amav_image_loss_forward", b"NULL"), name
    null, _ = _views(None)
    for name in ("x", "y"):
        assert _refused(lib, _fwd(lib, **{name: ctypes.byref(null)}), ERR_INVALID, b"amav_image_loss_forward", b"NULL")
    need = lib.amav_image_loss_workspace_bytes(N, H, W)
    assert _refused(lib, _fwd(lib, ws_bytes=need - 1), ERR_WORKSPACE, b"amav_image_loss_forward", b"workspace")
    assert _refused(lib, _fwd(lib, ws=None), ERR_WORKSPACE, b"amav_image_loss_forward", b"workspace")


def test_backward_refusals(lib):
    for size in ("N", "H", "W"):
        assert _refused(lib, _bwd(lib, **{size: -1}), ERR_INVALID, b"amav_image_loss_backward", b"negative"), size
    for channels in (0, 5):
        assert _refused(lib, _bwd(lib, C=channels), ERR_INVALID, b"amav_image_loss_backward", b"channels"), channels
    assert _refused(lib, _bwd(lib, H=1 << 15, W=1 << 15, C=2), ERR_INVALID, b"amav_image_loss_backward", b"2^31 - 1")
    for name in ("x", "y", "window", "maps", "g_l1", "g_ssim", "grad_x"):
        assert _refused(lib, _bwd(lib, **{name: None}), ERR_INVALID, b"amav_image_loss_backward", b"NULL"), name
    null, _ = _views(None)
    for name in ("x", "y"):
        assert _refused(lib, _bwd(lib, **{name: ctypes.byref(null)}), ERR_INVALID, b"amav_image_loss_backward", b"NULL")


def test_empty_problems_return_ok_without_a_pointer(lib):
    nothing = dict(x=None, y=None, window=None)
    for empty in (dict(N=0), dict(H=0), dict(W=0)):
        assert _fwd(lib, sums=None, maps=None, ws=None, ws_bytes=0, **nothing, **empty) == 0, empty
        assert _bwd(lib, maps=None, g_l1=None, g_ssim=None, grad_x=None, **nothing, **empty) == 0, empty
    assert _refused(lib, _fwd(lib, N=0, C=5), ERR_INVALID, b"channels")      # the sizes are still checked


def test_ops_refuse_on_the_host():
    """Before anything reaches the library: CPU tensors, five channels, a target that wants a gradient."""
    import pytest
    import torch

    from audio_motion_avatar_amd import losses, ops

    x = torch.rand(1, 2, 8, 8, 3)
    with pytest.raises(ops.AmavError, match="only runs on an MI355X"):
        losses.image_losses(x, x.clone())
    with pytest.raises(ops.AmavError, match="only runs on an MI355X"):
        ops.image_loss_sums(x[0], x[0], False)
    with pytest.raises(ValueError, match=r"\[B,T,H,W,C\]"):
        losses.image_losses(x[0], x[0])
