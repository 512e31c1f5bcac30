"""Host-side checks of the transposing operand split (csrc/attention_rows.hip, amav_split_operand_transposed; DESIGN.md section
4.19) and of the names the training GEMMs add.  No kernel is launched: every call below is refused before it reaches the
device."""
import ctypes

from abi_support import ERR_INVALID, FAKE, lib  # noqa: F401 (lib: fixture)


def _split(lib, rows=40, k=16, x=FAKE, stride=16, weights=0, out_rows=None, out_t=FAKE):
    return lib.amav_split_operand_transposed(rows, k, x, stride, weights, out_rows, out_t, None)


def _refused(lib, rc, word):
    assert rc == ERR_INVALID
    msg = lib.amav_last_error()
    assert b"amav_split_operand_transposed" in msg and word in msg, msg


def test_symbols_and_bindings_agree(lib):
    from audio_motion_avatar_amd import _lib, ops, transformer

    i, l, p = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    assert _lib.SIGNATURES["amav_split_transposed_rows"] == (l, [l])
    assert _lib.SIGNATURES["amav_split_operand_transposed"] == (i, [l, i, p, l, i, p, p, p])
    for name in ("split_operand_transposed", "linear_split_differentiable"):
        assert callable(getattr(ops, name))
    assert callable(transformer.train_linear)


def test_padded_rows(lib):
    assert [lib.amav_split_transposed_rows(r) for r in (1, 8, 9, 6304)] == [8, 8, 16, 6304]
    assert [lib.amav_split_transposed_rows(r) for r in (0, -5)] == [0, 0]
    assert lib.amav_split_transposed_rows(2 ** 40 + 1) == 2 ** 40 + 8  # 64-bit in and out


def test_refusals(lib):
    for kw in (dict(rows=0), dict(rows=-1), dict(k=0), dict(k=-8), dict(k=12, stride=12)):
        _refused(lib, _split(lib, **kw), b"multiple of 8")
    for kw in (dict(x=None), dict(out_t=None)):
        _refused(lib, _split(lib, **kw), b"NULL")
    for stride in (8, 18):
        _refused(lib, _split(lib, stride=stride), b"stride")
    for kw in (dict(x=FAKE + 4), dict(out_t=FAKE + 8), dict(out_rows=FAKE + 2)):
        _refused(lib, _split(lib, **kw), b"aligned")
    _refused(lib, _split(lib, k=64 * 65536, stride=64 * 65536), b"grid")


def test_train_linear_is_f_linear_off_the_device(monkeypatch):
    """Under either setting a CPU product is the library's: the split path is for device tensors only."""
    import torch
    import torch.nn.functional as F

    from audio_motion_avatar_amd import transformer

    g = torch.Generator().manual_seed(1)
    x, w, b = torch.randn(300, 16, generator=g), torch.randn(8, 16, generator=g), torch.randn(8, generator=g)
    for value in ("f32", "split"):
        monkeypatch.setenv("AMAV_TRAIN_GEMM", value)
        assert torch.equal(transformer.train_linear(x, w, b), F.linear(x, w, b))
