"""Host side of the fused optimizer step (amav_grad_norm_clip / amav_adam_step): the chunk tables, the generated structs
against the header, the refusals that come back before the device is touched, and what optim.Adam refuses on the host."""
import ctypes
import re

import pytest

from abi_support import ERR_INVALID, FAKE, HEADER, lib  # noqa: F401 (lib: fixture)

SYMBOLS = ("amav_grad_norm_clip", "amav_adam_step")


def _norm(lib, **over):
    a = dict(tensors=FAKE, T=3, chunks=FAKE, C=5, chunk=64, max_norm=1.0, partial=FAKE, norm=FAKE)
    a.update(over)
    return lib.amav_grad_norm_clip(a["tensors"], a["T"], a["chunks"], a["C"], a["chunk"], a["max_norm"], a["partial"],
                                   a["norm"], None)


def _adam(lib, **over):
    from audio_motion_avatar_amd import ops

    a = dict(tensors=FAKE, T=3, chunks=FAKE, C=5, chunk=64, groups=(ops.OptimGroup * 1)(), G=1, coef=None, zero=0)
    a.update(over)
    return lib.amav_adam_step(a["tensors"], a["T"], a["chunks"], a["C"], a["chunk"], a["groups"], a["G"], a["coef"],
                              a["zero"], None)


def _refused(lib, rc, *texts):
    message = lib.amav_last_error()
    return rc == ERR_INVALID and all(t in message for t in texts)


@pytest.mark.parametrize("chunk", [64, 4096, 5])
def test_tables_cover_every_element_once(chunk):
    from audio_motion_avatar_amd import ops

    numels = [1, 3, chunk - 1, chunk, chunk + 1, 3 * chunk + 5, 0]
    groups = [0, 1, 0, 2, 1, 0, 2]
    tensors, chunks = ops.optimizer_tables(numels, groups, chunk)
    assert [(t.numel, t.group) for t in tensors] == list(zip(numels, groups))
    assert all(t.param is None and t.grad is None and t.exp_avg is None and t.exp_avg_sq is None for t in tensors)
    seen = [[0] * n for n in numels]
    for c in chunks:
        assert 0 <= c.tensor < len(numels) and 0 <= c.start < numels[c.tensor], (c.tensor, c.start)
        assert c.start % chunk == 0
        for e in range(c.start, min(c.start + chunk, numels[c.tensor])):  # a chunk ends with its tensor
            seen[c.tensor][e] += 1
    assert all(count == 1 for row in seen for count in row)                # every element exactly once
    assert all(c.tensor != len(numels) - 1 for c in chunks)                # the empty tensor has no chunk
    keys = [(c.tensor, c.start) for c in chunks]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    assert len(chunks) == sum(-(-n // chunk) for n in numels)


def test_tables_refuse_bad_sizes():
    from audio_motion_avatar_amd import ops

    assert len(ops.optimizer_tables([], [], 64)[1]) == 0
    for bad in (lambda: ops.optimizer_tables([4], [0], 0), lambda: ops.optimizer_tables([4], [0, 1], 8),
                lambda: ops.optimizer_tables([-1], [0], 8), lambda: ops.optimizer_tables([4], [-1], 8)):
        with pytest.raises(ValueError, match="optimizer_tables"):
            bad()


def test_group_entry_is_torch_adams_bias_correction():
    from audio_motion_avatar_amd import ops

    g = ops.optimizer_group(1e-3, (0.9, 0.999), 1e-8, 0.01, 3)
    f = lambda x: ctypes.c_float(x).value  # noqa: E731
    assert g.step_size == f(1e-3 / (1 - 0.9 ** 3)) and g.inv_sqrt_bc2 == f(1 / (1 - 0.999 ** 3) ** 0.5)
    assert (g.beta1, g.beta2, g.one_minus_beta1, g.one_minus_beta2) == (f(0.9), f(0.999), f(1 - 0.9), f(1 - 0.999))
    assert (g.eps, g.weight_decay) == (f(1e-8), f(0.01))


def test_header_binding_and_library_agree(lib):
    from audio_motion_avatar_amd import _lib, ops

    with open(HEADER) as f:
        text = f.read()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1], name      # an export of the library
    ptr, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    tensor, chunk, group = (_lib.STRUCTS["amav_optim_" + n] for n in ("tensor", "chunk", "group"))
    assert tensor._fields_ == [("param", ptr), ("grad", ptr), ("exp_avg", ptr), ("exp_avg_sq", ptr), ("numel", i64),
                               ("group", i32), ("reserved", i32)]
    assert chunk._fields_ == [("start", i64), ("tensor", i32), ("reserved", i32)]
    assert group._fields_ == [(n, f32) for n in ("step_size", "inv_sqrt_bc2", "beta1", "beta2", "one_minus_beta1",
                                                 "one_minus_beta2", "eps", "weight_decay")]
    assert (ctypes.sizeof(tensor), ctypes.sizeof(chunk), ctypes.sizeof(group)) == (48, 16, 32)
    # the header's own field order, read independently of the binding's parser
    for struct in (tensor, chunk, group):
        body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}" % struct.__name__, text, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        assert re.findall(r"(\w+)\s*;", body) == [n for n, _ in struct._fields_], struct.__name__
    c_int = ctypes.c_int
    assert _lib.SIGNATURES["amav_grad_norm_clip"] == (c_int, [ptr, c_int, ptr, c_int, c_int, f32, ptr, ptr, ptr])
    assert _lib.SIGNATURES["amav_adam_step"] == (c_int, [ptr, c_int, ptr, c_int, c_int, ctypes.POINTER(group), c_int, ptr,
                                                         c_int, ptr])
    assert ops.OPTIM_MAX_GROUPS == _lib.DEFINES["AMAV_OPTIM_MAX_GROUPS"] == 16
    assert (ops.OptimTensor, ops.OptimChunk, ops.OptimGroup) == (tensor, chunk, group)


def test_norm_refusals(lib):
    for name in ("tensors", "chunks"):
        assert _refused(lib, _norm(lib, **{name: None}), b"amav_grad_norm_clip", b"NULL table"), name
    for name in ("T", "C"):
        assert _refused(lib, _norm(lib, **{name: -1}), b"amav_grad_norm_clip", b"negative"), name
    for chunk in (0, -4):
        assert _refused(lib, _norm(lib, chunk=chunk), b"amav_grad_norm_clip", b"chunk"), chunk
    for name in ("partial", "norm"):
        assert _refused(lib, _norm(lib, **{name: None}), b"amav_grad_norm_clip", b"NULL"), name
    assert _refused(lib, _norm(lib, T=0, tensors=None, chunks=None, partial=None, norm=None), b"NULL pointer (norm)")
    assert _refused(lib, _norm(lib, T=0, chunk=0), b"chunk")        # an empty problem still has its sizes checked


def test_adam_refusals(lib):
    for name in ("tensors", "chunks"):
        assert _refused(lib, _adam(lib, **{name: None}), b"amav_adam_step", b"NULL table"), name
    for name in ("T", "C"):
        assert _refused(lib, _adam(lib, **{name: -1}), b"amav_adam_step", b"negative"), name
    for chunk in (0, -4):
        assert _refused(lib, _adam(lib, chunk=chunk), b"amav_adam_step", b"chunk"), chunk
    assert _refused(lib, _adam(lib, groups=None), b"amav_adam_step", b"group")
    for count in (0, -1, 17):
        assert _refused(lib, _adam(lib, G=count), b"amav_adam_step", b"group"), count
    # nothing to update: no table, no group and no launch are needed
    assert _adam(lib, T=0, tensors=None, chunks=None, groups=None, G=0) == 0
    assert _adam(lib, C=0, tensors=None, chunks=None, groups=None, G=0) == 0


def test_python_names_exist():
    from audio_motion_avatar_amd import harness, ops, optim, triplane_net

    for name in ("optimizer_tables", "optimizer_group", "optimizer_table_to_device", "grad_norm_clip", "adam_step"):
        assert callable(getattr(ops, name)), name
    assert issubclass(optim.Adam, __import__("torch").optim.Optimizer)
    assert callable(harness.AudioDrivenAvatar.configure_optimizers)
    assert callable(triplane_net.TriplaneGaussianAvatar.configure_optimizers)


def test_adam_refuses_on_the_host(monkeypatch):
    """What the constructor refuses before anything reaches the device: parameters that are not contiguous fp32 on the
    HIP device (named by index), an unknown backend or AMAV_OPTIMIZER, a negative max_grad_norm."""
    import torch

    from audio_motion_avatar_amd import optim

    good = torch.nn.Parameter(torch.zeros(4))
    with pytest.raises(ValueError, match="parameter 0"):
        optim.Adam([good])                                                 # on the host
    with pytest.raises(ValueError, match="parameter 0"):
        optim.Adam([good], backend="library")                              # the comparison path has the same contract
    with pytest.raises(ValueError, match="backend"):
        optim.Adam([good], backend="eager")
    with pytest.raises(ValueError, match="max_grad_norm"):
        optim.Adam([good], max_grad_norm=-1.0)
    monkeypatch.setenv("AMAV_OPTIMIZER", "library")
    assert optim.default_backend() == "library"
    monkeypatch.setenv("AMAV_OPTIMIZER", "triton")
    with pytest.raises(ValueError, match="AMAV_OPTIMIZER"):
        optim.default_backend()
    monkeypatch.delenv("AMAV_OPTIMIZER")
    assert optim.default_backend() == "hip"
