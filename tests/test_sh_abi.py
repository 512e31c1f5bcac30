"""Host side of the spherical-harmonic colours (amav_sh_colors, amav_sh_colors_backward): the header, the generated
binding and the library agree on the two symbols and the struct, the Python names exist, every refusal comes back with
its code and message before the device is touched, the empty problems return 0, RGB2SH / SH2RGB round-trip, and the
torch model of the tests equals the reference's fp32 colours of the fixture within the forward tolerance."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import sh_model as sm
from abi_support import ERR_INVALID, FAKE, HEADER, ROOT, lib  # noqa: F401 (lib: fixture)

SYMBOLS = ("amav_sh_colors", "amav_sh_colors_backward")
F, N = 2, 100


def _args(**over):
    from audio_motion_avatar_amd import _lib

    a = dict(F=F, N=N, degree=3, K=16, means3d=FAKE, means_stride=3, sh=FAKE, sh_stride=None, campos=FAKE)
    a.update(over)
    if a["sh_stride"] is None:
        a["sh_stride"] = 3 * a["K"]
    s = _lib.ShArgs()
    s.num_frames, s.num_gaussians, s.degree, s.num_coeffs = a["F"], a["N"], a["degree"], a["K"]
    s.means3d = _lib.Attr(a["means3d"], a["N"] * a["means_stride"], a["means_stride"], 0)
    s.sh = _lib.Attr(a["sh"], 0, a["sh_stride"], 0)
    s.campos = a["campos"]
    return s


def _fwd(lib, colors=FAKE, **over):
    return lib.amav_sh_colors(ctypes.byref(_args(**over)), colors, None)


def _bwd(lib, grad_colors=FAKE, grad_sh=FAKE, grad_means3d=FAKE, **over):
    return lib.amav_sh_colors_backward(ctypes.byref(_args(**over)), grad_colors, grad_sh, grad_means3d, None)


def _refused(lib, rc, *texts):
    message = lib.amav_last_error()
    return rc == ERR_INVALID and all(t in message for t in texts)


def test_header_binding_and_library_agree(lib):
    from audio_motion_avatar_amd import _lib

    with open(HEADER) as f:
        text = f.read()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1], name      # an export of the library
    args = _lib.STRUCTS["amav_sh_args"]
    assert args is _lib.ShArgs
    assert [(n, t) for n, t in args._fields_] == [
        ("num_frames", ctypes.c_int32), ("num_gaussians", ctypes.c_int32), ("degree", ctypes.c_int32),
        ("num_coeffs", ctypes.c_int32), ("means3d", _lib.Attr), ("sh", _lib.Attr), ("campos", ctypes.c_void_p)]
    assert ctypes.sizeof(args) == 16 + 2 * 24 + 8
    ptr = ctypes.POINTER(args)
    assert _lib.SIGNATURES["amav_sh_colors"] == (ctypes.c_int, [ptr, ctypes.c_void_p, ctypes.c_void_p])
    assert _lib.SIGNATURES["amav_sh_colors_backward"] == (ctypes.c_int, [ptr] + [ctypes.c_void_p] * 4)


def test_python_names_exist():
    from audio_motion_avatar_amd import ops, renderer

    for name in ("sh_colors", "sh_colors_backward", "sh_colors_differentiable"):
        assert callable(getattr(ops, name)), name
    assert callable(renderer.RGB2SH) and callable(renderer.SH2RGB)
    assert ops.SH_MAX_DEGREE == 4


@pytest.mark.parametrize("call,name", [(_fwd, b"amav_sh_colors"), (_bwd, b"amav_sh_colors_backward")])
def test_refusals(lib, call, name):
    assert _refused(lib, lib.amav_sh_colors(None, FAKE, None), b"amav_sh_colors", b"NULL")
    for degree in (-1, 5, 17):
        assert _refused(lib, call(lib, degree=degree, K=400), name, b"degree", b"0..4"), degree
    for degree, K in ((0, 0), (1, 3), (2, 8), (3, 15), (4, 24), (3, -1)):
        assert _refused(lib, call(lib, degree=degree, K=K), name, b"num_coeffs", b"(degree+1)^2"), (degree, K)
    for size in ("F", "N"):
        assert _refused(lib, call(lib, **{size: -1}), name, b"negative"), size
    assert _refused(lib, call(lib, sh_stride=47), name, b"sh element stride", b"below")
    assert _refused(lib, call(lib, degree=1, K=16, sh_stride=12), name, b"sh element stride", b"below")
    assert _refused(lib, call(lib, means_stride=2), name, b"means3d element stride", b"below")
    for pointer in ("means3d", "sh", "campos"):
        assert _refused(lib, call(lib, **{pointer: None}), name, b"NULL"), pointer


def test_output_pointers(lib):
    assert _refused(lib, _fwd(lib, colors=None), b"amav_sh_colors", b"NULL")
    assert _refused(lib, _bwd(lib, grad_colors=None), b"amav_sh_colors_backward", b"NULL")
    assert _refused(lib, _bwd(lib, grad_sh=None), b"amav_sh_colors_backward", b"NULL")


def test_empty_problems_return_ok_without_a_pointer(lib):
    nothing = dict(means3d=None, sh=None, campos=None)
    for empty in (dict(F=0), dict(N=0), dict(F=0, N=0)):
        assert _fwd(lib, colors=None, **nothing, **empty) == 0, empty
        assert _bwd(lib, grad_colors=None, grad_sh=None, grad_means3d=None, **nothing, **empty) == 0, empty
    assert _refused(lib, _fwd(lib, F=0, degree=5), b"degree")      # the sizes are still checked


def test_ops_refuse_on_the_host():
    """Before anything reaches the library: CPU tensors, a degree out of range, too few coefficients, a wrong shape."""
    from audio_motion_avatar_amd import ops

    p, sh, cam = torch.zeros(1, 4, 3), torch.zeros(1, 4, 16, 3), torch.zeros(1, 3)
    with pytest.raises(ops.AmavError, match="only runs on an MI355X"):
        ops.sh_colors(p, sh, cam, 3)
    with pytest.raises(ops.AmavError, match="degree 5 outside 0..4"):
        ops.sh_colors(p, sh, cam, 5)
    with pytest.raises(ops.AmavError, match="only runs on an MI355X"):
        ops.sh_colors_differentiable(p, sh, cam, 3)
    with pytest.raises(ops.AmavError, match="only runs on an MI355X"):
        ops.sh_colors_backward(p, sh, cam, 3, torch.zeros(1, 4, 3))


def test_rgb_sh_round_trip():
    from audio_motion_avatar_amd import renderer

    x = torch.rand(1000, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    assert (renderer.SH2RGB(renderer.RGB2SH(x)) - x).abs().max().item() <= 2 ** -52
    x32 = x.float()
    assert (renderer.SH2RGB(renderer.RGB2SH(x32)) - x32).abs().max().item() <= 2 ** -22
    assert renderer.SH_C0 == sm.C0 or abs(renderer.SH_C0 - sm.C0) < 1e-16
    # a degree-0 coefficient RGB2SH(c) gives the colour c
    c = torch.rand(1, 50, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(6))
    out = sm.colors(torch.randn(1, 50, 3, dtype=torch.float64), renderer.RGB2SH(c)[:, :, None, :],
                    torch.tensor([[0.0, 0.0, 3.0]], dtype=torch.float64), 0)
    assert (out - c).abs().max().item() < 1e-15


def test_model_equals_the_reference_fixture():
    """tests/sh_model.py against the reference's own fp32 colours (tests/golden/ref_sh.npz, tier 1): float64 within the
    forward tolerance with e32 = the stored result's own error, which must itself be of fp32 size; the fp32 model too."""
    data = np.load(os.path.join(ROOT, "tests", "golden", "ref_sh.npz"))
    assert int(data["_tier"]) == 1
    for name in ("deg0", "deg1", "deg2", "deg3", "deg4", "deg1_k16"):
        c = {k: torch.from_numpy(data[f"{name}/{k}"]) for k in ("means3d", "sh", "campos", "colors")}
        degree, Fc = int(data[f"{name}/degree"]), c["campos"].shape[0]
        assert c["means3d"].shape == (1, 257, 3) and Fc == 3 and c["sh"].shape[2] >= sm.num_coeffs(degree)
        means3d, sh = c["means3d"].expand(Fc, -1, -1), c["sh"].expand(Fc, -1, -1, -1)
        assert (means3d - c["campos"][:, None]).norm(dim=-1).min().item() >= 0.5
        f64 = sm.colors(means3d.double(), sh.double(), c["campos"].double(), degree)
        f32 = sm.colors(means3d, sh, c["campos"], degree)
        e32 = (c["colors"].double() - f64).abs().max().item()
        assert e32 <= 32 * 2.0 ** -24 * max(1.0, f64.abs().max().item()), (name, e32)   # the model is the reference's function
        sm.check_forward("model fp32 vs fixture " + name, f32, f64, c["colors"])
