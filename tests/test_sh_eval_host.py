"""The spherical-harmonic arithmetic of the device kernels (csrc/sh_eval.h) on the CPU: tools/sh_eval_host.cpp is built
with -fsanitize=address,undefined and evaluates the forward and the backward of the fixture's cases (and of seeded dense
ones, one per degree).  Its results are held to the tolerances of tests/sh_model.py against the float64 model, and the sanitizers must
stay silent: the polynomials, their derivatives and the clamp gate are checked here before any GPU visit."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

import sh_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_sh.npz")
NAMES = ("deg0", "deg1", "deg2", "deg3", "deg4", "deg1_k16")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    compiler = next((c for c in ("g++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++")
                     if shutil.which(c)), None)
    assert compiler, "no host C++ compiler found"
    exe = str(tmp_path_factory.mktemp("sh_host") / "sh_eval_host")
    subprocess.run([compiler, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "sh_eval_host.cpp"), "-o", exe], check=True)
    return exe


def golden_cases():
    data = np.load(GOLDEN)
    cases = []
    for i, name in enumerate(NAMES):
        c = {k: torch.from_numpy(data[f"{name}/{k}"]) for k in ("means3d", "sh", "campos", "colors")}
        F, N = c["campos"].shape[0], c["means3d"].shape[1]
        c.update(degree=int(data[f"{name}/degree"]), K=c["sh"].shape[2], name=name,
                 grad_colors=torch.randn(F, N, 3, generator=torch.Generator().manual_seed(900 + i)))
        cases.append(c)
    return cases


def run(program, tmp_path, cases):
    """cases: sh_model.case() dicts -> [(colors [F,N,3], grad_sh [F,N,K,3], grad_means3d [F,N,3])], fp32."""
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as fh:
        fh.write(struct.pack("<i", len(cases)))
        for c in cases:
            means3d, sh = sm.expanded(c)
            F, N = means3d.shape[0], means3d.shape[1]
            fh.write(struct.pack("<4i", c["degree"], c["K"], F, N))
            for t in (means3d, c["campos"], sh, c["grad_colors"]):
                fh.write(t.contiguous().numpy().astype("<f4").tobytes())
    done = subprocess.run([program, src, dst], capture_output=True, text=True)
    assert done.returncode == 0 and not done.stderr, done.stderr[-4000:]
    blob, at, out = np.fromfile(dst, dtype="<f4"), 0, []
    for c in cases:
        F, N, K = c["campos"].shape[0], c["means3d"].shape[1], c["K"]
        parts = []
        for shape in ((F, N, 3), (F, N, K, 3), (F, N, 3)):
            n = int(np.prod(shape))
            parts.append(torch.from_numpy(blob[at:at + n].reshape(shape).copy()))
            at += n
        out.append(tuple(parts))
    assert at == blob.size
    return out


def test_fixture_cases_forward_and_backward(program, tmp_path):
    cases = golden_cases()
    for c, (colors, grad_sh, grad_means3d) in zip(cases, run(program, tmp_path, cases)):
        truth, fp32 = sm.yardstick(c)
        # e32 of the fixture: the reference's own stored fp32 result
        sm.check_forward("host " + c["name"], colors, truth["colors"], c["colors"])
        sm.check_gradients("host " + c["name"], grad_sh, grad_means3d, truth, fp32)
        used = sm.num_coeffs(c["degree"])
        assert torch.equal(grad_sh[:, :, used:], torch.zeros_like(grad_sh[:, :, used:]))
        clamped = (colors == 0).float().mean().item()
        if c["degree"] == 0:    # 0.5 + C0 * N(0, 0.5^2) is negative 3.5 sigma out: the higher degrees exercise the gate
            continue
        assert 0.02 <= clamped <= 0.25, f"{c['name']}: {clamped:.3f} of the colours clamped; the gate is not exercised"


@pytest.mark.parametrize("degree", [0, 1, 2, 3, 4])
def test_seeded_dense_cases(program, tmp_path, degree):
    c = sm.case(7000 + degree, degree, 2, 65)
    (colors, grad_sh, grad_means3d), = run(program, tmp_path, [c])
    truth, fp32 = sm.yardstick(c)
    sm.check_forward(f"host dense deg {degree}", colors, truth["colors"], fp32["colors"].float())
    sm.check_gradients(f"host dense deg {degree}", grad_sh, grad_means3d, truth, fp32)


def test_gate_is_the_forward_clamp(program, tmp_path):
    """Where the forward clamped (colour exactly 0) the coefficient gradient of that channel is exactly 0, and nowhere
    else is a whole column zero: the backward's gate is the forward's comparison."""
    c = sm.case(7100, 3, 1, 257)
    (colors, grad_sh, _), = run(program, tmp_path, [c])
    clamped = colors == 0                                                    # [F,N,3]
    dead = (grad_sh == 0).all(dim=2)                                         # [F,N,3]
    assert clamped.any() and torch.equal(clamped, dead)
