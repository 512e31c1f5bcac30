"""Spherical-harmonic colours restated with torch: the yardstick of the sh_colors tests.  In float64 it is the truth; in
float32 it is "the same statements evaluated in fp32", whose distance to the truth (e32 / e32g) sets the tolerances:

    forward    max|got - f64| <= max(2 e32, 4 * 2^-24 * max(1, max|f64|))          per case
    gradients  max|got - f64| <= max(2 e32g, 1e-6 * max|grad f64|)                   per tensor

(the factor 2 covers FMA contraction and another order of at most 25 additions).  Colour values whose float64 value
before the clamp lies within 1e-5 of 0 are left out of the gradient comparison of their channel -- the gate may flip
there -- and may be at most 0.5 % of a case.

    d = (p - campos) / |p - campos|,  colour = clamp_min(sum_k B_k(d) sh[k][c] + 0.5, 0)

with the real SH basis of degree 0..4, k = l*l + l + m, odd m with the Condon-Shortley sign (the order and signs of the
reference's eval_sh, src/utils/graphic_utils.py:707-762, which tests/golden/ref_sh.npz pins)."""
import math

import torch

_PI = math.pi
C0 = 1.0 / (2.0 * math.sqrt(_PI))
C1 = math.sqrt(3.0 / (4.0 * _PI))
C2 = (math.sqrt(15.0 / _PI) / 2.0, math.sqrt(5.0 / _PI) / 4.0, math.sqrt(15.0 / _PI) / 4.0)
C3 = (math.sqrt(35.0 / (2.0 * _PI)) / 4.0, math.sqrt(105.0 / _PI) / 2.0, math.sqrt(21.0 / (2.0 * _PI)) / 4.0,
      math.sqrt(7.0 / _PI) / 4.0, math.sqrt(105.0 / _PI) / 4.0)
C4 = (3.0 * math.sqrt(35.0 / _PI) / 4.0, 3.0 * math.sqrt(35.0 / (2.0 * _PI)) / 4.0, 3.0 * math.sqrt(5.0 / _PI) / 4.0,
      3.0 * math.sqrt(5.0 / (2.0 * _PI)) / 4.0, 3.0 / (16.0 * math.sqrt(_PI)), 3.0 * math.sqrt(5.0 / _PI) / 8.0,
      3.0 * math.sqrt(35.0 / _PI) / 16.0)
GATE_BAND = 1e-5
GATE_SHARE = 0.005


def num_coeffs(degree):
    return (degree + 1) ** 2


def basis(degree, d):
    """d [...,3] unit directions -> the (degree+1)^2 basis values, a list of [...] tensors."""
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    B = [torch.full_like(x, C0)]
    if degree >= 1:
        B += [-C1 * y, C1 * z, -C1 * x]
    if degree >= 2:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        B += [C2[0] * xy, -C2[0] * yz, C2[1] * (2.0 * zz - xx - yy), -C2[0] * xz, C2[2] * (xx - yy)]
    if degree >= 3:
        B += [-C3[0] * y * (3.0 * xx - yy), C3[1] * xy * z, -C3[2] * y * (4.0 * zz - xx - yy),
              C3[3] * z * (2.0 * zz - 3.0 * xx - 3.0 * yy), -C3[2] * x * (4.0 * zz - xx - yy), C3[4] * z * (xx - yy),
              -C3[0] * x * (xx - 3.0 * yy)]
    if degree >= 4:
        B += [C4[0] * xy * (xx - yy), -C4[1] * yz * (3.0 * xx - yy), C4[2] * xy * (7.0 * zz - 1.0),
              -C4[3] * yz * (7.0 * zz - 3.0), C4[4] * (zz * (35.0 * zz - 30.0) + 3.0), -C4[3] * xz * (7.0 * zz - 3.0),
              C4[5] * (xx - yy) * (7.0 * zz - 1.0), -C4[1] * xz * (xx - 3.0 * yy),
              C4[6] * (xx * (xx - 3.0 * yy) - yy * (3.0 * xx - yy))]
    return B


def pre_clamp(means3d, sh, campos, degree):
    """means3d [F,N,3], sh [F,N,K,3], campos [F,3] (one dtype) -> the colour before the clamp [F,N,3]."""
    diff = means3d - campos[:, None, :]
    d = diff / diff.norm(dim=-1, keepdim=True)
    B = basis(degree, d)
    acc = B[0][..., None] * sh[..., 0, :]
    for k in range(1, num_coeffs(degree)):
        acc = acc + B[k][..., None] * sh[..., k, :]
    return acc + 0.5


def colors(means3d, sh, campos, degree):
    return torch.clamp_min(pre_clamp(means3d, sh, campos, degree), 0.0)


def evaluate(means3d, sh, campos, degree, grad_colors, dtype):
    """Forward and autograd gradients in `dtype`: dict(colors, pre, grad_sh [F,N,K,3], grad_means3d [F,N,3]), float64
    tensors of the values computed in `dtype`."""
    p = means3d.to(dtype).clone().requires_grad_()
    s = sh.to(dtype).clone().requires_grad_()
    pre = pre_clamp(p, s, campos.to(dtype), degree)
    out = torch.clamp_min(pre, 0.0)
    g_sh, g_p = torch.autograd.grad((out * grad_colors.to(dtype)).sum(), [s, p], allow_unused=True)
    g_p = torch.zeros_like(p) if g_p is None else g_p                       # degree 0 does not depend on the position
    return dict(colors=out.detach().double(), pre=pre.detach().double(), grad_sh=g_sh.double(), grad_means3d=g_p.double())


def case(seed, degree, F, N, K=None, shared=False):
    """Seeded inputs: positions in a unit-ish cloud, camera centres 2.4 to 3 away from its middle (every |p - campos| >=
    0.5), coefficients ~ N(0, 0.5^2), a random colour gradient.  shared: one [1,N,.] set for all frames."""
    g = torch.Generator().manual_seed(seed)
    K = num_coeffs(degree) if K is None else K
    Fs = 1 if shared else F
    means3d = (torch.rand(Fs, N, 3, generator=g) - 0.5) * 1.6
    sh = torch.randn(Fs, N, K, 3, generator=g) * 0.5
    away = torch.nn.functional.normalize(torch.randn(F, 3, generator=g), dim=-1)
    campos = away * (2.4 + 0.6 * torch.rand(F, 1, generator=g))
    grad_colors = torch.randn(F, N, 3, generator=g)
    return dict(degree=degree, K=K, means3d=means3d, sh=sh, campos=campos, grad_colors=grad_colors)


def expanded(c):
    """The case's [F,N,.] inputs (a shared set expanded over the frames, stride 0)."""
    F = c["campos"].shape[0]
    return c["means3d"].expand(F, -1, -1), c["sh"].expand(F, -1, -1, -1)


def yardstick(c):
    """(f64 results, fp32 results) of a case, both as float64 tensors."""
    means3d, sh = expanded(c)
    return (evaluate(means3d, sh, c["campos"], c["degree"], c["grad_colors"], torch.float64),
            evaluate(means3d, sh, c["campos"], c["degree"], c["grad_colors"], torch.float32))


def forward_bound(f64, e32):
    return max(2.0 * e32, 4.0 * 2.0 ** -24 * max(1.0, f64.abs().max().item()))


def check_forward(name, got, f64, f32_colors):
    """got, f32_colors: fp32 colours; f64: the truth.  Prints the figures, then asserts the forward bound."""
    e32 = (f32_colors.double() - f64).abs().max().item()
    err = (got.double() - f64).abs().max().item()
    bound = forward_bound(f64, e32)
    print(f"sh forward {name}: err {err:.3e}  e32 {e32:.3e}  err/e32 {err / max(e32, 1e-300):.2f}  bound {bound:.3e}")
    assert err <= bound, f"{name}: colours off by {err:.3e} > {bound:.3e} (e32 {e32:.3e})"
    return err, e32


def check_gradients(name, got_sh, got_means3d, truth, fp32):
    """got_sh [F,N,K,3] and got_means3d [F,N,3] against yardstick()'s pair.  Entries of grad_sh whose channel's value
    before the clamp is within GATE_BAND of 0 are left out (at most GATE_SHARE of the case); grad_means3d mixes the
    three channels, so a Gaussian with such a channel is left out of it."""
    near = truth["pre"].abs() < GATE_BAND                                    # [F,N,3]
    share = near.double().mean().item()
    assert share <= GATE_SHARE, f"{name}: {share:.4f} of the values sit on the clamp"
    keep_sh = (~near)[..., None, :].expand_as(truth["grad_sh"])
    keep_p = (~near.any(dim=-1))[..., None].expand_as(truth["grad_means3d"])
    out = {}
    for key, got, keep in (("grad_sh", got_sh, keep_sh), ("grad_means3d", got_means3d, keep_p)):
        if got is None:
            continue
        ref = truth[key]
        e32g = ((fp32[key] - ref).abs() * keep).max().item()
        err = ((got.double() - ref).abs() * keep).max().item()
        bound = max(2.0 * e32g, 1e-6 * ref.abs().max().item())
        print(f"sh backward {name} {key}: err {err:.3e}  e32g {e32g:.3e}  err/e32g {err / max(e32g, 1e-300):.2f}  "
              f"bound {bound:.3e}  left out {int(near.sum())}")
        assert err <= bound, f"{name}: {key} off by {err:.3e} > {bound:.3e} (e32g {e32g:.3e})"
        out[key] = (err, e32g)
    return out
