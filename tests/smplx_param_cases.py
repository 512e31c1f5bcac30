"""Shared inputs, float64 references and the error rule of the SMPL-X parameter-term tests (tests/test_smplx_params_abi.py
on the host, tests/test_smplx_params_gpu.py on the device).

Yardstick: the Python statement (smplx_decoder.matrix_to_axis_angle(rotation_6d_to_matrix(.)), losses.smplx_param_loss)
in float64 on the CPU, float64 autograd for gradients.  For a compared tensor, e_hip is the fused path's max-abs error
against it and e_lib the error of the library's fp32 evaluation on the device on the same inputs; the rule is

    e_hip <= max(4 * e_lib, 8 * 2^-24 * max|ref|)

(both paths are a few dozen fp32 roundings in different orders; the floor covers what the library gets exactly).
References are computed once per process and never modified."""
import functools
import math

import torch

FLOOR = 8 * 2.0 ** -24
W_MIN = 1e-3            # rows whose float64 quaternion has |w| below this are not compared: axis-angle flips sign at w = 0
COS_EDGE = 1e-5         # rotation rows with | |cos| - 0.999 | below this are not compared in the gradient
KEY_ORDER = ("global_orient", "body_pose", "left_hand_pose", "right_hand_pose", "jaw_pose", "leye_pose", "reye_pose",
             "betas", "expression", "transl")
SHAPES = {"global_orient": (3,), "body_pose": (21, 3), "left_hand_pose": (15, 3), "right_hand_pose": (15, 3),
          "jaw_pose": (3,), "leye_pose": (3,), "reye_pose": (3,), "betas": (10,), "expression": (10,), "transl": (3,)}
WEIGHTS = {"betas": 0.5, "global_orient": 2.0, "body_pose": 1.5, "left_hand_pose": 0.25, "jaw_pose": 3.0,
           "expression": 0.75, "transl": 4.0}   # right_hand_pose, leye_pose, reye_pose: the default 1.0 of weights.get

STRUCTURED = torch.tensor([
    [1.0, 0.0, 0.0, 0.0, 1.0, 0.0],          # identity, and scaled: exactly 0 through the series branch
    [1e-3, 0.0, 0.0, 0.0, 1e-3, 0.0],
    [1e3, 0.0, 0.0, 0.0, 1e3, 0.0],
    [1.0, 0.0, 0.0, 0.0, -1.0, 0.0],         # pi about x, y, z: one per non-w candidate, w = 0, no flip
    [-1.0, 0.0, 0.0, 0.0, 1.0, 0.0],
    [-1.0, 0.0, 0.0, 0.0, -1.0, 0.0],
    [1.0, 1e-4, 0.0, -1e-4, 1.0, 0.0],       # (0, 0, -1e-4)
])
PI_ROWS = (3, 4, 5)


def check_rule(name, hip, lib, ref, keep=None):
    """Assert the rule for one tensor; `keep` (bool, leading axes of the tensors) selects the compared rows."""
    hip, lib, ref = hip.detach().double().cpu(), lib.detach().double().cpu(), ref.detach().double().cpu()
    assert hip.shape == ref.shape == lib.shape, (name, hip.shape, lib.shape, ref.shape)
    if keep is not None:
        hip, lib, ref = hip[keep], lib[keep], ref[keep]
    assert torch.isfinite(hip).all(), name
    e_hip, e_lib = float((hip - ref).abs().max()), float((lib - ref).abs().max())
    scale = float(ref.abs().max())
    bound = max(4 * e_lib, FLOOR * scale)
    print(f"\n{name}: e_hip {e_hip:.2e}, e_lib {e_lib:.2e}, max|ref| {scale:.3g}, bound {bound:.2e}")
    assert e_hip <= bound, (name, e_hip, e_lib, scale)
    return e_hip, e_lib


# ---------------------------------------------------------------------------------------------------- conversion
def conversion_statement(d6):
    from audio_motion_avatar_amd.smplx_decoder import matrix_to_axis_angle, rotation_6d_to_matrix

    return matrix_to_axis_angle(rotation_6d_to_matrix(d6))


def conversion_reference(d6, grad_aa):
    """float64 on the CPU -> (aa, grad_d6)."""
    x = d6.detach().double().cpu().requires_grad_()
    aa = conversion_statement(x)
    aa.backward(grad_aa.detach().double().cpu())
    return aa.detach(), x.grad


def quaternion_facts(d6):
    """float64: (w of the chosen quaternion per row after the flip, the picked candidate per row, the gap between the
    two largest q^2 per row)."""
    from audio_motion_avatar_amd.smplx_decoder import rotation_6d_to_matrix

    m = rotation_6d_to_matrix(d6.double()).reshape(-1, 9)
    m00, m11, m22 = m[:, 0], m[:, 4], m[:, 8]
    q2 = torch.stack([1 + m00 + m11 + m22, 1 + m00 - m11 - m22, 1 - m00 + m11 - m22, 1 - m00 - m11 + m22], -1)
    top = q2.topk(2, dim=-1).values
    angle = conversion_statement(d6.double()).reshape(-1, 3).norm(dim=-1)
    return torch.cos(angle / 2), q2.argmax(-1), top[:, 0] - top[:, 1]


@functools.lru_cache(maxsize=None)
def random_conversion():
    """(d6 [3,55,6], grad_aa [3,55,3], float64 aa, float64 grad_d6, rows to compare [3,55])."""
    g = torch.Generator().manual_seed(101)
    d6 = torch.randn(3, 55, 6, generator=g)
    grad_aa = torch.randn(3, 55, 3, generator=g)
    aa, grad_d6 = conversion_reference(d6, grad_aa)
    w, _, _ = quaternion_facts(d6)
    return d6, grad_aa, aa, grad_d6, (w.abs() >= W_MIN).reshape(3, 55)


@functools.lru_cache(maxsize=None)
def structured_conversion():
    """(d6 [7,6], grad_aa [7,3], float64 aa, float64 grad_d6)."""
    grad_aa = torch.randn(STRUCTURED.shape[0], 3, generator=torch.Generator().manual_seed(102))
    return (STRUCTURED, grad_aa) + conversion_reference(STRUCTURED, grad_aa)


# ---------------------------------------------------------------------------------------------------------- loss
@functools.lru_cache(maxsize=None)
def loss_inputs(F):
    """(pred, gt): dicts of fp32 CPU tensors in the decoder's shapes, with the planted rows."""
    g = torch.Generator().manual_seed(202 + F)
    pred, gt = {}, {}
    for key in KEY_ORDER:
        pred[key] = 0.5 * torch.randn(F, *SHAPES[key], generator=g)
        gt[key] = pred[key] + 0.3 * torch.randn(F, *SHAPES[key], generator=g)
    gt["body_pose"][0, :3] = pred["body_pose"][0, :3]                 # cos clamped high: acos(0.999), no gradient
    pred["body_pose"][1, 0] = torch.tensor([3.1, 0.0, 0.0])           # cos clamped low: no gradient
    gt["body_pose"][1, 0] = torch.tensor([0.0, 0.0, 0.02])
    pred["left_hand_pose"][0, 0] = 0.0
    gt["left_hand_pose"][0, 0] = 0.0
    pred["right_hand_pose"][0, 0] = 0.0                               # the 1e-8 keeps the Rodrigues derivative finite
    gt["transl"][0] = pred["transl"][0] + torch.tensor([2.5, -0.3, 1.0])   # both smooth-L1 branches and |d| = 1
    gt["expression"][0, :2] = pred["expression"][0, :2]               # sign(0)
    return pred, gt


def geodesic_cos(pred, gt):
    """float64 cos of rotation_geodesic_loss before its clamp, per row."""
    from audio_motion_avatar_amd.losses import batch_rodrigues

    Rp, Rg = batch_rodrigues(pred.double().reshape(-1, 3)), batch_rodrigues(gt.double().reshape(-1, 3))
    return ((Rp * Rg).sum((1, 2)) - 1) / 2


def grad_masks(pred, gt):
    """{key: bool tensor of the rows / elements whose gradient is compared}."""
    keep = {}
    for key in KEY_ORDER:
        if key in ("betas", "expression"):
            keep[key] = torch.ones(pred[key].shape, dtype=torch.bool)
        elif key == "transl":
            keep[key] = (pred[key].double() - gt[key].double()).abs() != 1.0     # the smooth-L1 edge itself
        else:
            cos = geodesic_cos(pred[key], gt[key])
            keep[key] = ((cos.abs() - 0.999).abs() >= COS_EDGE).reshape(pred[key].shape[:-1])
    return keep


def total_with_grads(fn, pred, gt, weights, dtype, device):
    """(total, parts, {key: grad of total with respect to pred[key]}) of fn(pred, gt, weights) on `device` in `dtype`."""
    p = {k: v.detach().to(device=device, dtype=dtype).requires_grad_() for k, v in pred.items()}
    t = {k: v.detach().to(device=device, dtype=dtype) for k, v in gt.items()}
    total, parts = fn(p, t, weights)
    total.backward()
    return total.detach(), {k: v.detach() for k, v in parts.items()}, {k: v.grad for k, v in p.items()}


@functools.lru_cache(maxsize=None)
def loss_reference(F, weighted):
    """float64 on the CPU: (total, parts, grads) of losses.smplx_param_loss with the default or with WEIGHTS."""
    from audio_motion_avatar_amd import losses

    pred, gt = loss_inputs(F)
    return total_with_grads(losses.smplx_param_loss, pred, gt, WEIGHTS if weighted else None, torch.float64, "cpu")


def pi_rows_are_exact(aa):
    want = torch.zeros(3, 3, dtype=torch.float64)
    for i in range(3):
        want[i, i] = math.pi
    return float((aa[list(PI_ROWS)].double().cpu() - want).abs().max())
