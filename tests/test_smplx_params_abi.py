"""Host side of the SMPL-X parameter term (amav_rot6d_to_axis_angle*, amav_smplx_param_loss_*): the header, the generated
binding and the library agree, the Python names exist, every refusal comes back before the device is touched, the empty
problems return 0, and the inputs of tests/test_smplx_params_gpu.py are what their exclusions were worked out for."""
import ctypes
import re

import pytest
import torch

import smplx_param_cases as cases
from abi_support import ERR_INVALID, ERR_WORKSPACE, FAKE, HEADER, lib  # noqa: F401 (lib: fixture)

SYMBOLS = ("amav_rot6d_to_axis_angle", "amav_rot6d_to_axis_angle_backward", "amav_smplx_param_loss_workspace_bytes",
           "amav_smplx_param_loss_forward", "amav_smplx_param_loss_backward")


def _terms(frames=4, over=None):
    """Every term present on fake pointers, in the decoder's shapes; over: {term index: SmplxTerm fields}."""
    from audio_motion_avatar_amd import _lib, ops

    terms = ops.SmplxTerms()
    for k, key in enumerate(ops.SMPLX_TERM_KEYS):
        per_frame = cases.SHAPES[key][0] if len(cases.SHAPES[key]) == 2 or not 1 <= k <= 7 else 1
        width = 3 if 1 <= k <= 7 else 1
        fields = dict(pred=FAKE, gt=FAKE, frames=frames, per_frame=per_frame, pred_stride=per_frame * width,
                      gt_stride=per_frame * width)
        fields.update((over or {}).get(k, {}))
        terms.term[k] = _lib.STRUCTS["amav_smplx_term"](**fields)
    return terms


def _grads(ptr=FAKE):
    from audio_motion_avatar_amd import ops

    grads = ops.SmplxGrads()
    for k in range(len(ops.SMPLX_TERM_KEYS)):
        grads.grad[k] = ptr
    return grads


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
    term = _lib.STRUCTS["amav_smplx_term"]
    assert [(n, t) for n, t in term._fields_] == [("pred", ctypes.c_void_p), ("gt", ctypes.c_void_p), ("frames", ctypes.c_int),
                                                  ("per_frame", ctypes.c_int), ("pred_stride", ctypes.c_int64),
                                                  ("gt_stride", ctypes.c_int64)]
    terms, grads = _lib.STRUCTS["amav_smplx_terms"], _lib.STRUCTS["amav_smplx_grads"]
    assert ctypes.sizeof(terms) == 10 * ctypes.sizeof(term) and ctypes.sizeof(grads) == 10 * ctypes.sizeof(ctypes.c_void_p)
    assert _lib.DEFINES["AMAV_SMPLX_TERMS"] == 10 and _lib.DEFINES["AMAV_SMPLX_PARTS"] == 12
    assert _lib.SIGNATURES["amav_rot6d_to_axis_angle"] == (
        ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p])
    assert _lib.SIGNATURES["amav_smplx_param_loss_forward"][1][0] == ctypes.POINTER(terms)
    assert _lib.SIGNATURES["amav_smplx_param_loss_backward"][1][2] == ctypes.POINTER(grads)
    assert _lib.SIGNATURES["amav_smplx_param_loss_workspace_bytes"] == (ctypes.c_size_t, [ctypes.POINTER(terms)])


def test_python_names_exist():
    from audio_motion_avatar_amd import losses, ops
    from audio_motion_avatar_amd.smplx_decoder import rot6d_to_axis_angle

    for name in ("rot6d_to_axis_angle", "rot6d_to_axis_angle_backward", "rot6d_to_axis_angle_differentiable",
                 "smplx_param_loss_forward", "smplx_param_loss_backward", "smplx_param_loss_differentiable"):
        assert callable(getattr(ops, name)), name
    assert callable(losses.smplx_param_losses) and callable(losses.training_smplx_term) and callable(rot6d_to_axis_angle)
    assert losses.SMPLX_PARAMS_DEFAULT == "library"
    assert ops.SMPLX_TERM_KEYS[1:8] == losses.ROTATION_KEYS
    assert ops.SMPLX_PART_NAMES == ("betas_mse", "betas_prior") + tuple(k + "_geo" for k in losses.ROTATION_KEYS) + (
        "expression_l1", "expression_prior", "transl_smoothl1")


def test_conversion_empty_and_refusals(lib):
    fwd, bwd = lib.amav_rot6d_to_axis_angle, lib.amav_rot6d_to_axis_angle_backward
    assert fwd(0, None, 6, None, None) == 0 and bwd(0, None, 6, None, None, None) == 0     # n = 0: no pointer is looked at
    for n, text in ((-1, b"negative"), (-(1 << 31), b"negative"), (1 << 30, b"2^31 - 1")):
        assert _refused(lib, fwd(n, FAKE, 6, FAKE, None), ERR_INVALID, b"amav_rot6d_to_axis_angle", text), n
        assert _refused(lib, bwd(n, FAKE, 6, FAKE, FAKE, None), ERR_INVALID, b"amav_rot6d_to_axis_angle_backward", text), n
    for args in ((None, 6, FAKE), (FAKE, 6, None)):
        assert _refused(lib, fwd(5, *args, None), ERR_INVALID, b"amav_rot6d_to_axis_angle", b"NULL"), args
    for args in ((None, 6, FAKE, FAKE), (FAKE, 6, None, FAKE), (FAKE, 6, FAKE, None)):
        assert _refused(lib, bwd(5, *args, None), ERR_INVALID, b"amav_rot6d_to_axis_angle_backward", b"NULL"), args


def test_loss_refusals_come_before_any_launch(lib):
    grads = _grads()
    fwd = lambda t, parts=FAKE: lib.amav_smplx_param_loss_forward(t, parts, None, 0, None)          # noqa: E731
    bwd = lambda t, g=ctypes.byref(grads), gp=FAKE: lib.amav_smplx_param_loss_backward(t, gp, g, None)   # noqa: E731
    assert _refused(lib, fwd(None), ERR_INVALID, b"amav_smplx_param_loss_forward", b"NULL")
    assert _refused(lib, bwd(None), ERR_INVALID, b"amav_smplx_param_loss_backward", b"NULL")
    assert _refused(lib, fwd(ctypes.byref(_terms()), None), ERR_INVALID, b"NULL pointer (parts)")
    assert _refused(lib, bwd(ctypes.byref(_terms()), None), ERR_INVALID, b"NULL pointer (grads)")
    assert _refused(lib, bwd(ctypes.byref(_terms()), gp=None), ERR_INVALID, b"NULL pointer (grad_parts)")
    for k in (0, 2, 9):
        for field in ("frames", "per_frame"):
            bad = ctypes.byref(_terms(over={k: {field: -1}}))
            assert _refused(lib, fwd(bad), ERR_INVALID, b"negative count in term %d" % k), (k, field)
            assert _refused(lib, bwd(bad), ERR_INVALID, b"negative count in term %d" % k), (k, field)
            assert lib.amav_smplx_param_loss_workspace_bytes(bad) == 0
        for field in ("pred", "gt"):                       # a present term with one NULL pointer
            bad = ctypes.byref(_terms(over={k: {field: None}}))
            assert _refused(lib, fwd(bad), ERR_INVALID, b"NULL pointer in term %d" % k), (k, field)
            assert _refused(lib, bwd(bad), ERR_INVALID, b"NULL pointer in term %d" % k), (k, field)
    huge = ctypes.byref(_terms(over={2: {"frames": 1 << 26}}))            # 2^26 x 21 rows x 3 floats
    assert _refused(lib, fwd(huge), ERR_INVALID, b"term 2 exceeds")


def test_loss_workspace_query_and_refusal(lib):
    q = lib.amav_smplx_param_loss_workspace_bytes
    assert q(None) == 0
    assert q(ctypes.byref(_terms(frames=64))) == 0                     # every training size: one workgroup, no workspace
    assert q(ctypes.byref(_terms(frames=195))) == 0                    # 4095 body_pose rows
    assert q(ctypes.byref(_terms(frames=196))) == 2 * 12 * 8           # 4116 rows: two workgroups of twelve doubles
    many = _terms(frames=2000)                                         # 42000 rows: eleven workgroups
    assert q(ctypes.byref(many)) == 11 * 12 * 8
    assert _refused(lib, lib.amav_smplx_param_loss_forward(ctypes.byref(many), FAKE, None, 0, None), ERR_WORKSPACE,
                    b"amav_smplx_param_loss_forward", b"workspace")
    assert _refused(lib, lib.amav_smplx_param_loss_forward(ctypes.byref(many), FAKE, FAKE, 11 * 12 * 8 - 1, None),
                    ERR_WORKSPACE, b"workspace")


def test_backward_without_a_wanted_gradient_is_ok_without_a_launch(lib):
    from audio_motion_avatar_amd import ops

    assert lib.amav_smplx_param_loss_backward(ctypes.byref(_terms()), None, ctypes.byref(ops.SmplxGrads()), None) == 0
    assert lib.amav_smplx_param_loss_backward(ctypes.byref(_terms(frames=0)), None, ctypes.byref(_grads()), None) == 0


def test_ops_and_losses_on_the_host():
    """What is decided before anything reaches the library: CPU tensors are refused by ops and handed to the library
    statement by losses.smplx_param_losses; a rotation-key shape mismatch is rotation_geodesic_loss's AssertionError; the
    switch takes two values."""
    from audio_motion_avatar_amd import losses, ops

    with pytest.raises(ops.AmavError, match="only runs on an MI355X"):
        ops.rot6d_to_axis_angle(torch.zeros(2, 6))
    pred, gt = cases.loss_inputs(3)
    with pytest.raises(ops.AmavError, match="only runs on an MI355X"):
        ops.smplx_param_loss_forward(pred, gt)
    total, parts = losses.smplx_param_losses(pred, gt)
    want_total, want_parts = losses.smplx_param_loss(pred, gt)
    assert torch.equal(total, want_total) and list(parts) == list(want_parts)
    with pytest.raises(AssertionError, match="Shape mismatch"):
        losses.smplx_param_losses(pred, {**gt, "body_pose": gt["body_pose"][:, :2]})


def test_the_switch_is_read_per_call(monkeypatch):
    from audio_motion_avatar_amd import losses

    monkeypatch.delenv("AMAV_SMPLX_PARAMS", raising=False)
    assert losses.smplx_params_path() == "library"
    monkeypatch.setenv("AMAV_SMPLX_PARAMS", "hip")
    assert losses.smplx_params_path() == "hip"
    monkeypatch.setenv("AMAV_SMPLX_PARAMS", "fast")
    with pytest.raises(ValueError, match="AMAV_SMPLX_PARAMS"):
        losses.smplx_params_path()
    monkeypatch.setenv("AMAV_SMPLX_PARAMS", "library")
    pred, gt = cases.loss_inputs(3)
    assert torch.equal(losses.training_smplx_term(pred, gt), losses.smplx_param_loss(pred, gt)[0])


def test_fold_reads_views_in_place():
    from audio_motion_avatar_amd import ops

    aa = torch.zeros(4, 55, 3)
    assert ops._fold(aa[:, 1:22], 1) == (4, 165) and ops._fold(aa[:, 1:22], 0) is None
    assert ops._fold(aa[:, 1:22], 2) is None                            # the rows of two frames do not fold
    assert ops._fold(aa[:, 52], 1) == (4, 165)
    wide = torch.zeros(3, 55, 8)
    assert ops._fold(wide[..., :6], 2) == (165, 8)
    assert ops._fold(aa.reshape(2, 2, 55, 3)[:, :, 22:37], 2) == (4, 165)
    assert ops._fold(aa.permute(1, 0, 2), 2) is None


def test_the_random_conversion_case_is_the_one_the_exclusions_were_checked_for():
    d6, _, _, _, keep = cases.random_conversion()
    w, pick, gap = cases.quaternion_facts(d6)
    assert bool(keep.all()) and float(w.abs().min()) > 6e-3             # no row is excluded (at most 2 % may be)
    assert (~keep).float().mean() <= 0.02
    assert torch.bincount(pick, minlength=4).tolist() == [42, 41, 41, 41]   # every candidate is picked
    assert 6e-3 < float(gap.min()) < 7e-3                               # no argmax sits on a tie


def test_the_structured_rows_are_what_they_are_named_for():
    d6, _, aa, grad_d6 = cases.structured_conversion()
    assert torch.equal(aa[:3], torch.zeros(3, 3, dtype=torch.float64))
    assert cases.pi_rows_are_exact(aa) <= 1e-15
    w, pick, _ = cases.quaternion_facts(d6)
    assert pick[list(cases.PI_ROWS)].tolist() == [1, 2, 3] and float(w[list(cases.PI_ROWS)].abs().max()) < 1e-15
    assert (aa[6] - torch.tensor([0.0, 0.0, -1e-4], dtype=torch.float64)).abs().max() < 1e-11
    assert torch.isfinite(grad_d6).all()


@pytest.mark.parametrize("F", (3, 13))
def test_the_loss_case_is_the_one_the_exclusions_were_checked_for(F):
    pred, gt = cases.loss_inputs(F)
    masks = cases.grad_masks(pred, gt)
    rows = sum(m.numel() for k, m in masks.items() if k in cases.KEY_ORDER[:7])
    excluded = sum(int((~m).sum()) for k, m in masks.items() if k in cases.KEY_ORDER[:7])
    assert excluded == 0 and excluded <= 0.01 * rows
    body = cases.geodesic_cos(pred["body_pose"], gt["body_pose"])
    assert int((body > 0.999).sum()) == 3 and int((body < -0.999).sum()) == 1
    assert float(cases.geodesic_cos(pred["left_hand_pose"], gt["left_hand_pose"])[0]) > 0.999
    nearest = min(float((cases.geodesic_cos(pred[k], gt[k]).abs() - 0.999).abs().min()) for k in cases.KEY_ORDER[:7])
    assert nearest > 1e-4                                               # far from the 1e-5 exclusion band
    d = pred["transl"][0].double() - gt["transl"][0].double()
    assert abs(float(d[0])) > 1 and abs(float(d[1])) < 1 and abs(abs(float(d[2])) - 1) < 1e-6
    assert torch.equal(pred["expression"][0, :2], gt["expression"][0, :2])
    _, _, grads = cases.loss_reference(F, False)
    assert all(torch.isfinite(g).all() for g in grads.values())
    assert float(grads["body_pose"][0, :3].abs().max()) == 0 and float(grads["body_pose"][1, 0].abs().max()) == 0
