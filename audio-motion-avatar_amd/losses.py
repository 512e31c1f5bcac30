"""Image and SMPL-X parameter metrics of the reference (src/utils/loss_utils.py), as the demo prints them per window
(src/main2.py:205-211) and the training step sums them (src/models/lightning_model_wrapper.py:495-530).

Same names, arguments and reductions as the reference, evaluated where the tensors live (on the MI355X for rendered
frames: elementwise work and an 11 x 11 depthwise window through the library's convolution -- none of it is on the
rendering hot path, so there is no hand-written kernel here).  Pinned by reference-run fixtures: l1 / l2 / ssim / window
exactly as shipped (tier 1), the geodesic and SMPL-X parameter losses with smplx's absent `batch_rodrigues` restated
(tier 2) -- tests/test_reference_golden.py.  `LPIPS` needs the `lpips` package and its VGG weights, neither of which is
available offline: constructing it raises.
"""
import math

import torch
import torch.nn.functional as F


def l1_loss(network_output, gt):
    """loss_utils.py:18-19"""
    return torch.abs(network_output - gt).mean()


def l2_loss(network_output, gt):
    """loss_utils.py:21-22"""
    return ((network_output - gt) ** 2).mean()


def psnr(network_output, gt):
    """10 log10(1 / MSE) over everything (BASELINE.json's quality metric; the reference implements no PSNR)."""
    return 10.0 * torch.log10(1.0 / l2_loss(network_output, gt).clamp_min(1e-20))


def gaussian(window_size, sigma):
    """loss_utils.py:24-26: normalised 1-D Gaussian taps."""
    g = torch.tensor([math.exp(-(x - window_size // 2) ** 2 / float(2 * sigma ** 2)) for x in range(window_size)])
    return g / g.sum()


def create_window(window_size, channel):
    """loss_utils.py:28-32: [channel, 1, window, window] separable Gaussian (sigma 1.5)."""
    w1 = gaussian(window_size, 1.5).unsqueeze(1)
    w2 = w1.mm(w1.t()).float().unsqueeze(0).unsqueeze(0)
    return w2.expand(channel, 1, window_size, window_size).contiguous()


def _ssim(img1, img2, window, window_size, channel, size_average=True):
    """loss_utils.py:63-84"""
    pad = window_size // 2
    mu1 = F.conv2d(img1, window, padding=pad, groups=channel)
    mu2 = F.conv2d(img2, window, padding=pad, groups=channel)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    sigma1_sq = F.conv2d(img1 * img1, window, padding=pad, groups=channel) - mu1_sq
    sigma2_sq = F.conv2d(img2 * img2, window, padding=pad, groups=channel) - mu2_sq
    sigma12 = F.conv2d(img1 * img2, window, padding=pad, groups=channel) - mu1_mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    ssim_map = ((2 * mu1_mu2 + C1) * (2 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2))
    return ssim_map.mean() if size_average else ssim_map.mean(1).mean(1).mean(1)


def ssim(img1, img2, window_size=11, size_average=True):
    """loss_utils.py:44-61: img1, img2 [B, T, H, W, C] (the renderer's frame layout)."""
    img1 = img1.reshape(-1, *img1.shape[2:]).permute(0, 3, 1, 2)
    img2 = img2.reshape(-1, *img2.shape[2:]).permute(0, 3, 1, 2)
    channel = img1.size(1)
    window = create_window(window_size, channel).to(img1.device).type_as(img1)
    return _ssim(img1, img2, window, window_size, channel, size_average)


class LPIPS(torch.nn.Module):
    """loss_utils.py:87-105 wraps lpips.LPIPS(net='vgg'): a pretrained network that cannot be fetched here."""

    def __init__(self):
        super().__init__()
        raise RuntimeError("LPIPS needs the `lpips` package and its pretrained VGG weights, which are not available offline; "
                           "l1_loss / ssim / psnr are implemented")


def batch_rodrigues(rot_vecs, epsilon=1e-8):
    """smplx.lbs.batch_rodrigues (absent here): axis-angle [N,3] -> [N,3,3]."""
    angle = torch.norm(rot_vecs + epsilon, dim=1, keepdim=True)
    rot_dir = rot_vecs / angle
    cos, sin = torch.cos(angle)[:, None], torch.sin(angle)[:, None]
    rx, ry, rz = torch.split(rot_dir, 1, dim=1)
    zeros = torch.zeros_like(rx)
    K = torch.cat([zeros, -rz, ry, rz, zeros, -rx, -ry, rx, zeros], dim=1).view(-1, 3, 3)
    ident = torch.eye(3, dtype=rot_vecs.dtype, device=rot_vecs.device)[None]
    return ident + sin * K + (1 - cos) * torch.bmm(K, K)


def rotation_geodesic_loss(rot_vec_pred, rot_vec_gt):
    """loss_utils.py:109-135: mean geodesic angle between two sets of axis-angle rotations [..., 3]."""
    if rot_vec_pred.shape != rot_vec_gt.shape:
        raise AssertionError(f"Shape mismatch: {rot_vec_pred.shape} vs {rot_vec_gt.shape}")
    if rot_vec_pred.shape[-1] != 3:
        raise AssertionError("the last dimension must be 3")
    R_pred = batch_rodrigues(rot_vec_pred.reshape(-1, 3))
    R_gt = batch_rodrigues(rot_vec_gt.reshape(-1, 3))
    RT = torch.matmul(R_pred.transpose(1, 2), R_gt)
    cos = (torch.diagonal(RT, dim1=1, dim2=2).sum(-1) - 1) / 2
    return torch.acos(torch.clamp(cos, -0.999, 0.999)).mean()


ROTATION_KEYS = ("global_orient", "body_pose", "left_hand_pose", "right_hand_pose", "jaw_pose", "leye_pose", "reye_pose")


def smplx_param_loss(pred_params, gt_params, weights=None):
    """loss_utils.py:137-182 -> (total, dict of the parts under the reference's names)."""
    if weights is None:
        weights = {k: 1.0 for k in ("betas",) + ROTATION_KEYS + ("expression", "transl")}
    losses = {}
    total = 0.0
    if "betas" in pred_params and "betas" in gt_params:
        losses["betas_mse"] = F.mse_loss(pred_params["betas"], gt_params["betas"])
        losses["betas_prior"] = torch.mean(pred_params["betas"] ** 2)
        total = total + weights["betas"] * losses["betas_mse"] + 0.01 * losses["betas_prior"]
    for key in ROTATION_KEYS:
        if key in pred_params and key in gt_params:
            losses[f"{key}_geo"] = rotation_geodesic_loss(pred_params[key], gt_params[key])
            total = total + weights.get(key, 1.0) * losses[f"{key}_geo"]
    if "expression" in pred_params and "expression" in gt_params:
        losses["expression_l1"] = F.l1_loss(pred_params["expression"], gt_params["expression"])
        losses["expression_prior"] = torch.mean(pred_params["expression"] ** 2)
        total = total + weights["expression"] * losses["expression_l1"] + 0.01 * losses["expression_prior"]
    if "transl" in pred_params and "transl" in gt_params:
        losses["transl_smoothl1"] = F.smooth_l1_loss(pred_params["transl"], gt_params["transl"])
        total = total + weights["transl"] * losses["transl_smoothl1"]
    return total, losses


def _fused_smplx_terms(pred_params, gt_params):
    """Whether ops.smplx_param_loss_differentiable can take these dicts as they are."""
    keys = [k for k in ("betas",) + ROTATION_KEYS + ("expression", "transl") if k in pred_params and k in gt_params]
    for k in keys:
        p, g = pred_params[k], gt_params[k]
        if not (isinstance(p, torch.Tensor) and isinstance(g, torch.Tensor) and p.is_cuda and g.is_cuda):
            return False
        if p.dtype != torch.float32 or g.dtype != torch.float32 or p.shape != g.shape or p.device != g.device:
            return False
        if g.requires_grad and torch.is_grad_enabled():
            return False
    return bool(keys)


_smplx_weight_vectors = {}


def _smplx_weight_vector(weights, present, device):
    """[12] device tensor of the factors smplx_param_loss puts on its parts (0.01 on the two priors; 0 for a key that
    is not present, whose weight smplx_param_loss never looks up), cached per set of weights; None when a weight is not
    a plain number.  A present betas / expression / transl without a weight is smplx_param_loss's KeyError."""
    named = {k: weights[k] if k in present else 0.0 for k in ("betas", "expression", "transl")}
    values = [named["betas"], 0.01] + [weights.get(k, 1.0) for k in ROTATION_KEYS] + [named["expression"], 0.01,
                                                                                      named["transl"]]
    if not all(isinstance(v, (int, float)) for v in values):
        return None
    key = (tuple(float(v) for v in values), device)
    if key not in _smplx_weight_vectors:
        _smplx_weight_vectors[key] = torch.tensor(key[0], dtype=torch.float32, device=device)
    return _smplx_weight_vectors[key]


def smplx_param_losses(pred_params, gt_params, weights=None):
    """smplx_param_loss from the fused HIP kernels (ops.smplx_param_loss_differentiable; csrc/smplx_params.hip): the
    same (total, parts) -- the same part names, the same weights semantics, the same keys skipped when either dict
    lacks them -- from one forward launch and, under autograd, one backward launch for all pred tensors.  The twelve
    means come back as one [12] device tensor; the parts are views of it and total is its product with the weights,
    in torch.  pred tensors are read in place (slices of the decoder's [F,55,3] included); gt gets no gradient.

    It takes float32 device tensors with pred[k].shape == gt[k].shape.  A rotation key whose shapes differ raises the
    AssertionError of rotation_geodesic_loss.  Everything else it cannot take is handed to smplx_param_loss itself:
    CPU tensors, other dtypes, betas / expression / transl that broadcast, a gt that requires a gradient, weights that
    are not plain numbers.  smplx_param_loss remains the fixture-pinned statement of the reference."""
    from . import ops

    for key in ROTATION_KEYS:
        if key in pred_params and key in gt_params:
            if pred_params[key].shape != gt_params[key].shape:
                raise AssertionError(f"Shape mismatch: {pred_params[key].shape} vs {gt_params[key].shape}")
            if pred_params[key].shape[-1] != 3:
                raise AssertionError("the last dimension must be 3")
    if not _fused_smplx_terms(pred_params, gt_params):
        return smplx_param_loss(pred_params, gt_params, weights)
    if weights is None:
        weights = {k: 1.0 for k in ("betas",) + ROTATION_KEYS + ("expression", "transl")}
    present = [k for k in ops.SMPLX_TERM_KEYS if k in pred_params and k in gt_params]
    factors = _smplx_weight_vector(weights, present, pred_params[present[0]].device)
    if factors is None:
        return smplx_param_loss(pred_params, gt_params, weights)
    parts = ops.smplx_param_loss_differentiable(pred_params, gt_params)
    named = dict(zip(ops.SMPLX_PART_NAMES, parts.unbind(0)))
    losses = {name: named[name] for name in ops.SMPLX_PART_NAMES if _part_key(name) in present}
    return torch.dot(parts, factors), losses


def _part_key(name):
    """The parameter key a part of smplx_param_loss belongs to (`body_pose_geo` -> `body_pose`)."""
    return name.rsplit("_", 1)[0]


SMPLX_PARAMS_DEFAULT = "library"   # tools/bench_smplx_params.py has the numbers a later change of the default cites


def smplx_params_path():
    """AMAV_SMPLX_PARAMS, read per call like AMAV_IMAGE_LOSS: `library` (the torch statements of this module and of
    smplx_decoder.py) or `hip` (csrc/smplx_params.hip)."""
    import os

    path = os.environ.get("AMAV_SMPLX_PARAMS", SMPLX_PARAMS_DEFAULT)
    if path not in ("library", "hip"):
        raise ValueError(f"AMAV_SMPLX_PARAMS={path!r}: expected `library` or `hip`")
    return path


def training_smplx_term(pred_params, gt_params):
    """The SMPL-X parameter term of a training step, smplx_param_loss(pred, gt)[0]: the library statement, or with
    AMAV_SMPLX_PARAMS=hip the fused smplx_param_losses."""
    if smplx_params_path() == "hip":
        return smplx_param_losses(pred_params, gt_params)[0]
    return smplx_param_loss(pred_params, gt_params)[0]


def image_losses(img1, img2, size_average=True):
    """(l1_loss(img1, img2), ssim(img1, img2, 11, size_average)) for training, from the fused HIP kernels
    (ops.image_loss_differentiable; csrc/image_loss.hip): img1, img2 [B, T, H, W, C] on the device, C = 1..4, both read
    in place whatever their strides (the renderer's rgba[..., :3] view, a permuted [B,T,C,H,W] target).  One forward and,
    for whatever weights the caller puts on the two terms, one backward launch; the gradient reaches img1 only, and
    img2 must not require one.  The functions above remain the CPU-capable statement of the reference; this one has no
    CPU path.  l1 is the mean over everything; ssim the mean over everything, or per image [B*T] without size_average."""
    from . import ops

    if img1.dim() != 5 or img1.shape != img2.shape:
        raise ValueError(f"image_losses: expected two [B,T,H,W,C] tensors of one shape, got {tuple(img1.shape)} and "
                         f"{tuple(img2.shape)}")
    l1_sum, ssim_sum = ops.image_loss_differentiable(img1.reshape(-1, *img1.shape[2:]),
                                                     img2.reshape(-1, *img2.shape[2:]))
    per_image = img1.shape[2] * img1.shape[3] * img1.shape[4]
    l1 = l1_sum.sum() / (l1_sum.numel() * per_image)
    return l1, (ssim_sum.sum() / (ssim_sum.numel() * per_image) if size_average else ssim_sum / per_image)


IMAGE_LOSS_DEFAULT = "hip"   # tools/bench_image_loss.py: the fused path is the faster one at both training shapes


def training_image_terms(rendered, target):
    """(l1, 1 - ssim) of a training step: image_losses, or with AMAV_IMAGE_LOSS=library (read per call, like
    AMAV_CROSS_ATTN) the two library evaluations l1_loss and ssim."""
    import os

    if os.environ.get("AMAV_IMAGE_LOSS", IMAGE_LOSS_DEFAULT) == "library":
        return l1_loss(rendered, target), 1 - ssim(rendered, target)
    l1, s = image_losses(rendered, target)
    return l1, 1 - s
