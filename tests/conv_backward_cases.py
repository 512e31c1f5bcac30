"""Shared by the tests of the 3x3 cell convolution's backward (not collected): the forward restated on F.conv2d so that
torch's autograd gives every reference gradient -- in fp64 on the CPU (the reference) and in fp32 through the library's
convolutions on the device (err32 of the fp32-equivalence bound) -- and the bound itself."""
import torch
import torch.nn.functional as F

GRADS = ("x", "weight", "bias", "in_scale", "in_shift", "residual")
PLANE_ORIGINS = [[-3, -2], [14, 13], [4, 4], [-3, 13], [0, 8]]   # low corner, high corner, inside, mixed, far border


def forward(x, w, bias=None, *, upsample_input=False, in_scale=None, in_shift=None, origin=None, extent=0, relu_out=False,
            residual=None):
    """conv3x3_cells on F.conv2d in the tensors' own dtype and device: x [K,h,w,Cin] channels-last -> [K,H,W,Cout].  The
    operand is masked AFTER BatchNorm + ReLU and zero padded by the convolution."""
    v = x.permute(0, 3, 1, 2)
    if upsample_input:
        v = F.interpolate(v, scale_factor=2, mode="nearest")
    if in_scale is not None:
        v = torch.relu(v * in_scale[None, :, None, None] + in_shift[None, :, None, None])
    if origin is not None:
        K, _, H, W = v.shape
        o = origin.to(v.device).long()
        py = o[:, 0, None] + torch.arange(H, device=v.device)
        px = o[:, 1, None] + torch.arange(W, device=v.device)
        inside = ((py >= 0) & (py < extent))[:, :, None] & ((px >= 0) & (px < extent))[:, None, :]
        v = v * inside[:, None].to(v.dtype)
    y = F.conv2d(v, w, bias, padding=1)
    if relu_out:
        y = torch.relu(y)
    y = y.permute(0, 2, 3, 1)
    if residual is not None:
        y = y + residual
    return y


def draw(K, h, w, cin, cout, seed, *, bias=True, prologue=False, residual=False, upsample_input=False):
    """fp32 CPU inputs of one case: dict over GRADS (None where absent), weights scaled to unit output variance."""
    g = torch.Generator().manual_seed(seed)
    f = 2 if upsample_input else 1
    t = dict.fromkeys(GRADS)
    t["x"] = torch.randn(K, h, w, cin, generator=g)
    t["weight"] = torch.randn(cout, cin, 3, 3, generator=g) * (9 * cin) ** -0.5
    if bias:
        t["bias"] = torch.randn(cout, generator=g)
    if prologue:
        t["in_scale"] = torch.rand(cin, generator=g) + 0.5
        t["in_shift"] = torch.rand(cin, generator=g) + 0.25     # > 0: relu(in_shift) > 0 at every zero of the operand
    if residual:
        t["residual"] = torch.randn(K, f * h, f * w, cout, generator=g)
    grad_out = torch.randn(K, f * h, f * w, cout, generator=g)
    return t, grad_out


def autograd_gradients(tensors, grad_out, options, dtype, device, fn=forward):
    """{name: gradient on the CPU in fp64} of `fn` for every tensor of `tensors` that is there."""
    leaves = {k: v.to(device=device, dtype=dtype).requires_grad_() for k, v in tensors.items() if v is not None}
    opts = {k: v.to(device) if isinstance(v, torch.Tensor) else v for k, v in options.items()}
    out = fn(leaves["x"], leaves["weight"], leaves.get("bias"), in_scale=leaves.get("in_scale"),
             in_shift=leaves.get("in_shift"), residual=leaves.get("residual"), **opts)
    names = list(leaves)
    grads = torch.autograd.grad(out, [leaves[n] for n in names], grad_out.to(device=device, dtype=dtype))
    return {n: g.detach().cpu().double() for n, g in zip(names, grads)}, out.detach()


def library_gradients(tensors, grad_out, options):
    """The library's fp32 autograd on the device, deterministic convolutions."""
    before = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        return autograd_gradients(tensors, grad_out, options, torch.float32, "cuda")[0]
    finally:
        torch.backends.cudnn.deterministic = before


def within_bound(name, got, ref, lib32):
    """Print err, err32, max |ref| of one gradient and assert err <= max(1.5 err32, 2e-6 max |ref|)."""
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert torch.isfinite(got).all(), name
    err = float((got - ref).abs().max()) if ref.numel() else 0.0
    err32 = float((lib32 - ref).abs().max()) if ref.numel() else 0.0
    top = float(ref.abs().max()) if ref.numel() else 0.0
    print(f"{name:9s} err {err:.3e}  err32 {err32:.3e}  max|ref| {top:.3e}")
    assert err <= max(1.5 * err32, 2e-6 * top), (name, err, err32, top)
