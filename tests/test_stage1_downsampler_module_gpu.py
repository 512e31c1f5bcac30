"""Stage 1 with upsample_triplane on the MI355X: TriplaneDownsampler on the HIP kernels against the two reference-run
fixtures (tests/golden/make_downsampler_golden.py) and against the library path, SMPLXTriplaneEncoder at 3x cell
resolution, and TriplaneGaussianAvatar.training_step through the downsampler's HIP backwards.

Bounds.  With fp32 library GEMMs (AMAV_GEMM=f32) the `block` bound of tests/downsampler_cases.py: the library's fp32
error against the fp64 restatement (forward: CPU 2.5e-6, MI355X 8.6e-7, bound 1.2e-5; gradients of the whole module at
C = 256: CPU 1.7e-6, MI355X 1.8e-6, bound 8e-6) times 4 -- plus that error once more against a reference-run fp32 vector.
Measured for the HIP path on the MI355X: 1.3e-6 against the fixture, 8.6e-7 at C = 256, gradients up to 1.9e-6 (pwconv2's
weight, a library GEMM).  The two module cases added for the pass split and for a width without kernels (C = 64, 27
planes of 6 x 6; C = 32, 12 x 12) stay inside the same figures: the library measures 1.1e-6 / 7.2e-7 (forward) and 1.2e-6 /
1.2e-6 (gradients) at the first and 1.2e-6 / 1.1e-6 at the second (CPU / MI355X); the HIP path 3.5e-7 and 1.0e-6.  With the
products as bf16 x 3 split GEMMs (the inference default) the project's bound for that path, 2e-5 relative to the output
scale (close() of tests/test_stage1_gpu.py, as for the encoder and the transformer stack there)."""
from types import SimpleNamespace

import pytest
import torch

import downsampler_cases as dc
from helpers import _generator_module, ref_fixture, seeded_params, toy_body
from test_stage1_gpu import close

pytestmark = pytest.mark.gpu
SPLIT_GEMM_BOUND = 2e-5


def _module(cfg, params, prefix):
    from audio_motion_avatar_amd.triplane_net import TriplaneDownsampler

    ds = TriplaneDownsampler(SimpleNamespace(**cfg)).eval()
    ds.load_state_dict(seeded_params(params, prefix), strict=True)   # reference names, strict
    return ds.cuda()


def _check(kind, got, want, what, fp32_reference=False):
    """Against an fp64 reference: the bound of the kind.  Against a reference-run fp32 vector: plus the library's own error
    once more, which that vector carries."""
    limit = dc.bound(kind) + (dc.LIBRARY_ERR[kind] if fp32_reference else 0.0)
    err = dc.rel_err(got, want)
    print(f"{what}: {kind} error {err:.3e} (bound {limit:.1e})")
    assert err <= limit, f"{what}: {err:.3e} > {limit:.1e}"


def test_hip_path_equals_the_reference_downsampler(monkeypatch):
    a, meta, tier = ref_fixture("stage1_downsampler")
    assert tier == 1
    ds = _module(meta["cfg"], meta["params"], meta["param_prefix"])
    x = a["x"].cuda()
    planes = dc.planes_of(a["x"]).cuda()
    want = [dc.planes_of(a[k]) for k in ("after_block0", "after_block1", "y")]
    with torch.no_grad():
        for gemm, check in (("f32", lambda g, w, what: _check("block", g, w, what, fp32_reference=True)),
                            ("split", lambda g, w, what: close(g, w, SPLIT_GEMM_BOUND, what))):
            monkeypatch.setenv("AMAV_GEMM", gemm)
            b0 = ds.blocks[0].forward_planes(planes, hip=True)
            b1 = ds.blocks[1].forward_planes(b0, hip=True)
            y = ds(planes)
            for got, w, what in zip((b0, b1, y), want, ("block 0", "block 1", "output")):
                check(got.cpu(), w, f"hip, AMAV_GEMM={gemm}, {what}")
            y5 = ds(x)
            assert y5.shape == a["y"].shape and torch.equal(dc.planes_of(y5), y)      # both layouts, the same values
            assert torch.equal(y, ds(planes))                                           # deterministic
        monkeypatch.setenv("AMAV_STAGE1_DOWNSAMPLER", "library")
        close(ds(x), a["y"], 1e-5, "library path on the GPU (MIOpen)")
    # a reference-named state_dict round-trips
    sd = {k: v.clone() for k, v in ds.state_dict().items()}
    assert {k: list(v.shape) for k, v in sd.items()} == meta["params"]
    ds.load_state_dict(sd, strict=True)


def test_hip_against_library_at_the_reference_width(monkeypatch):
    """C = 256, R = 8, factor 3: both paths against the fp64 restatement (fp32 GEMMs), and under autograd the HIP path's
    gradients against the library's."""
    p, x, want = dc.module_case()
    ds = _module(dict(triplane_feature_dim=256, upsample_factor=3), {k: list(v.shape) for k, v in p.items()},
                 "triplane_downsampler.")
    xc = x.cuda()
    monkeypatch.setenv("AMAV_GEMM", "f32")
    with torch.no_grad():
        y_hip = ds(xc)
        monkeypatch.setenv("AMAV_STAGE1_DOWNSAMPLER", "library")
        y_lib = ds(xc)
        monkeypatch.delenv("AMAV_STAGE1_DOWNSAMPLER")
    print(f"library fp32 on the GPU: error {dc.rel_err(y_lib, want[2]):.3e}")
    _check("block", y_hip, want[2], "hip, C = 256")
    monkeypatch.delenv("AMAV_GEMM")
    with torch.no_grad():
        close(ds(xc), want[2].float(), SPLIT_GEMM_BOUND, "hip with split GEMMs, C = 256")
    # training: the forward under autograd is the inference forward with fp32 GEMMs bit for bit; gradients agree
    monkeypatch.setenv("AMAV_GEMM", "f32")
    g, want_grads = dc.module_backward_case()
    grads = {}
    for path in ("hip", "library"):
        monkeypatch.setenv("AMAV_STAGE1_DOWNSAMPLER", path)
        leaf = xc.clone().requires_grad_(True)
        ds.zero_grad(set_to_none=True)
        y = ds(leaf)
        if path == "hip":
            assert torch.equal(y.detach(), y_hip)
        y.backward(g.cuda())
        grads[path] = dict([("input", leaf.grad)] + [(n, q.grad.clone()) for n, q in ds.named_parameters()])
    assert set(grads["hip"]) == set(want_grads)
    lib = max(dc.rel_err(grads["library"][k], want_grads[k]) for k in want_grads)
    print(f"library fp32 autograd on the GPU: largest gradient error {lib:.3e}")
    for k in want_grads:
        _check("dmodule", grads["hip"][k], want_grads[k], f"hip, d {k}")


def test_split_gemms_under_autograd_keep_their_bound(monkeypatch):
    """AMAV_TRAIN_GEMM=split: pwconv1 and pwconv2 of both blocks run as bf16 x 3 split products (1728 rows; the strided
    convolution's 192 rows stay below train_linear's 256-row gate), and every gradient meets that path's existing bound,
    1e-5 max |grad| per tensor against fp64 autograd (tests/test_train_gemm_module_gpu.py)."""
    from audio_motion_avatar_amd import ops

    calls, real = [], ops.linear_split_differentiable

    def counted(x, weight, *a, **k):
        calls.append((x.numel() // weight.shape[1], weight.shape[1], weight.shape[0]))
        return real(x, weight, *a, **k)

    monkeypatch.setattr(ops, "linear_split_differentiable", counted)
    monkeypatch.setenv("AMAV_TRAIN_GEMM", "split")
    p, x, _ = dc.module_case()
    ds = _module(dict(triplane_feature_dim=256, upsample_factor=3), {k: list(v.shape) for k, v in p.items()},
                 "triplane_downsampler.")
    g, want = dc.module_backward_case()
    leaf = x.cuda().requires_grad_(True)
    ds(leaf).backward(g.cuda())
    assert sorted(calls) == [(1728, 256, 1024)] * 2 + [(1728, 1024, 256)] * 2
    got = dict([("input", leaf.grad)] + [(n, q.grad) for n, q in ds.named_parameters()])
    worst = max((dc.rel_err(got[k], want[k]), k) for k in want)
    print(f"AMAV_TRAIN_GEMM=split: largest gradient error {worst[0]:.3e} ({worst[1]})")
    assert worst[0] <= 1e-5, worst


def _encoder(meta, body):
    from audio_motion_avatar_amd.smplx_decoder import SMPLXDecoder
    from audio_motion_avatar_amd.triplane_net import SMPLXTriplaneEncoder

    cfg = SimpleNamespace(**meta["cfg"])

    class Encoder(SMPLXTriplaneEncoder):  # the same substitution the fixture's generator made for smplx.SMPLX
        def init_smplx_model(self):
            return body

    enc = Encoder(cfg, SMPLXDecoder(cfg)).eval()
    assert {k: list(v.shape) for k, v in enc.state_dict().items()} == meta["params_encoder"]
    enc.load_state_dict(seeded_params(meta["params_encoder"], "smplx_triplane_encoder."), strict=True)
    return enc.cuda()


def test_encoder_at_three_times_the_cell_resolution_equals_the_reference_run():
    a, meta, tier = ref_fixture("stage1_upsampled")
    assert tier == 2 and meta["cfg"]["upsample_triplane"] and meta["cfg"]["upsample_factor"] == 3
    gen = _generator_module()
    enc = _encoder(meta, toy_body(**meta["toy_body"]).cuda())
    B = meta["batch"]
    gt = {k: gen.rnd(meta["smpl_seed"] + i, B, 1, d, scale=meta["smpl_scale"]).cuda()
          for i, (k, d) in enumerate(meta["smpl_dims"].items())}
    tokens = gen.rnd(meta["img_tokens_seed"], *meta["img_tokens_shape"]).cuda()
    cam = {"intrinsic": torch.zeros(B, 1, 3, 3).cuda(), "extrinsic": torch.zeros(B, 1, 4, 4).cuda()}
    R, C = meta["cfg"]["triplane_resolution"], meta["cfg"]["triplane_feature_dim"]
    fine = []
    enc.triplane_downsampler.register_forward_pre_hook(lambda module, args: fine.append(args[0]))
    with torch.no_grad():
        planes, _, _ = enc(cam, tokens, gt, None)
        assert planes.shape == (B, 1, 3, C, R, R) and enc.triplane_resolution == R
        # the 3R x 3R planes handed to the downsampler: the cell indexing at 3x resolution (channels-last here)
        close(fine[0].permute(0, 3, 1, 2).reshape(B, 3, C, 3 * R, 3 * R), a["planes_fine"], SPLIT_GEMM_BOUND, "fine planes")
        close(planes, a["planes"], SPLIT_GEMM_BOUND, "geometry planes")
        # any number of frames: T = 2 with the frames flattened equals the two batch items
        gt2 = {k: v.reshape(1, B, *v.shape[2:]) for k, v in gt.items()}
        cam2 = {k: v.reshape(1, B, *v.shape[2:]) for k, v in cam.items()}
        planes2, _, _ = enc(cam2, tokens.reshape(1, B, *tokens.shape[2:]), gt2, None)
        assert torch.equal(planes2.reshape(planes.shape), planes)


def test_cell_kernels_at_96_squared_cells():
    """cell_pool_max / cell_splat_mean take any `cells`: the reference's 96^2 against the scatter restatements."""
    from audio_motion_avatar_amd import ops
    from oracle import triplane_net as o_tn

    g = torch.Generator().manual_seed(3)
    B, N, C, R = 1, 3000, 16, 96
    feat = torch.randn(B, N, C, generator=g)
    verts = torch.randn(B, N, 3, generator=g) * 0.6
    index = o_tn.cell_indices(verts, 1.4, R)
    cell_of = torch.stack([index[k][:, 0] for k in ("xy", "xz", "yz")], dim=1).to(torch.int32)
    assert int(cell_of.max()) > 32 * 32
    assert torch.equal(ops.cell_pool_max(feat.cuda(), cell_of.cuda(), R * R).cpu(), o_tn.pool_local(index, feat, R))
    want = o_tn.scatter_mean(feat.permute(0, 2, 1), index["xz"], R * R)
    close(ops.cell_splat_mean(feat.cuda(), cell_of[:, 1].contiguous().cuda(), R * R), want, 1e-6, "scatter_mean at 96^2")


def _training_cfg():
    from audio_motion_avatar_amd.config import Stage1Config

    return Stage1Config(image_size=(64, 48), subdivide_steps=0, smplx_transformer_layers=1, cross_transformer_layers=1,
                        upsample_triplane=True, num_upsample_blocks=1, differentiable_upsampler=True, device="cuda")


def test_training_step_reaches_the_downsampler_and_is_deterministic():
    from test_stage1_training_gpu import _inputs, _model

    cfg = _training_cfg()
    model = _model(cfg)
    ref, smpl, cam, tokens, test, test_cam = _inputs(cfg, 1, 2, seed=4)
    runs = []
    for _ in range(2):
        model.zero_grad(set_to_none=True)
        total, _ = model.training_step(ref, smpl, cam, tokens, test, test_cam)
        total.backward()
        runs.append({n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})
    assert bool(torch.isfinite(total))
    wanted = [n for n, _ in model.named_parameters() if ".triplane_downsampler." in n]
    assert len(wanted) == 18
    for n in wanted + ["smplx_triplane_encoder.vertex_emb.weight", "smplx_triplane_encoder.fc_pos.weight",
                       "image_feature.feature_reducer.weight"]:
        grad = runs[0].get(n)
        assert grad is not None and bool(torch.isfinite(grad).all()) and bool(grad.any()), n
    assert runs[0].keys() == runs[1].keys()
    # bit-equal between the two runs: everything but the renderer's upsampler weights, whose gradients come from the
    # library's convolution backward at this configuration (upsample_conv_grad="library")
    checked = [n for n in runs[0] if not n.startswith("renderer.triplane_upsampler.")]
    assert set(wanted) < set(checked) and "smplx_triplane_encoder.vertex_emb.weight" in checked
    differ = [n for n in checked if not torch.equal(runs[0][n], runs[1][n])]
    assert not differ, f"gradients differ between two runs in .eval(): {differ}"
    # the forward runs without autograd too, at the reference's output shape
    with torch.no_grad():
        fused = model(ref, smpl, cam, image_tokens=tokens)[2]
    assert fused.shape == (1, 2, 256, 3 * 32 * 32) and bool(torch.isfinite(fused).all())
    # a reference-named state_dict round-trips through load_state_dict(strict=True)
    sd = model.state_dict()
    assert "smplx_triplane_encoder.triplane_downsampler.down.weight" in sd
    model.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)


def _grads(ds, leaf):
    return dict([("input", leaf.grad)] + [(n, q.grad.clone()) for n, q in ds.named_parameters()])


def test_more_than_one_pass_is_the_concatenation_of_its_passes(monkeypatch):
    """C = 64, factor 3, nine frames of 6 x 6 planes: K = 27 planes, so forward_planes cuts at 3 * 8 = 24.  The output, and
    under autograd the input gradient, equal the module applied to frames 0-7 and to frame 8 on their own bit for bit;
    the parameter gradients (sums over both passes) meet the `dmodule` bound against fp64 autograd of the restatement."""
    from audio_motion_avatar_amd import triplane_net

    frames, cut = 9, 3 * triplane_net.DOWNSAMPLER_FRAMES_PER_PASS
    p, x, want = dc.module_case(C=64, R=2, factor=3, frames=frames)
    assert x.shape == (27, 6, 6, 64) and cut == 24 < x.shape[0]
    ds = _module(dict(triplane_feature_dim=64, upsample_factor=3), {k: list(v.shape) for k, v in p.items()},
                 "triplane_downsampler.")
    monkeypatch.setenv("AMAV_GEMM", "f32")
    xc = x.cuda()
    passes, real = [], ds.blocks[0].forward_planes

    def counted(part, *a, **k):
        passes.append(part.shape[0])
        return real(part, *a, **k)

    monkeypatch.setattr(ds.blocks[0], "forward_planes", counted)
    with torch.no_grad():
        y = ds(xc)
        assert passes == [24, 3]
        parts = [ds(xc[:cut].contiguous()), ds(xc[cut:].contiguous())]
    assert y.shape == (27, 2, 2, 64) and torch.equal(y, torch.cat(parts))
    _check("block", y, want[2], "hip, two passes")
    # the reference's layout splits at the same frame
    with torch.no_grad():
        x5 = xc.view(frames, 3, 6, 6, 64).permute(0, 1, 4, 2, 3)
        assert torch.equal(dc.planes_of(ds(x5)), y)
    g = dc.randn(42, *want[2].shape)
    want_grads = dc.module_grads(dc.to(p, torch.float64), x, g)
    gc = g.cuda()
    leaf = xc.clone().requires_grad_(True)
    ds.zero_grad(set_to_none=True)
    del passes[:]
    out = ds(leaf)
    assert passes == [24, 3] and torch.equal(out.detach(), y)
    out.backward(gc)
    got = _grads(ds, leaf)
    halves = []
    for part, gpart in ((xc[:cut], gc[:cut]), (xc[cut:], gc[cut:])):
        part_leaf = part.clone().requires_grad_(True)
        ds.zero_grad(set_to_none=True)
        ds(part_leaf).backward(gpart.contiguous())
        halves.append(part_leaf.grad)
    assert torch.equal(got["input"], torch.cat(halves))
    assert set(got) == set(want_grads)
    for k in want_grads:
        _check("dmodule", got[k], want_grads[k], f"hip, two passes, d {k}")


def test_a_width_the_kernels_are_not_built_for_takes_the_library(monkeypatch):
    """C = 32: ops.dwconv7_channels_ok refuses it, the module evaluates the library's operators on the GPU and meets the
    `block` bound; none of the downsampler's kernels is called."""
    from audio_motion_avatar_amd import ops

    p, x, want = dc.module_case(C=32, R=4, factor=3)
    ds = _module(dict(triplane_feature_dim=32, upsample_factor=3), {k: list(v.shape) for k, v in p.items()},
                 "triplane_downsampler.")
    assert not ops.dwconv7_channels_ok(32) and not ds._hip(x.cuda())

    def refuse(*a, **k):
        raise AssertionError("a HIP kernel of the downsampler ran at C = 32")

    for name in ("dwconv7_layernorm", "dwconv7_layernorm_differentiable", "gelu_bias", "gelu_bias_differentiable",
                 "patch4_gather", "patch4_gather_differentiable"):
        monkeypatch.setattr(ops, name, refuse)
    monkeypatch.setenv("AMAV_GEMM", "f32")
    with torch.no_grad():
        y = ds(x.cuda())
    assert y.shape == want[2].shape == (3, 4, 4, 32)
    _check("block", y, want[2], "library path on the GPU, C = 32")
