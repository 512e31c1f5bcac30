"""optim.Adam and configure_optimizers on the GPU: the trajectory against the library's, torch.optim.Adam's semantics
(missing gradients, lazy state, re-allocated gradients, state_dict round trip, LinearLR), the version counters that the
package's weight caches are keyed on, the stage-2 model end to end, and the AMAV_OPTIMIZER switch."""
import copy
import os
import subprocess
import sys

import pytest
import torch

import optimizer_cases as oc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP = float(torch.finfo(torch.float32).eps)


def _mlp(dtype=torch.float32, device="cuda"):
    g = torch.Generator().manual_seed(5)
    net = torch.nn.Sequential(torch.nn.Linear(32, 64), torch.nn.Tanh(), torch.nn.Linear(64, 8))
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.3)
    x, y = torch.randn(64, 32, generator=g), torch.randn(64, 8, generator=g)
    return net.to(device=device, dtype=dtype), x.to(device=device, dtype=dtype), y.to(device=device, dtype=dtype)


def _fit(make_optimizer, steps=10, dtype=torch.float32, device="cuda", zero=lambda opt: opt.zero_grad()):
    """`steps` of MSE descent on the MLP -> [per step: the parameters (CPU clones)]."""
    net, x, y = _mlp(dtype, device)
    opt = make_optimizer(list(net.parameters()))
    trace = []
    for _ in range(steps):
        zero(opt)
        torch.nn.functional.mse_loss(net(x), y).backward()
        opt.step()
        trace.append([p.detach().cpu().clone() for p in net.parameters()])
    return trace


def _library_cpu(dtype):
    def make(params):
        opt = torch.optim.Adam(params, lr=1e-2, foreach=False)
        inner = opt.step
        opt.step = lambda: (torch.nn.utils.clip_grad_norm_(params, 1.0, foreach=False), inner())[1]
        return opt
    return _fit(make, dtype=dtype, device="cpu")


def test_trajectory_against_the_library():
    """10 steps of the MLP: hip against library on the GPU, per tensor within 4 x the distance between the library's
    fp32 and fp64 trajectories on the CPU; grad_norm within 2^-17 of the fp64 norm of the gradients it was taken from."""
    from audio_motion_avatar_amd import optim

    hip = _fit(lambda ps: optim.Adam(ps, lr=1e-2, backend="hip"))
    library = _fit(lambda ps: optim.Adam(ps, lr=1e-2, backend="library"))
    lib32, lib64 = _library_cpu(torch.float32), _library_cpu(torch.float64)
    for i in range(len(hip[0])):
        yard = max(float((a[i].double() - b[i]).abs().max()) for a, b in zip(lib32, lib64))
        diff = max(float((a[i] - b[i]).abs().max()) for a, b in zip(hip, library))
        print(f"tensor {i}: hip - library {diff:.3e}, library fp32 - fp64 {yard:.3e}, ratio {diff / yard:.2f}")
        assert diff <= oc.FACTOR * yard, (i, diff, yard)
    assert not torch.equal(hip[0][0], hip[-1][0])

    # grad_norm, read after every step
    net, x, y = _mlp()
    opt = optim.Adam(net.parameters(), lr=1e-2)
    for _ in range(3):
        opt.zero_grad()
        torch.nn.functional.mse_loss(net(x), y).backward()
        want = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in net.parameters())))
        opt.step()
        assert opt.grad_norm.dim() == 0 and opt.grad_norm.is_cuda
        rel = abs(float(opt.grad_norm.double()) - want) / want
        print(f"grad_norm {float(opt.grad_norm):.6e}, relative error {rel:.2e}")
        assert rel <= oc.NORM_BOUND


def _three(seed=1):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(n, generator=g).cuda()) for n in (65, 130, 4097)]


def _grads(params, seed, skip=()):
    g = torch.Generator().manual_seed(seed)
    for i, p in enumerate(params):
        grad = torch.randn(p.shape, generator=g).cuda()
        p.grad = None if i in skip else grad


def _close(a, b):
    """Two fp32 evaluations of the same update: each rounds the parameter once, so they agree to 2 ulp of its size."""
    return float((a - b).abs().max()) <= 2 * ULP * max(1.0, float(a.abs().max()))


def test_a_parameter_without_gradient_is_left_alone():
    from audio_motion_avatar_amd import optim

    runs = {}
    for backend in optim.BACKENDS:
        params = _three()
        opt = optim.Adam(params, lr=1e-3, backend=backend)
        before = params[2].detach().clone()
        _grads(params, 10, skip=(2,))
        want = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in params[:2])))   # the library clips in place
        opt.step()
        assert abs(float(opt.grad_norm) - want) / want <= oc.NORM_BOUND            # the norm is over the two gradients
        assert torch.equal(params[2], before) and params[2] not in opt.state
        assert all(float(opt.state[p]["step"]) == 1 for p in params[:2])
        _grads(params, 11)
        opt.step()
        assert [float(opt.state[p]["step"]) for p in params] == [2, 2, 1]          # its own bias corrections
        assert opt.state[params[2]]["exp_avg"].shape == params[2].shape
        assert not torch.equal(params[2], before)
        runs[backend] = [p.detach().clone() for p in params]
    assert all(_close(a, b) for a, b in zip(runs["hip"], runs["library"]))


def test_without_a_clip_and_with_a_strided_gradient():
    """max_grad_norm=None: no norm is taken and the step is the library's unclipped Adam; a gradient that is a transposed
    view is made contiguous first and gives the bits of the contiguous one."""
    from audio_motion_avatar_amd import optim

    g = torch.Generator().manual_seed(2)
    start, grad = torch.randn(24, 40, generator=g), torch.randn(40, 24, generator=g)
    results = []
    for backend, strided in (("hip", True), ("hip", False), ("library", False)):
        p = torch.nn.Parameter(start.clone().cuda())
        opt = optim.Adam([p], lr=1e-2, max_grad_norm=None, backend=backend)
        for _ in range(2):
            p.grad = grad.cuda().t() if strided else grad.t().contiguous().cuda()
            assert p.grad.is_contiguous() != strided
            opt.step()
        assert opt.grad_norm is None
        results.append(p.detach().clone())
    assert torch.equal(results[0], results[1])
    assert _close(results[1], results[2])
    assert float((results[1] - start.cuda()).abs().min()) > 1e-2          # unclipped: every element moved by about lr per step


def test_non_finite_gradients_propagate_like_the_library():
    """One infinite gradient element: the norm is inf, the coefficient 0, that element's update NaN and every other
    element's 0 -- in both backends; nothing is skipped."""
    from audio_motion_avatar_amd import optim

    for backend in optim.BACKENDS:
        params = _three()
        before = [p.detach().clone() for p in params]
        opt = optim.Adam(params, lr=1e-3, backend=backend)
        _grads(params, 4)
        params[1].grad[7] = float("inf")
        opt.step()
        assert torch.isinf(opt.grad_norm)
        nan = [torch.isnan(p) for p in params]
        assert [int(n.sum()) for n in nan] == [0, 1, 0] and bool(nan[1][7])
        assert all(torch.equal(p[~n], b[~n]) for p, b, n in zip(params, before, nan))


def test_reallocated_gradients_and_gradients_zeroed_in_place_agree(monkeypatch):
    from audio_motion_avatar_amd import ops, optim

    uploads = []
    upload = ops.optimizer_table_to_device
    monkeypatch.setattr(ops, "optimizer_table_to_device", lambda *a: uploads.append(1) or upload(*a))
    make = lambda ps: optim.Adam(ps, lr=1e-2)                                       # noqa: E731
    fresh = _fit(make, steps=4)
    uploads.clear()
    kept = _fit(make, steps=4, zero=lambda opt: opt.zero_grad(set_to_none=False))
    assert len(uploads) == 2          # gradients that stay where they are: the two tables are uploaded once
    in_step = _fit(lambda ps: optim.Adam(ps, lr=1e-2, zero_grads_in_step=True), steps=4,
                   zero=lambda opt: opt.zero_grad(set_to_none=False))
    for a, b, c in zip(fresh, kept, in_step):
        assert all(torch.equal(x, y) and torch.equal(x, z) for x, y, z in zip(a, b, c))


def test_gradients_zeroed_in_the_step():
    from audio_motion_avatar_amd import optim

    params = _three()
    opt = optim.Adam(params, lr=1e-3, zero_grads_in_step=True)
    _grads(params, 3)
    grads = [p.grad for p in params]
    versions = [g._version for g in grads]
    opt.step()
    assert all(p.grad is g and bool((g == 0).all()) for p, g in zip(params, grads))
    assert all(g._version > v for g, v in zip(grads, versions))
    stamp = [g._version for g in grads]
    opt.zero_grad(set_to_none=False)                       # nothing left to do
    assert [g._version for g in grads] == stamp
    for g in grads:
        g.normal_()
    opt.step()
    grads[1].add_(1.0)                                     # something wrote a gradient after the step
    opt.zero_grad(set_to_none=False)
    assert all(bool((g == 0).all()) for g in grads)
    loss = opt.step(lambda: torch.tensor(3.0))
    assert float(loss) == 3.0


def test_constructor_names_the_offending_parameter():
    from audio_motion_avatar_amd import optim

    good = torch.nn.Parameter(torch.zeros(8, device="cuda"))
    with pytest.raises(ValueError, match="parameter 1"):
        optim.Adam([good, torch.nn.Parameter(torch.zeros(8, device="cuda", dtype=torch.float64))])
    with pytest.raises(ValueError, match="parameter 2"):
        optim.Adam([{"params": [good, torch.nn.Parameter(torch.zeros(8, device="cuda"))]},
                    {"params": [torch.nn.Parameter(torch.zeros(4, 4, device="cuda").t())], "lr": 1.0}])
    with pytest.raises(ValueError, match="parameter 1"):
        optim.Adam([good, torch.nn.Parameter(torch.zeros(8))])


def test_state_dict_round_trip_through_torch_adam():
    from audio_motion_avatar_amd import optim

    def run(round_trip):
        params = _three()
        opt = optim.Adam(params, lr=1e-3, weight_decay=0.01)
        for step in range(4):
            if step == 2 and round_trip:
                theirs = torch.optim.Adam([torch.nn.Parameter(p.detach().clone()) for p in params])
                theirs.load_state_dict(copy.deepcopy(opt.state_dict()))
                assert all(torch.equal(theirs.state[q]["exp_avg_sq"], opt.state[p]["exp_avg_sq"])
                           for q, p in zip(theirs.param_groups[0]["params"], params))
                for q in theirs.param_groups[0]["params"]:                     # the loaded state is usable there
                    q.grad = torch.zeros_like(q)
                theirs_state = copy.deepcopy(theirs.state_dict())
                theirs.step()
                opt = optim.Adam(params, lr=5.0)                               # every hyper-parameter comes from the state
                opt.load_state_dict(theirs_state)
                assert opt.param_groups[0]["lr"] == 1e-3 and opt.param_groups[0]["weight_decay"] == 0.01
            _grads(params, 20 + step)
            opt.step()
        return [p.detach().clone() for p in params], opt

    (plain, _), (tripped, opt) = run(False), run(True)
    assert all(torch.equal(a, b) for a, b in zip(plain, tripped))
    assert all(float(s["step"]) == 4 and not s["step"].is_cuda for s in opt.state.values())
    assert set(opt.state_dict()["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}


def test_linear_lr_reaches_the_kernel():
    """LinearLR(1.0 -> 0.01 over 10 steps) stepped after every update: update k + 1 runs at lr (1 - 0.99 k / 10), against
    the fp64 oracle with that rate and the library's own scheduled fp32 run as the yardstick."""
    from audio_motion_avatar_amd import optim

    case = oc.SCHEDULE
    p0, grads = oc.inputs(case)
    params = [torch.nn.Parameter(t.cuda()) for t in p0]
    lr = case.hypers[0][0]
    opt = optim.Adam(params, lr=lr)
    sched = torch.optim.lr_scheduler.LinearLR(opt, start_factor=1.0, end_factor=0.01, total_iters=case.schedule_total)
    run = []
    for k in range(case.steps):
        assert opt.param_groups[0]["lr"] == pytest.approx(lr * (1 - 0.99 * k / case.schedule_total), rel=1e-12)
        for p, g in zip(params, grads[k]):
            p.grad = g.cuda()
        opt.step()
        sched.step()
        run.append(dict(p=[p.detach().cpu().clone() for p in params], m=[opt.state[p]["exp_avg"].cpu().clone() for p in params],
                        v=[opt.state[p]["exp_avg_sq"].cpu().clone() for p in params]))
    oc.check_against_oracle(case, run, "LinearLR")
    unscheduled = oc.fp64_run(oc.Case(case.numels, case.group_of, case.hypers, case.grad_scale, steps=case.steps))
    oracle, yard = oc.reference(case)
    assert float((unscheduled[-1]["p"][1] - oracle[-1]["p"][1]).abs().max()) > 100 * yard["p"][1]   # the schedule matters


def _versions(params):
    return [p._version for p in params]


def test_a_step_invalidates_the_transformer_blocks_weight_caches():
    """The test this optimizer exists for: a forward fills the block's caches of derived weights (the fused q | k | v
    weight, the split operands of the GEMMs), a step writes the parameters through raw addresses, and the next forward
    must equal, bit for bit, the forward of a fresh block that was loaded with the stepped weights."""
    from audio_motion_avatar_amd import optim
    from audio_motion_avatar_amd.transformer import BasicTransformerBlock

    def block():
        return BasicTransformerBlock(256, 4, 64, cross_attention_dim=48).cuda()

    blk = block()
    g = torch.Generator().manual_seed(6)
    x, enc = torch.randn(1, 320, 256, generator=g).cuda(), torch.randn(1, 1, 48, generator=g).cuda()
    with torch.no_grad():
        first = blk(x, enc).clone()
        assert blk.attn1._qkv is not None                                  # a cache keyed on the version counters is warm
    blk(x, enc).square().mean().backward()
    stepped = [p for p in blk.parameters() if p.grad is not None]
    assert len(stepped) < len(list(blk.parameters()))                       # norm2, attn2.to_q / to_k: no gradient
    before = _versions(stepped)
    optim.Adam(blk.parameters(), lr=1e-3).step()
    assert all(b > a for a, b in zip(before, _versions(stepped)))
    with torch.no_grad():
        second = blk(x, enc).clone()
        cold = block()
        cold.load_state_dict(blk.state_dict())
        want = cold(x, enc)
    assert torch.equal(second, want)
    assert not torch.equal(second, first)


def test_a_step_invalidates_the_renderers_packed_heads():
    from audio_motion_avatar_amd import optim
    from audio_motion_avatar_amd.config import RendererConfig
    from audio_motion_avatar_amd.renderer import Renderer
    from audio_motion_avatar_amd.synthetic import init_random_heads, make_render_inputs

    cfg = RendererConfig(image_size=(64, 64), subdivide_steps=0, predict_smplx_params=False, device="cuda",
                         triplane_feature_dim=32, triplane_resolution=8)
    r = init_random_heads(Renderer(cfg).eval())
    tokens, smpl, cam = make_render_inputs(2, cfg, seed=3)
    st = torch.zeros(1, 2, 1, 1, device="cuda")
    with torch.no_grad():
        first = r(tokens, cam, st, smpl)[0].clone()
        assert r._packed is not None
    (r(tokens, cam, st, smpl)[0] - 0.5).square().mean().backward()
    heads = list(r.gaussian_decoder.parameters())
    assert all(p.grad is not None for p in heads)
    before = _versions(heads)
    optim.Adam([p for p in r.parameters() if p.requires_grad], lr=1e-3).step()
    assert all(b > a for a, b in zip(before, _versions(heads)))
    with torch.no_grad():
        second = r(tokens, cam, st, smpl)[0].clone()
        cold = Renderer(cfg).eval()
        cold.load_state_dict(r.state_dict())
        want = cold(tokens, cam, st, smpl)[0]
    assert torch.equal(second, want)
    assert not torch.equal(second, first)


def _stage2_losses():
    from audio_motion_avatar_amd import optim
    from test_audio_net_training_gpu import _stage2_batch, _stage2_model

    torch.manual_seed(20260)   # the modules _stage2_model leaves at their default initialisation draw from this generator
    model = _stage2_model(seed=1)
    tri, st, audio, cam, smpl = _stage2_batch(model, 9)
    tf = model.audio_triplane.transformer
    start = {k: v.detach().clone() for k, v in tf.state_dict().items()}
    with torch.no_grad():
        g = torch.Generator().manual_seed(3)
        for p in tf.parameters():
            p.add_(torch.randn(p.shape, generator=g).cuda() * 0.2 * (p.abs().mean() + 1e-3))
        images, _, pred, _, _ = model.audio_triplane(audio, tri, None, cam, st)
        target_video = images.permute(0, 1, 4, 2, 3).contiguous()
        target_smpl = {k: v.detach().clone() for k, v in pred.items()}
        tf.load_state_dict(start)
    model.renderer.requires_grad_(False)
    model.smpl_decoder.requires_grad_(False)
    opt, sched = model.configure_optimizers(lr=3e-5, total_steps=100)
    assert isinstance(opt, optim.Adam) and opt.backend == "hip" and opt.max_grad_norm == 1.0
    assert isinstance(sched, torch.optim.lr_scheduler.LinearLR)
    assert (sched.start_factor, sched.end_factor, sched.total_iters) == (1.0, 0.01, 100)
    covered = [id(p) for group in opt.param_groups for p in group["params"]]
    assert sorted(covered) == sorted(id(p) for p in model.parameters() if p.requires_grad) and len(set(covered)) == len(covered)
    assert 0 < len(covered) < len(list(model.parameters()))
    losses = []
    for _ in range(5):
        opt.zero_grad()
        loss, _ = model.training_step(tri, st, audio, cam, target_video, target_smpl)
        losses.append(float(loss.detach()))
        loss.backward()
        opt.step()
        sched.step()
    losses.append(float(model.training_step(tri, st, audio, cam, target_video, target_smpl)[0].detach()))
    assert opt.param_groups[0]["lr"] == pytest.approx(3e-5 * (1 - 0.99 * 5 / 100))
    return losses


def test_configure_optimizers_trains_the_stage2_model():
    """AudioDrivenAvatar.configure_optimizers at the small config: the reference's optimizer and schedule over exactly the
    parameters that require grad; five iterations lower the stage-2 loss, and a second run gives the same losses."""
    first, second = _stage2_losses(), _stage2_losses()
    print(f"stage-2 losses {['%.6e' % x for x in first]}")
    assert first[-1] < first[0]
    assert first == second


def test_defaults_of_configure_optimizers():
    from audio_motion_avatar_amd import optim

    net = torch.nn.Linear(8, 8).cuda()
    net.bias.requires_grad_(False)
    opt, sched = optim.configure_optimizers(net)
    assert [id(p) for p in opt.param_groups[0]["params"]] == [id(net.weight)]
    assert opt.param_groups[0]["lr"] == 1e-4 and opt.param_groups[0]["betas"] == (0.9, 0.999)
    assert opt.param_groups[0]["eps"] == 1e-8 and opt.param_groups[0]["weight_decay"] == 0.0 and opt.max_grad_norm == 1.0
    assert (sched.start_factor, sched.end_factor, sched.total_iters) == (1.0, 0.01, 200000)


def test_the_environment_selects_the_library_backend(monkeypatch):
    from audio_motion_avatar_amd import optim

    monkeypatch.delenv("AMAV_OPTIMIZER", raising=False)
    assert optim.Adam(_three()).backend == "hip"
    code = ("import torch; from audio_motion_avatar_amd import optim;"
            "p = torch.nn.Parameter(torch.ones(70, device='cuda')); opt = optim.Adam([p], lr=0.5);"
            "p.grad = torch.full_like(p, 2.0); opt.step();"
            "print(opt.backend, opt._tables is None, float(opt.grad_norm), float(p[0]))")
    proc = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, AMAV_OPTIMIZER="library"), cwd=ROOT,
                          capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr
    backend, untouched, norm, value = proc.stdout.split()[-4:]
    assert (backend, untouched) == ("library", "True")                      # no table was ever built: the kernels did not run
    assert float(norm) == pytest.approx(2 * 70 ** 0.5, rel=1e-6) and float(value) == pytest.approx(0.5, abs=1e-6)
