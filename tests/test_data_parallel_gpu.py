"""optim.Adam(process_group=...) end to end: two processes on the one GPU over gloo (RCCL needs a GPU per rank) against
a one-process emulation of the same data-parallel step, bit for bit; the participation rule; the gradients zeroed in
the pack; the library backend behind the same collective; dist.broadcast_module; two iterations of the stage-2 model;
and one rank over RCCL, where step() must not wait for the device.

The two ranks run every scenario in one pair of processes (module-scoped fixture: a process pays the imports and the
code objects once) and hand back plain flags; every test below asserts the flags of its own scenario on both ranks."""
import datetime
import os
import socket
import traceback

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import optimizer_cases as oc

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 63, 64, 65, 3 * 64 + 5, 12293)   # tests/test_grad_bucket_gpu.py's, without the empty tensor
GROUP_OF = (0, 1, 0, 1, 0, 1, 0)
LRS = (1e-3, 3e-4)
STEPS = 3


# ---- what both kinds of worker share ---------------------------------------------------------------------------------
def _start(n):
    g = torch.Generator().manual_seed(77)
    return [torch.randn(k, generator=g) for k in n]


def _rank_grads(rank, step, sizes=SIZES):
    """The gradients rank `rank` contributes to step `step`: every process can form every rank's."""
    g = torch.Generator().manual_seed(1000 * rank + step + 1)
    return [torch.randn(k, generator=g).cuda() for k in sizes]


def _optimizer(params, group_of=GROUP_OF, **kw):
    from audio_motion_avatar_amd import optim

    groups = [dict(params=[p for p, g in zip(params, group_of) if g == gi], lr=lr) for gi, lr in enumerate(LRS)]
    opt = optim.Adam([g for g in groups if g["params"]], **kw)
    return opt, torch.optim.lr_scheduler.LinearLR(opt, start_factor=1.0, end_factor=0.01, total_iters=10)


def _snapshot(params, opt):
    out = [p.detach().clone() for p in params]
    out += [opt.state[p]["exp_avg"].clone() for p in params] + [opt.state[p]["exp_avg_sq"].clone() for p in params]
    return out + [opt.grad_norm.clone().reshape(1)]


def _bits_equal(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32))
                                    for x, y in zip(a, b))


def _same_on_every_rank(tensors):
    flat = torch.cat([t.detach().reshape(-1).to(torch.float64) if t.dtype != torch.float32 else
                      t.detach().reshape(-1).view(torch.int32).to(torch.float64) for t in tensors])
    rows = torch.empty(dist.get_world_size(), flat.numel(), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    dist.all_gather_into_tensor(rows.view(-1), flat)
    return bool((rows == rows[0]).all())


def _run_assigned(world, rank, group, zero_in_step=False, steps=STEPS):
    """`steps` data-parallel steps on SIZES with assigned gradients, next to a shadow that a plain optim.Adam steps on
    0.5 g0 + 0.5 g1 -> (params, optimizer, per step: snapshot, per step: shadow's snapshot, flags)."""
    params = [torch.nn.Parameter(t.cuda()) for t in _start(SIZES)]
    shadow = [torch.nn.Parameter(t.cuda()) for t in _start(SIZES)]
    opt, sched = _optimizer(params, process_group=group, zero_grads_in_step=zero_in_step)
    shadow_opt, shadow_sched = _optimizer(shadow)
    mine, theirs, flags = [], [], {}
    half = torch.tensor(0.5)
    for step in range(steps):
        per_rank = [_rank_grads(r, step) for r in range(world)]
        for p, g in zip(params, per_rank[rank]):
            p.grad = g.clone()
        held = [p.grad for p in params]
        opt.step()
        sched.step()
        if zero_in_step:
            flags["gradients are zero"] = flags.get("gradients are zero", True) and all(
                p.grad is g and int(torch.count_nonzero(g)) == 0 for p, g in zip(params, held))
            versions = [g._version for g in held]
            opt.zero_grad(set_to_none=False)
            flags["zero_grad had nothing to do"] = (flags.get("zero_grad had nothing to do", True)
                                                    and versions == [g._version for g in held])
        for p, g0, g1 in zip(shadow, *per_rank):                             # world == 2: one possible rounding
            p.grad = half * g0 + half * g1
        shadow_opt.step()
        shadow_sched.step()
        mine.append(_snapshot(params, opt))
        theirs.append(_snapshot(shadow, shadow_opt))
    return params, opt, mine, theirs, flags


# ---- the scenarios of the two gloo ranks -----------------------------------------------------------------------------
def _assigned(world, rank, group, keep):
    params, opt, mine, theirs, _ = _run_assigned(world, rank, group)
    keep["assigned"] = mine
    flags = {"equals the emulation": all(_bits_equal(a, b) for a, b in zip(mine, theirs)),
             "equal between ranks": _same_on_every_rank(mine[-1]),
             "moved": not torch.equal(mine[0][0], mine[-1][0]),
             "clip active": float(mine[-1][-1]) > 1.0,
             "lr scheduled": opt.param_groups[0]["lr"] == pytest.approx(LRS[0] * (1 - 0.99 * STEPS / 10)),
             "step counts": all(float(opt.state[p]["step"]) == STEPS for p in params),
             "in sync": opt.replicas_in_sync()}
    if rank == 1:
        with torch.no_grad():
            params[-1][100] += 1e-3
    flags["out of sync after one element moved"] = not opt.replicas_in_sync()
    return flags


def _unused(world, rank, group, keep):
    sizes, group_of = (65, 3 * 64 + 5, 64), (0, 1, 0)
    params = [torch.nn.Parameter(t.cuda()) for t in _start(sizes)]
    shadow = [torch.nn.Parameter(t.cuda()) for t in _start(sizes)]
    opt, _ = _optimizer(params, group_of, process_group=group)
    shadow_opt, _ = _optimizer(shadow, group_of)
    per_rank = [_rank_grads(r, 0, sizes) for r in range(world)]
    per_rank[1][1] = None                                                    # rank 1 did not use parameter 1
    for r in range(world):
        per_rank[r][2] = None                                                # nobody used parameter 2
    for p, g in zip(params, per_rank[rank]):
        p.grad = g
    opt.step()
    half = torch.tensor(0.5)
    for p, g0, g1 in zip(shadow, *per_rank):
        zero = torch.zeros_like(p)
        p.grad = half * (zero if g0 is None else g0) + half * (zero if g1 is None else g1)
    shadow_opt.step()
    start = _start(sizes)
    state = opt.state[params[2]]
    return {"equals the emulation": _bits_equal(_snapshot(params, opt), _snapshot(shadow, shadow_opt)),
            "equal between ranks": _same_on_every_rank(_snapshot(params, opt)),
            "used parameters moved": all(not torch.equal(p.detach().cpu(), s) for p, s in zip(params[:2], start)),
            "unused parameter kept its bits": torch.equal(params[2].detach().cpu(), start[2]),
            "unused parameter has state": float(state["step"]) == 1 and state["exp_avg"].shape == params[2].shape
                                          and int(torch.count_nonzero(state["exp_avg"])) == 0
                                          and int(torch.count_nonzero(state["exp_avg_sq"])) == 0,
            "its gradient stayed None": params[2].grad is None,
            "in sync": opt.replicas_in_sync()}


def _zeroed_in_step(world, rank, group, keep):
    _, _, mine, theirs, flags = _run_assigned(world, rank, group, zero_in_step=True, steps=2)
    flags["same bits as without"] = all(_bits_equal(a, b) for a, b in zip(mine, keep["assigned"]))
    flags["equals the emulation"] = all(_bits_equal(a, b) for a, b in zip(mine, theirs))
    return flags


def _library(world, rank, group, keep):
    """backend="library" behind the collective, on gradients whose average is exactly oc.COVERAGE's: rank 0 holds 2 g
    at the even elements and 0 at the odd ones, rank 1 the complement.  The yardstick is optimizer_cases' own."""
    from audio_motion_avatar_amd import optim

    case = oc.COVERAGE
    p0, grads = oc.inputs(case)
    params = [torch.nn.Parameter(t.cuda()) for t in p0]
    groups = [dict(params=[p for p, g in zip(params, case.group_of) if g == gi], lr=lr, betas=betas, eps=eps, weight_decay=wd)
              for gi, (lr, betas, eps, wd) in enumerate(case.hypers)]
    opt = optim.Adam(groups, max_grad_norm=case.max_norm, backend="library", process_group=group)
    run, norms = [], []
    for step in range(case.steps):
        for p, g in zip(params, grads[step]):
            share = 2.0 * g
            share[(1 - rank)::2] = 0.0
            p.grad = share.cuda()
        opt.step()
        run.append(dict(p=[p.detach().cpu().clone() for p in params], m=[opt.state[p]["exp_avg"].cpu().clone() for p in params],
                        v=[opt.state[p]["exp_avg_sq"].cpu().clone() for p in params]))
        norms.append(float(opt.grad_norm))
    oracle, _ = oc.reference(case)
    try:
        worst = oc.check_against_oracle(case, run, f"library/data-parallel rank {rank}")
    except AssertionError as e:
        worst = f"outside the yardstick: {e}"
    norm_error = max(abs(n - float(o["norm"])) / float(o["norm"]) for n, o in zip(norms, oracle))
    return {"within the yardstick": worst if isinstance(worst, str) else worst <= oc.FACTOR,
            "norm of the averaged gradient": norm_error <= oc.NORM_BOUND,
            "equal between ranks": _same_on_every_rank([p for p in params])}


def _broadcast(world, rank, group, keep):
    from audio_motion_avatar_amd.dist import broadcast_module

    torch.manual_seed(100 + rank)
    net = torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.BatchNorm1d(16), torch.nn.Linear(16, 4))
    with torch.no_grad():
        net[1].running_mean.normal_()
        net[1].running_var.uniform_(0.5, 2.0)
        net[1].num_batches_tracked.fill_(3 + rank)
    net = net.cuda()
    tensors = list(net.parameters()) + list(net.buffers())
    differed = not _same_on_every_rank(tensors)
    mine_before = [t.detach().clone() for t in tensors]
    versions = [t._version for t in tensors]
    returned = broadcast_module(net, src=0)
    flags = {"replicas differed before": differed, "returns the module": returned is net,
             "equal to rank 0 afterwards": _same_on_every_rank(tensors),
             "rank 0 kept its values": rank != 0 or all(torch.equal(a, b) for a, b in zip(mine_before, tensors)),
             "every version moved": all(t._version > v for t, v in zip(tensors, versions)), "buffers": len(list(net.buffers())) == 3}
    # buffers=False leaves the buffers alone
    with torch.no_grad():
        net[1].running_mean.fill_(float(rank))
        net[0].bias.fill_(float(rank))
    broadcast_module(net, src=0, buffers=False)
    flags["buffers=False"] = float(net[1].running_mean[0]) == rank and float(net[0].bias.detach()[0]) == 0.0
    return flags


def _real_step(world, rank, group, keep):
    """AudioDrivenAvatar at the small config: two data-parallel iterations, each rank on its own window."""
    from audio_motion_avatar_amd.dist import broadcast_module
    from test_audio_net_training_gpu import _stage2_batch, _stage2_model

    def build():
        torch.manual_seed(4242)   # the modules _stage2_model leaves at their default initialisation
        return _stage2_model(seed=1)

    def train(model, window, process_group):
        tri, st, audio, cam, smpl = _stage2_batch(model, window)
        target = torch.full((1, 3, 3, 64, 64), 0.5, device="cuda")
        opt, sched = model.configure_optimizers(lr=1e-3, total_steps=100, process_group=process_group)
        for _ in range(2):
            opt.zero_grad()
            loss, _ = model.training_step(tri, st, audio, cam, target, smpl)
            loss.backward()
            opt.step()
            sched.step()
        return opt

    model = broadcast_module(build(), src=0)
    initial = {k: v.detach().clone() for k, v in model.state_dict().items()}
    opt = train(model, 9 + rank, group)
    used = {k for k, p in model.named_parameters() if p.grad is not None}
    names = [next(k for k, _ in model.named_parameters() if k.startswith(prefix) and k in used)
             for prefix in ("audio_triplane.transformer.", "renderer.gaussian_decoder.", "smpl_decoder.")]
    mine = dict(model.named_parameters())
    alone = build()
    alone.load_state_dict(initial)
    train(alone, 9, None)                                                    # rank 0's window, nobody else's gradient
    solo = dict(alone.named_parameters())
    unused = [k for k, p in model.named_parameters() if p.requires_grad and p.grad is None]
    return {"in sync": opt.replicas_in_sync(), "three named parameters": len(set(names)) == 3,
            "equal between ranks": _same_on_every_rank([mine[k] for k in names]),
            "moved": all(not torch.equal(mine[k], initial[k]) for k in names),
            "the other rank's gradient arrived": all(not torch.equal(mine[k], solo[k]) for k in names),
            "unused parameters kept their bits": len(unused) > 0 and all(torch.equal(mine[k], initial[k]) for k in unused),
            "finite": all(bool(torch.isfinite(p).all()) for p in model.parameters())}


SCENARIOS = {"assigned": _assigned, "unused": _unused, "zeroed": _zeroed_in_step, "library": _library,
             "broadcast": _broadcast, "real": _real_step}


def _worker(rank, world, port, out):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=240))
        try:
            group, keep, flags = dist.group.WORLD, {}, {}
            for name, scenario in SCENARIOS.items():
                flags[name] = scenario(world, rank, group, keep)
            gathered = [None] * world
            dist.all_gather_object(gathered, flags)
            if rank == 0:
                out.put(("flags", gathered))
            dist.barrier()
        finally:
            dist.destroy_process_group()
    except BaseException:
        out.put(("error", f"rank {rank}:\n{traceback.format_exc()}"))
        raise


def _spawn(target, world):
    """Run `target(rank, world, port, queue)` in `world` fresh processes -> what rank 0 put on the queue.  The first
    message decides: a rank that fails says so at once, and nobody waits for a time limit."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=target, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    kind, payload = "error", "no rank reported within the time limit"
    try:
        kind, payload = q.get(timeout=600)
    finally:
        for p in procs:
            p.join(timeout=60 if kind == "flags" else 5)
        for p in procs:
            if p.is_alive():
                p.kill()
    assert kind == "flags", payload
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    return payload


@pytest.fixture(scope="module")
def two_ranks():
    return _spawn(_worker, 2)


def _all_true(two_ranks, scenario, expected):
    for rank, flags in enumerate(two_ranks):
        print(f"rank {rank}: {flags[scenario]}")
        assert set(flags[scenario]) == set(expected), rank
        assert all(v is True for v in flags[scenario].values()), (rank, flags[scenario])


def test_assigned_gradients_equal_the_one_process_emulation(two_ranks):
    """Seven parameters in two groups, three steps under LinearLR, rank r's gradients seeded by (r, step): parameters,
    both moments and grad_norm equal, bit for bit, a plain optim.Adam stepped on 0.5 g0 + 0.5 g1, and each other;
    replicas_in_sync() sees it, and sees one moved element."""
    _all_true(two_ranks, "assigned", ["equals the emulation", "equal between ranks", "moved", "clip active", "lr scheduled",
                                      "step counts", "in sync", "out of sync after one element moved"])


def test_unused_parameters_take_part(two_ranks):
    _all_true(two_ranks, "unused", ["equals the emulation", "equal between ranks", "used parameters moved",
                                    "unused parameter kept its bits", "unused parameter has state", "its gradient stayed None",
                                    "in sync"])


def test_gradients_zeroed_in_the_pack(two_ranks):
    _all_true(two_ranks, "zeroed", ["gradients are zero", "zero_grad had nothing to do", "same bits as without",
                                    "equals the emulation"])


def test_library_backend_behind_the_collective(two_ranks):
    _all_true(two_ranks, "library", ["within the yardstick", "norm of the averaged gradient", "equal between ranks"])


def test_broadcast_module(two_ranks):
    _all_true(two_ranks, "broadcast", ["replicas differed before", "returns the module", "equal to rank 0 afterwards",
                                       "rank 0 kept its values", "every version moved", "buffers", "buffers=False"])


def test_two_iterations_of_the_stage2_model(two_ranks):
    _all_true(two_ranks, "real", ["in sync", "three named parameters", "equal between ranks", "moved",
                                  "the other rank's gradient arrived", "unused parameters kept their bits", "finite"])


# ---- one rank over RCCL ----------------------------------------------------------------------------------------------
def _rccl_worker(rank, world, port, out):
    try:
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
                                timeout=datetime.timedelta(seconds=240))
        try:
            group = dist.group.WORLD
            warm = torch.ones(4, device="cuda")
            dist.all_reduce(warm)                                            # the communicator is built in the first call
            torch.cuda.synchronize()
            with_group = [torch.nn.Parameter(t.cuda()) for t in _start(SIZES)]
            without = [torch.nn.Parameter(t.cuda()) for t in _start(SIZES)]
            a, a_sched = _optimizer(with_group, process_group=group)
            b, b_sched = _optimizer(without)
            equal = True
            for step in range(STEPS):
                for p, q, g in zip(with_group, without, _rank_grads(0, step)):
                    p.grad, q.grad = g.clone(), g.clone()
                for each in (a, a_sched, b, b_sched):
                    each.step()
                equal = equal and _bits_equal(_snapshot(with_group, a), _snapshot(without, b))
            flags = {"a group of one equals no group": equal, "in sync": a.replicas_in_sync()}
            # step() returns before the device is idle: 2e7 elements, 0.8 GB of traffic per step
            big = [torch.nn.Parameter(torch.zeros(5_000_000, device="cuda")) for _ in range(4)]
            opt, _ = _optimizer(big, (0, 1, 0, 1), process_group=group)
            grads = [torch.randn(5_000_000, device="cuda") for _ in big]
            pending = []
            for _ in range(3):
                for p, g in zip(big, grads):
                    p.grad = g
                torch.cuda.synchronize()
                opt.step()
                done = torch.cuda.Event()
                done.record()
                pending.append(not done.query())
            torch.cuda.synchronize()
            print(f"step() returned with device work pending: {pending}")
            flags["step() returned before the device was idle"] = any(pending)
            flags["the big set moved"] = all(float(p.detach().abs().max()) > 0 for p in big)
            out.put(("flags", [flags]))
        finally:
            dist.destroy_process_group()
    except BaseException:
        out.put(("error", f"rank {rank}:\n{traceback.format_exc()}"))
        raise


@pytest.mark.skipif(not dist.is_nccl_available(), reason="torch.distributed was built without RCCL")
def test_one_rank_over_rccl():
    """backend "nccl", world size 1, in a child of its own: three steps with the group equal three steps without one bit
    for bit (scale 1, a sum over one rank), and step() enqueues: an event recorded right after it has not completed at
    least once in three steps over 2e7 elements."""
    (flags,) = _spawn(_rccl_worker, 1)
    print(flags)
    assert set(flags) == {"a group of one equals no group", "in sync", "step() returned before the device was idle",
                          "the big set moved"}
    assert all(v is True for v in flags.values()), flags
