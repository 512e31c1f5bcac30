"""The tail of the reference's two training steps as one optimizer: Lightning's clip of the global gradient norm
(trainer_factory.py:44-45: gradient_clip_val = 1.0, algorithm "norm" = torch.nn.utils.clip_grad_norm_) followed by
torch.optim.Adam (lightning_model_wrapper.py:366-382, 642-658), in three HIP launches over all parameters
(csrc/optimizer.hip).

    opt = Adam(model.parameters(), lr=1e-4)            # clips to max_grad_norm = 1.0, like the reference's Trainer
    loss.backward(); opt.step(); opt.zero_grad()
    opt.grad_norm                                      # 0-dim device tensor: the norm before the clip, never synchronised

State and state_dict() are torch.optim.Adam's ({"step", "exp_avg", "exp_avg_sq"} per parameter, created in the first
step in which the parameter has a gradient), so a checkpoint moves between the two.  The kernels write parameters
through raw addresses; step() then bumps every written tensor's version counter, which is what the package's caches of
split weights are keyed on (transformer.py, renderer.py, point_transformer.py, body_model.py).

AMAV_OPTIMIZER=library (or backend="library") runs clip_grad_norm_ and the library's Adam inside step() instead: the
comparison path of the tests and of tools/time_optimizer.py.

Data-parallel training (one process per GPU, every rank holding a replica): Adam(..., process_group=group) averages the
gradients over the group inside step() -- a fourth launch packs them into one bucket, one all-reduce, and the norm and
the update read the averaged gradient where the collective left it ("Data-parallel step").
"""
import os

import torch
import torch.distributed
from torch.optim.adam import adam as _library_adam  # the functional form behind torch.optim.Adam.step

from . import ops

BACKENDS = ("hip", "library")


def default_backend():
    """AMAV_OPTIMIZER = hip (default) | library, read when an optimizer is constructed without `backend`."""
    backend = os.environ.get("AMAV_OPTIMIZER", "hip")
    if backend not in BACKENDS:
        raise ValueError(f"AMAV_OPTIMIZER={backend!r}: expected one of {BACKENDS}")
    return backend


class Adam(torch.optim.Optimizer):
    """torch.optim.Adam behind a clip of the global L2 norm of all gradients, over every parameter group at once.

    max_grad_norm=None: no clip and no norm launches (grad_norm stays None).  zero_grads_in_step=True: the update pass
    also stores zeros to the gradients it read, and a following zero_grad(set_to_none=False) finds nothing left to do.
    Parameters: fp32, CUDA, contiguous, one device.  Not supported: amsgrad, maximize, sparse gradients, graph capture of
    step(), more than ops.OPTIM_MAX_GROUPS distinct (parameter group, step count) pairs in one step.

    process_group (a torch.distributed group, world size 1 allowed; None: the single-process step, unchanged): step()
    averages the gradients over the group before the clip, so grad_norm is the norm of the averaged gradient, which is
    what Lightning clips under DDP.  The participation rule differs from the single-process step: EVERY parameter of the
    optimizer takes part in EVERY step, whether or not it has a gradient on this rank -- the ranks must agree on the
    bucket's layout without talking to each other.  State is created for all of them in the first step; a parameter
    without a gradient here contributes zeros to the average, and one that no rank used receives a zero gradient (its
    step count advances and its moments decay; from fresh state its value does not move).  Every rank must call step()
    the same number of times, on replicas that started equal (dist.broadcast_module).
    """

    def __init__(self, params, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=1.0, backend=None,
                 zero_grads_in_step=False, process_group=None):
        if max_grad_norm is not None and not max_grad_norm >= 0.0:
            raise ValueError(f"max_grad_norm={max_grad_norm}: expected None or a value >= 0")
        backend = default_backend() if backend is None else backend
        if backend not in BACKENDS:
            raise ValueError(f"backend={backend!r}: expected one of {BACKENDS}")
        # amsgrad / maximize: torch's names, kept in the groups so that a state_dict is torch.optim.Adam's
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False))
        self.max_grad_norm, self.backend, self.zero_grads_in_step = max_grad_norm, backend, zero_grads_in_step
        self.grad_norm = None
        self._check_groups()
        device, index = None, 0
        for group in self.param_groups:
            for p in group["params"]:
                if p.dtype != torch.float32 or not p.is_cuda or not p.is_contiguous() or p.is_sparse:
                    raise ValueError(f"parameter {index}: {p.dtype} on {p.device}, contiguous={p.is_contiguous()}; "
                                     "expected a contiguous fp32 tensor on the HIP device")
                if device is not None and p.device != device:
                    raise ValueError(f"parameter {index} is on {p.device}, the ones before it on {device}")
                device, index = p.device, index + 1
        self._device = device
        self._signature = None   # what the device tables were built from
        self._tables = None      # (tensors_dev, chunks_dev, host tensors, num_chunks)
        self._partial = self._norm = None
        self._zeroed = []        # (gradient, its version) of the last step, when that step zeroed them
        self._counts = {}        # parameter -> its step count as an int: state["step"] without a tensor read per step
        self.process_group = process_group
        self._replicas = None    # the data-parallel step's bucket and tables (_Replicas), built in its first step

    def _check_groups(self):
        for i, group in enumerate(self.param_groups):
            beta1, beta2 = group["betas"]
            if group.get("amsgrad") or group.get("maximize"):
                raise ValueError(f"parameter group {i}: amsgrad and maximize are not supported")
            if not (group["lr"] >= 0.0 and group["eps"] >= 0.0 and group["weight_decay"] >= 0.0
                    and 0.0 <= beta1 < 1.0 and 0.0 <= beta2 < 1.0):
                raise ValueError(f"parameter group {i}: lr={group['lr']} betas={group['betas']} eps={group['eps']} "
                                 f"weight_decay={group['weight_decay']}")

    def __setstate__(self, state):
        """load_state_dict ends here: accept torch.optim.Adam's state, with the step counts as fp32 tensors on the host
        (its default form; a fused or capturable optimizer keeps them on the device, where reading one would wait)."""
        super().__setstate__(state)
        self._check_groups()
        for s in self.state.values():
            if "step" in s:
                step = s["step"]
                s["step"] = torch.tensor(float(step), dtype=torch.float32) if not torch.is_tensor(step) else step.float().cpu()
        self._counts = {p: int(s["step"].item()) for p, s in self.state.items() if "step" in s}
        self._signature = None
        self._replicas = None

    # ---- the step ------------------------------------------------------------------------------------------------
    def _participants(self):
        """[(group index, parameter, fp32 contiguous gradient, state)] of the parameters that have a gradient, with the
        state created where this is their first one, as torch.optim.Adam does."""
        found = []
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if g.is_sparse:
                    raise RuntimeError("optim.Adam does not support sparse gradients")
                if g.dtype != torch.float32 or not g.is_contiguous():
                    g = g.to(torch.float32).contiguous()
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = torch.tensor(0.0, dtype=torch.float32)
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    self._counts[p] = 0
                found.append((gi, p, g, state))
        return found

    def _step_library(self, found):
        for _, p, _, _ in found:
            self._counts[p] += 1
        if self.max_grad_norm is not None:
            self.grad_norm = torch.nn.utils.clip_grad_norm_([p for _, p, _, _ in found], self.max_grad_norm)
        for gi, group in enumerate(self.param_groups):
            mine = [(p, s) for i, p, _, s in found if i == gi]
            if not mine:
                continue
            _library_adam([p for p, _ in mine], [p.grad for p, _ in mine], [s["exp_avg"] for _, s in mine],
                          [s["exp_avg_sq"] for _, s in mine], [], [s["step"] for _, s in mine], amsgrad=False,
                          beta1=group["betas"][0], beta2=group["betas"][1], lr=group["lr"],
                          weight_decay=group["weight_decay"], eps=group["eps"], maximize=False)

    def _step_hip(self, found):
        # one amav_optim_group per (parameter group, step count): a parameter that got its first gradient later than
        # its group's others has its own bias corrections
        keys, group_of, counts = {}, [], self._counts
        for gi, p, _, _ in found:
            counts[p] = step = counts[p] + 1
            group_of.append(keys.setdefault((gi, step), len(keys)))
        torch._foreach_add_([state["step"] for _, _, _, state in found], 1.0)   # the host tensors of the state: one call
        if len(keys) > ops.OPTIM_MAX_GROUPS:
            raise RuntimeError(f"optim.Adam: {len(keys)} distinct (parameter group, step count) pairs in one step, at most "
                               f"{ops.OPTIM_MAX_GROUPS}")
        groups = []
        for gi, step in keys:
            group = self.param_groups[gi]
            groups.append(ops.optimizer_group(group["lr"], group["betas"], group["eps"], group["weight_decay"], step))
        # the tables are uploaded again only when an address, the participating set or a group index changed
        numels = tuple(p.numel() for _, p, _, _ in found)
        signature = (numels, tuple(group_of), tuple((p.data_ptr(), g.data_ptr(), s["exp_avg"].data_ptr(),
                                                     s["exp_avg_sq"].data_ptr()) for _, p, g, s in found))
        if signature != self._signature:
            same_cut = self._signature is not None and self._signature[0] == numels
            if same_cut:
                _, chunks_dev, tensors, num_chunks = self._tables
            else:
                tensors, chunks = ops.optimizer_tables(numels, group_of, ops.OPTIM_CHUNK)
                chunks_dev, num_chunks = ops.optimizer_table_to_device(chunks, self._device), len(chunks)
            for entry, group, (param, grad, exp_avg, exp_avg_sq) in zip(tensors, group_of, signature[2]):
                entry.param, entry.grad, entry.exp_avg, entry.exp_avg_sq, entry.group = param, grad, exp_avg, exp_avg_sq, group
            self._tables = (ops.optimizer_table_to_device(tensors, self._device), chunks_dev, tensors, num_chunks)
            self._signature = signature
            if self._partial is None or self._partial.numel() < num_chunks:
                self._partial = torch.empty(max(num_chunks, 1), dtype=torch.float64, device=self._device)
        tensors_dev, chunks_dev, _, num_chunks = self._tables
        coef = None
        if self.max_grad_norm is not None:
            if self._norm is None:
                self._norm = torch.empty(2, device=self._device)
            ops.grad_norm_clip(tensors_dev, len(found), chunks_dev, num_chunks, ops.OPTIM_CHUNK, self.max_grad_norm,
                               partial=self._partial, norm=self._norm)
            self.grad_norm, coef = self._norm[0], self._norm[1:]
        ops.adam_step(tensors_dev, len(found), chunks_dev, num_chunks, ops.OPTIM_CHUNK, groups, coef=coef,
                      zero_grad=self.zero_grads_in_step)
        written = [t for _, p, _, s in found for t in (p, s["exp_avg"], s["exp_avg_sq"])]
        if self.zero_grads_in_step:
            for _, p, g, _ in found:
                if g is not p.grad:  # the kernel zeroed a converted copy
                    p.grad.zero_()
            grads = [p.grad for _, p, _, _ in found]
            torch.autograd.graph.increment_version(grads)
            self._zeroed = [(g, g._version) for g in grads]
        torch.autograd.graph.increment_version(written)

    # ---- the data-parallel step ----------------------------------------------------------------------------------
    def _all_reduce(self, t):
        """SUM over the group, in place, ordered on the current stream.  RCCL orders itself behind the stream that wrote
        `t`; a host-side backend (gloo) reads the memory from the CPU, so that stream is drained first (dist.send_frames)."""
        if torch.distributed.get_backend(self.process_group) != "nccl":
            torch.cuda.current_stream(self._device).synchronize()
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.SUM, group=self.process_group)

    def _everyone(self):
        """[(group index, parameter, state)] of every parameter, with the state created where it is missing."""
        found = []
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = torch.tensor(0.0, dtype=torch.float32)
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    self._counts[p] = 0
                found.append((gi, p, state))
        return found

    def _replica_tables(self, everyone, group_of):
        """The bucket and the step table (grad addresses inside the bucket), uploaded again only when a parameter or
        state address or a group index changed; the pack table's entries are refreshed by the caller."""
        r = self._replicas
        numels = tuple(p.numel() for _, p, _ in everyone)
        signature = (numels, tuple(group_of), tuple((p.data_ptr(), s["exp_avg"].data_ptr(), s["exp_avg_sq"].data_ptr())
                                                     for _, p, s in everyone))
        if r is None or r.numels != numels:
            r = self._replicas = _Replicas(numels, self._device)
        if r.signature != signature:
            base = r.bucket.data_ptr()
            for entry, group, offset, (param, exp_avg, exp_avg_sq) in zip(r.step_host, group_of, r.offsets, signature[2]):
                entry.param, entry.grad, entry.exp_avg, entry.exp_avg_sq = param, base + 4 * offset, exp_avg, exp_avg_sq
                entry.group = group
            r.step_dev = ops.optimizer_table_to_device(r.step_host, self._device)
            r.signature = signature
        return r

    def _step_replicas_hip(self):
        everyone = self._everyone()
        keys, group_of, counts = {}, [], self._counts
        for gi, p, _ in everyone:
            counts[p] = step = counts[p] + 1
            group_of.append(keys.setdefault((gi, step), len(keys)))
        torch._foreach_add_([state["step"] for _, _, state in everyone], 1.0)
        if len(keys) > ops.OPTIM_MAX_GROUPS:
            raise RuntimeError(f"optim.Adam: {len(keys)} distinct (parameter group, step count) pairs in one step, at most "
                               f"{ops.OPTIM_MAX_GROUPS}")
        groups = []
        for gi, step in keys:
            group = self.param_groups[gi]
            groups.append(ops.optimizer_group(group["lr"], group["betas"], group["eps"], group["weight_decay"], step))
        r = self._replica_tables(everyone, group_of)
        # the pack table follows the allocator: this step's gradient addresses, NULL where the rank has none
        sources = []
        for _, p, _ in everyone:
            g = p.grad
            if g is not None:
                if g.is_sparse:
                    raise RuntimeError("optim.Adam does not support sparse gradients")
                if g.dtype != torch.float32 or not g.is_contiguous():
                    g = g.to(torch.float32).contiguous()
            sources.append(g)
        addresses = tuple(None if g is None else g.data_ptr() for g in sources)
        if addresses != r.pack_signature:
            for entry, address in zip(r.pack_host, addresses):
                entry.grad = address
            r.pack_dev = ops.optimizer_table_to_device(r.pack_host, self._device)
            r.pack_signature = addresses
        n, world = len(everyone), torch.distributed.get_world_size(self.process_group)
        ops.grads_pack(r.pack_dev, n, r.chunks_dev, r.num_chunks, ops.OPTIM_CHUNK, r.offsets_dev, r.bucket,
                       scale=1.0 / world, zero_source=self.zero_grads_in_step)
        self._all_reduce(r.bucket)
        coef = None
        if self.max_grad_norm is not None:
            ops.grad_norm_clip(r.step_dev, n, r.chunks_dev, r.num_chunks, ops.OPTIM_CHUNK, self.max_grad_norm,
                               partial=r.partial, norm=r.norm)
            self.grad_norm, coef = r.norm[0], r.norm[1:]
        # the pack has zeroed the gradients where that was asked for: zeroing here would only clear the bucket
        ops.adam_step(r.step_dev, n, r.chunks_dev, r.num_chunks, ops.OPTIM_CHUNK, groups, coef=coef, zero_grad=False)
        if self.zero_grads_in_step:
            grads = []
            for (_, p, _), g in zip(everyone, sources):
                if g is not None:
                    if g is not p.grad:  # the kernel zeroed a converted copy
                        p.grad.zero_()
                    grads.append(p.grad)
            torch.autograd.graph.increment_version(grads)
            self._zeroed = [(g, g._version) for g in grads]
        torch.autograd.graph.increment_version([t for _, p, s in everyone for t in (p, s["exp_avg"], s["exp_avg_sq"])])

    def _step_replicas_library(self):
        """The comparison path: every p.grad (zeros where None) summed over the group and divided by its size, then the
        library step over all of them."""
        world = torch.distributed.get_world_size(self.process_group)
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    p.grad = torch.zeros_like(p)
                self._all_reduce(p.grad)
                p.grad.div_(world)
        self._step_library(self._participants())

    def replicas_in_sync(self):
        """True iff every rank of the group holds the same parameters and moments, as far as a fingerprint can tell: the
        three wrap-around sums of the bit patterns of param, exp_avg and exp_avg_sq (ops.tensors_fingerprint) are
        all-gathered, 3 x 8 bytes per rank, and compared.  Synchronises: meant for every N-th step and for tests.  The
        limit: a sum does not see two elements swapped, nor changes that cancel; replicas that drifted apart through
        arithmetic differ in it."""
        if self.process_group is None:
            raise RuntimeError("optim.Adam.replicas_in_sync: constructed without a process_group")
        with torch.no_grad():
            everyone = self._everyone()
            r = self._replicas
            # the fingerprint reads no group index: the last step's stand (before the first step: zeros) keeps the table
            known = r is not None and r.signature is not None and len(r.signature[1]) == len(everyone)
            r = self._replica_tables(everyone, r.signature[1] if known else [0] * len(everyone))
            mine = torch.empty(3, dtype=torch.int64, device=self._device)
            for i, which in enumerate(("param", "exp_avg", "exp_avg_sq")):
                ops.tensors_fingerprint(r.step_dev, len(everyone), r.chunks_dev, r.num_chunks, ops.OPTIM_CHUNK, which,
                                        partial=r.fingerprint_partial, out=mine[i])
            world = torch.distributed.get_world_size(self.process_group)
            everyones = torch.empty(world, 3, dtype=torch.int64, device=self._device)
            if torch.distributed.get_backend(self.process_group) != "nccl":
                torch.cuda.current_stream(self._device).synchronize()
            torch.distributed.all_gather_into_tensor(everyones.view(-1), mine, group=self.process_group)
            return bool((everyones == everyones[0]).all().item())

    @torch.no_grad()
    def step(self, closure=None):
        """One clipped Adam update of every parameter that has a gradient (with a process_group: of every parameter, on
        the gradients averaged over the group); no host synchronisation on a stream-ordered backend."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._zeroed = []
        if self.process_group is not None:
            if self.max_grad_norm is None:
                self.grad_norm = None
            if self.backend == "library":
                self._step_replicas_library()
            else:
                self._step_replicas_hip()
            return loss
        found = self._participants()
        if self.max_grad_norm is None:
            self.grad_norm = None
        if self.backend == "library":
            self._step_library(found)
        elif found:
            self._step_hip(found)
        elif self.max_grad_norm is not None:
            self.grad_norm = torch.zeros((), device=self._device)
        return loss

    def zero_grad(self, set_to_none=True):
        """torch's zero_grad; with set_to_none=False the gradients that the last step zeroed in its own pass, and that
        nothing has written since, are left alone."""
        if set_to_none or not self._zeroed:
            self._zeroed = []
            return super().zero_grad(set_to_none=set_to_none)
        clean = {id(g) for g, version in self._zeroed if g._version == version}
        self._zeroed = []
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is not None and id(p.grad) not in clean:
                    if p.grad.grad_fn is not None:
                        p.grad.detach_()
                    else:
                        p.grad.requires_grad_(False)
                    p.grad.zero_()


class _Replicas:
    """What the data-parallel step keeps between steps, for one cut of the parameters: the bucket (zero-filled once: the
    gaps between tensors are never written and stay zero), the chunk table and the offsets (uploaded once), the pack
    table (follows the gradients' addresses) and the step table (its grad addresses point into the bucket)."""

    def __init__(self, numels, device):
        self.numels = numels
        self.offsets, total = ops.bucket_offsets(numels)
        self.bucket = torch.zeros(total, dtype=torch.float32, device=device)
        self.offsets_dev = torch.tensor(self.offsets, dtype=torch.int64).pin_memory().to(device, non_blocking=True)
        self.pack_host, chunks = ops.optimizer_tables(numels, [0] * len(numels), ops.OPTIM_CHUNK)
        self.step_host, _ = ops.optimizer_tables(numels, [0] * len(numels), ops.OPTIM_CHUNK)
        self.chunks_dev, self.num_chunks = ops.optimizer_table_to_device(chunks, device), len(chunks)
        self.pack_dev = self.step_dev = None
        self.pack_signature = self.signature = None
        self.partial = torch.empty(max(self.num_chunks, 1), dtype=torch.float64, device=device)
        self.fingerprint_partial = torch.empty(max(self.num_chunks, 1), dtype=torch.int64, device=device)
        self.norm = torch.empty(2, device=device)


def configure_optimizers(module, lr=1e-4, total_steps=200000, max_grad_norm=1.0, process_group=None):
    """The reference's `configure_optimizers` plus its Trainer's clip, for `module`: (Adam over the parameters that
    require grad, LinearLR(start_factor=1.0, end_factor=0.01, total_iters=total_steps)).  The scheduler is the library's:
    scheduler.step() after every optimizer.step() rewrites param_group["lr"] on the host and the next step reads it.
    process_group: handed to Adam (the data-parallel step); None keeps the single-process step."""
    optimizer = Adam([p for p in module.parameters() if p.requires_grad], lr=lr, max_grad_norm=max_grad_norm,
                     process_group=process_group)
    scheduler = torch.optim.lr_scheduler.LinearLR(optimizer, start_factor=1.0, end_factor=0.01, total_iters=total_steps)
    return optimizer, scheduler
