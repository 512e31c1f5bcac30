"""The kernels of the data-parallel step on the GPU, in one process: amav_grads_pack against torch bit for bit (scales,
chunk sizes, a missing gradient, a view at an odd offset, gaps and a guard band that must stay untouched, tables that point
outside), amav_tensors_fingerprint against the sum formed on the host, and a step that reads its gradients from the
bucket against the same step on ordinary allocations."""
import pytest
import torch

import optimizer_cases as oc

pytestmark = pytest.mark.gpu

NUMELS = (1, 3, 63, 64, 65, 3 * 64 + 5, 0, 12293)
MISSING, VIEW = 2, 4          # the tensor without a gradient; the tensor whose gradient starts one float into its storage
GUARD = 64                    # sentinel floats behind the bucket


@pytest.fixture(scope="module")
def grads():
    """fp32 device gradients of NUMELS, read-only: every test packs from clones."""
    g = torch.Generator().manual_seed(11)
    return [torch.randn(n, generator=g).cuda() for n in NUMELS]


def _sources(grads):
    """Fresh device gradients (None for MISSING; a [1:] view for VIEW, so its first element is not 16-byte aligned)."""
    out = []
    for i, g in enumerate(grads):
        if i == MISSING:
            out.append(None)
        elif i == VIEW:
            base = torch.full((g.numel() + 1,), oc.SENTINEL, device="cuda")
            base[1:].copy_(g)
            assert base[1:].data_ptr() % 16 == 4
            out.append(base[1:])
        else:
            out.append(g.clone())
    return out


def _tables(sources, chunk, numels=NUMELS, edit_chunks=None):
    from audio_motion_avatar_amd import ops

    tensors, chunks = ops.optimizer_tables(numels, [0] * len(numels), chunk)
    for t, s in zip(tensors, sources):
        t.grad = None if s is None else s.data_ptr()
    if edit_chunks is not None:
        edit_chunks(chunks)
    return (ops.optimizer_table_to_device(tensors, "cuda"), len(tensors), ops.optimizer_table_to_device(chunks, "cuda"),
            len(chunks), chunk)


def _bucket(offsets=None):
    from audio_motion_avatar_amd import ops

    if offsets is None:
        offsets, total = ops.bucket_offsets(NUMELS)
    else:
        total = ops.bucket_offsets(NUMELS)[1]
    storage = torch.full((total + GUARD,), oc.SENTINEL, device="cuda")
    return offsets, total, storage, torch.tensor(offsets, dtype=torch.int64, device="cuda")


def _check_bucket(storage, offsets, total, want):
    """want[i]: the tensor expected at offsets[i], or None where the range must still hold the sentinel; everything else
    in `storage` (the gaps, the guard band) must hold the sentinel too."""
    touched = torch.zeros(storage.numel(), dtype=torch.bool, device="cuda")
    for i, (o, n) in enumerate(zip(offsets, NUMELS)):
        if want[i] is not None:
            assert torch.equal(storage[o:o + n], want[i]), f"tensor {i} of {n} elements"
            touched[o:o + n] = True
    assert bool((storage[~touched] == oc.SENTINEL).all()), "written outside the tensors' ranges"
    assert int((~touched).sum()) >= GUARD + sum(1 for n in NUMELS if n % 64)


@pytest.mark.parametrize("chunk", [64, 4096])
@pytest.mark.parametrize("scale", [1.0, 0.5, 1.0 / 3.0])
def test_pack_equals_torch_bit_for_bit(grads, chunk, scale):
    from audio_motion_avatar_amd import ops

    sources = _sources(grads)
    offsets, total, storage, offsets_dev = _bucket()
    assert offsets == [0, 64, 128, 192, 256, 384, 640, 640] and total == 640 + 12352
    ops.grads_pack(*_tables(sources, chunk), offsets_dev, storage[:total], scale=scale)
    s = torch.tensor(scale, dtype=torch.float32)
    want = [torch.zeros(n, device="cuda") if src is None else g * s for g, src, n in zip(grads, sources, NUMELS)]
    _check_bucket(storage, offsets, total, want)
    for g, src in zip(grads, sources):                                       # zero_source = 0: the sources are only read
        assert src is None or torch.equal(src, g)


@pytest.mark.parametrize("chunk", [64, 4096])
def test_pack_zeroes_its_sources_when_asked(grads, chunk):
    from audio_motion_avatar_amd import ops

    sources = _sources(grads)
    offsets, total, storage, offsets_dev = _bucket()
    ops.grads_pack(*_tables(sources, chunk), offsets_dev, storage[:total], scale=0.5, zero_source=True)
    half = torch.tensor(0.5)
    want = [torch.zeros(n, device="cuda") if src is None else g * half for g, src, n in zip(grads, sources, NUMELS)]
    _check_bucket(storage, offsets, total, want)
    for src in sources:
        assert src is None or (int(torch.count_nonzero(src)) == 0 and not bool(torch.signbit(src).any()))
    assert float(sources[VIEW]._base[0]) == oc.SENTINEL                      # the float in front of the view is not the kernel's


def test_entries_that_point_outside_are_skipped(grads):
    """A chunk whose tensor index is out of range, a chunk whose start is past the tensor, an offset that would run past
    bucket_numel or lies in front of the bucket: that tensor's range keeps the sentinel, every other tensor is packed and
    the call succeeds."""
    from audio_motion_avatar_amd import ops

    one = torch.tensor(1.0)
    victim = 5                                                               # 197 elements: four chunks of 64

    def retarget(index):
        def edit(chunks):
            for c in chunks:
                if c.tensor == victim:
                    c.tensor = index
        return edit

    def restart(chunks):
        for c in chunks:
            if c.tensor == victim:
                c.start = NUMELS[victim] + c.start                           # NUMELS[victim], NUMELS[victim] + 64, ...

    base_offsets, total = ops.bucket_offsets(NUMELS)
    past_end = list(base_offsets)
    past_end[victim] = total - NUMELS[victim] + 1
    in_front = list(base_offsets)
    in_front[victim] = -64
    cases = [(retarget(len(NUMELS)), None), (retarget(-1), None), (restart, None), (None, past_end), (None, in_front)]
    for edit, offsets in cases:
        sources = _sources(grads)
        offsets, total, storage, offsets_dev = _bucket(offsets)
        ops.grads_pack(*_tables(sources, 64, edit_chunks=edit), offsets_dev, storage[:total], scale=1.0)
        want = [torch.zeros(n, device="cuda") if src is None else g * one for g, src, n in zip(grads, sources, NUMELS)]
        want[victim] = None
        _check_bucket(storage, base_offsets, total, want)


def _host_fingerprint(tensors):
    total = 0
    for x in tensors:
        if x is not None:
            total += int((x.cpu().contiguous().view(torch.int32).to(torch.int64) & 0xffffffff).sum())
    return total % 2 ** 64


@pytest.mark.parametrize("chunk", [64, 4096])
def test_fingerprint_equals_the_host_sum(chunk):
    from audio_motion_avatar_amd import ops

    g = torch.Generator().manual_seed(12)
    arrays = {}
    for which in ("param", "grad", "exp_avg", "exp_avg_sq"):
        arrays[which] = [torch.randn(n, generator=g).cuda() * 10.0 ** k for k, n in enumerate(NUMELS)]
    arrays["grad"] = _sources(arrays["grad"])                                # one NULL address, one view at an odd offset
    arrays["exp_avg"][-1][5] = float("nan")                                  # any bit pattern counts
    arrays["exp_avg"][-1][6] = -0.0
    tensors, chunks = ops.optimizer_tables(NUMELS, [0] * len(NUMELS), chunk)
    for i, t in enumerate(tensors):
        t.param, t.exp_avg, t.exp_avg_sq = (arrays[w][i].data_ptr() for w in ("param", "exp_avg", "exp_avg_sq"))
        t.grad = None if arrays["grad"][i] is None else arrays["grad"][i].data_ptr()
    tables = (ops.optimizer_table_to_device(tensors, "cuda"), len(tensors), ops.optimizer_table_to_device(chunks, "cuda"),
              len(chunks), chunk)
    got = {}
    for index, which in enumerate(("param", "grad", "exp_avg", "exp_avg_sq")):
        out = ops.tensors_fingerprint(*tables, which)
        assert out.dtype == torch.int64 and out.dim() == 0 and out.is_cuda
        got[which] = int(out) % 2 ** 64
        assert got[which] == _host_fingerprint(arrays[which]), which
        assert int(ops.tensors_fingerprint(*tables, index)) % 2 ** 64 == got[which]
    assert len(set(got.values())) == 4
    # one bit of one element
    bits = arrays["param"][-1].view(torch.int32)
    bits[12000] ^= 1 << 7
    flipped = int(ops.tensors_fingerprint(*tables, "param")) % 2 ** 64
    assert flipped != got["param"] and flipped == _host_fingerprint(arrays["param"])
    assert abs(flipped - got["param"]) == 1 << 7


def test_fingerprint_of_nothing_is_zero():
    from audio_motion_avatar_amd import ops

    tensors, chunks = ops.optimizer_tables(NUMELS, [0] * len(NUMELS), 64)    # every address NULL
    tables = (ops.optimizer_table_to_device(tensors, "cuda"), len(tensors), ops.optimizer_table_to_device(chunks, "cuda"),
              len(chunks), 64)
    out = torch.full((), -1, dtype=torch.int64, device="cuda")
    for which in ("param", "grad", "exp_avg", "exp_avg_sq"):
        out.fill_(-1)
        assert int(ops.tensors_fingerprint(*tables, which, out=out)) == 0
    empty = torch.empty(0, dtype=torch.uint8, device="cuda")
    out.fill_(-1)
    assert int(ops.tensors_fingerprint(empty, 0, empty, 0, 64, "param", out=out)) == 0   # no table: the 0 is still written


@pytest.mark.parametrize("chunk", [64, 4096])
def test_a_step_from_the_bucket_equals_a_step_from_ordinary_allocations(chunk):
    """grads_pack at scale 1 + grad_norm_clip + adam_step with the step table's gradients inside the bucket, against the
    same three steps with every gradient in an allocation of its own: p, m, v and the norm bit for bit.  This is what
    bucket_offsets' alignment of 64 elements is for: the chunks take the same 16-byte or scalar path on both sides, so
    every sum runs in the same order."""
    from audio_motion_avatar_amd import ops

    case = oc.COVERAGE                                                       # two groups, weight decay, the clip active
    p0, grads = oc.inputs(case)
    n = len(case.numels)

    def fresh():
        return ([t.cuda() for t in p0], [torch.zeros(k, device="cuda") for k in case.numels],
                [torch.zeros(k, device="cuda") for k in case.numels], [torch.empty(k, device="cuda") for k in case.numels])

    def table(p, g_ptrs, m, v):
        tensors, chunks = ops.optimizer_tables(case.numels, case.group_of, chunk)
        for i, t in enumerate(tensors):
            t.param, t.grad, t.exp_avg, t.exp_avg_sq = p[i].data_ptr(), g_ptrs[i], m[i].data_ptr(), v[i].data_ptr()
        return (ops.optimizer_table_to_device(tensors, "cuda"), n, ops.optimizer_table_to_device(chunks, "cuda"), len(chunks),
                chunk)

    def groups(step):
        return [ops.optimizer_group(*h, step) for h in case.hypers]

    # the plain path
    p, m, v, g = fresh()
    plain_table = table(p, [t.data_ptr() for t in g], m, v)
    plain = []
    for step in range(1, case.steps + 1):
        for dst, src in zip(g, grads[step - 1]):
            dst.copy_(src)
        norm = ops.grad_norm_clip(*plain_table, case.max_norm)
        ops.adam_step(*plain_table, groups(step), coef=norm[1:])
        plain.append([t.clone() for t in p + m + v] + [norm.clone()])

    # the bucket path
    p, m, v, g = fresh()
    offsets, total = ops.bucket_offsets(case.numels)
    bucket = torch.zeros(total, device="cuda")
    offsets_dev = torch.tensor(offsets, dtype=torch.int64, device="cuda")
    pack_table = table(p, [t.data_ptr() for t in g], m, v)
    step_table = table(p, [bucket.data_ptr() + 4 * o for o in offsets], m, v)
    for step in range(1, case.steps + 1):
        for dst, src in zip(g, grads[step - 1]):
            dst.copy_(src)
        ops.grads_pack(*pack_table, offsets_dev, bucket, scale=1.0, zero_source=True)
        norm = ops.grad_norm_clip(*step_table, case.max_norm)
        ops.adam_step(*step_table, groups(step), coef=norm[1:])
        got = p + m + v + [norm]
        assert all(torch.equal(a, b) for a, b in zip(got, plain[step - 1])), step
        assert all(int(torch.count_nonzero(t)) == 0 for t in g)
    assert float(plain[-1][-1][1]) < 1.0                                     # the clip was active
    assert not torch.equal(plain[0][0], plain[-1][0])
