"""Backward of the point refiner (csrc/cloud_backward.hip) against fp64 torch autograd of the
oracle/ptv3.py restatements on the CPU.

Bound per gradient tensor, the form and the constants of test_default_width_network_matches_fp64_oracle:
    max|g - g64| <= max(4 * err32, 2e-5 * max|g64|),   err32 = max|g32 - g64| of the same restatement run in fp32.
Every comparison prints err, err32 and max|g64| before it asserts."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _mods():
    from audio_motion_avatar_amd import ops, point_transformer

    return ops, point_transformer


def _clouds(seed, F, N, extent=(0.3, 0.5, 0.2)):
    g = torch.Generator().manual_seed(seed)
    d = torch.nn.functional.normalize(torch.randn(F, N, 3, generator=g), dim=-1)
    pts = d * torch.tensor(extent) * (1.0 + 0.05 * torch.randn(F, N, 1, generator=g))
    pts[:, N - N // 8:] = pts[:, : N // 8] + 0.002 * torch.randn(F, N // 8, 3, generator=g)  # shared voxels
    return pts + torch.randn(F, 1, 3, generator=g) * 0.3


def _check(name, got, g64, g32):
    """The module's bound; returns err / bound."""
    g64 = g64.double()
    err = float((got.detach().cpu().double() - g64).abs().max())
    err32 = float((g32.double() - g64).abs().max())
    big = float(g64.abs().max())
    bound = max(4 * err32, 2e-5 * big)
    print(f"{name}: err {err:.3e}  err32 {err32:.3e}  max|g64| {big:.3e}  err/bound {err / max(bound, 1e-300):.3f}")
    assert err <= bound, (name, err, err32, big)
    return err / max(bound, 1e-300)


def _level(pts):
    ops, pt = _mods()
    F, N = pts.shape[:2]
    n = F * N
    cloud_of = torch.arange(F, dtype=torch.int32).repeat_interleave(N).cuda()
    grid, depth = ops.cloud_voxelize(pts.reshape(n, 3).cuda(), cloud_of, F)
    return pt.Level(grid, cloud_of, depth, np.full(F, N), ops.cloud_codes(grid, cloud_of, depth))


# ------------------------------------------------------------------------------------------------- 1. convolution
def _conv_reference(conv, pts, feat, dout, ksize, dtype):
    from oracle import ptv3 as o_pt

    F, N = pts.shape[:2]
    x = feat.detach().clone().to(dtype).requires_grad_()
    w = conv.weight.detach().cpu().to(dtype).requires_grad_()
    b = conv.bias.detach().cpu().to(dtype).requires_grad_()
    outs = []
    for f in range(F):
        nbr = o_pt.neighbor_table(o_pt.frame_grid(pts[f]), torch.zeros(N, dtype=torch.long), ksize)
        outs.append(o_pt.subm_conv3d(x[f * N:(f + 1) * N], nbr, w, b))
    torch.cat(outs).backward(dout.to(dtype))
    return dict(feat=x.grad, weight=w.grad, bias=b.grad)


@pytest.mark.parametrize("cin,cout,ksize,F,N", [(12, 32, 5, 1, 400), (64, 64, 3, 2, 700), (768, 32, 5, 1, 900),
                                                 (256, 256, 3, 2, 500), (96, 160, 3, 1, 300), (32, 64, 3, 1, 300),
                                                 (512, 512, 3, 1, 300), (128, 128, 3, 2, 500)])
def test_subm_conv_backward_matches_fp64_autograd(cin, cout, ksize, F, N):
    """dfeat (the transposed ordered sum over a CSR by source row), dweight in the parameter's layout (split-K over pair
    chunks) and dbias; the inputs do exercise a source row with two pairs of one tap (shared voxels: the pair relation is
    not symmetric) and a tap whose pair count is not a multiple of the split-K chunk.  Also: the differentiable forward
    is the inference forward bit for bit, the weight gradient does not depend on whether feat requires grad, a second
    backward is bitwise the same, and the tap-swept feature gradient is the one-buffer feature gradient bit for bit.
    The (C_in, C_out) pairs reach every weight-gradient tile: <32,32> (12 -> 32, 96 -> 160), <32,64> (32 -> 64), <64,32>
    (768 -> 32) and <64,64> (64, 128, 256 and the default network's widest, 512 -> 512: a grid of 8 x 8 tiles per slice).
    Worst err / bound of the three last cases, as measured: 0.027 (512 -> 512, d feat)."""
    ops, pt = _mods()
    pts = _clouds(7, F, N)
    n = F * N
    level = _level(pts)
    gen = torch.Generator().manual_seed(8)
    feat = torch.randn(n, cin, generator=gen)
    conv = pt.SubMConv3d(cin, cout, ksize, bias=True)
    with torch.no_grad():
        conv.bias.copy_(torch.randn(cout, generator=gen) * 0.1)
    dout = torch.randn(n, cout, generator=gen)
    conv = conv.cuda()

    pairs = level.pairs(ksize)
    tap_of = torch.searchsorted(pairs.tap_start.long(), torch.arange(pairs.count, device="cuda"), right=True) - 1
    key = tap_of * n + pairs.pair_src.long()
    assert int(torch.unique(key).numel()) < pairs.count, "no source row owns two pairs of one tap"
    assert torch.equal(pairs.pair_of[pairs.pair_dst.long(), tap_of], torch.arange(pairs.count, device="cuda", dtype=torch.int32))
    chunk, _, slices = pairs.wgrad_slices(cin + (-cin % 32), cout)
    counts = np.diff(pairs.tap_start_host.astype(np.int64))
    assert chunk % ops.SUBM_WGRAD_CHUNK == 0 and (counts % chunk != 0).any(), (chunk, counts)
    if (cin, N) == (12, 400):
        assert (counts == 0).any() and (counts > 0).any()  # the sparse 5^3 case has empty taps: they write zeros

    def run(feat_grad):
        x = feat.cuda().requires_grad_(feat_grad)
        conv.zero_grad(set_to_none=True)
        out = conv(x, level, differentiable=True)
        out.backward(dout.cuda())
        return out.detach(), dict(feat=x.grad, weight=conv.weight.grad.clone(), bias=conv.bias.grad.clone())

    out, got = run(True)
    with torch.no_grad():
        assert torch.equal(out, conv(feat.cuda(), level))
    _, again = run(True)
    for k in got:
        assert torch.equal(got[k], again[k]), k
    _, frozen = run(False)
    assert frozen["feat"] is None and torch.equal(frozen["weight"], got["weight"]) and torch.equal(frozen["bias"], got["bias"])

    g64 = _conv_reference(conv, pts, feat, dout, ksize, torch.float64)
    g32 = _conv_reference(conv, pts, feat, dout, ksize, torch.float32)
    for k in ("feat", "weight", "bias"):
        assert got[k].shape == g64[k].shape
        _check(f"conv {cin}->{cout} k{ksize} d{k}", got[k], g64[k], g32[k])

    pad = -cin % 32
    wt = conv.weight.detach().reshape(cout, -1, cin).permute(1, 0, 2)
    wt = torch.nn.functional.pad(wt, (0, pad)).contiguous()
    whole = ops.subm_feat_grad(dout.cuda(), wt, pairs)
    swept = ops.subm_feat_grad(dout.cuda(), wt, pairs, max_buffer_bytes=pairs.count * (cin + pad) * 4 // 5)
    assert torch.equal(whole[:, :cin], got["feat"]) and torch.equal(whole, swept)


# --------------------------------------------------------------------------------------------------- 2. attention
def _attention_reference(qkv, order, counts, heads, dim, patch, dout, dtype, scale=None):
    """fp autograd of the padded-patch restatement (patch_layout + softmax, as oracle.ptv3.serialized_attention) ->
    (out, lse [n, heads], d qkv).  Cloud by cloud, each with a backward of its own on its slice of dout (a row belongs
    to one cloud), so the score matrices of one cloud at a time are alive."""
    from oracle import ptv3 as o_pt

    C = heads * dim
    scale = dim ** -0.5 if scale is None else scale
    x_all = qkv.detach().clone().to(dtype).requires_grad_()
    outs, lses = [], []
    start = 0
    for c in counts:
        o = order[start:start + c] - start
        inv = torch.empty_like(o)
        inv[o] = torch.arange(c)
        K, pad, unpad = o_pt.patch_layout(c, patch)
        x = x_all[start:start + c][o[pad]]
        q, k, v = x.reshape(-1, K, 3, heads, dim).permute(2, 0, 3, 1, 4).unbind(0)
        s = (q * scale) @ k.transpose(-2, -1)
        out = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(-1, C)[unpad[inv]]
        lses.append(torch.logsumexp(s, -1).transpose(1, 2).reshape(-1, heads)[unpad[inv]].detach())
        out.backward(dout[start:start + c].to(dtype))
        outs.append(out.detach())
        start += c
    return torch.cat(outs), torch.cat(lses), x_all.grad


def _attention_case(heads, dim, counts, patch):
    _, pt = _mods()
    C = heads * dim
    n = sum(counts)
    gen = torch.Generator().manual_seed(11)
    qkv = torch.randn(n, 3 * C, generator=gen)
    order = torch.cat([torch.randperm(c, generator=gen) + s for c, s in zip(counts, np.cumsum([0] + counts[:-1]))])
    dout = torch.randn(n, C, generator=gen)
    level = pt.Level.__new__(pt.Level)
    level.counts, level.starts_host = counts, np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    level.grid, level._patches = qkv.cuda(), {}
    desc, max_patch = level.patches(patch)
    return qkv, order, dout, desc, max_patch


@pytest.mark.parametrize("heads,dim,counts,patch", [(4, 64, [1300, 512, 70], 512), (2, 32, [300, 130], 128),
                                                    (2, 16, [257, 33, 64], 128), (1, 64, [5], 512)])
def test_patch_attention_backward_matches_fp64_autograd(heads, dim, counts, patch):
    """The LSE entry's out is patch_attention's bit for bit, its lse the fp64 one to 1e-5; d qkv within the module's
    bound; a second backward is bitwise the same."""
    ops, _ = _mods()
    qkv, order, dout, desc, max_patch = _attention_case(heads, dim, counts, patch)
    out, lse = ops.patch_attention_lse(qkv.cuda(), order.cuda(), desc, heads, max_patch)
    assert torch.equal(out, ops.patch_attention(qkv.cuda(), order.cuda(), desc, heads, max_patch))
    o64, l64, g64 = _attention_reference(qkv, order, counts, heads, dim, patch, dout, torch.float64)
    _, _, g32 = _attention_reference(qkv, order, counts, heads, dim, patch, dout, torch.float32)
    lse_err = float((lse.cpu().double() - l64).abs().max())
    print(f"lse err {lse_err:.3e}")
    assert lse_err <= 1e-5

    def run():
        x = qkv.cuda().requires_grad_()
        y = ops.patch_attention_differentiable(x, order.cuda(), desc, heads, max_patch)
        y.backward(dout.cuda())
        return y.detach(), x.grad

    y, got = run()
    assert torch.equal(y, out)
    assert torch.equal(run()[1], got)
    C = heads * dim
    for i, part in enumerate(("dq", "dk", "dv")):
        sl = slice(i * C, (i + 1) * C)
        _check(f"attention h{heads} d{dim} {counts} {part}", got[:, sl], g64[:, sl], g32[:, sl])


_WIDE_COUNTS = [1, 63, 65, 513, 1300]


@pytest.mark.parametrize("peaked", [False, True])
@pytest.mark.parametrize("heads,dim,counts", [(2, 16, _WIDE_COUNTS), (4, 32, _WIDE_COUNTS), (4, 64, _WIDE_COUNTS),
                                              (32, 16, [65, 700]), (16, 32, [65, 700])])
def test_patch_attention_backward_default_widths(heads, dim, counts, peaked):
    """Patch 512 at every head dim the default network runs (16: the encoder, 32 / 64: the decoder) and at its widest
    stages (32 x 16 and 16 x 32: C = 512, an lse row stride of 32, pa_borrow_add_kernel over 256 float4 per row).
    Clouds of 1 and 63 points (below one 32-row tile), 65 (a row past two tiles), 513 (a full 512-slot patch and a patch
    of one own query with 511 borrowed keys) and 1300 (two full patches and a borrowed tail): four slot blocks per patch
    and sweeps of 16 tiles, which at D < 64 had only been run with one block and at most 5 tiles.  An explicit scale
    that is not D^-0.5 (0.37), or queries x 10 (a peaked softmax, logits ~100).  The LSE entry's out is
    patch_attention's bit for bit; its lse is the fp64 one to max(1e-5, 4 x the fp32 restatement's own lse error) -- at
    logits ~100 one fp32 rounding is already 8e-6; dq, dk, dv within the module's bound; a second backward is bitwise
    the same.  Worst err / bound as measured: 0.27 peaked (4 x 64; 0.25 at D < 64), 0.09 with the explicit scale; lse
    error at most 1.6e-5 where the fp32 restatement's is 1.9e-5 (peaked), 5.0e-6 against 3.9e-6 (scale 0.37)."""
    ops, _ = _mods()
    qkv, order, dout, desc, max_patch = _attention_case(heads, dim, counts, 512)
    assert max_patch == 512
    C = heads * dim
    scale = None if peaked else 0.37
    if peaked:
        qkv[:, :C] *= 10.0
    out, lse = ops.patch_attention_lse(qkv.cuda(), order.cuda(), desc, heads, max_patch, scale=scale)
    assert torch.equal(out, ops.patch_attention(qkv.cuda(), order.cuda(), desc, heads, max_patch, scale=scale))
    _, l64, g64 = _attention_reference(qkv, order, counts, heads, dim, 512, dout, torch.float64, scale)
    _, l32, g32 = _attention_reference(qkv, order, counts, heads, dim, 512, dout, torch.float32, scale)
    lse_err, lse_err32 = float((lse.cpu().double() - l64).abs().max()), float((l32.double() - l64).abs().max())
    print(f"attention h{heads} d{dim} peaked={peaked} lse: err {lse_err:.3e}  err32 {lse_err32:.3e}  "
          f"max|lse64| {float(l64.abs().max()):.3e}")
    assert lse_err <= max(1e-5, 4 * lse_err32)

    def run():
        x = qkv.cuda().requires_grad_()
        y = ops.patch_attention_differentiable(x, order.cuda(), desc, heads, max_patch, scale=scale)
        y.backward(dout.cuda())
        return y.detach(), x.grad

    y, got = run()
    assert torch.equal(y, out)
    assert torch.equal(run()[1], got)
    worst = 0.0
    for i, part in enumerate(("dq", "dk", "dv")):
        sl = slice(i * C, (i + 1) * C)
        worst = max(worst, _check(f"attention h{heads} d{dim} peaked={peaked} {part}", got[:, sl], g64[:, sl], g32[:, sl]))
    print(f"worst err / bound: {worst:.3f}")


def test_patch_attention_backward_borrowed_keys_carry_both_contributions():
    """counts [257, ...], patch 128: the first cloud's last patch has one own query (sorted position 256) and 127
    borrowed keys, sorted positions 129..255 (the 130th..256th).  Their dK is the own patch's part plus the borrowing
    patch's: zeroing d out of that one query changes the dK of every one of them, and of no other row.  The same with
    counts [513], patch 512: the last patch's one own query (sorted position 512) borrows sorted positions 1..511, whose
    key slots lie in all four 128-slot blocks of the patch."""
    ops, _ = _mods()
    for heads, dim, counts, patch in ((2, 16, [257, 33, 64], 128), (2, 16, [513], 512)):
        qkv, order, dout, desc, max_patch = _attention_case(heads, dim, counts, patch)
        assert max_patch == patch
        C = heads * dim
        last = counts[0] - 1  # sorted position of the last patch's one own query
        assert last % patch == 0
        out, lse = ops.patch_attention_lse(qkv.cuda(), order.cuda(), desc, heads, max_patch)
        full = ops.patch_attention_backward(qkv.cuda(), order.cuda(), desc, out, lse, dout.cuda(), heads, max_patch).cpu()
        cut = dout.clone()
        cut[order[last]] = 0
        part = ops.patch_attention_backward(qkv.cuda(), order.cuda(), desc, out, lse, cut.cuda(), heads, max_patch).cpu()
        changed = ((full[:, C:2 * C] - part[:, C:2 * C]).abs().amax(1) > 0)
        want = torch.zeros(sum(counts), dtype=torch.bool)
        want[order[last - patch + 1:last]] = True
        want[order[last]] = True  # the last patch's own point is a key of its own patch too
        assert torch.equal(changed, want), (counts, int(changed.sum()), int(want.sum()))


@pytest.mark.parametrize("S", [5, 33, 129])
def test_patch_attention_backward_of_one_patch_is_the_dense_backward(S):
    """One cloud of S points in one patch without a borrowed slot is self-attention over qkv[order].  Both entries run the
    kernels of csrc/attention_backward_core.h, so from the same out, lse and d out they agree bit for bit.  S: below one
    tile of 32, one row past a tile, one row past a workgroup's 128."""
    ops, _ = _mods()
    heads, dim = 2, 64
    qkv, order, dout, desc, max_patch = _attention_case(heads, dim, [S], 512)
    assert desc.tolist() == [[0, S, S, 0]] and max_patch == S
    qkv, order, dout = qkv.cuda(), order.cuda(), dout.cuda()
    out, lse = ops.patch_attention_lse(qkv, order, desc, heads, max_patch)
    got = ops.patch_attention_backward(qkv, order, desc, out, lse, dout, heads, max_patch)
    dense = ops.selfattn_backward(qkv[order][None], out[order][None], lse[order].t()[None], dout[order][None], heads)
    want = torch.empty_like(got)
    want[order] = dense[0]
    assert torch.equal(got, want)


# --------------------------------------------------------------------------------------------- 3. segment kernels
def _segments(gen, C, clusters=12):
    """-> (sizes, n, members, seg, the last cluster of 8).  12 clusters: three whole blocks of four waves; any other
    count: sizes cycling through 1..8 (151 = 37 blocks and a last one of three clusters, whose fourth wave leaves)."""
    sizes = [1, 2, 3, 4, 5, 6, 7, 8, 1, 8, 2, 5] if clusters == 12 else [i % 8 + 1 for i in range(clusters)]
    n = sum(sizes)
    members = torch.randperm(n, generator=gen)
    seg = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64)
    return sizes, n, members, seg, len(sizes) - 1 - sizes[::-1].index(8)


def _cluster_max_backward_check(label, x, members, seg, scale, shift, dout):
    """cluster_max_differentiable's forward (== cluster_max bit for bit) and its dx, dscale, dshift against fp64 autograd
    on the CPU with the first-occurrence tie convention, bound 4e-6 of the tensor's largest reference value -> dx."""
    ops, _ = _mods()
    clusters = seg.shape[0] - 1
    xg, sg, bg = x.cuda().requires_grad_(), scale.cuda().requires_grad_(), shift.cuda().requires_grad_()
    out = ops.cluster_max_differentiable(xg, members.cuda(), seg.cuda(), sg, bg)
    assert torch.equal(out, ops.cluster_max(x.cuda(), members.cuda(), seg.cuda(), scale.cuda(), shift.cuda()))
    out.backward(dout.cuda())

    x64 = x.double().requires_grad_()
    s64, b64 = scale.double().requires_grad_(), shift.double().requires_grad_()
    rows = []
    for j in range(clusters):
        m = x64[members[seg[j]:seg[j + 1]]]
        first = torch.from_numpy(np.argmax(m.detach().numpy(), axis=0))  # numpy: the first occurrence
        rows.append(m.gather(0, first[None])[0])
    torch.nn.functional.gelu(torch.stack(rows) * s64 + b64).backward(dout.double())
    for name, got, ref in (("dx", xg.grad, x64.grad), ("dscale", sg.grad, s64.grad), ("dshift", bg.grad, b64.grad)):
        err, big = float((got.cpu().double() - ref).abs().max()), float(ref.abs().max())
        print(f"cluster_max_backward {label} {name}: err {err:.3e} max|ref| {big:.3e} err/bound {err / (4e-6 * big):.3f}")
        assert err <= 4e-6 * big, (name, err, big)
    assert int((xg.grad != 0).sum()) <= clusters * x.shape[1]  # one row per (cluster, channel)
    return xg.grad


def _sequential_sums(x, members, seg):
    """The segment sums of x [n, C] in fp32, one add per member in segment order."""
    want = torch.empty(seg.shape[0] - 1, x.shape[1])
    for j in range(seg.shape[0] - 1):
        acc = x[members[seg[j]]].clone()
        for r in range(int(seg[j]) + 1, int(seg[j + 1])):
            acc = acc + x[members[r]]
        want[j] = acc
    return want


@pytest.mark.parametrize("C", [4, 32, 260, 512, 1024])
def test_cluster_max_backward_matches_fp64(C):
    """dx, and the scale / shift gradients of the autograd node, against fp64 on the CPU with the tie convention (the
    first maximal member in segment order takes the whole gradient), incl. a deliberate tie: two equal rows in one
    cluster.  Bound 4e-6 of the tensor's largest reference value: gelu'(z) in fp32 is an erf, an exp and five
    multiply-adds (each a few ulp of 6e-8 on values <= ~1), z = max * scale + shift carries one rounding of |z| <= ~10
    through |gelu''| <= 0.8, and the two column sums add <= 12 such terms (151 in the second variant: the sums' rounding
    grows with their count no faster than the largest sum, which the bound scales with).
    12 clusters (whole blocks) and 151 (the last block holds three: its fourth wave takes the j >= clusters exit);
    C = 4 is one live lane of a wave, C = 1024 four float4 per lane (the c += 64 loop runs four times).  Worst
    err / bound as measured: 0.035 (C = 512, 12 clusters, dscale)."""
    for clusters in (12, 151):
        gen = torch.Generator().manual_seed(51 + C)
        sizes, n, members, seg, tie = _segments(gen, C, clusters)
        assert len(sizes) == clusters and sizes[tie] == 8
        x = torch.randn(n, C, generator=gen)
        tie_first, tie_second = int(members[seg[tie]]), int(members[seg[tie] + 3])  # the cluster of 8
        x[tie_first] = x[tie_second] = 6.0  # both rows are the maximum of every channel
        scale, shift = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen) * 0.3
        dout = torch.randn(len(sizes), C, generator=gen)
        dx = _cluster_max_backward_check(f"C={C} clusters={clusters}", x, members, seg, scale, shift, dout)
        assert float(dx[tie_first].abs().min()) > 0 and float(dx[tie_second].abs().max()) == 0.0


@pytest.mark.parametrize("C", [4, 32, 260, 512, 1024])
def test_cluster_sum_is_the_sequential_fp32_sum(C):
    """Bit for bit, and as the backward of the up[cluster] gather; 12 clusters and 151, C as in the test above."""
    ops, _ = _mods()
    for clusters in (12, 151):
        gen = torch.Generator().manual_seed(61 + C)
        sizes, n, members, seg, _ = _segments(gen, C, clusters)
        x = torch.randn(n, C, generator=gen)
        got = ops.cluster_sum(x.cuda(), members.cuda(), seg.cuda()).cpu()
        want = _sequential_sums(x, members, seg)
        assert torch.equal(got, want)
        # as the backward of the gather
        up = torch.randn(len(sizes), C, generator=gen).cuda().requires_grad_()
        cluster = torch.empty(n, dtype=torch.int64)
        for j in range(len(sizes)):
            cluster[members[seg[j]:seg[j + 1]]] = j
        y = ops.cluster_gather_differentiable(up, cluster.cuda(), members.cuda(), seg.cuda())
        assert torch.equal(y, up.detach()[cluster.cuda()])
        y.backward(x.cuda())
        assert torch.equal(up.grad.cpu(), want)


def test_segment_kernels_on_a_real_pooling():
    """members / seg as SerializedPooling hands them over (Level.pool of two clouds, as test_cluster_max_on_a_real_pooling
    builds them), 512 channels as the default network pools into.  The clouds are dense enough that a cluster has more
    than 8 members, and their cluster count is not a multiple of the 4 waves of a block (both asserted).  dx, dscale and
    dshift against fp64 with the 4e-6 rule of test_cluster_max_backward_matches_fp64 (the column sums run over every
    cluster, and so does the largest of them); cluster_sum is the sequential fp32 sum bit for bit.  Worst err / bound
    as measured: 0.044 (dscale; 411 clusters, the largest of 29 members)."""
    ops, _ = _mods()
    level = _level(_clouds(301, 2, 1500, extent=(0.06, 0.1, 0.04)))  # a fifth of the usual extent: 203 + 208 clusters
    child, cluster, seg = level.pool()
    members, seg = level.order[0].cpu(), seg.cpu()
    sizes = torch.diff(seg)
    print(f"pooling: {level.n} rows, {child.n} clusters, largest {int(sizes.max())}")
    assert child.n % 4 != 0 and int(sizes.max()) > 8 and int(sizes.min()) >= 1
    assert torch.equal(cluster.cpu()[members], torch.repeat_interleave(torch.arange(child.n), sizes))
    gen = torch.Generator().manual_seed(302)
    C = 512
    x = torch.randn(level.n, C, generator=gen)
    scale, shift = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen) * 0.3
    dout = torch.randn(child.n, C, generator=gen)
    _cluster_max_backward_check(f"pooling C={C} clusters={child.n}", x, members, seg, scale, shift, dout)
    got = ops.cluster_sum(x.cuda(), members.cuda(), seg.cuda()).cpu()
    assert torch.equal(got, _sequential_sums(x, members, seg))


# ------------------------------------------------------------------------------------------------------ 4. network
PCFG = dict(stride=(2, 2), enc_depths=(1, 1, 1), enc_channels=(32, 64, 128), enc_num_head=(2, 4, 4),
            enc_patch_size=(256, 256, 256), dec_depths=(1, 1), dec_channels=(64, 64), dec_num_head=(1, 2),
            dec_patch_size=(256, 256))
IN_CHANNELS = 48


def _network(differentiable=True, pcfg=None, in_channels=IN_CHANNELS):
    _, pt = _mods()
    torch.manual_seed(0)
    pcfg = PCFG if pcfg is None else pcfg
    net = pt.PointTransformerV3(in_channels=in_channels, differentiable=differentiable, **pcfg).eval()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_mean.normal_(0, 0.2)
                m.running_var.uniform_(0.5, 1.5)
    return net


def _inputs(F, N):
    pts = _clouds(41, F, N)
    feat = torch.randn(F, N, IN_CHANNELS, generator=torch.Generator().manual_seed(42))
    dout = torch.randn(F * N, PCFG["dec_channels"][0], generator=torch.Generator().manual_seed(43))
    return pts, feat, dout


def _oracle_grads(net, pts, feat, dout, dtype, pcfg=None):
    """oracle.ptv3.ptv3_cloud on one cloud under torch autograd -> (out, {name: grad}, d feat); pcfg: the
    configuration the network was built with (default PCFG)."""
    from oracle import ptv3 as o_pt

    pcfg = PCFG if pcfg is None else pcfg
    cfg = {k: list(pcfg[k]) for k in ("enc_depths", "enc_num_head", "enc_patch_size", "dec_depths", "dec_num_head",
                                      "dec_patch_size")}
    names = {k for k, _ in net.named_parameters()}
    p = {k: v.detach().cpu().to(dtype).requires_grad_(k in names) for k, v in net.state_dict().items()
         if v.is_floating_point()}
    x = feat.detach().clone().to(dtype).requires_grad_()
    out = o_pt.ptv3_cloud(p, "", o_pt.frame_grid(pts), x, cfg)
    out.backward(dout.to(dtype))
    return out.detach(), {k: p[k].grad for k in names}, x.grad


@functools.lru_cache(maxsize=None)
def _reference():
    """The fp64 reference and the fp32 yardstick of the 700-point case, computed once for the module."""
    net = _network()
    pts, feat, dout = _inputs(1, 700)
    return _oracle_grads(net, pts[0], feat[0], dout, torch.float64), _oracle_grads(net, pts[0], feat[0], dout, torch.float32)


def _hip_grads(net, pts, feat, dout):
    net.zero_grad(set_to_none=True)
    x = feat.cuda().requires_grad_()
    out = net(pts.cuda(), x)
    out.backward(dout.cuda())
    return out.detach(), {k: v.grad.clone() for k, v in net.named_parameters()}, x.grad


def test_network_gradients_match_fp64_oracle():
    """The small configuration of test_renderer_with_point_refiner_matches_oracle (48 input channels, randomised
    BatchNorm statistics) on one cloud of 700 = 2 * 256 + 188 points (a borrowed tail at level 0): every parameter
    gradient and d feat against oracle.ptv3.ptv3_cloud, and the differentiable forward with the forward test's bound."""
    (o64, p64, f64), (o32, p32, f32) = _reference()
    net = _network().cuda()
    assert len(p64) == len(list(net.named_parameters())) > 100  # every parameter tensor, and feat, gets a gradient
    assert all(g is not None for g in p64.values()) and f64 is not None
    pts, feat, dout = _inputs(1, 700)
    out, grads, dfeat = _hip_grads(net, pts, feat, dout)
    assert out.requires_grad is False and all(g is not None for g in grads.values())
    err, err32, big = (float((out.cpu().double() - o64).abs().max()), float((o32.double() - o64).abs().max()),
                       float(o64.abs().max()))
    print(f"forward: err {err:.3e} err32 {err32:.3e} largest |out| {big:.3f}")
    assert err <= min(max(4 * err32, 2e-5 * big), 1e-4 * max(1.0, big))
    worst = max(_check(k, grads[k], p64[k], p32[k]) for k in sorted(p64))
    worst = max(worst, _check("d feat", dfeat[0], f64, f32))
    print(f"worst err / bound: {worst:.3f}")


def test_network_batched_clouds_equal_single_clouds():
    """Two clouds of 420 points in one batch: d feat of each cloud within 2e-5 (relative) of the cloud run alone -- the
    forward test's allowance for library GEMMs that split a [2N, C] and an [N, C] product differently."""
    net = _network().cuda()
    pts, feat, dout = _inputs(2, 420)
    _, _, both = _hip_grads(net, pts, feat, dout)
    for f in range(2):
        _, _, alone = _hip_grads(net, pts[f:f + 1], feat[f:f + 1], dout[f * 420:(f + 1) * 420])
        err, big = float((both[f] - alone[0]).abs().max()), float(alone.abs().max())
        print(f"cloud {f}: |batched - alone| {err:.3e}, largest |d feat| {big:.3e}")
        assert err <= 2e-5 * big, (f, err, big)


def _default_pcfg():
    """RendererConfig's point refiner (the reference's ptv3_encoder.yaml: encoder 32..512 channels with 2..32 heads,
    decoder 256/128/256/512, patch 512) with every depth 1 -> (pcfg, the stem's input channels)."""
    from audio_motion_avatar_amd.config import RendererConfig

    rc = RendererConfig()
    pcfg = {k: tuple(getattr(rc, k)) for k in ("stride", "enc_channels", "enc_num_head", "enc_patch_size", "dec_channels",
                                                "dec_num_head", "dec_patch_size")}
    pcfg["enc_depths"], pcfg["dec_depths"] = (1,) * len(rc.enc_depths), (1,) * len(rc.dec_depths)
    return pcfg, 3 * rc.triplane_feature_dim


def _default_inputs():
    pcfg, in_channels = _default_pcfg()
    N = 1500
    pts = _clouds(41, 1, N)
    feat = torch.randn(1, N, in_channels, generator=torch.Generator().manual_seed(42))
    dout = torch.randn(N, pcfg["dec_channels"][0], generator=torch.Generator().manual_seed(43))
    return pts, feat, dout


@functools.lru_cache(maxsize=None)
def _default_reference():
    """The fp64 reference and the fp32 yardstick of the default-width case, computed once for the module."""
    pcfg, in_channels = _default_pcfg()
    net = _network(pcfg=pcfg, in_channels=in_channels)
    pts, feat, dout = _default_inputs()
    return (_oracle_grads(net, pts[0], feat[0], dout, torch.float64, pcfg),
            _oracle_grads(net, pts[0], feat[0], dout, torch.float32, pcfg))


def test_default_width_network_gradients_match_fp64_oracle(monkeypatch):
    """The backward counterpart of test_default_width_network_matches_fp64_oracle: PointTransformerV3 as RendererConfig
    configures it (a 768-channel stem input, encoder 32..512 channels, decoder 256/128/256/512, patch 512), every depth
    1 -- all widths are still there -- on one cloud of 1500 points, whose levels all but the last have patches beyond
    128 slots.  The forward with the forward test's bound, every parameter gradient (213 tensors) and d feat with the
    module's, and a second run bitwise the same.  Also checks that the run reached what it is meant to pin: the
    attention backward at head dims 16 / 32 / 64 on 512-slot patches, the weight gradient at 768 -> 32 and 512 -> 512,
    cluster_max_backward into 512 channels.  Worst err / bound as measured: 0.103 over the 214 gradients; forward err
    3.1e-6 where the fp32 oracle's is 2.7e-6."""
    ops, _ = _mods()
    pcfg, in_channels = _default_pcfg()
    assert in_channels == 768 and pcfg["enc_channels"][-1] == 512
    assert set(pcfg["enc_patch_size"] + pcfg["dec_patch_size"]) == {512}
    (o64, p64, f64), (o32, p32, f32) = _default_reference()
    net = _network(pcfg=pcfg, in_channels=in_channels).cuda()
    assert len(p64) == len(list(net.named_parameters())) == 213
    assert all(g is not None for g in p64.values()) and f64 is not None

    seen = set()
    attention_backward, wgrad = ops.patch_attention_backward, ops.subm_pair_wgrad
    cluster_max_backward = ops.cluster_max_backward

    def rec_attention_backward(qkv, order, patch_desc, out, lse, grad_out, heads, max_patch, scale=None):
        seen.add(("patch_attention_backward", qkv.shape[1] // 3 // heads, max_patch))
        return attention_backward(qkv, order, patch_desc, out, lse, grad_out, heads, max_patch, scale)

    def rec_wgrad(feat, grad_out, *args):
        seen.add(("subm_pair_wgrad", feat.shape[1], grad_out.shape[1]))
        return wgrad(feat, grad_out, *args)

    def rec_cluster_max_backward(x, *args):
        seen.add(("cluster_max_backward", x.shape[1]))
        return cluster_max_backward(x, *args)

    monkeypatch.setattr(ops, "patch_attention_backward", rec_attention_backward)
    monkeypatch.setattr(ops, "subm_pair_wgrad", rec_wgrad)
    monkeypatch.setattr(ops, "cluster_max_backward", rec_cluster_max_backward)
    pts, feat, dout = _default_inputs()
    out, grads, dfeat = _hip_grads(net, pts, feat, dout)
    print("recorded:", sorted(seen))
    assert {("patch_attention_backward", 16, 512), ("patch_attention_backward", 32, 512),
            ("patch_attention_backward", 64, 512), ("subm_pair_wgrad", 768, 32), ("subm_pair_wgrad", 512, 512),
            ("cluster_max_backward", 512)} <= seen
    assert out.requires_grad is False and all(g is not None for g in grads.values())

    err, err32, big = (float((out.cpu().double() - o64).abs().max()), float((o32.double() - o64).abs().max()),
                       float(o64.abs().max()))
    print(f"forward: err {err:.3e} err32 {err32:.3e} largest |out| {big:.3f}")
    assert err <= min(max(4 * err32, 2e-5 * big), 1e-4 * max(1.0, big))
    worst = max(_check(k, grads[k], p64[k], p32[k]) for k in sorted(p64))
    worst = max(worst, _check("d feat", dfeat[0], f64, f32))
    print(f"worst err / bound: {worst:.3f}")

    out_b, grads_b, dfeat_b = _hip_grads(net, pts, feat, dout)
    assert torch.equal(out, out_b) and torch.equal(dfeat, dfeat_b)
    for k in grads:
        assert torch.equal(grads[k], grads_b[k]), k


# -------------------------------------------------------------------------------------------------- 5. determinism
def test_network_gradients_are_bitwise_reproducible():
    net = _network().cuda()
    pts, feat, dout = _inputs(1, 700)
    out_a, grads_a, dfeat_a = _hip_grads(net, pts, feat, dout)
    out_b, grads_b, dfeat_b = _hip_grads(net, pts, feat, dout)
    assert torch.equal(out_a, out_b) and torch.equal(dfeat_a, dfeat_b)
    for k in grads_a:
        assert torch.equal(grads_a[k], grads_b[k]), k


# ----------------------------------------------------------------------------------------------------- 6. switches
def test_switches_keep_the_inference_path():
    pts, feat, _ = _inputs(1, 700)
    off = _network(differentiable=False).cuda()
    assert all(p.requires_grad for p in off.parameters())
    with torch.no_grad():
        want = off(pts.cuda(), feat.cuda())
    got = off(pts.cuda(), feat.cuda().requires_grad_())   # the default, under grad mode
    assert got.requires_grad is False and torch.equal(got, want)
    on = _network(differentiable=True).cuda()
    with torch.no_grad():
        got = on(pts.cuda(), feat.cuda().requires_grad_())  # the flag on, grad mode off
    assert got.requires_grad is False and torch.equal(got, want)
    assert on(pts.cuda(), feat.cuda().requires_grad_()).requires_grad is True


def test_renderer_still_refuses_autograd_with_a_differentiable_refiner():
    from audio_motion_avatar_amd.config import RendererConfig
    from audio_motion_avatar_amd.renderer import Renderer
    from audio_motion_avatar_amd.synthetic import init_random_heads, make_render_inputs

    cfg = RendererConfig(image_size=(64, 64), subdivide_steps=0, triplane_feature_dim=16, triplane_resolution=8,
                         predict_smplx_params=False, no_point_refiner=False, num_gaussians=1500,
                         differentiable_refiner=True, **PCFG)
    assert RendererConfig().differentiable_refiner is False
    r = init_random_heads(Renderer(cfg).eval(), std=0.05)
    assert r.point_encoder.point_transformer.differentiable is True
    tokens, smpl, cam = make_render_inputs(2, cfg, seed=4)
    with pytest.raises(NotImplementedError, match="point refiner"):
        r(tokens.requires_grad_(), cam, torch.zeros(1, 2, 1, 1, device="cuda"), smpl)


# ----------------------------------------------------------------------------------------------------- 7. it trains
def test_network_trains():
    """16 Adam steps (lr 1e-3) on the MSE to a fixed random target at N = 300: the loss at least halves (the CPU oracle
    on this set-up goes 2.58 -> 0.87)."""
    net = _network().cuda()
    pts, feat, target = _inputs(1, 300)
    pts, feat, target = pts.cuda(), feat.cuda(), target.cuda()
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    losses = []
    for _ in range(16):
        opt.zero_grad(set_to_none=True)
        loss = torch.nn.functional.mse_loss(net(pts, feat), target)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    print("losses:", " ".join(f"{v:.4f}" for v in losses))
    assert losses[-1] < 0.5 * losses[0], losses
