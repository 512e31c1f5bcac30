"""The point refiner's HIP kernels (csrc/cloud.hip) one by one, through their ops wrappers, against plain restatements
in fp64 on the CPU unless a test says otherwise.  Shapes are the ones the reference's default ptv3_encoder.yaml runs
(256 / 512 / 768 channels, 512-point patches, head dims 16 / 32 / 64) and the edges of each kernel's launch geometry
(dead rows of the last block, channel loops that repeat, partial pair and key tiles, several column blocks)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_point_refiner_gpu import _clouds

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23  # fp32 spacing at 1.0


def _mods():
    from audio_motion_avatar_amd import ops, point_transformer

    return ops, point_transformer


def _level(pts):
    """The Level PointTransformerV3.forward builds for clouds pts [F,N,3]."""
    ops, pt = _mods()
    Fc, N, _ = pts.shape
    cloud_of = torch.arange(Fc, dtype=torch.int32).repeat_interleave(N).cuda()
    grid, depth = ops.cloud_voxelize(pts.reshape(-1, 3).cuda(), cloud_of, Fc)
    return pt.Level(grid, cloud_of, depth, np.full(Fc, N), ops.cloud_codes(grid, cloud_of, depth))


def _bn_folded(C, gen):
    """(scale, shift) on the device from a BatchNorm1d with randomised affine parameters and running statistics."""
    _, pt = _mods()
    bn = pt._bn(C)
    with torch.no_grad():
        bn.weight.copy_(1.0 + 0.5 * torch.randn(C, generator=gen))
        bn.bias.copy_(0.3 * torch.randn(C, generator=gen))
        bn.running_mean.copy_(0.5 * torch.randn(C, generator=gen))
        bn.running_var.copy_(0.5 + torch.rand(C, generator=gen))
    return pt._bn_fold(bn.eval().cuda())


def _bn_gelu_reference(x, scale, shift):
    """-> (gelu(x * scale + shift) in fp64, its bound): 4 fp32 ulps of |x * scale| + |shift| + 1, i.e. the rounding of
    the affine step, of erff and of the three products of gelu, each a fraction of an ulp of that magnitude."""
    x, s, b = x.double().cpu(), scale.double().cpu(), shift.double().cpu()
    return F.gelu(x * s + b), 4 * ULP * ((x * s).abs() + b.abs() + 1.0)


# ------------------------------------------------------------------------------------------------------- rows_norm
ROWS_PER_BLOCK = {32: 32, 64: 16, 128: 8, 256: 4, 512: 4}  # 4 waves x 64 / G rows; G = 8, 16, 32, 64, 64 lanes per row


def _norms(C, gen, eps=1e-5):
    out = []
    for _ in range(2):
        ln = torch.nn.LayerNorm(C, eps=eps)
        with torch.no_grad():
            ln.weight.copy_(1.0 + 0.5 * torch.randn(C, generator=gen))
            ln.bias.copy_(0.3 * torch.randn(C, generator=gen))
        out.append(ln.cuda())
    return out


def _ln64(x, ln):
    return F.layer_norm(x.double().cpu(), x.shape[-1:], ln.weight.detach().double().cpu(),
                        ln.bias.detach().double().cpu(), ln.eps)


def _row_counts(C):
    rpb = ROWS_PER_BLOCK[C]
    return (1, rpb - 1, rpb + 1, 1001)


@pytest.mark.parametrize("with_a", [False, True])
@pytest.mark.parametrize("C", [32, 64, 128, 256, 512])
def test_rows_norm_matches_fp64(C, with_a):
    """s = base + (LN_a(x) if norm_a else x), n = LN_b(s) at every built width, for row counts that leave part of the
    last block's rows dead (1, rows per block -+ 1, a large odd count).  Without norm_a, s is one fp32 add: bit for bit.
    Bound otherwise: 2e-6 of the largest |value| -- a few fp32 ulps of the normalised values, from two-pass statistics
    over at most 512 floats."""
    ops, _ = _mods()
    gen = torch.Generator().manual_seed(C + with_a)
    norm_a, norm_b = _norms(C, gen)
    for rows in _row_counts(C):
        x = torch.randn(rows, C, generator=gen) * 2.0 + 0.5
        base = torch.randn(rows, C, generator=gen)
        s, n = ops.rows_norm(x.cuda(), base.cuda(), norm_b, norm_a=norm_a if with_a else None)
        s, n = s.cpu(), n.cpu()
        if with_a:
            s64 = base.double() + _ln64(x, norm_a)
            assert float((s.double() - s64).abs().max()) <= 2e-6 * float(s64.abs().max()), rows
        else:
            assert torch.equal(s, base + x), rows
            s64 = s.double()
        n64 = _ln64(s64, norm_b)
        err = float((n.double() - n64).abs().max())
        assert err <= 2e-6 * float(n64.abs().max()), (rows, err)


@pytest.mark.parametrize("with_a", [False, True])
@pytest.mark.parametrize("C", [32, 64, 128, 256, 512])
def test_rows_norm_large_mean_rows_against_torch(C, with_a):
    """Rows whose mean is hundreds of standard deviations (cancellation in the variance): the kernel's error, measured
    against fp64, is at most 4x that of torch's own fp32 LayerNorm chain on the device, plus 1e-6 of the largest output."""
    ops, _ = _mods()
    gen = torch.Generator().manual_seed(100 + C + with_a)
    norm_a, norm_b = _norms(C, gen)
    rows = 1001
    x = (30.0 + 0.03 * torch.randn(rows, C, generator=gen)).cuda()
    base = (-20.0 + 0.02 * torch.randn(rows, C, generator=gen)).cuda()
    s, n = ops.rows_norm(x, base, norm_b, norm_a=norm_a if with_a else None)
    with torch.no_grad():
        s_t = base + (norm_a(x) if with_a else x)
        n_t = norm_b(s_t)
    s64 = base.double().cpu() + (_ln64(x, norm_a) if with_a else x.double().cpu())
    n64 = _ln64(s64, norm_b)
    for got, torch_fp32, want in ((s, s_t, s64), (n, n_t, n64)):
        err = float((got.double().cpu() - want).abs().max())
        err_torch = float((torch_fp32.double().cpu() - want).abs().max())
        print(f"rows_norm C={C} norm_a={with_a}: kernel {err:.3e}, torch {err_torch:.3e}")
        assert err <= 4 * err_torch + 1e-6 * float(want.abs().max()), (err, err_torch)


@pytest.mark.parametrize("C", [32, 64, 128, 256, 512])
def test_rows_norm_constant_rows_are_exact(C):
    """Constant rows whose sums are exact in fp32 take the zero-variance path: LN(row) == bias exactly.  Without norm_a:
    s = x, n == bias_b.  With norm_a: LN_a(x) == bias_a (here a constant 0.5), so s == base + 0.5 and, base constant per
    row, n == bias_b."""
    ops, _ = _mods()
    gen = torch.Generator().manual_seed(200 + C)
    norm_a, norm_b = _norms(C, gen)
    with torch.no_grad():
        norm_a.bias.fill_(0.5)
    rows = 1001
    values = torch.tensor([0.75, -3.0, 5.5, 0.0, 1024.0, -0.125])
    x = values[torch.arange(rows) % len(values)][:, None].expand(rows, C).contiguous()
    s, n = ops.rows_norm(x.cuda(), torch.zeros(rows, C).cuda(), norm_b)
    assert torch.equal(s.cpu(), x)
    assert torch.equal(n.cpu(), norm_b.bias.detach().cpu().expand(rows, C))
    base = values[(torch.arange(rows) * 7 + 3) % len(values)][:, None].expand(rows, C).contiguous()
    s, n = ops.rows_norm(x.cuda(), base.cuda(), norm_b, norm_a=norm_a)
    assert torch.equal(s.cpu(), base + 0.5)
    assert torch.equal(n.cpu(), norm_b.bias.detach().cpu().expand(rows, C))


# ----------------------------------------------------------------------------------------------------- cluster_max
def _cluster_reference(x, members, seg, scale, shift):
    m = seg.shape[0] - 1
    cid = torch.repeat_interleave(torch.arange(m), torch.diff(seg))
    of_row = torch.empty_like(cid)
    of_row[members] = cid
    pooled = torch.full((m, x.shape[1]), -float("inf")).scatter_reduce(0, of_row[:, None].expand_as(x), x, "amax")
    return pooled, _bn_gelu_reference(pooled, scale, shift)


@pytest.mark.parametrize("C", [4, 252, 256, 260, 512, 1024])
def test_cluster_max_matches_fp64(C):
    """gelu(max over a cluster's rows * scale + shift) with 151 clusters (not a multiple of the four waves of a block) of
    1, 2 and 8 rows, one of 400 rows in the last, partial block, members a random permutation, and whole clusters below
    zero (a max seeded with 0 would show).  C / 4 sits on both sides of the 64 lanes of a wave and above 128 (the
    channel loop runs 1 to 4 times).  The max is exact; bound per element as _bn_gelu_reference."""
    ops, _ = _mods()
    gen = torch.Generator().manual_seed(300 + C)
    m = 151
    sizes = torch.randint(1, 7, (m,), generator=gen)
    sizes[:3] = torch.tensor([1, 2, 8])
    sizes[-1] = 400
    seg = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(sizes, 0)])
    n = int(seg[-1])
    members = torch.randperm(n, generator=gen)
    x = torch.randn(n, C, generator=gen) * 2.0
    negative = torch.arange(m) % 5 == 1
    for j in negative.nonzero()[:, 0].tolist():
        rows = members[seg[j]:seg[j + 1]]
        x[rows] = -(x[rows].abs() + 0.1)
    scale, shift = _bn_folded(C, gen)
    got = ops.cluster_max(x.cuda(), members.cuda(), seg.cuda(), scale, shift).cpu()
    pooled, (want, tol) = _cluster_reference(x, members, seg, scale, shift)
    assert bool((pooled[negative] < 0).all())
    err = (got.double() - want).abs()
    assert bool((err <= tol).all()), float((err - tol).max())


def test_cluster_max_on_a_real_pooling():
    """members / seg as SerializedPooling hands them over (Level.pool of two clouds), 512 channels as the default
    network pools into; the pool's `cluster` map agrees with its segments.  Bound per element as _bn_gelu_reference."""
    ops, _ = _mods()
    level = _level(_clouds(301, 2, 3000))
    child, cluster, seg = level.pool()
    members = level.order[0]
    seg_c, members_c = seg.cpu(), members.cpu()
    cid = torch.repeat_interleave(torch.arange(child.n), torch.diff(seg_c))
    assert torch.equal(cluster.cpu()[members_c], cid)
    assert int(torch.diff(seg_c).max()) > 1
    gen = torch.Generator().manual_seed(302)
    C = 512
    x = torch.randn(level.n, C, generator=gen)
    scale, shift = _bn_folded(C, gen)
    got = ops.cluster_max(x.cuda(), members, seg, scale, shift).cpu()
    _, (want, tol) = _cluster_reference(x, members_c, seg_c, scale, shift)
    assert bool(((got.double() - want).abs() <= tol).all())


# ---------------------------------------------------------------------------------------------- bn_gelu, unpool_merge
@pytest.mark.parametrize("C", [4, 36, 256, 512, 768])
def test_bn_gelu_and_unpool_merge_match_fp64(C):
    """gelu(x * scale + shift) with BatchNorm folded from randomised running statistics, 1001 rows (rows * C / 4 is not
    a multiple of the 256-thread block), and unpool_merge's gathered add through a many-to-one map (37 parents for
    1001 rows): sum == skip + up[cluster] bit for bit (one fp32 add).  Bound per element as _bn_gelu_reference."""
    ops, _ = _mods()
    gen = torch.Generator().manual_seed(400 + C)
    rows, m = 1001, 37
    assert (rows * C // 4) % 256
    x = torch.randn(rows, C, generator=gen) * 2.0
    scale, shift = _bn_folded(C, gen)
    up = torch.randn(m, C, generator=gen).cuda()
    cluster = torch.randint(0, m, (rows,), generator=gen).cuda()
    want, tol = _bn_gelu_reference(x, scale, shift)
    out = ops.bn_gelu(x.cuda(), scale, shift).cpu()
    assert bool(((out.double() - want).abs() <= tol).all())
    skip, total = ops.unpool_merge(x.cuda(), scale, shift, up, cluster)
    assert bool(((skip.cpu().double() - want).abs() <= tol).all())
    assert torch.equal(total, skip + up[cluster])


# ------------------------------------------------------------------------------------------------------ subm_pair_sum
@pytest.mark.parametrize("taps,cout,bias", [(27, 64, True), (27, 36, False), (125, 32, True), (125, 4, False)])
def test_subm_pair_sum_bit_exact(taps, cout, bias):
    """out = bias (or 0) + products[pair_of[:, t]] for t ascending, one fp32 add each: equal bit for bit to the same
    adds in torch, with rows that hold only the centre tap and taps without any pair.  Products span six decades, so
    any other order of the adds gives other bits (checked)."""
    ops, _ = _mods()
    gen = torch.Generator().manual_seed(500 + taps + cout)
    n = 700
    hit = torch.rand(n, taps, generator=gen) < 0.3
    hit[:, taps // 2] = True                         # the centre tap is the point itself
    hit[:60] = False
    hit[:60, taps // 2] = True                       # rows with only the centre tap
    hit[:, [0, 5, taps - 1]] = False                 # taps with no pairs
    flat = hit.t().reshape(-1)
    idx = torch.cumsum(flat, 0) - 1
    pair_of = torch.where(flat, idx, -1).view(taps, n).t().contiguous().to(torch.int32)
    P = int(flat.sum())
    products = torch.randn(P, cout, generator=gen) * 10.0 ** (6 * torch.rand(P, cout, generator=gen) - 3)
    b = torch.randn(cout, generator=gen) if bias else None
    got = ops.subm_pair_sum(products.cuda(), pair_of.cuda(), None if b is None else b.cuda()).cpu()

    def ordered_sum(taps_in_order):
        acc = b.expand(n, cout).clone() if bias else torch.zeros(n, cout)
        for t in taps_in_order:
            rows = (pair_of[:, t] >= 0).nonzero()[:, 0]
            acc[rows] = acc[rows] + products[pair_of[rows, t].long()]
        return acc

    assert torch.equal(got, ordered_sum(range(taps)))
    assert not torch.equal(got, ordered_sum(reversed(range(taps))))


# ------------------------------------------------------------------------------------------ subm_pair_gemm (both forms)
_GEMM_F, _GEMM_N = 2, 600


@functools.lru_cache(maxsize=None)
def _gemm_clouds():
    return _clouds(600, _GEMM_F, _GEMM_N)


@functools.lru_cache(maxsize=None)
def _oracle_neighbors(ksize):
    from oracle import ptv3 as o_pt

    pts = _gemm_clouds()
    return [o_pt.neighbor_table(o_pt.frame_grid(pts[f]), torch.zeros(_GEMM_N, dtype=torch.long), ksize)
            for f in range(_GEMM_F)]


@pytest.mark.parametrize("ksize", [3, 5])
@pytest.mark.parametrize("cin", [32, 768])
@pytest.mark.parametrize("cout", [32, 96, 64, 192, 128, 512])
def test_subm_pair_gemm_matches_fp64(monkeypatch, cout, cin, ksize):
    """The gather-GEMM's products (fp32 MFMA form, AMAV_SUBM=f32, and the default fp16 x 3 split form) against per-tap
    fp64 products, and SubMConv3d in both forms against oracle.ptv3.subm_conv3d in fp64.  C_out covers every tile width
    (32 / 64 / 128) with one and with several column blocks; C_in one K chunk and the stem's 768; taps whose pair
    count is not a multiple of the 128-pair tile.  Bound: 1e-5 of max(1, largest |value|), as the existing conv test."""
    from oracle import ptv3 as o_pt

    ops, pt = _mods()
    pts = _gemm_clouds()
    level = _level(pts)
    pairs = level.pairs(ksize)
    counts = torch.diff(pairs.tap_start.cpu())
    assert bool((counts % 128 != 0).any()) and int(counts.max()) > 128
    gen = torch.Generator().manual_seed(cin + cout + ksize)
    feat = torch.randn(level.n, cin, generator=gen)
    conv = pt.SubMConv3d(cin, cout, ksize, bias=True)
    with torch.no_grad():
        conv.bias.copy_(0.1 * torch.randn(cout, generator=gen))
    conv = conv.cuda()
    w = conv.tap_weights()
    taps = w.shape[0]

    ts, src = pairs.tap_start.cpu().tolist(), pairs.pair_src.cpu().long()
    f64, w64 = feat.double(), w.cpu().double()
    want = torch.empty(pairs.count, cout, dtype=torch.float64)
    for t in range(taps):
        want[ts[t]:ts[t + 1]] = f64[src[ts[t]:ts[t + 1]]] @ w64[t]
    tol = 1e-5 * max(1.0, float(want.abs().max()))
    args = (feat.cuda(), pairs.pair_src, pairs.tap_start, pairs.tile_start, pairs.tiles)
    got32 = ops.subm_pair_gemm(*args, w).cpu()
    got16 = ops.subm_pair_gemm_split(*args, ops.subm_prepare_weights_split(w), taps, cout).cpu()
    assert float((got32.double() - want).abs().max()) <= tol
    assert float((got16.double() - want).abs().max()) <= tol

    weight, bias = conv.weight.detach().cpu().double(), conv.bias.detach().cpu().double()
    for form in ("f32", "split"):
        monkeypatch.setenv("AMAV_SUBM", form)
        got = conv(feat.cuda(), level).cpu()
        for f, nbr in enumerate(_oracle_neighbors(ksize)):
            rows = slice(f * _GEMM_N, (f + 1) * _GEMM_N)
            ref = o_pt.subm_conv3d(f64[rows], nbr, weight, bias)
            err = float((got[rows].double() - ref).abs().max())
            assert err <= 1e-5 * max(1.0, float(ref.abs().max())), (form, f, err)


# ---------------------------------------------------------------------------------------------------- patch_attention
@pytest.mark.parametrize("peaked", [False, True])
@pytest.mark.parametrize("heads,dim", [(32, 16), (2, 16), (16, 32), (4, 64)])
def test_patch_attention_default_widths(heads, dim, peaked):
    """Patch 512 at every head dim the default network runs, clouds of 1, 63, 64, 65, 511, 512, 513 and 1300 points in
    one call: clouds smaller than a key tile, partial key tiles, borrowed tails and several query blocks per patch.  An
    explicit scale that is not D^-0.5, or queries x 10 (a peaked softmax).  Restatement and bound of
    test_patch_attention_matches_oracle (2e-6 of the largest output); with logits of magnitude ~100 (the peaked case)
    their fp32 rounding alone moves the probabilities by more than that, so the bound there is 4x the error of the same
    restatement run in fp32."""
    from oracle import ptv3 as o_pt

    ops, pt = _mods()
    counts = [1, 63, 64, 65, 511, 512, 513, 1300]
    C, n = heads * dim, sum(counts)
    gen = torch.Generator().manual_seed(700 + heads + dim + peaked)
    qkv = torch.randn(n, 3 * C, generator=gen)
    scale = None if peaked else 0.37
    if peaked:
        qkv[:, :C] *= 10.0
    starts = np.concatenate([[0], np.cumsum(counts)])
    order = torch.cat([torch.randperm(c, generator=gen) + int(s) for c, s in zip(counts, starts)])
    level = pt.Level.__new__(pt.Level)
    level.counts, level.starts_host = counts, starts.astype(np.int32)
    level.grid, level._patches = qkv.cuda(), {}
    desc, max_patch = level.patches(512)
    assert max_patch == 512
    got = ops.patch_attention(qkv.cuda(), order.cuda(), desc, heads, max_patch, scale=scale).cpu()
    s = dim ** -0.5 if scale is None else scale

    def restated(dtype):
        out = torch.empty(n, C, dtype=dtype)
        for c, start in zip(counts, starts):
            o = order[start:start + c] - start
            inv = torch.empty_like(o)
            inv[o] = torch.arange(c)
            K, pad, unpad = o_pt.patch_layout(c, 512)
            x = qkv[start:start + c].to(dtype)[o[pad]]
            q, k, v = x.reshape(-1, K, 3, heads, dim).permute(2, 0, 3, 1, 4).unbind(0)
            att = torch.softmax((q * s) @ k.transpose(-2, -1), -1)
            out[start:start + c] = (att @ v).transpose(1, 2).reshape(-1, C)[unpad[inv]]
        return out

    want = restated(torch.float64)
    err = float((got.double() - want).abs().max())
    err32 = float((restated(torch.float32).double() - want).abs().max())
    print(f"patch_attention heads={heads} dim={dim} peaked={peaked}: {err:.3e}, fp32 restatement {err32:.3e} "
          f"(largest |out| {float(want.abs().max()):.2f})")
    assert err <= max(2e-6 * max(1.0, float(want.abs().max())), 4 * err32 if peaked else 0.0)


# -------------------------------------------------------------------------------------------- serialisation bookkeeping
def test_serialisation_of_mixed_cloud_sizes_bit_exact():
    """Clouds of 1-3 points between two of ~2000 in one pass: grid, depth, the four keys, the orders and the neighbour
    tables (k = 3, 5) of every cloud equal oracle.ptv3's for that cloud alone, and Level.patches gives every cloud its
    own patches (the positions each patch reads are the cloud's own, in the reference's padding layout)."""
    from oracle import ptv3 as o_pt

    ops, pt = _mods()
    counts = [2000, 1, 3, 2, 1900]
    gen = torch.Generator().manual_seed(800)
    clouds = []
    for f, c in enumerate(counts):
        if c > 100:
            clouds.append(_clouds(801 + f, 1, c)[0])
        else:
            clouds.append(torch.randn(1, 3, generator=gen) * 0.3 + 0.02 * torch.randn(c, 3, generator=gen))
    pts = torch.cat(clouds)
    cloud_of = torch.repeat_interleave(torch.arange(len(counts), dtype=torch.int32), torch.tensor(counts)).cuda()
    grid, depth = ops.cloud_voxelize(pts.cuda(), cloud_of, len(counts))
    level = pt.Level(grid, cloud_of, depth, np.asarray(counts), ops.cloud_codes(grid, cloud_of, depth))
    starts = level.starts_host
    keys, order = level.keys.cpu(), level.order.cpu()
    for f, c in enumerate(counts):
        a, b = int(starts[f]), int(starts[f + 1])
        g = o_pt.frame_grid(pts[a:b])
        assert torch.equal(grid[a:b].cpu().long(), g), f
        code, o_order, _, d = o_pt.serialization(g, torch.zeros(c, dtype=torch.long))
        assert int(depth[f]) == d, f
        assert torch.equal(keys[:, a:b] & ((1 << 48) - 1), code), f
        assert bool((keys[:, a:b] >> 48 == f).all()), f
        assert torch.equal(order[:, a:b] - a, o_order), f
        for ksize in (3, 5):
            nbr = level.neighbors(ksize)[a:b].cpu().long()
            nbr = torch.where(nbr >= 0, nbr - a, nbr)
            assert torch.equal(nbr, o_pt.neighbor_table(g, torch.zeros(c, dtype=torch.long), ksize)), (f, ksize)
    desc, max_patch = level.patches(512)
    assert max_patch == 512
    desc = desc.cpu().tolist()
    for f, c in enumerate(counts):
        a = int(starts[f])
        mine = [(first, K, own) for first, K, own, _ in desc if a <= first < int(starts[f + 1])]
        K, pad, _ = o_pt.patch_layout(c, 512)
        assert len(mine) == len(pad) // K, f
        for i, (first, k, own) in enumerate(mine):
            assert k == K and 0 < own <= K, (f, i)
            reads = [first + j - (K if j >= own else 0) - a for j in range(K)]
            assert reads == pad[i * K:(i + 1) * K].tolist(), (f, i)
    assert len(desc) == sum((c + min(c, 512) - 1) // min(c, 512) for c in counts)


# ------------------------------------------------------------------------------------------ Block with two LayerNorm eps
def _block64(block, feat, nbr, order, inverse, cpe_eps):
    """pointtransformer_v3.py:595-615 in fp64 with every LayerNorm's own eps (cpe.2's given)."""
    from oracle import ptv3 as o_pt

    p = {k: v.detach().cpu().double() for k, v in block.state_dict().items()}
    ln = lambda x, name, eps: F.layer_norm(x, x.shape[-1:], p[name + ".weight"], p[name + ".bias"], eps)
    x = o_pt.subm_conv3d(feat, nbr, p["cpe.0.weight"], p["cpe.0.bias"])
    feat = feat + ln(F.linear(x, p["cpe.1.weight"], p["cpe.1.bias"]), "cpe.2", cpe_eps)
    attn = block.attn
    feat = feat + o_pt.serialized_attention(p, "attn.", ln(feat, "norm1.0", block.norm1[0].eps), order, inverse,
                                            attn.num_heads, attn.patch_size)
    x = ln(feat, "norm2.0", block.norm2[0].eps)
    x = F.linear(F.gelu(F.linear(x, p["mlp.0.fc1.weight"], p["mlp.0.fc1.bias"])), p["mlp.0.fc2.weight"],
                 p["mlp.0.fc2.bias"])
    return feat + x


def test_block_with_its_own_cpe_eps_matches_fp64():
    """A Block whose cpe.2 LayerNorm has eps 1e-3 (norm1: 1e-5) is normalised with that eps.  cpe.1 is scaled so its
    output variance is ~1e-3, where the two eps give outputs far apart (checked).  Bound: the network tests' 1e-4."""
    from oracle import ptv3 as o_pt

    _, pt = _mods()
    C, N = 64, 900
    pts = _clouds(900, 1, N)
    level = _level(pts)
    block = pt.Block(C, 4, 128, 4, 1)
    block.cpe[2].eps = 1e-3
    gen = torch.Generator().manual_seed(901)
    feat = torch.randn(N, C, generator=gen)
    grid = o_pt.frame_grid(pts[0])
    nbr = o_pt.neighbor_table(grid, torch.zeros(N, dtype=torch.long), 3)
    _, order, inverse, _ = o_pt.serialization(grid, torch.zeros(N, dtype=torch.long))
    with torch.no_grad():
        x = o_pt.subm_conv3d(feat.double(), nbr, block.cpe[0].weight.double(), block.cpe[0].bias.double())
        y = F.linear(x, block.cpe[1].weight.double(), block.cpe[1].bias.double())
        f = float((1e-3 / y.var(-1, unbiased=False).mean()) ** 0.5)
        block.cpe[1].weight.mul_(f)
        block.cpe[1].bias.mul_(f)
    with torch.no_grad():
        got = block.cuda()(feat.cuda(), level).cpu()
    want = _block64(block, feat.double(), nbr, order[1], inverse[1], 1e-3)
    other = _block64(block, feat.double(), nbr, order[1], inverse[1], 1e-5)
    tol = 1e-4 * max(1.0, float(want.abs().max()))
    assert float((other - want).abs().max()) > 100 * tol
    err = float((got.double() - want).abs().max())
    assert err <= tol, err
