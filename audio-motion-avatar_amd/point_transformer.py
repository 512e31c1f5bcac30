"""Point refiner: the reference's PTv3Encoder / PointTransformerV3 on MI355X.

Mirrors src/models/point_transformer/point_encoder.py:6-40 and pointtransformer_v3.py:795-991 -- same constructor
arguments, same module tree, so `point_encoder.point_transformer.*` checkpoint keys load -- with the deterministic
semantics of DESIGN.md section 4.5 (the reference permutes its serialisation orders with an unseeded randperm, feeds
negative grid coordinates to its encoders and puts several points into one voxel of spconv's hash: it defines no
reproducible output):

  * orders keep their configured sequence (z, z-trans, hilbert, hilbert-trans);
  * every cloud (frame) is processed as the reference processes a batch of ONE: grid origin, serialisation depth and
    attention patch size are the cloud's own, so frames stay independent (they are the unit of data parallelism);
  * sorts are stable; a voxel is seen by neighbouring voxels through its lowest-index point.

All clouds of a pass run batched: one key sort per order, one neighbour / pair table per level, one gather-GEMM per
convolution (only the voxel pairs that exist) + an ordered sum, one attention launch per block (patches of all clouds).  The sparse /
serialised operators are HIP kernels (csrc/cloud.hip); Linear / LayerNorm / sort / prefix sums are torch library calls
on the same stream.

Inference by default.  `PointTransformerV3(..., differentiable=True)` (cfg.differentiable_refiner for PTv3Encoder) makes
the network trainable: under grad mode, when `feat` or a parameter requires grad, the forward records an autograd graph
whose sparse / serialised operators have HIP backwards (csrc/cloud_backward.hip) and whose Linear /
LayerNorm / GELU / BatchNorm arithmetic differentiates through torch.  What is differentiated is the function the
inference forward computes: the deterministic serialisation, BatchNorm with its RUNNING statistics (constants; weight and
bias receive gradients), DropPath as the identity.  `.train()` changes nothing: this is fine-tuning with frozen
statistics, the reference's train-mode batch statistics and stochastic depth are not reproduced.  Gradients go to `feat`
and to every floating-point parameter; `points` get none (the network sees coordinates through the integer grid only).
Gradients are bitwise reproducible (no atomics).

`PointTransformerV3(..., batch_statistics=True)` (cfg.refiner_batch_statistics for PTv3Encoder) opts into the reference's
training function, and only while the module is in `.train()`: the 13 BatchNorm1d layers (stem, poolings, both branches
of the unpoolings) normalise with the statistics of the batch -- every row of every cloud of one forward call, at a
pooling the pooled rows --, differentiate through them (csrc/cloud_norm.hip) and update their
running buffers on the device; every Block applies DropPath per point to its attention and MLP branches (not to the
cpe branch) with rates rising to `drop_path`, the masks drawn from `drop_path_generator`.  With the flag on, `.eval()` is
the forward described above bit for bit; with it off (the default) so is `.train()`.
"""
import os
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from ._lib import AmavError

ORDERS = ("z", "z-trans", "hilbert", "hilbert-trans")
_CODE_MASK = (1 << 48) - 1


class SubMConv3d(nn.Module):
    """Parameter holder with spconv 2.x's SubMConv3d layout: weight [C_out, k, k, k, C_in] (+ bias)."""

    def __init__(self, in_channels, out_channels, kernel_size, bias=True):
        super().__init__()
        self.in_channels, self.out_channels, self.kernel_size = in_channels, out_channels, kernel_size
        k = kernel_size
        self.weight = nn.Parameter(torch.empty(out_channels, k, k, k, in_channels))
        nn.init.kaiming_uniform_(self.weight.view(out_channels, -1), a=5 ** 0.5)
        self.bias = nn.Parameter(torch.zeros(out_channels)) if bias else None
        self._flat = None
        self._split = None  # (the tap_weights() tensor it was made from, its fp16 x 2 form)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        w = state_dict.get(prefix + "weight")
        k = self.kernel_size
        if w is not None and tuple(w.shape) == (k, k, k, self.in_channels, self.out_channels) != tuple(self.weight.shape):
            state_dict[prefix + "weight"] = w.permute(4, 0, 1, 2, 3).contiguous()  # spconv 1.x / 2.0 layout
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def tap_weights(self):
        """[taps, C_in (padded to a multiple of 32), C_out]: one B operand per tap."""
        ver = (ops.tensor_version(self.weight), self.weight.data_ptr())
        if self._flat is None or self._flat[0] != ver:
            w = self.weight.detach().reshape(self.out_channels, -1, self.in_channels).permute(1, 2, 0)
            pad = -self.in_channels % 32
            self._flat = (ver, (F.pad(w, (0, 0, 0, pad)) if pad else w).contiguous())
        return self._flat[1]

    def forward(self, feat, level, differentiable=False):
        """feat [n, C_in] -> [n, C_out]: gather-GEMM over the level's (row, neighbour row) pairs, then the ordered sum.
        differentiable: the same kernels as an autograd node (ops.subm_conv_differentiable)."""
        pairs = level.pairs(self.kernel_size)
        if differentiable:
            return ops.subm_conv_differentiable(feat, self, pairs)
        return self.run_kernels(feat, pairs)

    def run_kernels(self, feat, pairs):
        pad = -self.in_channels % 32
        if pad:
            feat = F.pad(feat, (0, pad))
        w = self.tap_weights()
        if os.environ.get("AMAV_SUBM", "split") == "f32":  # the fp32 MFMA form
            products = ops.subm_pair_gemm(feat, pairs.pair_src, pairs.tap_start, pairs.tile_start, pairs.tiles, w)
        else:  # three fp16 partial products per fp32 product (csrc/cloud.hip, pair_gemm_f16_kernel)
            if self._split is None or self._split[0] is not w:
                self._split = (w, ops.subm_prepare_weights_split(w))
            products = ops.subm_pair_gemm_split(feat.contiguous(), pairs.pair_src, pairs.tap_start, pairs.tile_start,
                                                pairs.tiles, self._split[1], w.shape[0], w.shape[2])
        return ops.subm_pair_sum(products, pairs.pair_of, None if self.bias is None else self.bias.detach())


def _bn_fold(bn):
    """BatchNorm1d in eval mode as (scale, shift)."""
    ver = tuple(ops.tensor_version(t) for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var)) + (bn.weight.data_ptr(),)
    cached = getattr(bn, "_amav_fold", None)
    if cached is None or cached[0] != ver:
        scale = bn.weight.detach() / torch.sqrt(bn.running_var + bn.eps)
        cached = (ver, scale.contiguous(), (bn.bias.detach() - bn.running_mean * scale).contiguous())
        bn._amav_fold = cached
    return cached[1], cached[2]


def _bn_live(bn):
    """_bn_fold from the live parameters, for autograd: weight and bias receive gradients, the statistics are constants."""
    scale = bn.weight / torch.sqrt(bn.running_var + bn.eps)
    return scale, bn.bias - bn.running_mean * scale


def _bn_gelu_live(x, bn):
    scale, shift = _bn_live(bn)
    return F.gelu(x * scale + shift)


def _bn(channels):
    return nn.BatchNorm1d(channels, eps=1e-3, momentum=0.01)  # pointtransformer_v3.py:857


def _bn_track(bn, mean, var, rows):
    """BatchNorm1d's train-mode buffer update from the batch's mean and BIASED variance over `rows` rows, on the device."""
    if bn.momentum is None:
        raise AmavError("train-mode BatchNorm: momentum=None (the cumulative average) is not built")
    with torch.no_grad():
        m = float(bn.momentum)
        bn.running_mean.mul_(1.0 - m).add_(mean, alpha=m)
        bn.running_var.mul_(1.0 - m).add_(var, alpha=m * rows / (rows - 1.0))
        bn.num_batches_tracked += 1


def _bn_rows(x, where):
    rows = int(x.shape[0])
    if rows < 2:
        raise AmavError(f"{where}: {rows} row(s) -- train-mode BatchNorm needs at least 2 values per channel")
    return rows


def _bn_gelu_train(x, bn, where):
    """gelu(BatchNorm(x)) with the statistics of the rows of x (differentiable through them when a graph is recorded),
    and the update of bn's running buffers."""
    rows = _bn_rows(x, where)
    out, mean, var = ops.bn_gelu_train_differentiable(x, bn.weight, bn.bias, bn.eps)
    _bn_track(bn, mean, var, rows)
    return out


def _drop_path_mask(n, rate, generator):
    """The keep mask of DropPath over n points, float [n, 1] of 0 / 1: a point keeps a branch with probability 1 - rate
    (timm's DropPath on `point.feat [N, C]`, pointtransformer_v3.py:591-610: one draw per row)."""
    return torch.empty(n, 1, device=generator.device).bernoulli_(1.0 - rate, generator=generator)


class MLP(nn.Module):
    def __init__(self, channels, hidden):
        super().__init__()
        self.fc1, self.fc2 = nn.Linear(channels, hidden), nn.Linear(hidden, channels)

    def forward(self, x):
        return self.fc2(F.gelu(self.fc1(x)))


class SerializedAttention(nn.Module):
    """pointtransformer_v3.py:328-499 (enable_flash=False: patch = min(points of the cloud, patch_size))."""

    def __init__(self, channels, num_heads, patch_size, order_index):
        super().__init__()
        if channels % num_heads or channels // num_heads not in (16, 32, 64):
            raise AmavError(f"SerializedAttention: head dim {channels}/{num_heads} (16, 32 and 64 are built)")
        self.channels, self.num_heads, self.patch_size, self.order_index = channels, num_heads, patch_size, order_index
        self.qkv = nn.Linear(channels, channels * 3)
        self.proj = nn.Linear(channels, channels)

    def forward(self, feat, level, differentiable=False):
        desc, max_patch = level.patches(self.patch_size)
        attention = ops.patch_attention_differentiable if differentiable else ops.patch_attention
        out = attention(self.qkv(feat), level.order[self.order_index], desc, self.num_heads, max_patch)
        return self.proj(out)


class Block(nn.Module):
    """pointtransformer_v3.py:528-615 (pre-norm; DropPath is the identity at inference).  drop_path: the Block's rate,
    applied only when forward is handed a generator (PointTransformerV3 with batch_statistics, in .train())."""

    def __init__(self, channels, num_heads, patch_size, mlp_ratio, order_index, drop_path=0.0):
        super().__init__()
        self.drop_path = float(drop_path)
        self.cpe = nn.Sequential(SubMConv3d(channels, channels, 3), nn.Linear(channels, channels), nn.LayerNorm(channels))
        self.norm1 = nn.Sequential(nn.LayerNorm(channels))
        self.attn = SerializedAttention(channels, num_heads, patch_size, order_index)
        self.norm2 = nn.Sequential(nn.LayerNorm(channels))
        self.mlp = nn.Sequential(MLP(channels, int(channels * mlp_ratio)))

    def forward(self, feat, level, conv_in=None, differentiable=False, drop_generator=None):
        x = self.cpe[0](feat if conv_in is None else conv_in, level, differentiable)
        if drop_generator is not None and self.drop_path > 0.0:
            keep = 1.0 - self.drop_path
            feat = feat + self.cpe[2](self.cpe[1](x))
            branch = self.attn(self.norm1(feat), level, differentiable)
            feat = feat + branch * (_drop_path_mask(feat.shape[0], self.drop_path, drop_generator) / keep)
            branch = self.mlp(self.norm2(feat))
            return feat + branch * (_drop_path_mask(feat.shape[0], self.drop_path, drop_generator) / keep)
        # feat += LayerNorm(cpe linear); norm1 -- and feat += attention; norm2 -- as one pass over the rows each (the
        # fused pass normalises with one eps; it has no backward, so the differentiable path takes the library branch)
        if not differentiable and feat.shape[1] in (32, 64, 128, 256, 512) and self.cpe[2].eps == self.norm1[0].eps:
            feat, n1 = ops.rows_norm(self.cpe[1](x), feat, self.norm1[0], norm_a=self.cpe[2])
            feat, n2 = ops.rows_norm(self.attn(n1, level), feat, self.norm2[0])
            return feat + self.mlp(n2)
        feat = feat + self.cpe[2](self.cpe[1](x))  # other widths or two eps: library LayerNorm
        feat = feat + self.attn(self.norm1(feat), level, differentiable)
        return feat + self.mlp(self.norm2(feat))


class SerializedPooling(nn.Module):
    """pointtransformer_v3.py:618-721: stride-2 grid pooling along the z-order (max), BatchNorm, GELU."""

    def __init__(self, in_channels, out_channels, stride):
        super().__init__()
        if stride != 2:
            raise AmavError(f"SerializedPooling: stride {stride} (the reference configures 2 everywhere)")
        self.proj = nn.Linear(in_channels, out_channels)
        self.norm = nn.Sequential(_bn(out_channels))
        self.level = 1  # the level it pools into (PointTransformerV3 numbers its poolings), for error messages

    def forward(self, feat, level, differentiable=False, batch_stats=False):
        """-> (pooled features, child level, cluster, (members, seg): the clusters' member lists).
        batch_stats: BatchNorm with the statistics of the pooled rows (module docstring)."""
        child, cluster, seg = level.pool()
        if batch_stats:
            bn = self.norm[0]
            if child.n < 2:
                raise AmavError(f"pooling into level {self.level}: {child.n} pooled row(s) -- train-mode BatchNorm needs at least 2 values per "
                                "channel; use a larger cloud or fewer stages")
            pooled, mean, var = ops.cluster_max_bn_train_differentiable(self.proj(feat), level.order[0], seg, bn.weight,
                                                                        bn.bias, bn.eps)
            _bn_track(bn, mean, var, child.n)
        elif differentiable:
            pooled = ops.cluster_max_differentiable(self.proj(feat), level.order[0], seg, *_bn_live(self.norm[0]))
        else:
            pooled = ops.cluster_max(self.proj(feat), level.order[0], seg, *_bn_fold(self.norm[0]))
        return pooled, child, cluster, (level.order[0], seg)


class SerializedUnpooling(nn.Module):
    """pointtransformer_v3.py:724-759: both branches Linear + BatchNorm + GELU, parent += child[cluster]."""

    def __init__(self, in_channels, skip_channels, out_channels):
        super().__init__()
        self.proj = nn.Sequential(nn.Linear(in_channels, out_channels), _bn(out_channels))
        self.proj_skip = nn.Sequential(nn.Linear(skip_channels, out_channels), _bn(out_channels))

    def forward(self, child_feat, parent_feat, cluster, members=None, batch_stats=False, where="unpooling"):
        """members: (members, seg) of the pooling that made the child level -> the differentiable path.
        batch_stats: both BatchNorms with the statistics of their own rows (module docstring)."""
        if batch_stats and members is not None:
            up = _bn_gelu_train(self.proj[0](child_feat), self.proj[1], where + " (proj)")
            skip = _bn_gelu_train(self.proj_skip[0](parent_feat), self.proj_skip[1], where + " (proj_skip)")
            return skip, skip + ops.cluster_gather_differentiable(up, cluster, *members)
        if batch_stats:  # forward only: the statistics kernel, then the fused inference kernels on (scale, shift)
            up = _bn_gelu_train(self.proj[0](child_feat), self.proj[1], where + " (proj)")
            x, bn = self.proj_skip[0](parent_feat), self.proj_skip[1]
            rows = _bn_rows(x, where + " (proj_skip)")
            if ops.refiner_bn_library():
                skip = _bn_gelu_train(x, bn, where + " (proj_skip)")
                return skip, skip + up[cluster]
            scale, shift, mean, var, _ = ops.bn_train_fold(x, bn.weight, bn.bias, bn.eps)
            _bn_track(bn, mean, var, rows)
            return ops.unpool_merge(x, scale, shift, up, cluster)
        if members is not None:
            up = _bn_gelu_live(self.proj[0](child_feat), self.proj[1])
            skip = _bn_gelu_live(self.proj_skip[0](parent_feat), self.proj_skip[1])
            return skip, skip + ops.cluster_gather_differentiable(up, cluster, *members)
        up = ops.bn_gelu(self.proj[0](child_feat), *_bn_fold(self.proj[1]))
        # -> (skip branch, sum): the next block's convolution reads the skip branch alone (the reference refreshes the
        # parent's sparse tensor in proj_skip, :250-255, but not after the sum at :755), its shortcut is the sum
        return ops.unpool_merge(self.proj_skip[0](parent_feat), *_bn_fold(self.proj_skip[1]), up, cluster)


class Pairs(SimpleNamespace):
    """The pair tables of one (level, kernel size), Level.pairs(); the backward's tables are built on first use, on the
    device, without a host synchronisation."""

    @property
    def pair_dst(self):
        """int32 [P]: the row that owns each pair (pair_of inverted)."""
        if "_pair_dst" not in self.__dict__:
            n, taps = self.pair_of.shape
            dev = self.pair_of.device
            slot = torch.where(self.pair_of >= 0, self.pair_of, self.count).long().reshape(-1)  # misses -> a spare slot
            buf = torch.empty(self.count + 1, dtype=torch.int32, device=dev)
            buf[slot] = torch.arange(n, dtype=torch.int32, device=dev).repeat_interleave(taps)
            self._pair_dst = buf[:self.count].contiguous()
        return self._pair_dst

    def _csr(self):
        if "_src_pairs" not in self.__dict__:
            sorted_src, perm = torch.sort(self.pair_src, stable=True)
            rows = torch.arange(self.pair_of.shape[0] + 1, dtype=torch.int32, device=perm.device)
            self._src_pairs = perm.to(torch.int32)
            self._src_start = torch.searchsorted(sorted_src, rows).to(torch.int32)
        return self._src_start, self._src_pairs

    @property
    def src_start(self):
        """int32 [n+1]: CSR by source row over src_pairs."""
        return self._csr()[0]

    @property
    def src_pairs(self):
        """int32 [P]: the stable sort of pair_src, so a row's pairs ascend."""
        return self._csr()[1]

    def wgrad_slices(self, cin, cout):
        """-> (chunk, slice_start int32 [taps+1] on the device, slices) of ops.subm_pair_wgrad for these widths."""
        key = ("_slices", cin, cout)
        if key not in self.__dict__:
            chunk, table = ops.subm_wgrad_slices(np.diff(self.tap_start_host.astype(np.int64)), cin, cout)
            self.__dict__[key] = (chunk, torch.from_numpy(table).to(self.pair_of.device), int(table[-1]))
        return self.__dict__[key]


class Level:
    """Serialisation state of all clouds at one resolution (what the reference keeps in a `Point`)."""

    def __init__(self, grid, cloud_of, depth, counts, keys):
        self.grid, self.cloud_of, self.depth, self.counts, self.keys = grid, cloud_of, depth, counts, keys
        self.n = int(grid.shape[0])
        dev = grid.device
        starts = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        self.starts_host = starts
        self.cloud_start = torch.from_numpy(starts).to(dev)
        self.sorted_keys, self.order = torch.sort(keys, dim=1, stable=True)  # [4,n] each
        self._nbr, self._patches, self._pairs = {}, {}, {}

    def neighbors(self, ksize):
        if ksize not in self._nbr:
            self._nbr[ksize] = ops.cloud_neighbors(self.grid, self.cloud_of, self.depth, self.cloud_start,
                                                   self.sorted_keys[0], self.order[0], ksize)
        return self._nbr[ksize]

    def pairs(self, ksize):
        """The (neighbour row -> row) pairs of a ksize^3 submanifold convolution, grouped by tap (rows ascending inside
        a tap): pair_src int32 [P], pair_of int32 [n, taps] (-1: empty voxel), tap_start / tile_start int32 [taps+1]
        (tiles of 128 pairs, what amav_subm_pair_gemm launches); pair_dst / src_start / src_pairs (the backward's tables)
        on first use."""
        if ksize not in self._pairs:
            nbr = self.neighbors(ksize)
            taps, dev = nbr.shape[1], nbr.device
            hit = nbr.t() >= 0                                   # [taps, n]
            flat = hit.reshape(-1)
            idx = torch.cumsum(flat, 0) - 1
            ends = (idx[self.n - 1::self.n] + 1).cpu().numpy()   # one host sync per (level, kernel size)
            tap_start = np.concatenate([[0], ends]).astype(np.int32)
            counts = np.diff(tap_start).astype(np.int64)
            tile_start = np.concatenate([[0], np.cumsum((counts + 127) // 128)]).astype(np.int32)
            pair_of = torch.where(flat, idx, -1).view(taps, self.n).t().contiguous().to(torch.int32)
            self._pairs[ksize] = Pairs(
                pair_src=nbr.t()[hit].contiguous(), pair_of=pair_of, tap_start=torch.from_numpy(tap_start).to(dev),
                tile_start=torch.from_numpy(tile_start).to(dev), tiles=int(tile_start[-1]), count=int(tap_start[-1]),
                tap_start_host=tap_start, tile_start_host=tile_start)
        return self._pairs[ksize]

    def patches(self, patch_size):
        """patch_desc [P,4] int32 (first, K, own, 0) for every patch of every cloud + the largest K."""
        if patch_size not in self._patches:
            rows = []
            for f, c in enumerate(self.counts):
                if c <= 0:
                    continue
                K = min(int(c), patch_size)
                base = int(self.starts_host[f])
                rows += [(base + p, K, min(K, int(c) - p), 0) for p in range(0, int(c), K)]
            desc = torch.from_numpy(np.asarray(rows, dtype=np.int32).reshape(-1, 4)).to(self.grid.device)
            self._patches[patch_size] = (desc, max(r[1] for r in rows))
        return self._patches[patch_size]

    def pool(self):
        """-> (child Level, cluster int64 [n]: child row of every point, seg int64 [m+1] over order[0])."""
        dev = self.grid.device
        shift = (self.depth >= 1).to(torch.int64)                 # pointtransformer_v3.py:649-651, per cloud
        sh3 = (shift * 3)[self.cloud_of.long()]
        pkeys = (self.keys & ~_CODE_MASK) | ((self.keys & _CODE_MASK) >> sh3)
        order0 = self.order[0]
        sp = pkeys[0][order0]
        first = torch.ones(self.n, dtype=torch.bool, device=dev)
        first[1:] = sp[1:] != sp[:-1]
        cid = torch.cumsum(first, 0) - 1
        seg_head = torch.nonzero(first)[:, 0]
        m = int(seg_head.shape[0])
        seg = torch.cat([seg_head, torch.tensor([self.n], device=dev)])
        head = order0[seg_head]
        cluster = torch.empty(self.n, dtype=torch.int64, device=dev)
        cluster[order0] = cid
        ccloud = self.cloud_of[head]
        counts = torch.bincount(ccloud.long(), minlength=len(self.counts)).cpu().numpy()
        cgrid = self.grid[head] >> shift[ccloud.long()].to(torch.int32)[:, None]
        child = Level(cgrid.contiguous(), ccloud.contiguous(), (self.depth - shift.to(torch.int32)).contiguous(), counts,
                      pkeys[:, head].contiguous())
        assert child.n == m
        return child, cluster, seg


class PointTransformerV3(nn.Module):
    """pointtransformer_v3.py:795-991 (cls_mode=False, no PDNorm, no RPE, no flash): constructor arguments by the
    reference's names; `drop_path`, `shuffle_orders`, `enable_flash` are accepted and have no effect at inference /
    are replaced by the deterministic semantics above.  `batch_statistics`: in .train(), BatchNorm with batch statistics
    and running-buffer updates, and DropPath with rates linspace(0, drop_path) over the encoder's blocks and over the
    decoder's (reversed inside a stage, :879-937), masks from `drop_path_generator` (a torch.Generator on the device,
    made on first use; assign or seed it to fix a run); off by default, and then .train() changes nothing.  `differentiable`: record an autograd graph when something
    requires grad (module docstring); off by default, and then `forward` is the inference path whatever the grad mode."""

    def __init__(self, in_channels=6, order=ORDERS, stride=(2, 2, 2, 2), enc_depths=(2, 2, 2, 6, 2),
                 enc_channels=(32, 64, 128, 256, 512), enc_num_head=(2, 4, 8, 16, 32),
                 enc_patch_size=(1024, 1024, 1024, 1024, 1024), dec_depths=(2, 2, 2, 2), dec_channels=(64, 64, 128, 256),
                 dec_num_head=(4, 4, 8, 16), dec_patch_size=(1024, 1024, 1024, 1024), mlp_ratio=4, drop_path=0.3,
                 shuffle_orders=True, enable_flash=False, grid_resolution=100, differentiable=False, batch_statistics=False):
        super().__init__()
        self.differentiable = bool(differentiable)
        self.batch_statistics = bool(batch_statistics)
        self.drop_path = float(drop_path)
        self.drop_path_generator = None
        enc_rates = torch.linspace(0, self.drop_path, sum(enc_depths)).tolist()  # :879-881
        dec_rates = torch.linspace(0, self.drop_path, sum(dec_depths)).tolist()  # :924-926
        if tuple(order) != ORDERS:
            raise AmavError(f"PointTransformerV3: orders {tuple(order)} (the kernels build {ORDERS})")
        stages = len(enc_depths)
        if not (stages == len(stride) + 1 == len(enc_channels) == len(enc_num_head) == len(enc_patch_size)
                == len(dec_depths) + 1 == len(dec_channels) + 1 == len(dec_num_head) + 1 == len(dec_patch_size) + 1):
            raise AmavError("PointTransformerV3: stage lists of inconsistent length")  # :835-843
        self.num_stages, self.grid_resolution = stages, float(grid_resolution)
        self.enc_depths, self.dec_depths = tuple(enc_depths), tuple(dec_depths)
        self.embedding = nn.Module()
        self.embedding.stem = nn.Module()
        self.embedding.stem.conv = SubMConv3d(in_channels, enc_channels[0], 5, bias=False)  # :776-784 (padding ignored)
        self.embedding.stem.norm = _bn(enc_channels[0])
        self.enc = nn.Module()
        for s in range(stages):
            enc = nn.Module()
            if s > 0:
                enc.down = SerializedPooling(enc_channels[s - 1], enc_channels[s], stride[s - 1])
                enc.down.level = s
            rates = enc_rates[sum(enc_depths[:s]):sum(enc_depths[:s + 1])]
            for i in range(enc_depths[s]):
                setattr(enc, f"block{i}", Block(enc_channels[s], enc_num_head[s], enc_patch_size[s], mlp_ratio,
                                                i % len(ORDERS), rates[i]))
            setattr(self.enc, f"enc{s}", enc)
        self.dec = nn.Module()
        dec_channels = list(dec_channels) + [enc_channels[-1]]
        for s in reversed(range(stages - 1)):
            dec = nn.Module()
            dec.up = SerializedUnpooling(dec_channels[s + 1], enc_channels[s], dec_channels[s])
            rates = dec_rates[sum(dec_depths[:s]):sum(dec_depths[:s + 1])][::-1]  # :931-934
            for i in range(dec_depths[s]):
                setattr(dec, f"block{i}", Block(dec_channels[s], dec_num_head[s], dec_patch_size[s], mlp_ratio,
                                                i % len(ORDERS), rates[i]))
            setattr(self.dec, f"dec{s}", dec)
        self.out_channels = dec_channels[0]

    def forward(self, points, feat):
        """points [F,N,3], feat [F,N,C_in] (fp32, HIP device) -> [F*N, dec_channels[0]] in the input's point order.
        Runs under no_grad unless the network was built with differentiable=True, grad mode is on and `feat` or a
        parameter requires grad; then gradients reach `feat` and the parameters (never `points`)."""
        if (self.differentiable and torch.is_grad_enabled()
                and (feat.requires_grad or any(p.requires_grad for p in self.parameters()))):
            return self._run(points.detach(), feat, True)
        with torch.no_grad():
            return self._run(points, feat, False)

    def _run(self, points, feat, diff):
        Fc, N, _ = points.shape
        n = Fc * N
        dev = points.device
        cloud_of = torch.arange(Fc, device=dev, dtype=torch.int32).repeat_interleave(N)
        grid, depth = ops.cloud_voxelize(points.reshape(n, 3), cloud_of, Fc, self.grid_resolution)
        level = Level(grid, cloud_of, depth, np.full(Fc, N, dtype=np.int64), ops.cloud_codes(grid, cloud_of, depth))
        stem = self.embedding.stem
        x = stem.conv(feat.reshape(n, -1).float().contiguous(), level, diff)
        stats = self.batch_statistics and self.training  # the reference's training function (module docstring)
        gen = None
        if stats and self.drop_path > 0.0:
            if self.drop_path_generator is None:
                self.drop_path_generator = torch.Generator(device=dev)
            gen = self.drop_path_generator
        if stats:
            x = _bn_gelu_train(x, stem.norm, "stem")
        else:
            x = _bn_gelu_live(x, stem.norm) if diff else ops.bn_gelu(x, *_bn_fold(stem.norm))
        stack = []
        for s in range(self.num_stages):
            enc = getattr(self.enc, f"enc{s}")
            if s > 0:
                x_child, child, cluster, members = enc.down(x, level, diff, stats)
                stack.append((level, x, cluster, members))
                level, x = child, x_child
            for i in range(self.enc_depths[s]):
                x = getattr(enc, f"block{i}")(x, level, differentiable=diff, drop_generator=gen)
        for s in reversed(range(self.num_stages - 1)):
            dec = getattr(self.dec, f"dec{s}")
            parent, x_parent, cluster, members = stack.pop()
            skip, x = dec.up(x, x_parent, cluster, members if diff else None, stats, f"unpooling into level {s}")
            level = parent
            for i in range(self.dec_depths[s]):
                x = getattr(dec, f"block{i}")(x, level, conv_in=skip if i == 0 else None, differentiable=diff,
                                              drop_generator=gen)
        return x


class PTv3Encoder(nn.Module):
    """point_encoder.py:6-40.  cfg: input_dim, stride, enc_channels, enc_depths, dec_channels, dec_depths,
    enc_num_head, dec_num_head, enc_patch_size, dec_patch_size, enable_flash (reference names); optional
    `refiner_clouds_per_pass` bounds the working set (clouds are independent, so the split changes nothing); optional
    `differentiable_refiner` (default False) builds the trainable network (module docstring); optional
    `refiner_batch_statistics` (default False) is PointTransformerV3's batch_statistics: in .train() the population of a
    BatchNorm statistic is every row of every cloud of one call -- the reference's batch --, so all clouds then run in ONE
    pass whatever the two bounds say (a split would change the function) and memory is the caller's to bound."""

    def __init__(self, cfg=None):
        super().__init__()
        from .tuning import use_tuned_gemms

        use_tuned_gemms()  # library kernel selection for the fixed level-0 GEMM shapes (tuning.py)
        in_channels = getattr(cfg, "input_dim", None) or 3 * cfg.triplane_feature_dim  # ptv3_encoder.yaml:5
        self.point_transformer = PointTransformerV3(
            in_channels=in_channels, stride=cfg.stride, enc_channels=cfg.enc_channels, enc_depths=cfg.enc_depths,
            dec_channels=cfg.dec_channels, dec_depths=cfg.dec_depths, enc_num_head=cfg.enc_num_head,
            dec_num_head=cfg.dec_num_head, enc_patch_size=cfg.enc_patch_size, dec_patch_size=cfg.dec_patch_size,
            enable_flash=getattr(cfg, "enable_flash", False),
            differentiable=getattr(cfg, "differentiable_refiner", False),
            batch_statistics=getattr(cfg, "refiner_batch_statistics", False))
        self.grid_resolution = 100
        self.clouds_per_pass = int(getattr(cfg, "refiner_clouds_per_pass", 32))
        self.points_per_pass = int(getattr(cfg, "refiner_points_per_pass", 320_000))

    def forward(self, pts, feats):
        """pts [B,N,3], feats [B,N,C] -> [B*N, dec_channels[0]]."""
        B = pts.shape[0]
        step = max(1, min(self.clouds_per_pass, self.points_per_pass // max(int(pts.shape[1]), 1)))
        if self.point_transformer.batch_statistics and self.point_transformer.training:
            step = max(B, 1)  # batch statistics are over the whole call
        outs = [self.point_transformer(pts[s:s + step], feats[s:s + step]) for s in range(0, B, step)]
        return outs[0] if len(outs) == 1 else torch.cat(outs)
