"""Transformer1D_nn and its blocks (mirror of the live part of src/models/transformers.py).

Same module tree and parameter names as the reference, so `audio_triplane.transformer.*` checkpoint keys load:
    norm, proj_in, transformer_blocks.N.{norm1, attn1.{to_q,to_k,to_v,to_out.0}, norm2, attn2.{...}, norm3,
    ff.net.0.proj, ff.net.2}, proj_out          (transformers.py:980-1011,225-275,438-444,497)
Only the configuration AudioTriplaneNet uses is built (norm_type="layer_norm", GEGLU feed-forward, no dropout,
attention_bias=False, cross-attention to the audio token; triplane_audio_net.py:132-141).

What runs where:
  * self-attention (attn1, S = 6304 tokens, 8 x 64): the hand-written MFMA flash kernel (csrc/attention.hip),
    fed by ONE fused q/k/v projection GEMM whose output it reads in place through a row stride;
  * cross-attention (attn2) to one key: the context is a single audio token (triplane_audio_net.py:211), so softmax
    over one key is exactly 1 and the layer is to_out(to_v(audio)) broadcast over the tokens -- computed exactly that way
    (two [1,768]x[768,512] products instead of 6304 x 512 x 2 of wasted Q/K work);
  * cross-attention to many keys (stage 1: the fusion network's 3152 and the SMPL-X predictor's 80 queries over the 4096
    Sapiens tokens): the same fp16 x 2 MFMA kernels with separate query and key counts (ops.crossattn, always fp16 x 2)
    over q and ONE fused k | v projection, with the HIP backward under autograd (ops.crossattn_differentiable), for HIP
    fp32 tensors, dim_head 64 and bias-free to_q / to_k / to_v.  Everything else (CPU, other dtypes or head dims,
    biases) and AMAV_CROSS_ATTN=library (read per call) stay on the library's fused attention;
  * the four big projections of a block (q/k/v, to_out, both feed-forward layers) at inference: fp32-equivalent
    products on the low-precision matrix pipe -- both operands split into parts whose partial products are ONE library
    GEMM with fp32 accumulation over the parts concatenated along K (csrc/attention_rows.hip, split_operand kernels):
      - inside a block (forward_fused) two fp16 parts, three partial products, K' = 3 K.  fp16 has 5 exponent bits, so
        every operand is pre-scaled by a power of two (exact) taken from a PROVEN bound on its magnitude -- LayerNorm
        rows are bounded by sqrt(dim) max|w| + max|b|, projections of them by Cauchy-Schwarz, softmax averages by their
        values' bound (`_fp16_plan`) -- and the product is scaled back through the GEMM's alpha;
      - `linear()` on inputs without such a bound: three bf16 parts, six partial products, K' = 6 K (any finite input).
    Both are 2.5-3x / 1.5-2x faster than the library's fp32 GEMM and 2-3x closer to fp64 (tools/gemm_split_probe.py).
    AMAV_GEMM=f32 keeps the fp32 GEMMs, AMAV_GEMM=bf16 the bf16 format everywhere;
  * under autograd on the GPU (width 256..1024, single key): the row passes of a block -- residual adds + LayerNorm, GEGLU
    -- on the same HIP kernels as inference, with HIP backwards (csrc/attention_rows_backward.hip).
    AMAV_TRAIN_ROWS=library keeps the library's LayerNorm / gelu / mul there.  The projections under autograd (q|k|v,
    to_out, both feed-forward layers, the three of many-key cross-attention) go through `train_linear`:
    AMAV_TRAIN_GEMM=f32 (the default) is the library's fp32 F.linear; AMAV_TRAIN_GEMM=split runs them as bf16 x 3 split
    products over operands from the split kernels, the backward's from the transposing one
    (ops.linear_split_differentiable: forward, dgrad and wgrad), except the products measured slower than the library's
    fp32 GEMM at the reference shapes -- today every wgrad.  In .train() with
    gradient_checkpointing=True every block is checkpointed, as in the reference;
  * GroupNorm, proj_in / proj_out, CPU: library kernels through torch (fp32 GEMMs).
"""
import math
import os
import warnings
import weakref

import torch
import torch.nn as nn
import torch.nn.functional as F
import torch.utils.checkpoint

from . import ops, tuning

_MEMO = {}  # (name, ids of the tensors it was derived from) -> (their versions, weak references, value)
SPLIT_GEMM_MIN_ROWS = 256  # below this the operand split costs more than the faster GEMM saves
SPLIT_GEMM_MAX_K = 1024    # bf16 x 3 format only: the 2048 -> 512 feed-forward output projection ran 126 + 35 (split) us
#                            against 120 us for the tuned fp32 GEMM (6304 rows; K' = 12288 leaves ~100 output tiles)
# train_linear under AMAV_TRAIN_GEMM=split, per product (6304 rows, split path with its split kernels against the library's
# fp32 GEMM; tools/bench_train_gemm.py).  The forward obeys SPLIT_GEMM_MAX_K: 2048 -> 512 ran 126.7
# against 118.7 us here too.
TRAIN_SPLIT_DGRAD_MAX_N = 1536  # dgrad contracts over N: 91.9 against 119.6 us at N = 1536 (K = 512), 317.9 against 229.6 us
#                                 at N = 4096 (K = 512; K' = 24576 leaves ~200 output tiles)
TRAIN_SPLIT_WGRAD = False       # wgrad contracts over 6 x rows = 37824 into an [N, K] result of 16..128 tiles: 205.1 / 124.0 /
#                                 430.9 / 219.2 us against 90.3 / 49.2 / 182.8 / 100.7 us (512 -> 1536, 512 -> 512, 512 -> 4096,
#                                 2048 -> 512): it loses at every reference shape and stays on the library
FP16_TARGET = 32768.0      # a tensor's bound is scaled to at most this (fp16 max 65504: 2x margin for rounding)
# The fp16 x 2 parts keep a value exact down to 2^-17 of the scaled bound (absolute error bound * 2^-40 below that).  With
# the largest actual value at bound * 2^-k, a 2048-term dot product stays at the fp32 level (2^-22 of its largest term)
# while k <= 12: beyond that overshoot a block takes the bf16 x 3 format, which needs no bounds.
FP16_MAX_OVERSHOOT = 4096.0


_version_of = ops.tensor_version


def _memo(name, tensors, make):
    """make() cached until one of `tensors` is modified in place, reallocated or freed."""
    key = (name,) + tuple(id(t) for t in tensors)
    # inference tensors (anything created under torch.inference_mode(), e.g. the fused q/k/v weight on a first forward
    # inside it) carry no version counter and cannot be modified in place outside inference mode: identity + storage
    version = tuple((_version_of(t), t.data_ptr()) for t in tensors)
    hit = _MEMO.get(key)
    if hit is None or hit[0] != version or any(ref() is not t for ref, t in zip(hit[1], tensors)):
        if hit is None or any(ref() is not t for ref, t in zip(hit[1], tensors)):
            for t in tensors:
                weakref.finalize(t, _MEMO.pop, key, None)
        hit = (version, tuple(weakref.ref(t) for t in tensors), make())
        _MEMO[key] = hit
    return hit[2]


def _scale_exp(bound):
    """The largest e with bound * 2^e <= FP16_TARGET."""
    return max(-100, min(100, int(math.floor(math.log2(FP16_TARGET / max(float(bound), 1e-30))))))


def _split_weight(weight):
    return _memo("bf16x3", (weight,), lambda: ops.split_operand(weight.detach(), weights=True))


def _split_weight_fp16(weight):
    """-> (the fp16 x 2 weight operand [N, 3K], its scale exponent)"""
    def make():
        e = _scale_exp(weight.detach().abs().max().item())
        return ops.split_operand(weight.detach(), weights=True, fmt=ops.SPLIT_FP16X2, scale_exp=e), e
    return _memo("fp16x2", (weight,), make)


def gemm_fp16(a, a_exp, weight):
    """a: fp16 x 2 activation operand [rows, 3K] pre-scaled by 2^a_exp -> [rows, N] fp32 = x weight^T, scaled back
    exactly through the GEMM's alpha (beta = 0: the `input` of addmm is a placeholder)."""
    b, b_exp = _split_weight_fp16(weight)
    # hipBLASLt through the C ABI, with the kernel the shipped table names for this shape (tuning.split_gemm_index: the
    # library's first heuristic answer -- what torch.addmm runs -- is 5-18 % slower on these four shapes)
    return ops.gemm_split_fp16(a, b, 2.0 ** -(a_exp + b_exp), tuning.split_gemm_index(a.shape[0], b.shape[0], a.shape[1]))


def split_gemm_ok(rows, K):
    """Whether a [rows, K] activation goes through the bf16 x 3 split GEMM (inference callers check device / dtype /
    autograd)."""
    return (rows >= SPLIT_GEMM_MIN_ROWS and K % 8 == 0 and K <= SPLIT_GEMM_MAX_K
            and os.environ.get("AMAV_GEMM", "split") != "f32")


def fp16_gemm_ok(rows, K):
    """Whether a block's projections go through the fp16 x 2 split GEMMs (forward_fused)."""
    return rows >= SPLIT_GEMM_MIN_ROWS and K % 8 == 0 and os.environ.get("AMAV_GEMM", "split") == "split"


def linear_presplit(a, weight, bias=None):
    """a: the [rows, 6 K] bf16 activation operand (ops.split_operand / ops.add_layernorm(split=SPLIT_BF16X3)) -> [rows, N] fp32
    = x weight^T (+ bias).  A bias costs a pass over the output here (the library adds it as a pre-filled C): callers on
    the hot path hand it to the kernel that consumes the result instead (ops.geglu / ops.add_layernorm)."""
    b = _split_weight(weight)
    if bias is None:
        return torch.mm(a, b.t(), out_dtype=torch.float32)
    return torch.addmm(bias, a, b.t(), out_dtype=torch.float32)


def linear(x, weight, bias=None):
    """F.linear(x, weight, bias) with an fp32-equivalent result.  On the inference path (fp32 CUDA tensors, no autograd,
    at least SPLIT_GEMM_MIN_ROWS rows) the product runs on the bf16 matrix pipe over split operands (module docstring);
    everywhere else it is F.linear."""
    K = weight.shape[1]
    rows = x.numel() // K
    if (not x.is_cuda or x.dtype != torch.float32 or weight.dtype != torch.float32 or torch.is_grad_enabled()
            or not split_gemm_ok(rows, K)):
        return F.linear(x, weight, bias)
    x2 = x.reshape(rows, K)
    if x2.stride(1) != 1 or x2.stride(0) % 4 or x2.data_ptr() % 16:
        x2 = x2.contiguous()
    return linear_presplit(ops.split_operand(x2), weight, bias).view(*x.shape[:-1], weight.shape[0])


def _train_gemm_split(x, weight, bias):
    """Whether train_linear sends this product down the split path."""
    if os.environ.get("AMAV_TRAIN_GEMM", "f32") != "split":
        return False
    N, K = weight.shape
    return (x.is_cuda and weight.is_cuda and x.dtype == weight.dtype == torch.float32
            and (bias is None or (bias.is_cuda and bias.dtype == torch.float32))
            and x.numel() // K >= SPLIT_GEMM_MIN_ROWS and K % 8 == 0 and N % 8 == 0)


def train_linear(x, weight, bias=None, sources=None):
    """F.linear(x, weight, bias) under autograd, the sibling of `linear`.  AMAV_TRAIN_GEMM, read per call like
    AMAV_TRAIN_ROWS: `f32` (the default) is F.linear itself; `split` runs the forward and both backward products of HIP
    fp32 tensors with at least SPLIT_GEMM_MIN_ROWS rows and K, N multiples of 8 as bf16 x 3 split GEMMs
    (ops.linear_split_differentiable) and everything else as F.linear.  A product measured slower
    than the library's at the reference shapes stays an fp32 GEMM (SPLIT_GEMM_MAX_K, TRAIN_SPLIT_DGRAD_MAX_N,
    TRAIN_SPLIT_WGRAD).  Both weight operands are memoised on `sources`, the parameters `weight` was made from (default:
    `weight` itself; the concatenated q | k | v and k | v weights are new tensors every call), so an optimizer step or an
    in-place update rebuilds them."""
    if not _train_gemm_split(x, weight, bias):
        return F.linear(x, weight, bias)
    N, K = weight.shape
    library = tuple(name for name, lost in (("forward", K > SPLIT_GEMM_MAX_K), ("dgrad", N > TRAIN_SPLIT_DGRAD_MAX_N),
                                            ("wgrad", not TRAIN_SPLIT_WGRAD)) if lost)
    if len(library) == 3:
        return F.linear(x, weight, bias)
    keys = (weight,) if sources is None else tuple(sources)
    name = "bf16x3" if sources is None else "bf16x3_cat"  # one parameter: the operand `linear` memoises too
    w = weight.detach()
    return ops.linear_split_differentiable(
        x, weight, bias,
        weight_split=lambda: _memo(name, keys, lambda: ops.split_operand(w, weights=True)),
        weight_split_t=lambda: _memo(name + "_t", keys, lambda: ops.split_operand_transposed(w, weights=True)),
        library=library)


class Attention(nn.Module):
    """diffusers `Attention` as configured by the reference: q/k/v without bias, out with
    bias, scale 1/sqrt(dim_head), no mask."""

    def __init__(self, query_dim, cross_attention_dim=None, heads=8, dim_head=64, dropout=0.0, bias=False):
        super().__init__()
        inner = heads * dim_head
        self.heads, self.dim_head, self.inner_dim = heads, dim_head, inner
        self.is_cross = cross_attention_dim is not None
        ctx = cross_attention_dim if self.is_cross else query_dim
        self.to_q = nn.Linear(query_dim, inner, bias=bias)
        self.to_k = nn.Linear(ctx, inner, bias=bias)
        self.to_v = nn.Linear(ctx, inner, bias=bias)
        self.to_out = nn.ModuleList([nn.Linear(inner, query_dim), nn.Dropout(dropout)])
        self._qkv = self._kv = None

    def _qkv_weight(self):
        ws = (self.to_q.weight, self.to_k.weight, self.to_v.weight)
        version = tuple((_version_of(w), w.data_ptr()) for w in ws)
        if self._qkv is None or self._qkv[0] != version:
            self._qkv = (version, torch.cat([w.detach() for w in ws], dim=0).contiguous())
        return self._qkv[1]

    def _kv_weight(self):
        ws = (self.to_k.weight, self.to_v.weight)
        version = tuple((_version_of(w), w.data_ptr()) for w in ws)
        if self._kv is None or self._kv[0] != version:
            self._kv = (version, torch.cat([w.detach() for w in ws], dim=0).contiguous())
        return self._kv[1]

    def _cross_hip(self, hidden_states, context):
        """Whether many-key cross-attention runs on the HIP kernels (module docstring)."""
        return (hidden_states.is_cuda and context.is_cuda and hidden_states.dtype == context.dtype == torch.float32
                and self.to_q.weight.dtype == torch.float32 and self.dim_head == 64
                and self.to_q.bias is None and self.to_k.bias is None and self.to_v.bias is None
                and os.environ.get("AMAV_CROSS_ATTN", "hip") != "library")

    def attend(self, qkv, out_bias=True, out_exp=None, bounds=None):
        """qkv [B,S,3*inner] (the fused projection's output, read in place) -> to_out(softmax(q k^T / sqrt(d)) v);
        out_bias=False leaves to_out's bias to the caller (forward_fused adds it in its next pass); out_exp: the scale
        exponent of the attention output's proven bound, which sends to_out through the fp16 x 2 GEMM; bounds: proven
        (|q|, |k|, |v|) bounds for the kernel's operand scaling."""
        i = self.inner_dim
        if out_exp is None:
            out = ops.selfattn(qkv[..., :i], qkv[..., i:2 * i], qkv[..., 2 * i:], self.heads, bounds=bounds)
            return linear(out, self.to_out[0].weight, self.to_out[0].bias if out_bias else None)
        # the kernel's last pass writes to_out's fp16 x 2 operand itself (no fp32 result, no split pass over it)
        a = ops.selfattn(qkv[..., :i], qkv[..., i:2 * i], qkv[..., 2 * i:], self.heads, bounds=bounds, split_out_exp=out_exp)
        y = gemm_fp16(a, out_exp, self.to_out[0].weight).view(*qkv.shape[:-1], -1)
        return y + self.to_out[0].bias if out_bias else y

    def forward(self, hidden_states, encoder_hidden_states=None, attention_mask=None):
        if attention_mask is not None:
            raise NotImplementedError("attention masks are not used on this path (transformers.py:1026-1031)")
        if encoder_hidden_states is None:
            if torch.is_grad_enabled() and (hidden_states.requires_grad or any(
                    w.requires_grad for w in (self.to_q.weight, self.to_k.weight, self.to_v.weight,
                                              self.to_out[0].weight, self.to_out[0].bias))):
                return self._forward_differentiable(hidden_states)
            qkv = linear(hidden_states, self._qkv_weight())            # [B,S,3*inner], one GEMM
            return self.attend(qkv)
        if encoder_hidden_states.shape[1] != 1:
            # Many context tokens (stage 1: 4096 Sapiens tokens, triplane_net.py:104-113,320-329): the fp16 x 2 MFMA
            # kernels with separate query and key counts (ops.crossattn), the library's fused attention elsewhere
            if self._cross_hip(hidden_states, encoder_hidden_states):
                return self._forward_cross(hidden_states, encoder_hidden_states)
            B, S, _ = hidden_states.shape
            split = lambda t: t.view(B, t.shape[1], self.heads, self.dim_head).transpose(1, 2)
            q = split(self.to_q(hidden_states))
            k, v = split(self.to_k(encoder_hidden_states)), split(self.to_v(encoder_hidden_states))
            o = F.scaled_dot_product_attention(q, k, v)
            return self.to_out[0](o.transpose(1, 2).reshape(B, S, self.inner_dim))
        # one key: softmax == 1, so the output is to_out(to_v(context)) for every query
        ctx = self.to_out[0](self.to_v(encoder_hidden_states))        # [B,1,query_dim]
        return ctx.expand(-1, hidden_states.shape[1], -1)

    def _forward_cross(self, hidden_states, context):
        """Cross-attention to many keys on the GPU in fp32: k | v from one projection over the concatenated to_k / to_v
        weights, read in place by the kernels.  Without grad the projections go through `linear`; under autograd they are
        `train_linear` and the attention is ops.crossattn_differentiable, whose backward returns dq and a fused dk | dv."""
        out_w, out_b = self.to_out[0].weight, self.to_out[0].bias
        if torch.is_grad_enabled() and (hidden_states.requires_grad or context.requires_grad or any(
                w.requires_grad for w in (self.to_q.weight, self.to_k.weight, self.to_v.weight, out_w, out_b))):
            q = train_linear(hidden_states, self.to_q.weight)
            kv = train_linear(context, torch.cat([self.to_k.weight, self.to_v.weight], dim=0),
                              sources=(self.to_k.weight, self.to_v.weight))                   # [B,Sk,2*inner]
            return train_linear(ops.crossattn_differentiable(q, kv, self.heads, self.dim_head ** -0.5), out_w, out_b)
        i = self.inner_dim
        q = linear(hidden_states, self.to_q.weight)
        kv = linear(context, self._kv_weight())
        return linear(ops.crossattn(q, kv[..., :i], kv[..., i:], self.heads), out_w, out_b)

    def _forward_differentiable(self, hidden_states):
        """Self-attention under autograd: one `train_linear` over the concatenated q/k/v weights (so that gradients reach
        all three), the MFMA flash kernel with its HIP backward on the GPU (ops.selfattn_differentiable), the library's
        SDPA on the CPU, then to_out."""
        ws = (self.to_q.weight, self.to_k.weight, self.to_v.weight)
        qkv = train_linear(hidden_states, torch.cat(ws, dim=0), sources=ws)   # [B,S,3*inner]
        if qkv.is_cuda and qkv.dtype == torch.float32:
            out = ops.selfattn_differentiable(qkv, self.heads, self.dim_head ** -0.5)
        elif qkv.is_cuda:
            raise NotImplementedError(f"self-attention under autograd runs in fp32 on the GPU, got {qkv.dtype}")
        else:
            B, S, _ = qkv.shape
            q, k, v = (t.view(B, S, self.heads, self.dim_head).transpose(1, 2) for t in qkv.split(self.inner_dim, -1))
            out = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, S, self.inner_dim)
        return train_linear(out, self.to_out[0].weight, self.to_out[0].bias)


class GEGLU(nn.Module):
    """transformers.py:484-508: proj to 2*inner, first half = value, second half = gate, exact-erf GELU."""

    def __init__(self, dim_in, dim_out):
        super().__init__()
        self.proj = nn.Linear(dim_in, dim_out * 2)

    def forward(self, hidden_states):
        proj = linear(hidden_states, self.proj.weight, self.proj.bias)
        if proj.is_cuda and proj.dtype == torch.float32 and not torch.is_grad_enabled() and proj.shape[-1] % 8 == 0:
            return ops.geglu(proj.contiguous())  # one fused pass (csrc/attention_rows.hip)
        hidden_states, gate = proj.chunk(2, dim=-1)  # CPU construction / autograd
        return hidden_states * F.gelu(gate)


class FeedForward(nn.Module):
    """transformers.py:402-452 with activation_fn='geglu': net = [GEGLU, Dropout, Linear]."""

    def __init__(self, dim, mult=4, dropout=0.0):
        super().__init__()
        inner = int(dim * mult)
        self.net = nn.ModuleList([GEGLU(dim, inner), nn.Dropout(dropout), nn.Linear(inner, dim)])

    def forward(self, hidden_states):
        hidden_states = self.net[1](self.net[0](hidden_states))
        return linear(hidden_states, self.net[2].weight, self.net[2].bias)


class BasicTransformerBlock(nn.Module):
    """transformers.py:140-399, layer_norm variant: LN -> self-attn -> LN -> cross-attn -> LN -> GEGLU FF."""

    def __init__(self, dim, num_attention_heads, attention_head_dim, dropout=0.0, cross_attention_dim=None):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim)
        self.attn1 = Attention(dim, None, num_attention_heads, attention_head_dim, dropout)
        self.norm2 = nn.LayerNorm(dim)
        self.attn2 = Attention(dim, cross_attention_dim, num_attention_heads, attention_head_dim, dropout)
        self.norm3 = nn.LayerNorm(dim)
        self.ff = FeedForward(dim, dropout=dropout)

    def forward_fused(self, h, pending, row):
        """Inference path of Transformer1D_nn: `pending` is the previous block's (feed-forward output, its bias or None)
        whose residual add has not happened yet (None for the first block), `row` [B,1,dim] this block's cross-attention
        output (one row per batch item: a single audio key).  -> (h, pending) with the same meaning.  Three residual
        adds and two LayerNorms run as two passes (ops.add_layernorm) instead of five."""
        B, S, dim = h.shape
        ff_in, ff_out = self.ff.net[0].proj, self.ff.net[2]
        pending, pending_bias = pending if pending is not None else (None, None)
        if fp16_gemm_ok(B * S, dim) and self._fp16_overshoot_ok(h, pending, pending_bias, row):
            # every projection as an fp16 x 2 split GEMM: each pass writes its rows as the split operand of the GEMM that
            # follows, pre-scaled from the proven bounds of _fp16_plan, and the projections' biases are added by the
            # pass that reads their output
            e_n1, e_attn, e_n3, e_ff, qkv_bounds = self._fp16_plan()
            h, n1 = ops.add_layernorm(h, pending, None, self.norm1.weight, self.norm1.bias, self.norm1.eps,
                                      add_bias=pending_bias, split=ops.SPLIT_FP16X2, split_exp=e_n1)
            qkv = gemm_fp16(n1, e_n1, self.attn1._qkv_weight()).view(B, S, -1)
            a1 = self.attn1.attend(qkv, out_bias=False, out_exp=e_attn, bounds=qkv_bounds)
            h, n3 = ops.add_layernorm(h, a1, row, self.norm3.weight, self.norm3.bias, self.norm3.eps,
                                      add_bias=self.attn1.to_out[0].bias, split=ops.SPLIT_FP16X2, split_exp=e_n3)
            gated = ops.geglu(gemm_fp16(n3, e_n3, ff_in.weight), bias=ff_in.bias, split_exp=e_ff)
            return h, (gemm_fp16(gated, e_ff, ff_out.weight).view(B, S, -1), ff_out.bias)
        if pending is not None and pending_bias is not None:
            pending = pending + pending_bias
        if split_gemm_ok(B * S, dim):
            # the bf16 x 3 format (AMAV_GEMM=bf16): no bounds needed
            h, n1 = ops.add_layernorm(h, pending, None, self.norm1.weight, self.norm1.bias, self.norm1.eps,
                                      split=ops.SPLIT_BF16X3)
            qkv = linear_presplit(n1, self.attn1._qkv_weight()).view(B, S, -1)
            a1 = self.attn1.attend(qkv, out_bias=False)
            h, n3 = ops.add_layernorm(h, a1, row, self.norm3.weight, self.norm3.bias, self.norm3.eps,
                                      add_bias=self.attn1.to_out[0].bias, split=ops.SPLIT_BF16X3)
            gated = ops.geglu(linear_presplit(n3, ff_in.weight).view(B, S, -1), bias=ff_in.bias)
            return h, (linear(gated, ff_out.weight, ff_out.bias), None)
        if pending is None:
            n1 = self.norm1(h)
        else:
            h, n1 = ops.add_layernorm(h, pending, None, self.norm1.weight, self.norm1.bias, self.norm1.eps)
        a1 = self.attn1(n1).contiguous()
        h, n3 = ops.add_layernorm(h, a1, row, self.norm3.weight, self.norm3.bias, self.norm3.eps)
        return h, (self.ff(n3), None)

    def _fp16_plan(self):
        """Scale exponents (e_n1, e_attn, e_n3, e_ff) of the four activation operands of forward_fused and the (|q|, |k|,
        |v|) bounds of the attention kernel's operands, each from a bound that holds for EVERY input:
          LayerNorm rows n = z w + b with |z_i| <= sqrt(dim) and ||z||_2 <= sqrt(dim):
              |n_i| <= sqrt(dim) max|w| + max|b|,      ||n||_2 <= sqrt(dim) max|w| + ||b||_2
          a projection of such a row: |W_j n (+ c_j)| <= max_j ||W_j||_2 ||n||_2 (+ max|c|)        (Cauchy-Schwarz)
          the attention output is a convex combination of value rows: |o_i| <= max|v|
          GEGLU: |h gelu(g)| <= |h| |g|.
        The bounds overshoot typical magnitudes by 2^4..2^9; fp16 keeps a value's residual exact down to 2^-17 of the
        scaled bound, so the headroom only costs precision on elements that are already negligible."""
        ff_in = self.ff.net[0].proj
        tensors = (self.norm1.weight, self.norm1.bias, self.norm3.weight, self.norm3.bias, self.attn1.to_q.weight,
                   self.attn1.to_k.weight, self.attn1.to_v.weight, ff_in.weight, ff_in.bias)

        def make():
            dim = self.norm1.weight.numel()
            inner = ff_in.weight.shape[0] // 2
            stats = torch.stack([
                self.norm1.weight.abs().max(), self.norm1.bias.abs().max(), self.norm1.bias.norm(),
                self.norm3.weight.abs().max(), self.norm3.bias.abs().max(), self.norm3.bias.norm(),
                self.attn1.to_v.weight.norm(dim=1).max(), self.attn1.to_q.weight.norm(dim=1).max(),
                self.attn1.to_k.weight.norm(dim=1).max(),
                ff_in.weight[:inner].norm(dim=1).max(), ff_in.weight[inner:].norm(dim=1).max(),
                ff_in.bias[:inner].abs().max(), ff_in.bias[inner:].abs().max()]).double().tolist()  # one host sync
            w1, b1, b1_l2, w3, b3, b3_l2, v_rows, q_rows, k_rows, h_rows, g_rows, h_bias, g_bias = stats
            root = math.sqrt(dim)
            n1_l2, n3_l2 = root * w1 + b1_l2, root * w3 + b3_l2
            v_bound = v_rows * n1_l2 + (self.attn1.to_v.bias.abs().max().item() if self.attn1.to_v.bias is not None else 0.0)
            ff_bound = (h_rows * n3_l2 + h_bias) * (g_rows * n3_l2 + g_bias)
            exps = tuple(_scale_exp(b) for b in (root * w1 + b1, v_bound, root * w3 + b3, ff_bound))
            self._fp16_bounds = (root * w1 + b1, v_bound, root * w3 + b3, ff_bound)
            return exps + ((q_rows * n1_l2, k_rows * n1_l2, v_bound),)  # attention_bias=False: no q / k bias

        return _memo("fp16_plan", tensors, make)

    def _fp16_overshoot_ok(self, h, pending, pending_bias, row):
        """Whether the proven bounds of _fp16_plan sit close enough to what the block actually produces for the fp16 x 2
        parts to carry fp32 precision (FP16_MAX_OVERSHOOT).  The bounds hold for every input, but they multiply two
        Cauchy-Schwarz bounds for the GEGLU product: LayerNorm gains of 30 and a few heavy weight rows (a trained
        checkpoint) put them 2^20 above the activations, and everything below 2^-17 of the bound loses bits.  Measured
        ONCE per weights version, on the first input the block sees (LayerNorm fixes the scale of what follows, so the
        ratio barely depends on the input): one extra pass in library fp32 and one host sync."""
        ff_in = self.ff.net[0].proj
        tensors = (self.norm1.weight, self.norm1.bias, self.norm3.weight, self.norm3.bias, self.attn1.to_q.weight,
                   self.attn1.to_k.weight, self.attn1.to_v.weight, ff_in.weight, ff_in.bias)

        def make():
            self._fp16_plan()
            x = h if pending is None else h + pending + (pending_bias if pending_bias is not None else 0.0)
            n1 = F.layer_norm(x, (x.shape[-1],), self.norm1.weight, self.norm1.bias, self.norm1.eps)
            i = self.attn1.inner_dim
            qkv = F.linear(n1, self.attn1._qkv_weight())
            B, S = x.shape[:2]
            heads = lambda t: t.reshape(B, S, self.attn1.heads, self.attn1.dim_head).transpose(1, 2)
            a = F.scaled_dot_product_attention(heads(qkv[..., :i]), heads(qkv[..., i:2 * i]), heads(qkv[..., 2 * i:]))
            a = a.transpose(1, 2).reshape(B, S, i)
            x3 = x + self.attn1.to_out[0](a) + row
            n3 = F.layer_norm(x3, (x3.shape[-1],), self.norm3.weight, self.norm3.bias, self.norm3.eps)
            hg = F.linear(n3, ff_in.weight, ff_in.bias)
            inner = hg.shape[-1] // 2
            gated = hg[..., :inner] * F.gelu(hg[..., inner:])
            actual = torch.stack([t.abs().max() for t in (n1, a, n3, gated)]).double().tolist()  # one host sync
            self._fp16_overshoot = tuple(b / max(v, 1e-30) for b, v in zip(self._fp16_bounds, actual))
            ok = max(self._fp16_overshoot) <= FP16_MAX_OVERSHOOT
            if not ok:
                warnings.warn("transformer block: the proven fp16 bounds overshoot the activations by "
                              f"{max(self._fp16_overshoot):.3g} (> {FP16_MAX_OVERSHOOT:g}); using the bf16 x 3 format")
            return ok

        return _memo("fp16_overshoot", tensors, make)

    def forward(self, hidden_states, encoder_hidden_states=None):
        h = hidden_states
        single_key = encoder_hidden_states is not None and encoder_hidden_states.shape[1] == 1
        if (single_key and h.is_cuda and h.dtype == torch.float32 and not torch.is_grad_enabled()
                and h.shape[-1] in (256, 512, 768, 1024)):
            # inference path: both residual adds and norm3 in one kernel.  With a single audio key the cross-attention
            # output is one row per batch item and does not depend on its queries, so norm2 has no consumer.
            a1 = self.attn1(self.norm1(h)).contiguous()
            row = self.attn2(h[:, :1], encoder_hidden_states)[:, :1].contiguous()  # [B,1,dim]
            h, n3 = ops.add_layernorm(h.contiguous(), a1, row, self.norm3.weight, self.norm3.bias, self.norm3.eps)
            return self.ff(n3) + h
        if single_key and self._train_rows_fused(h, encoder_hidden_states):
            # autograd path on the row kernels: the passes of the inference branch above, each with its HIP backward
            # (ops.add_layernorm_differentiable / geglu_differentiable).  The GEMMs are
            # train_linear: the library's fp32 products, or split products under AMAV_TRAIN_GEMM=split (section 4.19);
            # norm2 and attn2.to_q / to_k have no consumer with a single key and stay outside the graph.
            ff_in, ff_out = self.ff.net[0].proj, self.ff.net[2]
            h, n1 = ops.add_layernorm_differentiable(h, None, None, self.norm1.weight, self.norm1.bias, self.norm1.eps)
            a1 = self.attn1._forward_differentiable(n1)
            row = self.attn2(h[:, :1], encoder_hidden_states)[:, :1]   # [B,1,dim]; to_v / to_out get gradients
            h, n3 = ops.add_layernorm_differentiable(h, a1, row, self.norm3.weight, self.norm3.bias, self.norm3.eps)
            gated = ops.geglu_differentiable(train_linear(n3, ff_in.weight), bias=ff_in.bias)
            return train_linear(gated, ff_out.weight, ff_out.bias) + h
        h = self.attn1(self.norm1(h)) + h
        h = self.attn2(self.norm2(h), encoder_hidden_states) + h
        return self.ff(self.norm3(h)) + h

    def _train_rows_fused(self, h, context):
        """Whether a single-key block under autograd runs its row passes on the HIP kernels (the default) instead of the
        library's LayerNorm / add / gelu / mul.  AMAV_TRAIN_ROWS=library, read per call like AMAV_GEMM, keeps the library
        path."""
        if not (torch.is_grad_enabled() and h.is_cuda and h.dtype == torch.float32 and h.shape[-1] in (256, 512, 768, 1024)
                and self.attn2.to_v.bias is None and os.environ.get("AMAV_TRAIN_ROWS", "fused") != "library"):
            return False
        return h.requires_grad or context.requires_grad or any(p.requires_grad for p in self.parameters())


class Transformer1D_nn(nn.Module):
    """transformers.py:912-1074: [B,C,S] tokens (+ [B,1,ctx] audio) -> [B,C,S]."""

    def __init__(self, num_attention_heads=16, attention_head_dim=88, in_channels=None, out_channels=None,
                 num_layers=1, dropout=0.0, norm_num_groups=32, cross_attention_dim=None, norm_type="layer_norm",
                 enable_memory_efficient_attention=False, gradient_checkpointing=False, **unused):
        super().__init__()
        if in_channels is None:
            raise ValueError("in_channels must be defined")
        if norm_type != "layer_norm":
            raise NotImplementedError("only norm_type='layer_norm' is on the reference's path")
        inner = num_attention_heads * attention_head_dim
        self.in_channels = in_channels
        self.norm = nn.GroupNorm(norm_num_groups, in_channels, eps=1e-6, affine=True)
        self.proj_in = nn.Linear(in_channels, inner)
        self.transformer_blocks = nn.ModuleList([
            BasicTransformerBlock(inner, num_attention_heads, attention_head_dim, dropout, cross_attention_dim)
            for _ in range(num_layers)])
        self.proj_out = nn.Linear(inner, in_channels)
        self.gradient_checkpointing = bool(gradient_checkpointing)
        self._cross = None

    def _cross_rows(self, context):
        """Cross-attention outputs of ALL blocks for a single-key context [B,1,ctx]: softmax over one key is 1, so block
        l contributes to_out_l(to_v_l(context)) to every token.  Two batched products over the stacked weights instead
        of two tiny GEMVs inside every block.  -> [L,B,1,dim]"""
        mods = [b.attn2 for b in self.transformer_blocks]
        tensors = [t for m in mods for t in (m.to_v.weight, m.to_out[0].weight, m.to_out[0].bias)]
        version = tuple((_version_of(t), t.data_ptr()) for t in tensors)
        if self._cross is None or self._cross[0] != version:
            wv = torch.stack([m.to_v.weight.detach().t() for m in mods]).contiguous()        # [L,ctx,inner]
            wo = torch.stack([m.to_out[0].weight.detach().t() for m in mods]).contiguous()   # [L,inner,dim]
            bo = torch.stack([m.to_out[0].bias.detach() for m in mods])[:, None, :].contiguous()  # [L,1,dim]
            self._cross = (version, wv, wo, bo)
        _, wv, wo, bo = self._cross
        ctx = context[:, 0].unsqueeze(0).expand(len(mods), -1, -1)                           # [L,B,ctx]
        return torch.baddbmm(bo, torch.bmm(ctx, wv), wo).unsqueeze(2)

    def forward(self, hidden_states, encoder_hidden_states=None):
        batch, channels, seq_len = hidden_states.shape
        residual = hidden_states
        h = self.norm(hidden_states).permute(0, 2, 1)
        h = self.proj_in(h)
        ctx = encoder_hidden_states
        if (ctx is not None and ctx.shape[1] == 1 and h.is_cuda and h.dtype == torch.float32
                and not torch.is_grad_enabled() and h.shape[-1] in (256, 512, 768, 1024)
                and all(m.attn2.to_v.bias is None for m in self.transformer_blocks)):
            rows = self._cross_rows(ctx)
            h, pending = h.contiguous(), None
            for block, row in zip(self.transformer_blocks, rows):
                h, pending = block.forward_fused(h, pending, row)
            last, last_bias = pending  # the last feed-forward output (+ its bias, when its GEMM ran without one)
            h = (last if last_bias is None else last + last_bias) + h
        elif self.training and self.gradient_checkpointing and torch.is_grad_enabled():
            # transformers.py:1044-1056: a block keeps its input only and runs its forward again in the backward.  The HIP
            # Functions of a block are deterministic and keep no per-call state, so the second forward repeats the first
            # bit for bit.
            for block in self.transformer_blocks:
                h = torch.utils.checkpoint.checkpoint(block, h, ctx, use_reentrant=False)
        else:
            for block in self.transformer_blocks:
                h = block(h, ctx)
        h = self.proj_out(h).permute(0, 2, 1)
        return h + residual
