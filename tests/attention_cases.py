"""Inputs, reference, yardstick and bound shared by the self-attention forward tests: the GPU tests
(test_attention_forward_gpu.py), their forced-split child processes (attention_forced_split_child.py) and the CPU model
test (test_attention_model.py).  A plain module: it loads nothing from the HIP library.

Every case is CPU fp32 q, k, v of shape [B, S, H*64] drawn from an explicit torch.Generator, so the pytest process, a
child process and the CPU test see the same bits.

Reference: F.scaled_dot_product_attention in float64 on the CPU.
Yardstick: the same call in float32 on the CPU against the float64 result, err32 = max |sdpa32 - sdpa64| -- the
arithmetic the reference project runs (transformers.py:329-336), deterministic on every machine.
Bound, every variant, every case inside the documented envelope, over every output element:

    max |out - sdpa64|  <=  4 err32 + 2^-22 max |v|          and          <= 2e-5 max(1, max |sdpa64|)

4: the project's factor for "no worse than the library's fp32" (test_attention_backward_gpu.py).  2^-22 max |v|: the
documented product precision of the split formats times max |v|, every output being a convex
combination of value rows; it only matters where err32 happens to be tiny (q = 0, one-hot rows).
"""
import math
import zlib
from dataclasses import dataclass

import torch
import torch.nn.functional as F

D = 64                      # head dim (the only one the library builds)
L2E = 1.4426950408889634
FACTOR = 4.0                # x err32
FLOOR = 2.0 ** -22          # x max |v|
CEILING = 2e-5              # x max(1, max |ref|): the bar of tests/test_attention_gpu.py
LSE_BOUND = 1e-6            # x max(1, |lse|): the bar of tests/test_attention_backward_gpu.py
VARIANTS = ("default", "bf16", "f32")   # amav_set_option("attn", ...): fp16 x 2, bf16 x 3, fp32 MFMA
FP16_MAX_OVERSHOOT = 4096.0  # transformer.py: the largest slack of a proven bound the fp16 x 2 format is handed


@dataclass
class Case:
    name: str
    q: torch.Tensor
    k: torch.Tensor
    v: torch.Tensor
    heads: int
    scale: float = None        # None: 1 / sqrt(64)
    bounds: tuple = None       # proven (|q|, |k|, |v|) bounds handed to the fp16 x 2 kernel; None: measured
    in_envelope: bool = True   # False: documented degradation, held to the ceiling only

    @property
    def shape(self):
        return self.q.shape[0], self.q.shape[1], self.heads


def _heads(t, H):
    B, S, _ = t.shape
    return t.view(B, S, H, D).transpose(1, 2)


def sdpa(q, k, v, H, dtype, scale=None):
    """[B,S,H*64] in `dtype` on the CPU, one (batch, head) at a time (the scores of 6304 keys x 8 heads would not fit)."""
    B, S, HD = q.shape
    out = torch.empty(B, S, HD, dtype=dtype)
    qh, kh, vh, oh = _heads(q, H), _heads(k, H), _heads(v, H), _heads(out, H)
    for b in range(B):
        for h in range(H):
            oh[b, h] = F.scaled_dot_product_attention(qh[b, h].to(dtype)[None], kh[b, h].to(dtype)[None],
                                                      vh[b, h].to(dtype)[None], scale=scale)[0]
    return out


def logsumexp(q, k, H, dtype, scale=None):
    """Row log-sum-exp of q k^T scale, [B,H,S] in `dtype`."""
    B, S, _ = q.shape
    sc = D ** -0.5 if scale is None else scale
    qh, kh = _heads(q, H), _heads(k, H)
    lse = torch.empty(B, H, S, dtype=dtype)
    for b in range(B):
        for h in range(H):
            lse[b, h] = torch.logsumexp((qh[b, h].to(dtype) @ kh[b, h].to(dtype).T) * sc, dim=-1)
    return lse


@dataclass
class Reference:
    out64: torch.Tensor
    err32: float
    vmax: float
    lse64: torch.Tensor = None
    lse_err32: float = None

    @property
    def bound(self):
        return FACTOR * self.err32 + FLOOR * self.vmax

    @property
    def ceiling(self):
        return CEILING * max(1.0, float(self.out64.abs().max()))


def reference(case, lse=False):
    out64 = sdpa(case.q, case.k, case.v, case.heads, torch.float64, case.scale)
    out32 = sdpa(case.q, case.k, case.v, case.heads, torch.float32, case.scale)
    ref = Reference(out64, float((out32.double() - out64).abs().max()), float(case.v.abs().max()))
    if lse:
        ref.lse64 = logsumexp(case.q, case.k, case.heads, torch.float64, case.scale)
        lse32 = logsumexp(case.q, case.k, case.heads, torch.float32, case.scale)
        ref.lse_err32 = float((lse32.double() - ref.lse64).abs().max())
    return ref


# The one case held to 4 err32 + 2^-22 max |v| alone, without the 2e-5 ceiling.  q x 100 gives scores of magnitude 500;
# one fp32 rounding of such a score (2^-24 x 512 = 3e-5) moves a probability by 3e-5 of itself, and at 1000 keys the
# CPU's own float32 SDPA ends 1.64e-4 from float64 -- twice the ceiling of 8.4e-5 (at 193 keys: 8.6e-5 under 9.0e-5, the
# ceiling stays there).  No kernel that forms fp32 scores from fp32 inputs can meet it; measured on an MI355X: fp16 x 2
# 6.6e-5, fp32 MFMA 9.6e-5, bf16 x 3 1.62e-4 (0.40, 0.59 and 0.99 x err32).  The GPU test asserts err32 > ceiling there,
# so the waiver cannot outlive its reason.
CEILING_WAIVED = {("peaked_100", (1, 1000, 2))}


def check(out, ref, label, envelope=True, ceiling=True):
    """Print one line of figures, then assert the bound over every element of `out`.  Returns (error, error / err32,
    error / max |v|)."""
    assert out.shape == ref.out64.shape and out.dtype == torch.float32
    assert bool(torch.isfinite(out).all()), f"{label}: non-finite output"
    err = float((out.double() - ref.out64).abs().max())
    ratio, rel_v = err / max(ref.err32, 1e-300), err / max(ref.vmax, 1e-300)
    print(f"{label}: error {err:.3e} = {ratio:.3g} x err32 ({ref.err32:.3e}) = {rel_v:.3g} x max|v| ({ref.vmax:.3g}); "
          f"bound {ref.bound:.3e} ceiling {ref.ceiling:.3e}")
    if ceiling:
        assert err <= ref.ceiling, f"{label}: {err:.3e} above the ceiling {ref.ceiling:.3e}"
    if envelope:
        assert err <= ref.bound, f"{label}: {err:.3e} > 4 x {ref.err32:.3e} + 2^-22 x {ref.vmax:.3g} = {ref.bound:.3e}"
    return err, ratio, rel_v


def check_lse(lse, ref, label):
    """The forward's row log-sum-exp against fp64: <= 1e-6 max(1, |lse|) (tests/test_attention_backward_gpu.py)."""
    assert lse.shape == ref.lse64.shape and bool(torch.isfinite(lse).all()), f"{label}: bad lse"
    diff = (lse.double() - ref.lse64).abs()
    rel = float((diff / ref.lse64.abs().clamp_min(1.0)).max())
    print(f"{label}: lse error {float(diff.max()):.3e} abs, {rel:.3e} rel (fp32 logsumexp {ref.lse_err32:.3e} abs)")
    assert rel <= LSE_BOUND, f"{label}: lse off by {rel:.3e} rel, {float(diff.max()):.3e} abs"


# ---------------------------------------------------------------------------------------------------------- inputs
def _seed(*parts):
    return zlib.crc32(repr(parts).encode())


def _randn(B, S, H, seed):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(B, S, H * D, generator=g) for _ in range(3)) + (g,)


def unit_case(B, S, H):
    q, k, v, _ = _randn(B, S, H, _seed("unit", B, S, H))
    return Case(f"unit[{B},{S},{H}]", q, k, v, H)


def _channel(t, H, c=0):
    """Channel c of every head: a [B, S, H] view."""
    return _heads(t, H)[..., c].transpose(1, 2)


def late_spike_query(B, S, H):
    """(batch, head, query) whose largest score is the last valid key in the late_spike_one_lane case."""
    return B - 1, H - 1, (S // 2 + 5) % S


def magnitude_case(name, B, S, H):
    """The magnitude and softmax-bookkeeping cases.  The bookkeeping ones write one or two channels of q and k and
    leave the rest randn (63 channels of randn x randn / 8: scores of standard deviation ~1 on top; 0.25 for the two
    ramps)."""
    q, k, v, g = _randn(B, S, H, _seed("magnitude", name, B, S, H))
    pos = torch.arange(S, dtype=torch.float32).view(1, S, 1)
    if name == "peaked_10":
        q *= 10.0
    elif name == "peaked_100":
        q *= 100.0
    elif name == "uniform":
        q.zero_()
    elif name == "k_zero":
        k.zero_()
    elif name == "v_zero":
        v.zero_()
    elif name == "all_zero":
        q.zero_(), k.zero_(), v.zero_()
    elif name == "v_norms_6_decades":
        v *= 10.0 ** (torch.rand(B, S, 1, generator=g) * 6 - 3)
    elif name == "k_norms_4_decades":
        k *= 10.0 ** (torch.rand(B, S, 1, generator=g) * 4 - 2)
    elif name == "k_outlier_1e3":
        k[B - 1, 7 % S, 3] = 1e3
    elif name == "q_outlier_1e3":
        q[B - 1, 5 % S, H * D - 9] = 1e3
    elif name == "v_outlier_1e4":
        v[0, 11 % S, 2] = 1e4
    elif name == "tiny":
        q *= 1e-10
        k *= 1e-10
        v *= 1e-20
    elif name == "v_1e20":
        v *= 1e20
    elif name == "q_2^40_k_2^-40":
        q *= 2.0 ** 40
        k *= 2.0 ** -40
    elif name in ("rising", "falling"):
        # score of key j = +-0.04 j + noise of standard deviation 0.25 (q's other channels x 0.25): the running maximum
        # moves in every 64-key tile by 2.6 (rising) or only in the first (falling), while the scores stay within 40 --
        # the float32 yardstick itself leaves the 2e-5 ceiling once scores reach ~100
        q *= 0.25
        _channel(q, H)[:] = 8.0
        _channel(k, H)[:] = (0.04 if name == "rising" else -0.04) * pos
    elif name == "late_spike_one_lane":
        # key 0 leads every row by 40; for ONE query the last valid key (inside the masked tail tile) scores 160: its
        # slice's maximum is 2^173 above the first slice's, which a merge normalised by the wrong slice cannot hold
        _channel(q, H)[:] = 8.0
        _channel(k, H)[:, 0] = 40.0
        _channel(q, H, 1)[:] = 0.0
        b, h, i = late_spike_query(B, S, H)
        _channel(q, H, 1)[b, i, h] = 16.0
        _channel(k, H, 1)[b, S - 1, h] = 80.0
    elif name == "first_key_only":   # key 0 dominates every row by more than 60 in the exponent
        _channel(q, H)[:] = 8.0
        _channel(k, H)[:, 0] = 70.0
    elif name != "unit":
        raise KeyError(name)
    return Case(f"{name}[{B},{S},{H}]", q, k, v, H)


MAGNITUDE_NAMES = ("unit", "peaked_10", "peaked_100", "uniform", "k_zero", "v_zero", "all_zero", "v_norms_6_decades",
                   "k_norms_4_decades", "k_outlier_1e3", "q_outlier_1e3", "v_outlier_1e4", "tiny", "v_1e20",
                   "q_2^40_k_2^-40", "rising", "falling", "late_spike_one_lane", "first_key_only")
ZERO_OUTPUT = ("v_zero", "all_zero")   # the output must compare equal to zero


def _mx(t):
    return float(t.abs().max())


def _below(x):
    return float(torch.nextafter(torch.tensor(x, dtype=torch.float32), torch.tensor(0.0)))


def _above(x):
    return float(torch.nextafter(torch.tensor(x, dtype=torch.float32), torch.tensor(float("inf"))))


BOUNDS_MAGNITUDES = {"scaled": (3.0, 0.02, 50.0), "unit": (1.0, 1.0, 1.0)}   # "scaled": tests/test_attention_gpu.py
BOUNDS_SLACKS = (1.0, 40.0, 4096.0)
BOUNDS_TARGETS = ("qkv", "q", "k", "v")
BOUNDS_EDGES = ("pow2", "below_one", "one", "above_one")
BOUNDS_OUTSIDE = 2.0 ** 20   # beyond FP16_MAX_OVERSHOOT: documented degradation


def bounds_base(magnitudes, B=1, S=700, H=4):
    q, k, v, _ = _randn(B, S, H, _seed("bounds", B, S, H))
    mq, mk, mv = BOUNDS_MAGNITUDES[magnitudes]
    return q * mq, k * mk, v * mv


def bounds_case(magnitudes, slack, target, B=1, S=700, H=4):
    """Proven bounds = measured maxima x slack on the operands named in `target` (x 1 on the others)."""
    q, k, v = bounds_base(magnitudes, B, S, H)
    bounds = tuple(_mx(t) * (slack if n in target else 1.0) for n, t in zip("qkv", (q, k, v)))
    return Case(f"bounds[{magnitudes},x{slack:g},{target}]", q, k, v, H, bounds=bounds,
                in_envelope=slack <= FP16_MAX_OVERSHOOT)


def bounds_edge_case(edge, B=1, S=700, H=4):
    """The ilogb edge of the kernel's scale exponent: bounds that are exact powers of two, and bounds one ulp below, at
    and one ulp above the point where (bound of q) x scale x log2 e, the bound of k and the bound of v equal one."""
    q, k, v = bounds_base("unit", B, S, H)
    if edge == "pow2":
        bounds = tuple(2.0 ** math.ceil(math.log2(_mx(t))) for t in (q, k, v))
    else:
        q, k, v = (t * (0.999 / _mx(t)) for t in (q, k, v))      # max |.| = 0.999, under every bound below
        one = {"below_one": _below(1.0), "one": 1.0, "above_one": _above(1.0)}[edge]
        sl2 = float(torch.tensor(D ** -0.5 * L2E, dtype=torch.float32))
        q = q / sl2                                              # the kernel scales the q bound by scale x log2 e
        bounds = (float(torch.tensor(one, dtype=torch.float32) / torch.tensor(sl2, dtype=torch.float32)), one, one)
        assert _mx(q) <= bounds[0]
    return Case(f"bounds_edge[{edge}]", q, k, v, H, bounds=bounds)


def two_hot_codes(S):
    """S distinct pairs of channels (c1 < c2): two different codes share at most one channel."""
    pairs = [(a, b) for a in range(D) for b in range(a + 1, D)]
    assert S <= len(pairs)
    step = 37   # coprime with len(pairs) = 2016 = 2^5 3^2 7: spreads the codes over all channels
    return torch.tensor([pairs[(i * step) % len(pairs)] for i in range(S)])


def known_answer_case(scale, S=200):
    """Query i attends key (i + 1) mod S only: q_i = a (e_c1 + e_c2) with the two-hot code of i, the same vector as key
    (i + 1) mod S.  Its own score is 2 a^2 scale, every other at most a^2 scale; a^2 scale = 40, so the other 199 keys
    weigh less than 200 e^-40 = 1e-15.  The answer is v rolled by one row (asymmetric v: a transposed or off-by-one
    index map cannot pass)."""
    a = math.sqrt(40.0 / scale)
    codes = two_hot_codes(S)
    q, k = torch.zeros(1, S, D), torch.zeros(1, S, D)
    idx = torch.arange(S)
    for c in range(2):
        q[0, idx, codes[:, c]] = a
        k[0, (idx + 1) % S, codes[:, c]] = a
    v = torch.arange(S * D, dtype=torch.float32).view(1, S, D) / 100.0
    return Case(f"known_answer[scale={scale:g}]", q, k, v, 1, scale=scale)


# ---------------------------------------------------------------------------------------------------- split regime
SMALL_S = (1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 191, 257)
SMALL_BH = ((1, 1), (2, 3))
SPLIT_SHAPES = ((1, 960, 1), (1, 961, 1), (1, 1023, 1), (1, 1025, 3), (3, 1100, 5), (2, 2081, 3), (1, 3167, 2),
                (1, 6304, 8), (2, 6304, 1))
SHAPES = tuple((B, S, H) for S in SMALL_S for (B, H) in SMALL_BH) + SPLIT_SHAPES
FORCED_SPLITS = (1, 2, 3, 7, 16)
FORCED_SHAPES = ((1, 65, 1),      # 2 tiles: with split 2 the second slice holds one valid key
                 (1, 1025, 3), (2, 1984, 2),   # 17 tiles; 31 tiles: uneven slices
                 (1, 6304, 8))
SPLIT_OUT_EXP = 9   # |out| <= max |v| < 8 for unit randn: 2^9 keeps the first part far inside fp16


def nsplit_from_workspace_bytes(nbytes, B, S, H):
    """The key split the library took, read off amav_selfattn_workspace_bytes under the f32 variant: exactly
    nsplit B H S 66 4 rounded up to 256 for nsplit > 1, else 256 (csrc/attention.hip)."""
    row = B * H * S * (D + 2) * 4
    if nbytes == 256:
        return 1
    n = nbytes // row
    assert n > 1 and nbytes == (n * row + 255) // 256 * 256, (nbytes, B, S, H)
    return n


# -------------------------------------------------------------------------------------- the fp16 x 2 arithmetic model
def _scale_exp(amax):
    return 0 if not amax > 0 else max(-100, min(100, 14 - (math.frexp(amax)[1] - 1)))


def _split2(x):
    x = x.float()
    a = x.half()
    return a.double(), (x - a.float()).half().double()


def model_fp16x2(case):
    """A torch model of the default kernel's arithmetic (csrc/attention.hip, selfattn_f16_kernel):

        e(amax) = 0 if amax <= 0 else clamp(14 - ilogb(amax), -100, 100)
        eq = e(max|q| scale log2e), ek = e(max|k|), ev = e(max|v|)        # or from the caller's bounds
        split2(x): a = fp16(x); b = fp16(x - a)                            # x in fp32
        (q1,q2) = split2(q scale log2e 2^eq); (k1,k2) = split2(k 2^ek); (v1,v2) = split2(v 2^ev)
        s  = fp32(k2 q1^T + k1 q2^T + k1 q1^T) 2^-(eq+ek)                  # log2 domain, [key, query]
        p' = fp32(2^14 exp2(s - max_key s)); (p1,p2) = split2(p')
        out = (v2^T p1 + v1^T p2 + v1^T p1) / sum_key p' 2^-ev

    Sums are float64 here; the kernel accumulates in fp32, which the factor 4 of the bound covers."""
    q, k, v, H = case.q, case.k, case.v, case.heads
    scale = D ** -0.5 if case.scale is None else case.scale
    bq, bk, bv = case.bounds if case.bounds else (_mx(q), _mx(k), _mx(v))
    sl2 = float(torch.tensor(scale * L2E, dtype=torch.float32))
    eq = _scale_exp(float(torch.tensor(bq, dtype=torch.float32) * torch.tensor(sl2, dtype=torch.float32)))
    ek, ev = _scale_exp(bk), _scale_exp(bv)
    qs = torch.tensor(sl2, dtype=torch.float32) * torch.tensor(2.0 ** eq, dtype=torch.float32)
    B, S, HD = q.shape
    out = torch.empty(B, S, HD)
    qh, kh, vh, oh = _heads(q, H), _heads(k, H), _heads(v, H), _heads(out, H)
    for b in range(B):
        for h in range(H):
            q1, q2 = _split2(qh[b, h] * qs)
            k1, k2 = _split2(kh[b, h] * 2.0 ** ek)
            v1, v2 = _split2(vh[b, h] * 2.0 ** ev)
            s = (k2 @ q1.T + k1 @ q2.T + k1 @ q1.T).float().double() * 2.0 ** -(eq + ek)   # [key, query]
            p = (2.0 ** 14 * torch.exp2(s - s.max(dim=0, keepdim=True).values)).float()
            p1, p2 = _split2(p)
            o = (v2.T @ p1 + v1.T @ p2 + v1.T @ p1).float().double()                        # [d, query]
            oh[b, h] = (o / p.double().sum(0, keepdim=True) * 2.0 ** -ev).T.float()
    return out
