"""Inputs and references shared by the cross-attention tests (test_cross_attention_gpu.py): q [B, Sq, H*64] and a fused
kv [B, Sk, 2*H*64] (k | v) as seeded CPU fp32 tensors, and the float64 / float32 CPU SDPA of attention_cases, which
runs one (batch, head) at a time and takes the query and key counts from its operands.  A plain module: it loads
nothing from the HIP library.  The bound is attention_cases' (check, check_lse, FACTOR, FLOOR, CEILING); it is not
restated here.
"""
import functools
import zlib

import torch

import attention_cases as ac
from attention_cases import CEILING, FACTOR, FLOOR, check, check_lse  # noqa: F401 (the bound, for the tests)

D = ac.D
# (Sq, Sk): one query, one key, either side of the 32-query wave, the 64-key tile and the 128-query workgroup, both
# orders of Sq and Sk, and two shapes whose key sweep is split over workgroups
SMALL = ((1, 2), (1, 64), (31, 33), (33, 31), (64, 65), (127, 1), (128, 64), (129, 200), (200, 129))
SPLIT = ((5, 1030), (80, 4096))
BH = ((1, 1), (2, 3))
SHAPES = tuple((B, Sq, Sk, H) for (Sq, Sk) in SMALL + SPLIT for (B, H) in BH) + ((1, 3152, 4096, 8),)
REFERENCE_SHAPE = (1, 3152, 4096, 8)   # the fusion network's layer; the SMPL-X predictor's is (1, 80, 4096, 8)
Q_PAD, KV_PAD = 12, 20                 # floats of row padding the GPU tests read q and kv through


def _seed(*parts):
    return zlib.crc32(repr(parts).encode())


@functools.lru_cache(maxsize=None)
def inputs(B, Sq, Sk, H):
    """-> (q [B,Sq,H*64], kv [B,Sk,2*H*64]) CPU fp32, the same bits in every process.  Treat as read-only."""
    g = torch.Generator().manual_seed(_seed("cross", B, Sq, Sk, H))
    return torch.randn(B, Sq, H * D, generator=g), torch.randn(B, Sk, 2 * H * D, generator=g)


def grad_out(B, Sq, Sk, H):
    g = torch.Generator().manual_seed(_seed("cross dout", B, Sq, Sk, H))
    return torch.randn(B, Sq, H * D, generator=g)


def case(B, Sq, Sk, H):
    q, kv = inputs(B, Sq, Sk, H)
    return ac.Case(f"cross[{B},{Sq},{Sk},{H}]", q, kv[..., :H * D], kv[..., H * D:], H)


@functools.lru_cache(maxsize=None)
def reference(B, Sq, Sk, H):
    """attention_cases.Reference (float64 SDPA, the float32 yardstick's error, float64 log-sum-exp) of case(...),
    computed once per process.  Treat as read-only."""
    return ac.reference(case(B, Sq, Sk, H), lse=True)


def known_answer_case(Sq=150, Sk=200, shift=7, scale=0.125):
    """The two-hot construction of attention_cases.known_answer_case with separate query and key counts: query i
    carries the code of key (i + shift) mod Sk, whose score leads every other by a^2 scale = 40, so `out` is row
    (i + shift) mod Sk of an asymmetric v.  A transposed index map or swapped Sq / Sk cannot pass.
    -> (Case, the selected key of every query)"""
    a = (40.0 / scale) ** 0.5
    codes = ac.two_hot_codes(Sk)
    q, k = torch.zeros(1, Sq, D), torch.zeros(1, Sk, D)
    sel = (torch.arange(Sq) + shift) % Sk
    for c in range(2):
        q[0, torch.arange(Sq), codes[sel, c]] = a
        k[0, torch.arange(Sk), codes[:, c]] = a
    v = torch.arange(Sk * D, dtype=torch.float32).view(1, Sk, D) / 100.0
    return ac.Case(f"cross known answer[{Sq},{Sk}]", q, k, v, 1, scale=scale), sel
