"""numpy restatement of the float32-accumulated Sum of float16 / bfloat16
buffers (include/rdc_amd.h RdcAllreduceAcc32).

The rule, for element e of utils::Split chunk c, x[q] rank q's value:

    s = f32(x[c-1]);  for j = 2..n:  s = f32(x[c-j]) + s      (indices mod n)
    result = round_to_T(s)

float16 is numpy's: ``astype(np.float32)`` is exact, ``+`` on float32 arrays
is the IEEE binary32 add (RNE, subnormals kept), ``astype(np.float16)`` rounds
to nearest even once (overflow -> inf).  bfloat16 is uint16 bits: widened with
ops_ref.bf16_to_f32 (a shift), rounded with ops_ref.f32_to_bf16 (the oracle's
rdc_oracle_f32_to_bf16).  Chunks come from O.split, nothing else from the
oracle.
"""
import numpy as np

from oracle import oracle as O
from tests import ops_ref

DTYPES = (O.DT_FLOAT16, O.DT_BFLOAT16)


def widen(x, dtype):
    if dtype == O.DT_BFLOAT16:
        assert x.dtype == np.uint16
        return ops_ref.bf16_to_f32(x)
    assert dtype == O.DT_FLOAT16 and x.dtype == np.float16
    return x.astype(np.float32)


def narrow(s, dtype):
    assert s.dtype == np.float32
    with np.errstate(all="ignore"):
        if dtype == O.DT_BFLOAT16:
            return ops_ref.f32_to_bf16(s)
        return s.astype(np.float16)


def fold(vals, dtype):
    """round_to_T(((f32(v0) + f32(v1)) + ...)) with every step ``s = f32(v) + s``."""
    s = widen(vals[0], dtype)
    with np.errstate(all="ignore"):
        for v in vals[1:]:
            s = widen(v, dtype) + s
    return narrow(s, dtype)


def chunk_order(c, n):
    """The ranks in the order chunk c folds them: c-1, c-2, ..., c (mod n)."""
    return [(c - j) % n for j in range(1, n + 1)]


def allreduce(xs, dtype):
    """The rule: chunk c folds x[c-1], x[c-2], ..., x[c]."""
    n, count = len(xs), xs[0].size
    out = np.empty_like(xs[0])
    for c, (b, e) in enumerate(O.split(count, n)):
        out[b:e] = fold([xs[q][b:e] for q in chunk_order(c, n)], dtype)
    return out


def allreduce_in_order(xs, dtype, order):
    """Every element folded in one rank order (a wrong fold: the ascending
    order a reader would guess, or another chunk's order)."""
    return fold([xs[q] for q in order], dtype)


def same_sum(order_a, order_b):
    """True when two orders are one fold: equal, or equal but for the first
    two ranks swapped (the first add commutes; no later one does, since
    ``s = f32(x) + s`` rounds after every step)."""
    return list(order_a[2:]) == list(order_b[2:]) and set(order_a[:2]) == set(order_b[:2])


def reduce_scatter(xs, dtype):
    """Per rank: its input with Split chunk r replaced by the rule's."""
    full = allreduce(xs, dtype)
    out = []
    for r, (b, e) in enumerate(O.split(xs[0].size, len(xs))):
        x = np.array(xs[r], copy=True)
        x[b:e] = full[b:e]
        out.append(x)
    return out


def reduce_to(xs, dtype, root):
    """Per rank: the rule's result on root, the input everywhere else."""
    return [allreduce(xs, dtype) if r == root else np.array(xs[r], copy=True) for r in range(len(xs))]


def per_hop(xs, dtype):
    """The ordinary Sum's ring order (a rounding to 16 bits at every hop)."""
    return ops_ref.ring(xs, ops_ref.OP_SUM, dtype)


def gen_input(rng, count, dtype):
    """Random sign, full random mantissa, and exponents spread so that the
    float32 sums are inexact in 16 bits.  float16: exponent field uniform in
    1..26 (2^-14 <= |x| < 4096: twelve of them cannot overflow 65504).
    bfloat16: exponent field uniform in 107..147 (2^-20 <= |x| < 2^21)."""
    sign = rng.integers(0, 2, count).astype(np.uint16) << 15
    if dtype == O.DT_BFLOAT16:
        return (sign | (rng.integers(107, 148, count).astype(np.uint16) << 7) |
                rng.integers(0, 128, count).astype(np.uint16)).astype(np.uint16)
    assert dtype == O.DT_FLOAT16
    return (sign | (rng.integers(1, 27, count).astype(np.uint16) << 10) |
            rng.integers(0, 1024, count).astype(np.uint16)).astype(np.uint16).view(np.float16)


def gen_rank(seed, rank, count, dtype):
    """Rank ``rank``'s input of a run (a worker process generates its own)."""
    return gen_input(np.random.default_rng([seed, rank]), count, dtype)


def gen_inputs(seed, n, count, dtype):
    return [gen_rank(seed, r, count, dtype) for r in range(n)]


def from_f32(vals, dtype):
    """float32 values that are exact in the 16-bit format -> its arrays."""
    f = np.asarray(vals, dtype=np.float32)
    out = narrow(f, dtype)
    assert np.array_equal(widen(out, dtype), f), "value not representable"
    return out


def order_table(n, dtype, count=None):
    """Cancellation rows that show the fold order after the final rounding:
    one rank holds +B, one -B, one a small value t with more bits than B's
    ulp leaves room for, the rest 0 — in every assignment of (+B, -B, t) to
    three distinct ranks, tiled across ``count`` elements (default: a few
    tiles more than one assignment per chunk).  t + B rounds t away in
    float32 only when t meets B before -B does, so the result is t or a
    rounding of it depending on the order.
    float16: B = 32768, t = 2^-10 + 2^-20.  bfloat16: B = 2^20, t = 1 + 2^-7."""
    if dtype == O.DT_FLOAT16:
        big, t = 32768.0, 2.0 ** -10 + 2.0 ** -20
    else:
        big, t = 2.0 ** 20, 1.0 + 2.0 ** -7
    rows = [(p, m, s) for p in range(n) for m in range(n) for s in range(n) if len({p, m, s}) == 3]
    if count is None:
        count = n * len(rows) + 3
    f = np.zeros((n, count), dtype=np.float32)
    e = np.arange(count)
    pick = np.array(rows)[e % len(rows)]
    f[pick[:, 0], e], f[pick[:, 1], e], f[pick[:, 2], e] = big, -big, t
    return [from_f32(f[q], dtype) for q in range(n)]


def specials(n, dtype):
    """+-0, +-inf, inf - inf, subnormals of both formats, the largest finite
    values: one column per case, rank q's value in row q (ranks beyond the
    listed ones hold +0)."""
    if dtype == O.DT_FLOAT16:
        # bits: max 0x7BFF, least subnormal 0x0001, largest subnormal 0x03FF
        cols = [(0x0000, 0x8000), (0x8000, 0x8000), (0x7C00, 0x3C00), (0xFC00, 0x7BFF), (0x7C00, 0xFC00),
                (0x0001, 0x0001), (0x03FF, 0x0001), (0x8001, 0x0400), (0x7BFF, 0x7BFF), (0xFBFF, 0x7BFF),
                (0x7BFF, 0x0001), (0x0001, 0x8001), (0x7BFF, 0x5000)]
    else:
        # bits: max 0x7F7F, least subnormal 0x0001, largest subnormal 0x007F;
        # 0x0001 is also a float32 subnormal once widened (2^-133)
        cols = [(0x0000, 0x8000), (0x8000, 0x8000), (0x7F80, 0x3F80), (0xFF80, 0x7F7F), (0x7F80, 0xFF80),
                (0x0001, 0x0001), (0x007F, 0x0001), (0x8001, 0x0080), (0x7F7F, 0x7F7F), (0xFF7F, 0x7F7F),
                (0x7F7F, 0x0001), (0x0001, 0x8001), (0x7F7F, 0x7700)]
    bits = np.zeros((n, len(cols) * n), dtype=np.uint16)
    for k, col in enumerate(cols):
        for shift in range(n):  # every rotation, so every chunk's order meets the case
            for q, v in enumerate(col):
                bits[(q + shift) % n, k * n + shift] = v
    return [bits[q].copy() if dtype == O.DT_BFLOAT16 else bits[q].copy().view(np.float16) for q in range(n)]
