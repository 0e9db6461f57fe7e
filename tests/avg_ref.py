"""numpy restatement of Avg, the mean across ranks of float32 / float64 /
float16 / bfloat16 buffers (include/rdc_amd.h RdcAllreduceAvg).

The rule, for element e of utils::Split chunk c, x[q] rank q's value:

    float32 / float64 (T):   s = x[c-1];  for j = 2..n:  s = x[c-j] + s   in T
                             result = s / T(n)
    float16 / bfloat16 (T):  s = f32(x[c-1]);  for j = 2..n:  s = f32(x[c-j]) + s
                             q = s / float32(n);  result = round_to_T(q)

float32 / float64: ``ops_ref.ring`` is the ordinary Sum's ring order, numpy's
``/`` on arrays of one float type is the IEEE division (RNE, subnormals kept).
16-bit: the un-narrowed fold of tests/acc32_ref.py (its ``widen`` / ``narrow``),
divided by ``np.float32(n)``, narrowed once.  Chunks come from O.split.
"""
import numpy as np

from oracle import oracle as O
from tests import acc32_ref as A
from tests import ops_ref

F32, F64, F16, BF = O.DT_FLOAT32, O.DT_FLOAT64, O.DT_FLOAT16, O.DT_BFLOAT16
DTYPES = (F32, F64, F16, BF)
WIDE = (F32, F64)
NP_WIDE = {F32: np.float32, F64: np.float64}
ESIZE = {F32: 4, F64: 8, F16: 2, BF: 2}
BITS = {F32: np.uint32, F64: np.uint64, F16: np.uint16, BF: np.uint16}


def bits(a, dtype):
    return np.ascontiguousarray(a).view(BITS[dtype])


def fold_sum(vals, dtype):
    """The un-divided, un-narrowed fold ``s = v + s`` over vals in order: in T
    for float32 / float64, in float32 for the 16-bit types."""
    with np.errstate(all="ignore"):
        if dtype in WIDE:
            s = np.array(vals[0], copy=True)
            for v in vals[1:]:
                s = v + s
            return s
        s = A.widen(vals[0], dtype)
        for v in vals[1:]:
            s = A.widen(v, dtype) + s
        return s


def finish(s, n, dtype):
    """The division and, for the 16-bit types, the one rounding."""
    with np.errstate(all="ignore"):
        if dtype in WIDE:
            assert s.dtype == NP_WIDE[dtype]
            return s / NP_WIDE[dtype](n)
        q = s / np.float32(n)
        assert q.dtype == np.float32
    return A.narrow(q, dtype)


def fold(vals, dtype):
    return finish(fold_sum(vals, dtype), len(vals), dtype)


chunk_order = A.chunk_order
same_sum = A.same_sum


def allreduce(xs, dtype):
    """The rule: chunk c folds x[c-1], x[c-2], ..., x[c], then divides."""
    n, count = len(xs), xs[0].size
    if dtype in WIDE:
        return finish(ops_ref.ring(xs, ops_ref.OP_SUM, dtype), n, dtype)
    out = np.empty_like(xs[0])
    for c, (b, e) in enumerate(O.split(count, n)):
        out[b:e] = fold([xs[q][b:e] for q in chunk_order(c, n)], dtype)
    return out


def allreduce_in_order(xs, dtype, order):
    """Every element folded in one rank order (a wrong fold), then divided."""
    return fold([xs[q] for q in order], dtype)


def sum_round_then_divide(xs, dtype):
    """What a caller does today: the float32-accumulated Sum rounded to 16
    bits, then a second pass that divides and rounds again (16-bit types)."""
    assert dtype not in WIDE
    n = len(xs)
    s16 = A.allreduce(xs, dtype)
    with np.errstate(all="ignore"):
        return A.narrow(A.widen(s16, dtype) / np.float32(n), dtype)


def sum_times_reciprocal(xs, dtype):
    """The ring Sum multiplied by the rounded 1 / n (float32 / float64): what
    the rule forbids."""
    t = NP_WIDE[dtype]
    with np.errstate(all="ignore"):
        return ops_ref.ring(xs, ops_ref.OP_SUM, dtype) * (t(1) / t(len(xs)))


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


def gen_input(rng, count, dtype):
    """16-bit: acc32_ref's generator.  float32 / float64: random sign, full
    random mantissa, exponents spread over 2^-12 .. 2^12, so every add rounds
    and nothing overflows or goes subnormal."""
    if dtype not in WIDE:
        return A.gen_input(rng, count, dtype)
    t = NP_WIDE[dtype]
    m = rng.random(count).astype(t) + t(1)      # [1, 2), full mantissa of the format for float32
    if dtype == F64:
        m = (rng.integers(0, 1 << 52, count, dtype=np.uint64) | np.uint64(0x3FF0000000000000)).view(np.float64)
    e = rng.integers(-12, 13, count)
    sign = np.where(rng.integers(0, 2, count) == 1, t(-1), t(1))
    return (sign * np.ldexp(m, e)).astype(t)


def gen_rank(seed, rank, count, dtype):
    """Rank ``rank``'s input of a run (a worker process generates its own)."""
    return gen_input(np.random.default_rng([seed, rank]), count, dtype)


def gen_inputs(seed, n, count, dtype):
    return [gen_rank(seed, r, count, dtype) for r in range(n)]


def order_table(n, dtype, count=None):
    """Cancellation rows that still show the fold order after the division.
    16-bit: acc32_ref.order_table.  float32 / float64, the same construction:
    one rank holds +B, one -B, one a value t with a bit below B's ulp, the
    rest 0, in every assignment to three distinct ranks, tiled across
    ``count`` elements.  t + B rounds t's low bit away only when t meets B
    before -B does.  float32: B = 2^24, t = 1 + 2^-23.  float64: B = 2^53,
    t = 1 + 2^-52."""
    if dtype not in WIDE:
        return A.order_table(n, dtype, count=count)
    t = NP_WIDE[dtype]
    big, small = (t(2.0 ** 24), t(1.0) + t(2.0 ** -23)) if dtype == F32 else (t(2.0 ** 53), t(1.0) + t(2.0 ** -52))
    rows = [(p, m, s) for p in range(n) for m in range(n) for s in range(n) if len({p, m, s}) == 3]
    if count is None:
        count = n * len(rows) + 3
    f = np.zeros((n, count), dtype=t)
    e = np.arange(count)
    pick = np.array(rows)[e % len(rows)]
    f[pick[:, 0], e], f[pick[:, 1], e], f[pick[:, 2], e] = big, -big, small
    return [f[q].copy() for q in range(n)]


def specials(n, dtype):
    """+-0, +-inf, inf - inf, subnormals of the format, the largest finite
    values: one column per case in every rotation, rank q's value in row q
    (ranks beyond the listed ones hold +0).  16-bit: acc32_ref.specials plus
    the float16 overflow row (40000.0 on every rank: Sum overflows, the mean
    does not) and, for bfloat16, its largest finite value on every rank."""
    if dtype not in WIDE:
        base = A.specials(n, dtype)
        v = 0x78E2 if dtype == F16 else 0x7F7F      # float16 40000.0; bfloat16 max
        extra = np.full(n + 1, v, dtype=np.uint16)
        extra = extra if dtype == BF else extra.view(np.float16)
        return [np.concatenate([b, extra]) for b in base]
    t, u = NP_WIDE[dtype], BITS[dtype]
    fi = np.finfo(t)
    sub, inf, mx = np.array([1], dtype=u).view(t)[0], t(np.inf), fi.max
    lsub = np.nextafter(fi.tiny, t(0))          # largest subnormal
    cols = [(t(0.0), -t(0.0)), (-t(0.0), -t(0.0)), (inf, t(1)), (-inf, mx), (inf, -inf), (sub, sub), (lsub, sub),
            (-sub, fi.tiny), (mx, mx), (-mx, mx), (mx, sub), (sub, -sub), (mx, t(3.0)), (fi.tiny, t(0)),
            (t(1.0), t(0))]
    a = np.zeros((n, len(cols) * n), dtype=t)
    for k, col in enumerate(cols):
        for shift in range(n):
            for q, v in enumerate(col):
                a[(q + shift) % n, k * n + shift] = v
    return [a[q].copy() for q in range(n)]
