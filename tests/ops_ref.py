"""numpy restatement of Prod / BitAND / BitXOR (ops 8 / 9 / 10) and of the
orders the device path folds them in (the CPU oracle cannot grow an operator).

The rules (include/rdc_amd.h), dst = OP(dst, src):

    Prod:   dst * src.  Integers wrap modulo 2^bits (multiplied through the
            unsigned view).  float32 / float64: numpy's IEEE multiply.  float16:
            numpy's half multiply, which computes in float32 and rounds once;
            the float32 product of two halves is exact (11 x 11 significand
            bits), so that is the correctly rounded half product.  bfloat16
            (stored as uint16 bits): widened to float32, multiplied (exact,
            8 x 8 bits), rounded once with the oracle's rdc_oracle_f32_to_bf16.
    BitAND: dst & src, BitXOR: dst ^ src (integers).

``apply`` also folds with Max / Min / Sum (ops 0 / 1 / 2) through the oracle's
reducer — tests/test_ops_plan.py runs the ring and tree folds below with them
against O.allreduce_ring / O.allreduce_tree, which ties the order code here to
the oracle's.  The orders take O.split and O.tree_program from the oracle,
nothing else.
"""
import numpy as np

from oracle import oracle as O

OP_MAX, OP_MIN, OP_SUM, OP_BITOR = 0, 1, 2, 3
OP_PROD, OP_BITAND, OP_BITXOR = 8, 9, 10
NEW_OPS = (OP_PROD, OP_BITAND, OP_BITXOR)
INT_DTYPES = (0, 1, 2, 3, 4, 5, 8, 9)
# every (dtype, op) of the new set, the long long dtypes counted as dtypes
NEW_VALID = [(dt, OP_PROD) for dt in range(12)] + [(dt, op) for op in (OP_BITAND, OP_BITXOR) for dt in INT_DTYPES]
# the same without the long long aliases (they run int64 / uint64's kernels)
NEW_VALID_KERNELS = [(dt, op) for dt, op in NEW_VALID if dt not in (8, 9)]
UNSIGNED = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


def bf16_to_f32(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32)


def f32_to_bf16(f):
    """rdc_oracle_f32_to_bf16 element by element (RNE; a NaN stays a NaN)."""
    flat = np.ascontiguousarray(f, dtype=np.float32).ravel()
    u, inv = np.unique(flat.view(np.uint32), return_inverse=True)
    conv = O.lib().rdc_oracle_f32_to_bf16
    table = np.array([conv(float(v)) for v in u.view(np.float32)], dtype=np.uint16)
    return table[inv].reshape(np.shape(f))


def apply(op, dst, src, dtype=None):
    """OP(dst, src) element by element, as a new array.  ``dtype`` is the
    library's code; it is needed for bfloat16 (11, uint16 bits) only."""
    dst, src = np.ascontiguousarray(dst), np.ascontiguousarray(src)
    assert dst.dtype == src.dtype and dst.shape == src.shape
    if op in (OP_MAX, OP_MIN, OP_SUM, OP_BITOR):
        assert dtype is not None
        return O.reducer(src.copy(), dst.copy(), dtype, op)
    if dtype == O.DT_BFLOAT16:
        assert op == OP_PROD and dst.dtype == np.uint16
        with np.errstate(all="ignore"):
            return f32_to_bf16(bf16_to_f32(dst) * bf16_to_f32(src))
    if dst.dtype.kind == "f":
        assert op == OP_PROD
        with np.errstate(all="ignore"):
            return dst * src
    assert dst.dtype.kind in "iu"
    u = UNSIGNED[dst.dtype.itemsize]
    d, s = dst.view(u), src.view(u)
    if op == OP_PROD:
        with np.errstate(over="ignore"):
            r = d * s
    elif op == OP_BITAND:
        r = d & s
    elif op == OP_BITXOR:
        r = d ^ s
    else:
        raise ValueError(op)
    return r.astype(u).view(dst.dtype)


def ring(xs, op, dtype=None):
    """The ring order per utils::Split chunk r: partial = x[r-1]; for j = 2..n:
    partial = OP(dst = x[r-j], src = partial)."""
    n, count = len(xs), xs[0].size
    out = np.empty_like(xs[0])
    for r, (b, e) in enumerate(O.split(count, n)):
        partial = xs[(r - 1) % n][b:e]
        for j in range(2, n + 1):
            partial = apply(op, xs[(r - j) % n][b:e], partial, dtype)
        out[b:e] = partial
    return out


def tree(xs, op, dtype=None):
    """The tree order: acc[dst] = OP(dst = acc[dst], src = acc[src]) over
    O.tree_program(n); the result is acc[0]."""
    acc = [np.array(x, copy=True) for x in xs]
    for d, s in O.tree_program(len(xs)):
        acc[d] = apply(op, acc[d], acc[s], dtype)
    return acc[0]


def scan(xs, op, exclusive=False, dtype=None):
    """Per rank: y[0] = x[0], y[q] = OP(dst = y[q-1], src = x[q]); exclusive:
    rank r > 0 gets y[r-1]; rank 0 keeps its input in both modes."""
    y = [np.array(xs[0], copy=True)]
    for q in range(1, len(xs)):
        y.append(apply(op, y[q - 1], xs[q], dtype))
    if exclusive:
        return [y[0]] + y[:-1]
    return y


def reduce_scatter(xs, op, dtype=None):
    """Per rank: its input with Split chunk r replaced by the ring fold's."""
    full = ring(xs, op, dtype)
    out = []
    for r, (b, e) in enumerate(O.split(xs[0].size, len(xs))):
        x = np.array(xs[r], copy=True)
        x[b:e] = full[b:e]
        out.append(x)
    return out


def left_to_right(xs, op, dtype=None):
    """((x[0] OP x[1]) OP x[2]) ...: the order a reader would guess, which the
    ring's is not."""
    return scan(xs, op, False, dtype)[-1]


def gen_input(rng, count, dtype):
    """Integers: full range.  Floats (bfloat16 as uint16 bits): random sign,
    magnitude in [0.5, 2) with a full random mantissa, so a product of 8 stays
    finite and normal (2^-8 .. 2^8) and every step rounds."""
    npd = np.dtype(O.NP_DTYPE[dtype])
    if dtype == O.DT_BFLOAT16:
        # sign | exponent 126 or 127 | 7 random mantissa bits
        return ((rng.integers(0, 2, count) << 15) | ((126 + rng.integers(0, 2, count)) << 7) |
                rng.integers(0, 128, count)).astype(np.uint16)
    if npd.kind == "f":
        mant = {2: 10, 4: 23, 8: 52}[npd.itemsize]
        bias = {2: 15, 4: 127, 8: 1023}[npd.itemsize]
        u = UNSIGNED[npd.itemsize]
        bits = ((rng.integers(0, 2, count, dtype=np.uint64) << np.uint64(8 * npd.itemsize - 1)) |
                ((np.uint64(bias - 1) + rng.integers(0, 2, count, dtype=np.uint64)) << np.uint64(mant)) |
                rng.integers(0, 1 << mant, count, dtype=np.uint64))
        return bits.astype(u).view(npd)
    info = np.iinfo(npd)
    return rng.integers(info.min, info.max, count, dtype=npd, endpoint=True)


def gen_inputs(seed, n, count, dtype):
    rng = np.random.default_rng(seed)
    return [gen_input(rng, count, dtype) for _ in range(n)]


def is_nan(a, dtype):
    if dtype == O.DT_BFLOAT16:
        return (a & 0x7FFF) > 0x7F80
    return np.isnan(a) if a.dtype.kind == "f" else np.zeros(a.shape, dtype=bool)


def is_inf(a, dtype):
    if dtype == O.DT_BFLOAT16:
        return (a & 0x7FFF) == 0x7F80
    return np.isinf(a) if a.dtype.kind == "f" else np.zeros(a.shape, dtype=bool)


def assert_finite(a, dtype, what=""):
    """No NaN and no inf: tests/gpu_util.same_bits treats any two NaNs as
    equal, so expected data that held one could hide a difference."""
    assert not is_nan(a, dtype).any() and not is_inf(a, dtype).any(), ("NaN or inf in expected data", what)
