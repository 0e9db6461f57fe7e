"""numpy restatement of MaxLoc / MinLoc over (value, index) pairs and of the
orders the device path folds them in (the CPU oracle cannot grow a dtype).

The rule (include/rdc_amd.h, op 4 / 5):

    MaxLoc: dst = src when dst.value < src.value ||
                          (dst.value == src.value && src.index < dst.index)
    MinLoc: the same with > in the first comparison

``apply`` also folds plain arrays with Max (op 0) / Min (op 1), the oracle's
``dst = src when dst < src`` — tests/test_loc_plan.py runs the ring and tree
folds below with them against O.allreduce_ring / O.allreduce_tree, which ties
the order code here to the oracle's.  From the oracle: O.split and
O.tree_program, nothing else.
"""
import numpy as np

from oracle import oracle as O

OP_MAX, OP_MIN, OP_MAXLOC, OP_MINLOC = 0, 1, 4, 5
DT_F32_I32, DT_I32_I32 = 12, 13
F32_I32 = np.dtype([("value", np.float32), ("index", np.int32)])
I32_I32 = np.dtype([("value", np.int32), ("index", np.int32)])
NP_DTYPE = {DT_F32_I32: F32_I32, DT_I32_I32: I32_I32}

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
VALUES = {DT_F32_I32: np.array([-1.0, -0.0, 0.0, 2.5, np.nan], dtype=np.float32),
          DT_I32_I32: np.array([-1, 0, 0, 7, INT32_MIN], dtype=np.int32)}
INDEXES = np.array([-3, 0, 2, 9], dtype=np.int32)


def new_stats():
    return {"index_rule": 0, "full_tie": 0, "nan_dst": 0}


def take(op, dst, src, stats=None):
    """Boolean mask: where src replaces dst."""
    with np.errstate(invalid="ignore"):
        if op in (OP_MAX, OP_MIN):
            return dst < src if op == OP_MAX else dst > src
        dv, sv, di, si = dst["value"], src["value"], dst["index"], src["index"]
        better = dv < sv if op == OP_MAXLOC else dv > sv
        tie = dv == sv
        if stats is not None:
            stats["index_rule"] += int((tie & (si != di)).sum())
            stats["full_tie"] += int((tie & (si == di)).sum())
            if dv.dtype.kind == "f":
                stats["nan_dst"] += int(np.isnan(dv).sum())
        return better | (tie & (si < di))


def apply(op, dst, src, stats=None):
    """OP(dst, src) element by element, as a new array; dst's elements stay
    whole (value bits included) wherever src does not replace them."""
    out = np.array(dst, copy=True)
    m = take(op, dst, src, stats)
    out[m] = src[m]
    return out


def ring(xs, op, stats=None):
    """The ring order per utils::Split chunk r: partial = x[r-1]; for j = 2..n:
    partial = OP(dst = x[r-j], src = partial)."""
    n, count = len(xs), xs[0].size
    out = np.empty_like(xs[0])
    for r, (b, e) in enumerate(O.split(count, n)):
        partial = xs[(r - 1) % n][b:e]
        for j in range(2, n + 1):
            partial = apply(op, xs[(r - j) % n][b:e], partial, stats)
        out[b:e] = partial
    return out


def tree(xs, op, stats=None):
    """The tree order: acc[dst] = OP(dst = acc[dst], src = acc[src]) over
    O.tree_program(n); the result is acc[0]."""
    acc = [np.array(x, copy=True) for x in xs]
    for d, s in O.tree_program(len(xs)):
        acc[d] = apply(op, acc[d], acc[s], stats)
    return acc[0]


def scan(xs, op, exclusive=False, stats=None):
    """Per rank: y[0] = x[0], y[q] = OP(dst = y[q-1], src = x[q]); exclusive:
    rank r > 0 gets y[r-1]; rank 0 keeps its input in both modes."""
    y = [np.array(xs[0], copy=True)]
    for q in range(1, len(xs)):
        y.append(apply(op, y[q - 1], xs[q], stats))
    if exclusive:
        return [y[0]] + y[:-1]
    return y


def reduce_scatter(xs, op, stats=None):
    """Per rank: its input with Split chunk r replaced by the ring fold's."""
    full = ring(xs, op, stats)
    out = []
    for r, (b, e) in enumerate(O.split(xs[0].size, len(xs))):
        x = np.array(xs[r], copy=True)
        x[b:e] = full[b:e]
        out.append(x)
    return out


def gen_inputs(seed, n, count, dtype):
    """n per-rank arrays of pairs drawn from five values and four indexes, so
    ranks collide in value and in index."""
    rng = np.random.default_rng(seed)
    xs = []
    for _ in range(n):
        x = np.empty(count, dtype=NP_DTYPE[dtype])
        x["value"] = VALUES[dtype][rng.integers(0, 5, count)]
        x["index"] = INDEXES[rng.integers(0, 4, count)]
        xs.append(x)
    return xs


def assert_covers_ties(stats, dtype, what=""):
    """The three kinds of element a tie test must contain (counted over every
    fold step of the expected data)."""
    assert stats["index_rule"] > 0, ("no element decided by the index rule", what)
    assert stats["full_tie"] > 0, ("no full tie", what)
    if dtype == DT_F32_I32:
        assert stats["nan_dst"] > 0, ("no NaN in the first operand of a fold", what)


def _p(dtype, value, index):
    a = np.zeros(1, dtype=NP_DTYPE[dtype])
    a["value"], a["index"] = value, index
    return a


def rule_table(dtype):
    """[(case name, dst, src, MaxLoc result, MinLoc result)], each a 1-element
    pair array; "dst" / "src" as results name which operand is left there."""
    f = dtype == DT_F32_I32
    rows = [
        ("greater", (1, 5), (2, 9), "src", "dst"),
        ("less", (2, 5), (1, 1), "dst", "src"),
        ("equal value, lower index", (3, 5), (3, 4), "src", "src"),
        ("equal value, higher index", (3, 5), (3, 6), "dst", "dst"),
        ("equal value, equal index", (3, 5), (3, 5), "dst", "dst"),
        ("negative index is lower", (3, 0), (3, -1), "src", "src"),
        ("INT32_MIN index", (3, INT32_MAX), (3, INT32_MIN), "src", "src"),
        ("INT32_MAX index", (3, INT32_MIN), (3, INT32_MAX), "dst", "dst"),
    ]
    if f:
        nan, inf = np.float32("nan"), np.float32("inf")
        rows += [
            ("NaN in dst", (nan, 5), (1, 0), "dst", "dst"),
            ("NaN in src", (1, 5), (nan, 0), "dst", "dst"),
            ("both NaN", (nan, 5), (nan, 0), "dst", "dst"),
            ("+0 vs -0, lower index", (0.0, 5), (-0.0, 4), "src", "src"),
            ("-0 vs +0, higher index", (-0.0, 5), (0.0, 6), "dst", "dst"),
            ("+0 vs -0, equal index", (0.0, 5), (-0.0, 5), "dst", "dst"),
            ("-0 vs +0, equal index", (-0.0, 5), (0.0, 5), "dst", "dst"),
            ("+inf vs max", (inf, 1), (np.finfo(np.float32).max, 0), "dst", "src"),
            ("-inf vs lowest", (-inf, 1), (-np.finfo(np.float32).max, 0), "src", "dst"),
        ]
    else:
        rows += [
            ("INT32_MIN vs INT32_MAX value", (INT32_MIN, 1), (INT32_MAX, 2), "src", "dst"),
            ("INT32_MAX vs INT32_MIN value", (INT32_MAX, 1), (INT32_MIN, 0), "dst", "src"),
            ("INT32_MIN value tie", (INT32_MIN, 1), (INT32_MIN, 0), "src", "src"),
            ("-1 vs 0", (-1, 1), (0, 2), "src", "dst"),
        ]
    out = []
    for name, d, s, mx, mn in rows:
        dst, src = _p(dtype, *d), _p(dtype, *s)
        out.append((name, dst, src, src if mx == "src" else dst, src if mn == "src" else dst))
    return out


def table_arrays(dtype):
    """(dst, src, MaxLoc results, MinLoc results) of rule_table as arrays."""
    t = rule_table(dtype)
    return tuple(np.concatenate([row[k] for row in t]) for k in (1, 2, 3, 4))
