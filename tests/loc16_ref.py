"""The 16-byte (value, index) pairs of MaxLoc / MinLoc — dtypes 16 F64_I64
{double, int64} and 17 I64_I64 {int64, int64} — for the tests: numpy dtypes, a
generator, a rule table and wider fold statistics.

The rule and the fold orders are tests/loc_ref.py's, unchanged: its ``take``,
``apply``, ``ring``, ``tree``, ``scan`` and ``reduce_scatter`` are generic over
structured arrays with ``value`` / ``index`` fields and are tied to the
oracle's orders by tests/test_loc_plan.py.  What is new here is data that a
32-bit or float32 shortcut in a kernel would get wrong:

* two doubles that are equal as float32 (1.0 and 1.0 + 2**-40);
* values that differ only in their high dword (1 << 32 against 0; the doubles
  1.0 against 2.0), and values that differ only in the low dword with its top
  bit set (1 << 31 against 1: a signed compare of the low dword inverts it);
* INT64_MIN and INT64_MAX, as values and as indexes;
* indexes with the same properties, negative against positive among them;
* for float64 also NaN, -0 / +0 and +-inf against +-max.

``new_stats`` extends loc_ref's statistics by ``value_high`` and
``index_high``: fold steps decided by the value's (the index's) bits above bit
31 alone, the low dwords being equal.
"""
import numpy as np

from tests import loc_ref as L

OP_MAXLOC, OP_MINLOC = L.OP_MAXLOC, L.OP_MINLOC
DT_F64_I64, DT_I64_I64 = 16, 17
F64_I64 = np.dtype([("value", np.float64), ("index", np.int64)])
I64_I64 = np.dtype([("value", np.int64), ("index", np.int64)])
NP_DTYPE = {DT_F64_I64: F64_I64, DT_I64_I64: I64_I64}

INT64_MIN, INT64_MAX = -2 ** 63, 2 ** 63 - 1
F64_MAX = np.finfo(np.float64).max
VALUES = {
    DT_F64_I64: np.array([1.0, 1.0 + 2.0 ** -40, 2.0, -0.0, 0.0, np.nan, np.inf, F64_MAX, -np.inf, -F64_MAX],
                         dtype=np.float64),
    DT_I64_I64: np.array([1 << 32, 0, 1 << 31, 1, -1, INT64_MIN, INT64_MAX], dtype=np.int64),
}
INDEXES = np.array([1 << 32, 0, 1 << 31, 1, -5, INT64_MIN, INT64_MAX], dtype=np.int64)


def new_stats():
    st = L.new_stats()
    st.update({"value_high": 0, "index_high": 0})
    return st


def _low32(a):
    return a.view(np.uint64) & np.uint64(0xFFFFFFFF)


def count_wide(op, dst, src, stats):
    """Fold steps that only the upper 32 bits decide: the values differ (and
    compare unequal) with equal low dwords, or the values tie and the indexes
    differ with equal low dwords."""
    dv, sv, di, si = dst["value"], src["value"], dst["index"], src["index"]
    with np.errstate(invalid="ignore"):
        differ = (dv < sv) | (dv > sv)
        tie = dv == sv
    stats["value_high"] += int((differ & (_low32(dv) == _low32(sv))).sum())
    stats["index_high"] += int((tie & (si != di) & (_low32(di) == _low32(si))).sum())


def take(op, dst, src, stats=None):
    """loc_ref.take, counting the wide statistics too when ``stats`` has them."""
    if stats is not None and "value_high" in stats:
        count_wide(op, dst, src, stats)
    return L.take(op, dst, src, stats)


def apply(op, dst, src, stats=None):
    out = np.array(dst, copy=True)
    m = take(op, dst, src, stats)
    out[m] = src[m]
    return out


def _wide(fold):
    """loc_ref's fold, its steps going through ``apply`` above: the order code
    stays loc_ref's (the one tied to the oracle); only the step it calls is
    swapped for the duration of the call, and that step is loc_ref's own rule
    plus two counters."""
    def run(xs, op, *args, **kw):
        saved = L.apply
        L.apply = apply
        try:
            return fold(xs, op, *args, **kw)
        finally:
            L.apply = saved
    run.__name__ = fold.__name__
    run.__doc__ = fold.__doc__
    return run


ring, tree, scan, reduce_scatter = _wide(L.ring), _wide(L.tree), _wide(L.scan), _wide(L.reduce_scatter)


def gen_inputs(seed, n, count, dtype):
    """n per-rank arrays of pairs drawn from VALUES[dtype] and INDEXES, so
    ranks collide in value and in index."""
    rng = np.random.default_rng(seed)
    vals = VALUES[dtype]
    xs = []
    for _ in range(n):
        x = np.empty(count, dtype=NP_DTYPE[dtype])
        x["value"] = vals[rng.integers(0, vals.size, count)]
        x["index"] = INDEXES[rng.integers(0, INDEXES.size, count)]
        xs.append(x)
    return xs


def assert_covers(stats, dtype, what=""):
    """The kinds of element a test of the wide pairs must contain, counted
    over every fold step of the expected data."""
    L.assert_covers_ties(stats, L.DT_F32_I32 if dtype == DT_F64_I64 else L.DT_I32_I32, what)
    assert stats["value_high"] > 0, ("no element decided by bits above bit 31 of the value", what)
    assert stats["index_high"] > 0, ("no element decided by bits above bit 31 of the index", what)


def _p(dtype, value, index):
    a = np.zeros(1, dtype=NP_DTYPE[dtype])
    a["value"], a["index"] = value, index
    return a


def rule_table(dtype):
    """[(case name, dst, src, MaxLoc result, MinLoc result)], each a 1-element
    pair array; "dst" / "src" as results name which operand is left there."""
    rows = [
        ("greater", (1, 5), (2, 9), "src", "dst"),
        ("less", (2, 5), (1, 1), "dst", "src"),
        ("equal value, lower index", (3, 5), (3, 4), "src", "src"),
        ("equal value, higher index", (3, 5), (3, 6), "dst", "dst"),
        ("equal value, equal index", (3, 5), (3, 5), "dst", "dst"),
        ("negative index is lower", (3, 0), (3, -1), "src", "src"),
        ("INT64_MIN index", (3, INT64_MAX), (3, INT64_MIN), "src", "src"),
        ("INT64_MAX index", (3, INT64_MIN), (3, INT64_MAX), "dst", "dst"),
        ("index high dword only, src higher", (3, 0), (3, 1 << 32), "dst", "dst"),
        ("index high dword only, src lower", (3, 1 << 32), (3, 0), "src", "src"),
        ("index low dword top bit, src higher", (3, 1), (3, 1 << 31), "dst", "dst"),
        ("index low dword top bit, src lower", (3, 1 << 31), (3, 1), "src", "src"),
        ("index beyond int32 against a negative one", (3, 1 << 40), (3, -1), "src", "src"),
    ]
    if dtype == DT_F64_I64:
        nan, inf, eps = np.float64("nan"), np.float64("inf"), 2.0 ** -40
        rows += [
            ("equal as float32, src greater", (1.0, 1), (1.0 + eps, 2), "src", "dst"),
            ("equal as float32, src less", (1.0 + eps, 1), (1.0, 0), "dst", "src"),
            ("equal as float32 is no tie", (1.0 + eps, 5), (1.0, 4), "dst", "src"),
            ("value high dword only", (1.0, 1), (2.0, 2), "src", "dst"),
            ("beyond float32 range", (1e300, 1), (1e301, 2), "src", "dst"),
            ("NaN in dst", (nan, 5), (1, 0), "dst", "dst"),
            ("NaN in src", (1, 5), (nan, 0), "dst", "dst"),
            ("both NaN", (nan, 5), (nan, 0), "dst", "dst"),
            ("+0 vs -0, lower index", (0.0, 5), (-0.0, 4), "src", "src"),
            ("-0 vs +0, higher index", (-0.0, 5), (0.0, 6), "dst", "dst"),
            ("+0 vs -0, equal index", (0.0, 5), (-0.0, 5), "dst", "dst"),
            ("-0 vs +0, equal index", (-0.0, 5), (0.0, 5), "dst", "dst"),
            ("+inf vs max", (inf, 1), (F64_MAX, 0), "dst", "src"),
            ("-inf vs lowest", (-inf, 1), (-F64_MAX, 0), "src", "dst"),
        ]
    else:
        rows += [
            ("value high dword only, src greater", (0, 1), (1 << 32, 2), "src", "dst"),
            ("value high dword only, src less", (1 << 32, 1), (0, 2), "dst", "src"),
            ("value low dword top bit, src greater", (1, 1), (1 << 31, 2), "src", "dst"),
            ("value low dword top bit, src less", (1 << 31, 1), (1, 2), "dst", "src"),
            ("INT64_MIN vs INT64_MAX value", (INT64_MIN, 1), (INT64_MAX, 2), "src", "dst"),
            ("INT64_MAX vs INT64_MIN value", (INT64_MAX, 1), (INT64_MIN, 0), "dst", "src"),
            ("INT64_MIN value tie", (INT64_MIN, 1), (INT64_MIN, 0), "src", "src"),
            ("-1 vs 0", (-1, 1), (0, 2), "src", "dst"),
            ("-1 vs 1 << 32", (-1, 1), (1 << 32, 2), "src", "dst"),
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
