"""Avg, the mean across ranks of float32 / float64 / float16 / bfloat16 buffers,
without a GPU: the numpy restatement of its rule (tests/avg_ref.py) on
hand-checked rows, the conditions its input generator and its order table must
meet for the GPU tests to mean anything, the C ABI's refusals at a world size
of 1, the Python keyword and the C++ header.
"""
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from tests import acc32_ref
from tests import avg_ref as A
from tests import ops_ref
from tests.conftest import ROOT
from tests.test_capi import run_py

F32, F64, F16, BF = A.F32, A.F64, A.F16, A.BF


def differ(a, b, dtype):
    return A.bits(a, dtype) != A.bits(b, dtype)


def test_hand_checked_rows():
    """Four ranks of float16 40000.0: the float32 sum 160000 divided by 4 is
    40000.0, exact in float16, while the per-hop Sum passes 65504 at the second
    hop and the float32-accumulated Sum rounds 160000 to inf.
    float32 at n = 3: every rank holds 5/3 rounded (0x3FD55555); the sum is 5
    exactly (each add is exact here), 5 / 3 rounds back to 0x3FD55555, while
    5 * fl(1/3) = 5 * 0x3EAAAAAB rounds to 0x3FD55556."""
    xs = [np.full(8, 40000.0, dtype=np.float16) for _ in range(4)]
    assert (A.allreduce(xs, F16) == np.float16(40000.0)).all()
    with np.errstate(all="ignore"):
        assert np.isinf(ops_ref.ring(xs, ops_ref.OP_SUM, F16)).all()
        assert np.isinf(acc32_ref.allreduce(xs, F16)).all()
    third = np.array([0x3FD55555], dtype=np.uint32).view(np.float32)
    xs = [np.repeat(third, 6) for _ in range(3)]
    s = ops_ref.ring(xs, ops_ref.OP_SUM, F32)
    assert (s == np.float32(5.0)).all()
    assert (A.bits(A.allreduce(xs, F32), F32) == 0x3FD55555).all()
    assert (A.bits(A.sum_times_reciprocal(xs, F32), F32) == 0x3FD55556).all()


@pytest.mark.parametrize("n", [3, 5, 6, 7, 12])
@pytest.mark.parametrize("dtype", A.DTYPES)
def test_generator_tells_the_rule_from_the_two_pass_mean(dtype, n):
    """A kernel that divided after rounding the sum to 16 bits, or multiplied
    by a rounded 1 / n, must not pass.  On the generator's data the rule
    differs in at least 1 % of the elements from "sum, round, then divide" (16-bit
    types) and from ``s * (1 / n)`` (float32 / float64, where the composition
    rounds at the same place); the expected data hold no NaN and no inf."""
    xs = A.gen_inputs(1300 + n, n, 4099, dtype)
    want = A.allreduce(xs, dtype)
    ops_ref.assert_finite(want, dtype, (dtype, n))
    other = A.sum_times_reciprocal(xs, dtype) if dtype in A.WIDE else A.sum_round_then_divide(xs, dtype)
    frac = differ(want, other, dtype).mean()
    print("dtype %d n %d: %.1f %% of elements differ" % (dtype, n, 100 * frac))
    assert frac >= 0.01, frac


@pytest.mark.parametrize("n", [2, 4, 8])
@pytest.mark.parametrize("dtype", A.WIDE)
def test_power_of_two_division_is_the_reciprocal_multiply(dtype, n):
    """At a power-of-two n the division and the multiplication are the same
    bits (an implementation may multiply there), subnormal results included."""
    xs = A.gen_inputs(1350 + n, n, 4099, dtype) + []
    xs[0][:8] = np.finfo(A.NP_WIDE[dtype]).tiny      # the mean of these goes subnormal
    for q in range(1, n):
        xs[q][:8] = 0
    assert differ(A.allreduce(xs, dtype), A.sum_times_reciprocal(xs, dtype), dtype).sum() == 0


@pytest.mark.parametrize("n", [3, 4, 5, 8, 12])
@pytest.mark.parametrize("dtype", A.DTYPES)
def test_order_table_shows_the_fold_order(dtype, n):
    """The crafted cancellation rows still show the fold order after the
    division: in EVERY Split chunk the rule differs in at least one element
    from the ascending-rank fold and from every other chunk's order.  One
    exception is arithmetic, not a gap (tests/test_acc32_plan.py): where a
    wrong order is the chunk's own but for its first two ranks swapped (n = 3,
    chunk 2 folds x[1], x[0], x[2]; ascending is x[0], x[1], x[2]) the two are
    the same sum, because the first add commutes — that chunk is told from the
    other chunks' orders instead.  The expected values are finite."""
    for count in (None, 1001):   # 1001: the table of the multi-process runs
        xs = A.order_table(n, dtype, count=count)
        want = A.allreduce(xs, dtype)
        ops_ref.assert_finite(want, dtype, "order table")
        asc = list(range(n))
        for c, (b, e) in enumerate(O.split(xs[0].size, n)):
            mine = A.chunk_order(c, n)
            wrong = [asc] + [A.chunk_order(o, n) for o in range(n) if o != c]
            told = 0
            for order in wrong:
                if A.same_sum(order, mine):
                    continue
                told += 1
                assert differ(want, A.allreduce_in_order(xs, dtype, order), dtype)[b:e].any(), \
                    (dtype, n, count, c, order)
            assert told >= n - 2 and told >= 1, (dtype, n, c, told)


@pytest.mark.parametrize("dtype", A.DTYPES)
def test_specials_hold_what_they_claim(dtype):
    """The specials rows produce a NaN (inf - inf), an inf, a signed zero and a
    subnormal mean, and — float16 — the finite mean of an overflowing Sum."""
    for n in (2, 3):
        xs = A.specials(n, dtype)
        full = A.allreduce(xs, dtype)
        assert ops_ref.is_nan(full, dtype).any() and ops_ref.is_inf(full, dtype).any()
        if dtype == F16:
            assert (full[-(n + 1):] == np.float16(40000.0)).all()
            with np.errstate(all="ignore"):
                assert np.isinf(acc32_ref.allreduce(xs, dtype)[-(n + 1):]).all()


@pytest.mark.parametrize("dtype", A.DTYPES)
def test_reduce_scatter_and_reduce_to_forms(dtype):
    xs = A.gen_inputs(1400, 3, 1001, dtype)
    full = A.allreduce(xs, dtype)
    rs = A.reduce_scatter(xs, dtype)
    for r, (b, e) in enumerate(O.split(1001, 3)):
        assert rs[r][b:e].tobytes() == full[b:e].tobytes()
        assert rs[r][:b].tobytes() == xs[r][:b].tobytes() and rs[r][e:].tobytes() == xs[r][e:].tobytes()
    rt = A.reduce_to(xs, dtype, 1)
    assert rt[1].tobytes() == full.tobytes() and rt[0].tobytes() == xs[0].tobytes() and rt[2].tobytes() == xs[2].tobytes()


def test_declared_symbols_are_exported():
    import re
    import rdc_amd  # noqa: F401
    from rdc_amd._lib import _LIB
    decl = re.findall(r"^int (Rdc\w*Avg\w*)\(", open(os.path.join(ROOT, "include", "rdc_amd.h")).read(), re.M)
    assert sorted(decl) == sorted(["RdcAllreduceAvg", "RdcAllreduceAvgOn", "RdcReduceScatterAvg",
                                   "RdcReduceScatterAvgOn", "RdcReduceToAvg", "RdcReduceToAvgOn",
                                   "RdcCommAllreduceAvg", "RdcCommReduceScatterAvg", "RdcCommReduceToAvg"])
    for name in decl:
        assert getattr(_LIB, name) is not None, name


def test_world_size_one_and_argument_errors():
    out = run_py(r'''
import ctypes, numpy as np, rdc_amd as r
from rdc_amd._lib import _LIB
buf = np.arange(16, dtype=np.float64)
keep = buf.copy()
p = buf.ctypes.data_as(ctypes.c_void_p)
odd = ctypes.c_void_p(buf.ctypes.data + 1)
assert _LIB.RdcAllreduceAvg(p, 7, 6) != 0 and b"RdcInit" in _LIB.RdcGetLastError()
r.init([])
assert r.get_world_size() == 1
comm = r.get_comm("main")
entries = [
    ("RdcAllreduceAvg", lambda q, n, dt: _LIB.RdcAllreduceAvg(q, n, dt)),
    ("RdcReduceScatterAvg", lambda q, n, dt: _LIB.RdcReduceScatterAvg(q, n, dt)),
    ("RdcReduceToAvg", lambda q, n, dt: _LIB.RdcReduceToAvg(q, n, dt, 0)),
    ("RdcAllreduceAvgOn", lambda q, n, dt: _LIB.RdcAllreduceAvgOn(comm.handle, q, n, dt)),
    ("RdcReduceScatterAvgOn", lambda q, n, dt: _LIB.RdcReduceScatterAvgOn(comm.handle, q, n, dt)),
    ("RdcReduceToAvgOn", lambda q, n, dt: _LIB.RdcReduceToAvgOn(comm.handle, q, n, dt, 0)),
    ("RdcCommAllreduceAvg", lambda q, n, dt: _LIB.RdcCommAllreduceAvg(comm.handle, q, n, dt, None)),
    ("RdcCommReduceScatterAvg", lambda q, n, dt: _LIB.RdcCommReduceScatterAvg(comm.handle, q, n, dt, None)),
    ("RdcCommReduceToAvg", lambda q, n, dt: _LIB.RdcCommReduceToAvg(comm.handle, q, n, dt, 0, None)),
]
for name, call in entries:
    for dt in list(range(18)) + [99, -1]:
        if dt in (6, 7, 10, 11):
            assert call(p, 7, dt) == 0, (name, dt, _LIB.RdcGetLastError())
            assert call(p, 0, dt) == 0 and call(None, 0, dt) == 0, (name, dt)
            assert call(odd, 7, dt) != 0 and b"aligned" in _LIB.RdcGetLastError(), (name, dt)
        else:
            assert call(p, 7, dt) != 0, (name, dt)
            want = ("rdc: Avg takes float32, float64, float16 or bfloat16, got dtype %d" % dt).encode()
            assert _LIB.RdcGetLastError() == want, (name, dt, _LIB.RdcGetLastError())
for root in (1, -1):
    assert _LIB.RdcReduceToAvg(p, 7, 10, root) != 0 and b"root" in _LIB.RdcGetLastError()
    assert _LIB.RdcReduceToAvgOn(comm.handle, p, 7, 11, root) != 0 and b"root" in _LIB.RdcGetLastError()
    assert _LIB.RdcCommReduceToAvg(comm.handle, p, 7, 11, root, None) != 0 and b"root" in _LIB.RdcGetLastError()
assert _LIB.RdcAllreduceAvgOn(None, p, 7, 10) != 0
assert _LIB.RdcCommReduceScatterAvg(None, p, 7, 10, None) != 0
assert np.array_equal(buf, keep)

# the Python keyword: world size 1 leaves the data unchanged
assert [int(o) for o in r.Op] == [0, 1, 2, 3, 4, 5, 8, 9, 10]
import torch
for npd in (np.float32, np.float64, np.float16):
    a = np.arange(6, dtype=npd).reshape(2, 3)
    got = r.allreduce(a, r.Op.SUM, average=True)
    assert got.dtype == npd and np.array_equal(got, np.arange(6, dtype=npd))
    assert r.reduce(a, r.Op.SUM, 0, average=True) is a
    assert np.array_equal(r.reduce_scatter(a, r.Op.SUM, average=True), a.ravel())
    assert np.array_equal(comm.allreduce(a, r.Op.SUM, average=True), a.ravel())
    assert comm.reduce(a, r.Op.SUM, 0, average=True) is a
    assert np.array_equal(comm.reduce_scatter(a, r.Op.SUM, average=True), a.ravel())
    # average=False is the call as it was
    assert np.array_equal(r.allreduce(a, r.Op.SUM, average=False), a.ravel())
h = np.arange(6, dtype=np.float16)
w = np.arange(6, dtype=np.float32)
# 16-bit data: accumulate may be None or "float32"
assert np.array_equal(r.allreduce(h, r.Op.SUM, accumulate="float32", average=True), h)
assert np.array_equal(comm.reduce_scatter(h, r.Op.SUM, accumulate="float32", average=True), h)
bad = [
    lambda: r.allreduce(w, r.Op.MAX, average=True),
    lambda: r.allreduce(w, r.Op.PROD, average=True),
    lambda: r.allreduce(w.astype(np.int32), r.Op.SUM, average=True),
    lambda: r.allreduce(w.astype(np.uint16), r.Op.SUM, average=True),
    lambda: r.allreduce([1.0, 2.0], r.Op.SUM, average=True),
    lambda: r.allreduce(w, r.Op.SUM, accumulate="float32", average=True),
    lambda: r.allreduce(w.astype(np.float64), r.Op.SUM, accumulate="float32", average=True),
    lambda: r.allreduce(h, r.Op.SUM, accumulate="float64", average=True),
    lambda: r.allreduce(w, r.Op.SUM, accumulate="float32"),
    lambda: r.reduce_scatter(w, r.Op.MIN, average=True),
    lambda: r.reduce_scatter(w.astype(np.int64), r.Op.SUM, average=True),
    lambda: r.reduce(w, r.Op.BITOR, 0, average=True),
    lambda: r.reduce(w, r.Op.SUM, 0, accumulate="float32", average=True),
    lambda: comm.allreduce(w, r.Op.MAX, average=True),
    lambda: comm.allreduce(w, r.Op.SUM, algo="ring", average=True),
    lambda: comm.allreduce(w, r.Op.SUM, algo="oneshot", average=True),
    lambda: comm.reduce_scatter(w, r.Op.SUM, algo="direct", average=True),
    lambda: comm.reduce_scatter(w.astype(np.int8), r.Op.SUM, average=True),
    lambda: comm.reduce(w, r.Op.MIN, 0, average=True),
    lambda: comm.allreduce(w, r.Op.SUM, value="float32", average=True),
]
for k, f in enumerate(bad):
    try:
        f()
        raise SystemExit("bad call %d accepted" % k)
    except ValueError:
        pass
try:
    comm.allreduce(w, r.Op.SUM, algo="ring", average=True)
except ValueError as e:
    assert "average=True runs on the mesh only, got algo 'ring'" in str(e), e
for t in (torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int16)):
    for f in (lambda: r.allreduce(t, r.Op.SUM, average=True),
              lambda: comm.reduce_scatter(t, r.Op.SUM, average=True),
              lambda: comm.reduce(t, r.Op.SUM, 0, average=True)):
        try:
            f()
            raise SystemExit("bad tensor dtype accepted")
        except ValueError:
            pass
for dt in (torch.float32, torch.float64, torch.float16, torch.bfloat16):
    try:
        comm.allreduce(torch.zeros(4, dtype=dt), r.Op.MAX, average=True)
        raise SystemExit("Op.MAX accepted")
    except ValueError:
        pass
try:
    r.reduce(w, r.Op.SUM, 1, average=True)
    raise SystemExit("root 1 of 1 accepted")
except r.RdcError as e:
    assert "root" in str(e)
r.finalize()
print("OK")
''')
    assert "OK" in out


def test_cpp_avg_compiles_and_runs_at_world_one():
    src = os.path.join(ROOT, "tests", "cpp", "avg.cc")
    exe = os.path.join("/tmp", "rdc_avg_%d" % os.getpid())
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
                           "-L", os.path.join(ROOT, "rdc_amd"), "-lrdc_amd",
                           "-Wl,-rpath," + os.path.join(ROOT, "rdc_amd")])
    try:
        p = subprocess.run([exe, "7", "0"], env=dict(os.environ, RDC_WORLD_SIZE="1"), capture_output=True, text=True,
                           timeout=60)
    finally:
        os.unlink(exe)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "avg OK (world 1, N 7, root 0)" in p.stdout


def test_cpp_header_refuses_other_element_types(tmp_path):
    """AllreduceAvg<int> does not compile: only float, double, rdc::Float16 and
    rdc::BFloat16 have an AvgType (and the same source with float does compile)."""
    good = tmp_path / "good.cc"
    good.write_text('#include "rdc.h"\nvoid f(float* p) { rdc::AllreduceAvg(p, 4); rdc::ReduceToAvg(p, 4, 0); }\n')
    subprocess.check_call(["g++", "-std=c++11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(good)])
    src = tmp_path / "bad.cc"
    src.write_text('#include "rdc.h"\nvoid f(int* p) { rdc::AllreduceAvg(p, 4); }\n')
    p = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert p.returncode != 0 and "AvgType" in p.stderr
