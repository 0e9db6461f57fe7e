"""The float32-accumulated Sum of float16 / bfloat16 buffers without a GPU: the
numpy restatement of its rule (tests/acc32_ref.py) on hand-checked rows, its
agreement with the oracle's ordinary Sum at two ranks, the conditions its input
generator and its order table must meet for the GPU tests to mean anything, the
C ABI's refusals at a world size of 1, the Python keyword and the C++ header.
"""
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from tests import acc32_ref as A
from tests import ops_ref
from tests.conftest import ROOT
from tests.test_capi import run_py

BF, F16 = O.DT_BFLOAT16, O.DT_FLOAT16


def differ(a, b):
    return a.view(np.uint16) != b.view(np.uint16)


def test_hand_checked_rows():
    """bf16 256 + 1 + 1 + 1: the float32 sum 259 is a tie between 258 and 260
    and goes to the even one, 260; per hop 256 + 1 = 257 rounds back to 256
    three times.  f16 60000 + 60000 - 60000: 120000 is a float32, so the rule
    gives 60000 (exact in f16: 59968 + 32 = 60000, ulp 32); per hop the first
    add overflows to inf."""
    def rows(n, seq, dtype):
        """one element per rank's chunk; chunk c meets seq[0] on rank c-1, seq[1] on rank c-2, ..."""
        f = np.zeros((n, n), dtype=np.float32)
        for c, (b, e) in enumerate(O.split(n, n)):
            assert e - b == 1
            for j, v in enumerate(seq):
                f[(c - 1 - j) % n, b] = v
        return [A.from_f32(f[q], dtype) for q in range(n)]

    xs = rows(4, (256.0, 1.0, 1.0, 1.0), BF)
    assert (A.widen(A.allreduce(xs, BF), BF) == 260.0).all()
    assert (A.widen(A.per_hop(xs, BF), BF) == 256.0).all()
    xs = rows(3, (60000.0, 60000.0, -60000.0), F16)
    assert (A.allreduce(xs, F16) == np.float16(60000.0)).all()
    with np.errstate(all="ignore"):
        assert np.isinf(A.per_hop(xs, F16)).all()


@pytest.mark.parametrize("dtype", A.DTYPES)
def test_two_ranks_are_the_ordinary_sum(dtype):
    """One binary32 add of two 16-bit values, rounded once, is their correctly
    rounded 16-bit sum: the oracle's ring Sum bit for bit, on random values,
    the specials row and every finite-overflow neighbourhood it holds."""
    from tests.gpu_util import rand_input, same_bits
    rng = np.random.default_rng(1201 + dtype)
    cases = [A.gen_inputs(1202 + dtype, 2, 4099, dtype), A.specials(2, dtype),
             [rand_input(rng, 4099, dtype) for _ in range(2)]]
    for xs in cases:
        ring = [np.array(x, copy=True) for x in xs]
        O.allreduce_ring(ring, dtype, O.OP_SUM)
        got = A.allreduce(xs, dtype)
        assert same_bits(got, ring[0], dtype) and same_bits(got, ring[1], dtype)
        # and no NaN hides a difference in the finite cases
        nan = ops_ref.is_nan(got, dtype)
        assert got[~nan].tobytes() == ring[0][~nan].tobytes()


@pytest.mark.parametrize("n", [3, 4, 8, 12])
@pytest.mark.parametrize("dtype", A.DTYPES)
def test_generator_tells_the_rule_from_the_per_hop_sum(dtype, n):
    """A kernel that silently ran the ordinary Sum must not pass: on the
    generator's data the rule differs from the per-hop ring Sum in at least 2 %
    of the elements, and the expected data hold no NaN and no inf (same_bits
    treats any two NaNs as equal)."""
    xs = A.gen_inputs(1300 + n, n, 4099, dtype)
    want = A.allreduce(xs, dtype)
    ops_ref.assert_finite(want, dtype, (dtype, n))
    frac = differ(want, A.per_hop(xs, dtype)).mean()
    print("dtype %d n %d: %.1f %% of elements differ from the per-hop Sum" % (dtype, n, 100 * frac))
    assert frac >= 0.02, frac


@pytest.mark.parametrize("n", [3, 4, 5, 8, 12])
@pytest.mark.parametrize("dtype", A.DTYPES)
def test_order_table_shows_the_fold_order(dtype, n):
    """Random data almost never show the order after the final rounding, the
    crafted cancellation rows do: in EVERY Split chunk the ring-order rule
    differs in at least one element from the ascending-rank fold and from every
    other chunk's order.  One exception is arithmetic, not a gap: where a wrong
    order is the chunk's own but for its first two ranks swapped (at n = 3,
    chunk 2 folds x[1], x[0], x[2] and ascending is x[0], x[1], x[2]) the two
    are the same sum, because the first add commutes — that chunk is told from
    the other chunks' orders instead.  The expected values are finite."""
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
                assert differ(want, A.allreduce_in_order(xs, dtype, order))[b:e].any(), (dtype, n, count, c, order)
            assert told >= n - 2 and told >= 1, (dtype, n, c, told)


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


def test_world_size_one_and_argument_errors():
    out = run_py(r'''
import ctypes, numpy as np, rdc_amd as r
from rdc_amd._lib import _LIB
buf = np.arange(16, dtype=np.float16)
keep = buf.copy()
p = buf.ctypes.data_as(ctypes.c_void_p)
odd = ctypes.c_void_p(buf.ctypes.data + 1)
assert _LIB.RdcAllreduceAcc32(p, 7, 10) != 0 and b"RdcInit" in _LIB.RdcGetLastError()
r.init([])
assert r.get_world_size() == 1
comm = r.get_comm("main")
entries = [
    ("RdcAllreduceAcc32", lambda q, n, dt: _LIB.RdcAllreduceAcc32(q, n, dt)),
    ("RdcReduceScatterAcc32", lambda q, n, dt: _LIB.RdcReduceScatterAcc32(q, n, dt)),
    ("RdcReduceToAcc32", lambda q, n, dt: _LIB.RdcReduceToAcc32(q, n, dt, 0)),
    ("RdcAllreduceAcc32On", lambda q, n, dt: _LIB.RdcAllreduceAcc32On(comm.handle, q, n, dt)),
    ("RdcReduceScatterAcc32On", lambda q, n, dt: _LIB.RdcReduceScatterAcc32On(comm.handle, q, n, dt)),
    ("RdcReduceToAcc32On", lambda q, n, dt: _LIB.RdcReduceToAcc32On(comm.handle, q, n, dt, 0)),
    ("RdcCommAllreduceAcc32", lambda q, n, dt: _LIB.RdcCommAllreduceAcc32(comm.handle, q, n, dt, None)),
    ("RdcCommReduceScatterAcc32", lambda q, n, dt: _LIB.RdcCommReduceScatterAcc32(comm.handle, q, n, dt, None)),
    ("RdcCommReduceToAcc32", lambda q, n, dt: _LIB.RdcCommReduceToAcc32(comm.handle, q, n, dt, 0, None)),
]
for name, call in entries:
    for dt in list(range(14)) + [16, 17, 99, -1]:
        if dt in (10, 11):
            assert call(p, 7, dt) == 0, (name, dt, _LIB.RdcGetLastError())
            assert call(p, 0, dt) == 0 and call(None, 0, dt) == 0, (name, dt)
            assert call(odd, 7, dt) != 0 and b"aligned" in _LIB.RdcGetLastError(), (name, dt)
        else:
            assert call(p, 7, dt) != 0, (name, dt)
            want = ("rdc: float32-accumulated Sum needs float16 or bfloat16, got dtype %d" % dt).encode()
            assert _LIB.RdcGetLastError() == want, (name, dt, _LIB.RdcGetLastError())
for root in (1, -1):
    assert _LIB.RdcReduceToAcc32(p, 7, 10, root) != 0 and b"root" in _LIB.RdcGetLastError()
    assert _LIB.RdcReduceToAcc32On(comm.handle, p, 7, 11, root) != 0 and b"root" in _LIB.RdcGetLastError()
    assert _LIB.RdcCommReduceToAcc32(comm.handle, p, 7, 11, root, None) != 0 and b"root" in _LIB.RdcGetLastError()
assert _LIB.RdcAllreduceAcc32On(None, p, 7, 10) != 0
assert _LIB.RdcCommReduceScatterAcc32(None, p, 7, 10, None) != 0
assert np.array_equal(buf, keep)

# the Python keyword
assert [int(o) for o in r.Op] == [0, 1, 2, 3, 4, 5, 8, 9, 10]
a = np.arange(6, dtype=np.float16).reshape(2, 3)
got = r.allreduce(a, r.Op.SUM, accumulate="float32")
assert got.dtype == np.float16 and np.array_equal(got, np.arange(6, dtype=np.float16))
assert r.reduce(a, r.Op.SUM, 0, accumulate="float32") is a
assert np.array_equal(r.reduce_scatter(a, r.Op.SUM, accumulate="float32"), a.ravel())
assert np.array_equal(comm.allreduce(a, r.Op.SUM, accumulate="float32"), a.ravel())
assert comm.reduce(a, r.Op.SUM, 0, accumulate="float32") is a
assert np.array_equal(comm.reduce_scatter(a, r.Op.SUM, accumulate="float32"), a.ravel())
bad = [
    lambda: r.allreduce(a, r.Op.MAX, accumulate="float32"),
    lambda: r.allreduce(a, r.Op.PROD, accumulate="float32"),
    lambda: r.allreduce(a.astype(np.float32), r.Op.SUM, accumulate="float32"),
    lambda: r.allreduce(a.astype(np.uint16), r.Op.SUM, accumulate="float32"),
    lambda: r.allreduce(a, r.Op.SUM, accumulate="float64"),
    lambda: r.allreduce([1.0, 2.0], r.Op.SUM, accumulate="float32"),
    lambda: r.reduce_scatter(a, r.Op.MIN, accumulate="float32"),
    lambda: r.reduce_scatter(a.astype(np.float64), r.Op.SUM, accumulate="float32"),
    lambda: r.reduce(a, r.Op.BITOR, 0, accumulate="float32"),
    lambda: r.reduce(a.astype(np.int32), r.Op.SUM, 0, accumulate="float32"),
    lambda: comm.allreduce(a, r.Op.MAX, accumulate="float32"),
    lambda: comm.allreduce(a, r.Op.SUM, algo="ring", accumulate="float32"),
    lambda: comm.reduce_scatter(a.astype(np.float32), r.Op.SUM, accumulate="float32"),
    lambda: comm.reduce(a, r.Op.MIN, 0, accumulate="float32"),
]
for k, f in enumerate(bad):
    try:
        f()
        raise SystemExit("bad call %d accepted" % k)
    except ValueError:
        pass
import torch
for t in (torch.zeros(4, dtype=torch.float32), torch.zeros(4, dtype=torch.int16)):
    for f in (lambda: r.allreduce(t, r.Op.SUM, accumulate="float32"),
              lambda: comm.reduce_scatter(t, r.Op.SUM, accumulate="float32"),
              lambda: comm.reduce(t, r.Op.SUM, 0, accumulate="float32")):
        try:
            f()
            raise SystemExit("bad tensor dtype accepted")
        except ValueError:
            pass
for dt in (torch.float16, torch.bfloat16):
    try:
        comm.allreduce(torch.zeros(4, dtype=dt), r.Op.MAX, accumulate="float32")
        raise SystemExit("Op.MAX accepted")
    except ValueError:
        pass
try:
    r.reduce(a, r.Op.SUM, 1, accumulate="float32")
    raise SystemExit("root 1 of 1 accepted")
except r.RdcError as e:
    assert "root" in str(e)
r.finalize()
print("OK")
''')
    assert "OK" in out


def test_cpp_acc32_compiles_and_runs_at_world_one():
    src = os.path.join(ROOT, "tests", "cpp", "acc32.cc")
    exe = os.path.join("/tmp", "rdc_acc32_%d" % os.getpid())
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
                           "-L", os.path.join(ROOT, "rdc_amd"), "-lrdc_amd",
                           "-Wl,-rpath," + os.path.join(ROOT, "rdc_amd")])
    try:
        p = subprocess.run([exe, "7", "0"], env=dict(os.environ, RDC_WORLD_SIZE="1"), capture_output=True, text=True,
                           timeout=60)
    finally:
        os.unlink(exe)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "acc32 OK (world 1, N 7, root 0)" in p.stdout


def test_cpp_header_refuses_other_element_types(tmp_path):
    """AllreduceAcc32<float> does not compile: only rdc::Float16 / rdc::BFloat16 have an Acc32Type."""
    src = tmp_path / "bad.cc"
    src.write_text('#include "rdc.h"\nvoid f(float* p) { rdc::AllreduceAcc32(p, 4); }\n')
    p = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert p.returncode != 0 and "Acc32Type" in p.stderr
