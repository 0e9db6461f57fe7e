"""CPU: Prod / BitAND / BitXOR (ops 8 / 9 / 10) without a GPU — the numpy
restatement (tests/ops_ref.py) tied to the oracle's orders, the C ABI's
refusals, the Python constants, and include/rdc.h's host reducer."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from tests import ops_ref as R
from tests.conftest import ROOT

INC = os.path.join(ROOT, "include")
SRC = os.path.join(ROOT, "tests", "cpp", "op_prod_shim.cc")


# ------------------------------------------------------------- order check --
@pytest.mark.parametrize("n", [2, 3, 4, 5])
@pytest.mark.parametrize("op", [R.OP_SUM, R.OP_MAX])
def test_restated_orders_equal_the_oracle_with_sum_and_max(n, op):
    """ops_ref's ring and tree folds, run with Sum and Max, give the oracle's
    bits: a float Sum depends on the order as a float Prod does, and Max keeps
    a NaN or a zero's sign depending on the operand order."""
    rng = np.random.default_rng(7100 + 10 * n + op)
    differs = False
    for dtype in (O.DT_FLOAT32, O.DT_BFLOAT16, O.DT_INT8, O.DT_FLOAT64):
        for count in (1, n - 1, n + 1, 257):
            xs = R.gen_inputs(int(rng.integers(1 << 30)), n, count, dtype)
            if dtype == O.DT_FLOAT32 and count == 257:
                for x in xs:
                    x[:4] = np.array([np.nan, 0.0, -0.0, np.inf], dtype=np.float32)[rng.permutation(4)]
            want_ring = O.expected_allreduce(xs, dtype, op)
            want_tree = O.expected_tree(xs, dtype, op)
            assert R.ring(xs, op, dtype).tobytes() == want_ring.tobytes(), (n, op, dtype, count)
            assert R.tree(xs, op, dtype).tobytes() == want_tree.tobytes(), (n, op, dtype, count)
            differs |= want_ring.tobytes() != R.left_to_right(xs, op, dtype).tobytes()
    if n >= 3 and op == R.OP_SUM:
        assert differs  # the check can tell the ring order from a left-to-right fold


def test_generated_float_inputs_keep_products_finite_and_rounding():
    """gen_input's floats: magnitudes in [0.5, 2), both signs, and a product of
    8 is finite, normal and inexact (it differs from the float64 product)."""
    for dtype in (O.DT_FLOAT32, O.DT_FLOAT64, O.DT_FLOAT16, O.DT_BFLOAT16):
        xs = R.gen_inputs(5, 8, 4096, dtype)
        for x in xs:
            f = R.bf16_to_f32(x) if dtype == O.DT_BFLOAT16 else x
            assert (np.abs(f) >= 0.5).all() and (np.abs(f) < 2).all() and (f < 0).any() and (f > 0).any()
        got = R.ring(xs, R.OP_PROD, dtype)
        R.assert_finite(got, dtype)
        f = (R.bf16_to_f32(got) if dtype == O.DT_BFLOAT16 else got).astype(np.float64)
        assert (np.abs(f) >= 2.0 ** -8.5).all() and (np.abs(f) < 2.0 ** 8.5).all()
        if dtype != O.DT_FLOAT64:
            exact = np.prod([(R.bf16_to_f32(x) if dtype == O.DT_BFLOAT16 else x).astype(np.float64) for x in xs],
                            axis=0)
            assert (f != exact).mean() > 0.5


def test_restated_rules_by_hand():
    i8 = np.array([-128, -1, 127, 16, 3], dtype=np.int8)
    s8 = np.array([-1, -1, 127, 16, -5], dtype=np.int8)
    assert R.apply(R.OP_PROD, i8, s8).tolist() == [-128, 1, 1, 0, -15]
    assert R.apply(R.OP_BITAND, i8, s8).tolist() == [-128, -1, 127, 16, 3]
    assert R.apply(R.OP_BITXOR, i8, s8).tolist() == [127, 0, 0, 0, -8]
    # bf16: 1.5 * 1.5 = 2.25 (exact); (1 + 2^-7)^2 = 1 + 2^-6 + 2^-14 rounds down; the largest finite * 2 = inf
    b =np.array([0x3FC0, 0x3F81, 0x7F7F, 0x0001], dtype=np.uint16)
    got = R.apply(R.OP_PROD, b, np.array([0x3FC0, 0x3F81, 0x4000, 0x3F00], dtype=np.uint16), O.DT_BFLOAT16)
    assert got.tolist() == [0x4010, 0x3F82, 0x7F80, 0x0000]  # the last: half the least subnormal ties to even (0)


# --------------------------------------------------------------------- ABI --
def valid(dtype, op):
    if dtype in (12, 13):
        return False
    return op == R.OP_PROD or dtype not in O.FLOAT_DTYPES


def test_refusal_matrix_of_the_new_ops():
    """Ops 8, 9, 10 against every dtype 0..13 through RdcPlanScan and
    RdcPlanReduceTo: 12 + 8 + 8 valid combinations; a float dtype with BITAND /
    BITXOR is refused naming the operator, a pair dtype naming (dtype, op)."""
    from rdc_amd._lib import _LIB
    npieces = ctypes.c_int()

    def plan(dtype, op):
        rcs = [_LIB.RdcPlanScan(3, 1, 1001, dtype, op, 0, 0, 0, None, 0, ctypes.byref(npieces)),
               _LIB.RdcPlanReduceTo(3, 1, 0, 1001, dtype, op, 0, 0, 0, None, 0, ctypes.byref(npieces))]
        return rcs, _LIB.RdcGetLastError().decode()
    nvalid = 0
    for dtype in range(14):
        for op in R.NEW_OPS:
            rcs, err = plan(dtype, op)
            if valid(dtype, op):
                assert rcs == [0, 0], (dtype, op, err)
                assert (dtype, op) in R.NEW_VALID
                nvalid += 1
                continue
            assert rcs[0] != 0 and rcs[1] != 0, (dtype, op)
            if dtype in (12, 13):
                assert "unsupported (dtype, op) = (%d, %d)" % (dtype, op) in err, (dtype, op, err)
            else:
                assert {R.OP_BITAND: "BITAND", R.OP_BITXOR: "BITXOR"}[op] + " needs an integer dtype" in err, err
    assert nvalid == 12 + 8 + 8 == len(R.NEW_VALID)
    # 6 and 7 stay unassigned (older tests use each as the unknown operator), 11 is past the end; the older
    # operators are as they were
    for dtype, op in ((12, 6), (2, 6), (6, 7), (12, 7), (2, 11), (12, 11), (2, -1)):
        rcs, err = plan(dtype, op)
        assert rcs[0] != 0 and rcs[1] != 0 and "bad op %d" % op in err, (dtype, op, err)
    assert plan(2, 3)[0] == [0, 0] and plan(6, 2)[0] == [0, 0] and plan(12, 4)[0] == [0, 0]
    assert "BITOR needs an integer dtype" in plan(6, 3)[1]


def test_world_of_one_refusals_need_no_gpu():
    """RdcReduce looks its kernel up before it looks at its buffers: a (dtype,
    op) without one is refused by name, as a float with BITOR always was; a
    valid one with no elements succeeds without a launch."""
    from rdc_amd._lib import _LIB
    for dtype, op in ((6, 9), (7, 10), (11, 10), (10, 9), (12, 8), (13, 10), (2, 6), (6, 7), (2, 11), (6, 3)):
        assert _LIB.RdcReduce(None, None, 0, dtype, op, None) != 0, (dtype, op)
        err = _LIB.RdcGetLastError()
        assert b"unsupported (dtype, op) = (%d, %d)" % (dtype, op) in err, (dtype, op, err)
    for dtype, op in R.NEW_VALID:
        assert _LIB.RdcReduce(None, None, 0, dtype, op, None) == 0, (dtype, op, _LIB.RdcGetLastError())


# ---------------------------------------------------------- Python surface --
def test_python_constants():
    import rdc_amd
    Op = rdc_amd.Op
    assert (int(Op.PROD), int(Op.BITAND), int(Op.BITXOR)) == (8, 9, 10)
    assert [int(o) for o in (Op.MAX, Op.MIN, Op.SUM, Op.BITOR, Op.MAXLOC, Op.MINLOC)] == [0, 1, 2, 3, 4, 5]
    assert sorted(int(o) for o in Op) == [0, 1, 2, 3, 4, 5, 8, 9, 10]
    assert Op(8) is Op.PROD and Op(9) is Op.BITAND and Op(10) is Op.BITXOR
    for unassigned in (6, 7):
        with pytest.raises(ValueError):
            Op(unassigned)


# ------------------------------------------------------------ host reducer --
@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ops") / "op_prod_shim")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-I", INC, SRC, "-o", exe,
                           "-L", os.path.join(ROOT, "rdc_amd"), "-lrdc_amd",
                           "-Wl,-rpath," + os.path.join(ROOT, "rdc_amd")])
    return exe


def host_cases(tname):
    rng = np.random.default_rng(77)
    npd = {"i8": np.int8, "i32": np.int32, "u64": np.uint64, "f32": np.float32, "f64": np.float64}[tname]
    if tname == "i8":
        g = np.arange(-128, 128, dtype=np.int16).astype(np.int8)
        return np.repeat(g, 256), np.tile(g, 256)  # every pair of bytes
    if tname == "i32":
        d = rng.integers(-2 ** 31, 2 ** 31 - 1, 512, dtype=np.int32, endpoint=True)
        s = rng.integers(-2 ** 31, 2 ** 31 - 1, 512, dtype=np.int32, endpoint=True)
        d[:6] = [2 ** 31 - 1, -2 ** 31, -2 ** 31, 65536, 46341, -1]   # each overflows int32 (the last: -INT_MIN)
        s[:6] = [2 ** 31 - 1, -1, -2 ** 31, 65536, 46341, -2 ** 31]
        return d, s
    if tname == "u64":
        d = rng.integers(0, 2 ** 64 - 1, 512, dtype=np.uint64, endpoint=True)
        s = rng.integers(0, 2 ** 64 - 1, 512, dtype=np.uint64, endpoint=True)
        d[:2], s[:2] = [2 ** 64 - 1, 2 ** 32], [2 ** 64 - 1, 2 ** 32]
        return d, s
    fi = np.finfo(npd)
    d = (rng.standard_normal(512) * 10.0 ** rng.integers(-30, 30, 512)).astype(npd)
    s = (rng.standard_normal(512) * 10.0 ** rng.integers(-30, 30, 512)).astype(npd)
    sp_d = [fi.tiny, fi.max, -0.0, np.inf, np.nan, 1 + fi.eps, fi.smallest_subnormal, 3.0]
    sp_s = [0.5, 2.0, 5.0, 0.0, 1.0, 1 + fi.eps, 0.5, fi.tiny / 4]
    d[:8], s[:8] = np.array(sp_d, dtype=npd), np.array(sp_s, dtype=npd)
    return d, s


@pytest.mark.parametrize("tname", ["i8", "i32", "u64", "f32", "f64"])
def test_host_reducer_folds_the_restated_bits(shim, tmp_path, tname):
    """op::Reducer<op::Prod | op::BitAND | op::BitXOR, T> (include/rdc.h)
    against ops_ref.apply: every int8 pair, int32 with overflowing products
    (the host multiplies through the unsigned type), uint64, float and double
    with subnormal results, overflow, -0, inf * 0 and NaN."""
    d, s = host_cases(tname)
    fin = str(tmp_path / "in.bin")
    with open(fin, "wb") as f:
        f.write(d.tobytes() + s.tobytes())
    u = R.UNSIGNED[d.dtype.itemsize]
    for opname, op in (("prod", R.OP_PROD), ("bitand", R.OP_BITAND), ("bitxor", R.OP_BITXOR)):
        if d.dtype.kind == "f" and op != R.OP_PROD:
            continue
        out = subprocess.check_output([shim, opname, tname, fin], text=True)
        got = np.array([int(line, 16) for line in out.split()], dtype=np.uint64).astype(u).view(d.dtype)
        want = R.apply(op, d, s)
        assert got.size == d.size
        if d.dtype.kind == "f":
            assert np.isnan(want).sum() == 2 and np.isinf(want).any() and (want == 0).any()
            nan = np.isnan(want)
            assert np.array_equal(np.isnan(got), nan)
            assert got[~nan].tobytes() == want[~nan].tobytes(), (opname, tname)
        else:
            assert got.tobytes() == want.tobytes(), (opname, tname)
    if tname == "i32":
        assert R.apply(R.OP_PROD, d[:6], s[:6]).tolist() == [1, -2 ** 31, 0, 0, -2147479015, -2 ** 31]


@pytest.mark.parametrize("bad", [1, 2, 3])
def test_float_bit_operators_and_pairs_do_not_compile(bad):
    """op::BitAND on float (1), op::BitXOR on double (2), Allreduce<op::Prod,
    ValueIndex<float>> (3)."""
    p = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-I", INC, "-DBAD=%d" % bad, SRC],
                       capture_output=True, text=True)
    assert p.returncode != 0
    assert "error" in p.stderr
    ok = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-I", INC, SRC], capture_output=True, text=True)
    assert ok.returncode == 0, ok.stderr[-2000:]
