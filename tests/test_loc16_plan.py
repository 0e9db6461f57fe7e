"""CPU: the 16-byte MaxLoc / MinLoc pairs — dtype 16 F64_I64 {double, int64}
and 17 I64_I64 {int64, int64} — without a GPU: the generator's coverage, the
rule table through include/rdc.h's host reducer, the C ABI's sizes and
refusals, the Python surface's argument checks and the kernels' register
budgets.  The fold orders are tests/loc_ref.py's (tests/test_loc_plan.py ties
them to the oracle)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import loc16_ref as W
from tests import loc_ref as L
from tests.conftest import ROOT
from tests.test_capi import run_py

INC = os.path.join(ROOT, "include")
SRC = os.path.join(ROOT, "tests", "cpp", "loc16_reducer.cc")
DTYPES = [W.DT_F64_I64, W.DT_I64_I64]
PAIRS = (12, 13, 16, 17)


# ------------------------------------------------------------ reference ----
def test_wide_folds_are_loc_refs_folds():
    """The folds of loc16_ref are loc_ref's, step for step: equal bytes on the
    wide pairs, and loc_ref's own statistics equal too."""
    for dtype in DTYPES:
        xs = W.gen_inputs(11, 3, 257, dtype)
        for op in (W.OP_MAXLOC, W.OP_MINLOC):
            a, b = L.new_stats(), W.new_stats()
            assert W.ring(xs, op, b).tobytes() == L.ring(xs, op, a).tobytes()
            assert W.tree(xs, op, b).tobytes() == L.tree(xs, op, a).tobytes()
            for x, y in zip(W.scan(xs, op, True, b), L.scan(xs, op, True, a)):
                assert x.tobytes() == y.tobytes()
            assert {k: b[k] for k in a} == a
    assert L.apply is not W.apply  # the swap inside a fold is undone


@pytest.mark.parametrize("dtype", DTYPES)
def test_generated_inputs_cover_what_a_narrow_shortcut_gets_wrong(dtype):
    """Count 64, n = 3: every fold's expected data holds an element decided by
    the index rule, a full tie, (f64) a NaN first operand, an element decided
    by the value's upper 32 bits and one decided by the index's."""
    vals, idx = W.VALUES[dtype], W.INDEXES
    for need in (1 << 32, 0, 1 << 31, 1, W.INT64_MIN, W.INT64_MAX):
        assert need in idx and (dtype == W.DT_F64_I64 or need in vals)
    assert (idx < 0).any() and (idx > 0).any()
    if dtype == W.DT_F64_I64:
        assert np.float32(1.0 + 2.0 ** -40) == np.float32(1.0) and 1.0 + 2.0 ** -40 in vals and 1.0 in vals
        assert np.isnan(vals).any() and np.signbit(vals[vals == 0]).any() and not np.signbit(vals[vals == 0]).all()
        for v in (np.inf, -np.inf, W.F64_MAX, -W.F64_MAX):
            assert v in vals
    for fold in (W.ring, W.tree, W.scan):
        st = W.new_stats()
        fold(W.gen_inputs(7, 3, 64, dtype), W.OP_MAXLOC, stats=st)
        W.assert_covers(st, dtype, fold.__name__)


# -------------------------------------------------------------- rule check --
@pytest.fixture(scope="module")
def reducer_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("loc16") / "loc16_reducer")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-I", INC, SRC, "-o", exe,
                           "-L", os.path.join(ROOT, "rdc_amd"), "-lrdc_amd",
                           "-Wl,-rpath," + os.path.join(ROOT, "rdc_amd")])
    return exe


@pytest.mark.parametrize("dtype", DTYPES)
def test_rule_table_host_reducer_and_restatement(reducer_exe, tmp_path, dtype):
    """op::Reducer<op::MaxLoc / MinLoc, ValueIndex<double / int64_t>> and
    loc16_ref.apply both give the table's results, byte for byte."""
    dst, src, want_max, want_min = W.table_arrays(dtype)
    assert dst.dtype.itemsize == 16
    names = [row[0] for row in W.rule_table(dtype)]
    for need in ("greater", "less", "equal value, lower index", "equal value, higher index",
                 "equal value, equal index", "index high dword only, src lower", "index low dword top bit, src lower"):
        assert need in names
    assert any("NaN" in s for s in names) == (dtype == W.DT_F64_I64)
    assert any("equal as float32" in s for s in names) == (dtype == W.DT_F64_I64)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(dst.tobytes() + src.tobytes())
    for opname, op, want in (("maxloc", W.OP_MAXLOC, want_max), ("minloc", W.OP_MINLOC, want_min)):
        assert W.apply(op, dst, src).tobytes() == want.tobytes(), opname
        subprocess.check_call([reducer_exe, opname, "f64" if dtype == W.DT_F64_I64 else "i64", fin, fout])
        got = np.fromfile(fout, dtype=W.NP_DTYPE[dtype])
        for k, name in enumerate(names):
            assert got[k].tobytes() == want[k].tobytes(), (opname, name, got[k], want[k])


@pytest.mark.parametrize("bad", [1, 2])
def test_mismatched_op_and_element_type_do_not_compile(bad):
    """Allreduce<op::Sum, ValueIndex<double>> (1) and Allreduce<op::MaxLoc, double> (2)."""
    p = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-I", INC, "-DBAD=%d" % bad, SRC],
                       capture_output=True, text=True)
    assert p.returncode != 0
    assert "rdc::ValueIndex<V> elements" in p.stderr, p.stderr[-2000:]


# --------------------------------------------------------------------- ABI --
@pytest.mark.parametrize("dtype", DTYPES)
def test_wide_pairs_are_sixteen_bytes_in_the_plan_entries(dtype):
    """The byte models of dtype 16 / 17 at count c are int64's at count 2 c.
    The allreduce's model follows utils::Split, which cuts in elements: at a
    count that n does not divide, the chunks of c pairs and of 2 c int64 end
    one int64 apart (1001 pairs over 3: 334 + 334 + 333 pairs against 668 +
    667 + 667 int64), so that model is compared at counts n divides, where the
    chunks are the same bytes; the scan's model has no chunks and is compared
    at odd counts too."""
    from rdc_amd._lib import _LIB
    a, b = (ctypes.c_uint64 * 5)(), (ctypes.c_uint64 * 5)()
    for count in (1002, 4098, 100002):
        assert count % 3 == 0
        assert _LIB.RdcPlanHbmBytes(3, count, dtype, 2, a) == 0, _LIB.RdcGetLastError()
        assert _LIB.RdcPlanHbmBytes(3, 2 * count, 4, 2, b) == 0
        assert list(a) == list(b) and a[0] > 0
    for count in (1001, 4096, 100003):
        assert _LIB.RdcPlanScanBytes(3, 1, count, dtype, a) == 0, _LIB.RdcGetLastError()
        assert _LIB.RdcPlanScanBytes(3, 1, 2 * count, 4, b) == 0
        assert list(a) == list(b) and a[0] > 0


def valid(dtype, op):
    if op in (6, 7):
        return False
    if dtype in PAIRS or op in (4, 5):
        return dtype in PAIRS and op in (4, 5)
    return not (op in (3, 9, 10) and dtype in (6, 7, 10, 11))


def test_refusal_matrix_of_dtypes_and_ops():
    """Ops 0..10 against the four pair dtypes and float32 through RdcPlanScan
    and RdcPlanReduceTo: MAXLOC / MINLOC go with the pair dtypes only and the
    pair dtypes with them only; a refusal on that ground names both.  Codes 14
    and 15 stay unassigned."""
    from rdc_amd._lib import _LIB
    npieces = ctypes.c_int()
    nvalid = 0
    for dtype in PAIRS + (6,):
        for op in range(11):
            rcs = [_LIB.RdcPlanScan(3, 1, 1001, dtype, op, 0, 0, 0, None, 0, ctypes.byref(npieces)),
                   _LIB.RdcPlanReduceTo(3, 1, 0, 1001, dtype, op, 0, 0, 0, None, 0, ctypes.byref(npieces))]
            err = _LIB.RdcGetLastError().decode()
            if valid(dtype, op):
                assert rcs == [0, 0], (dtype, op, err)
                nvalid += 1
                continue
            assert rcs[0] != 0 and rcs[1] != 0, (dtype, op)
            if op in (6, 7):
                assert "bad op %d" % op in err
            elif dtype in PAIRS or op in (4, 5):
                assert "(dtype, op) = (%d, %d)" % (dtype, op) in err and "MAXLOC" in err, (dtype, op, err)
    assert nvalid == 4 * 2 + 4  # float32: MAX, MIN, SUM, PROD
    for dtype in (14, 15, 18):
        for op in (0, 4):
            assert _LIB.RdcPlanScan(3, 1, 1001, dtype, op, 0, 0, 0, None, 0, ctypes.byref(npieces)) != 0
            assert b"bad dtype %d" % dtype in _LIB.RdcGetLastError()
        a = (ctypes.c_uint64 * 5)()
        assert _LIB.RdcPlanHbmBytes(3, 1001, dtype, 2, a) != 0


def test_world_of_one_refusals_need_no_gpu():
    """RdcReduce and RdcFill refuse as they do for dtype 12; RdcAllreduce at a
    world size of 1 refuses a wide pair buffer at base + 8 and takes it at base."""
    from rdc_amd._lib import _LIB
    for dtype in DTYPES:
        assert _LIB.RdcReduce(None, None, 0, dtype, 2, None) != 0
        assert b"(dtype, op) = (%d, 2)" % dtype in _LIB.RdcGetLastError()
        assert _LIB.RdcReduce(None, None, 0, 7, 4, None) != 0
        assert b"(dtype, op) = (7, 4)" in _LIB.RdcGetLastError()
        assert _LIB.RdcFill(None, 0, dtype, 1, 0, None) != 0
        assert b"pair dtype %d" % dtype in _LIB.RdcGetLastError()
    out = run_py(r'''
import ctypes, numpy as np, rdc_amd as r
from rdc_amd._lib import _LIB
r.init([])
assert r.get_world_size() == 1
raw = np.zeros(16 * 8 + 32, dtype=np.uint8)
base = raw.ctypes.data + (-raw.ctypes.data) % 16
for dtype in (16, 17):
    for op in (4, 5):
        assert _LIB.RdcAllreduce(ctypes.c_void_p(base), 8, dtype, op, None, None) == 0, _LIB.RdcGetLastError()
        assert _LIB.RdcAllreduce(ctypes.c_void_p(base + 8), 7, dtype, op, None, None) != 0
        assert b"buffer not aligned to its element size" in _LIB.RdcGetLastError()
    assert _LIB.RdcAllreduce(ctypes.c_void_p(base), 8, dtype, 2, None, None) != 0
    assert b"(dtype, op) = (%d, 2)" % dtype in _LIB.RdcGetLastError()
x = np.zeros(5, dtype=r.F64_I64)
x["value"], x["index"] = [1.5, np.nan, -0.0, 2.0, 1e300], [1 << 40, -1, 0, 7, -2 ** 63]
y = r.allreduce(x, r.Op.MAXLOC)
assert y.dtype == r.F64_I64 and y.tobytes() == x.tobytes()
print("OK")
''')
    assert "OK" in out


# ---------------------------------------------------------- Python surface --
def test_python_constants_and_structured_dtypes():
    import rdc_amd
    for dt, code, vkind in ((rdc_amd.F64_I64, 16, "f"), (rdc_amd.I64_I64, 17, "i")):
        assert rdc_amd.DTYPE_ENUM__[dt] == code
        assert dt.itemsize == 16 and dt.names == ("value", "index")
        assert dt.fields["value"][1] == 0 and dt.fields["index"][1] == 8
        assert dt.fields["value"][0].kind == vkind and dt.fields["value"][0].itemsize == 8
        assert dt.fields["index"][0] == np.dtype(np.int64)
    assert rdc_amd.F64_I64 == W.F64_I64 and rdc_amd.I64_I64 == W.I64_I64
    assert 14 not in rdc_amd.DTYPE_ENUM__.values() and 15 not in rdc_amd.DTYPE_ENUM__.values()
    for name in ("F64_I64", "I64_I64", "pack_pairs16", "unpack_pairs16"):
        assert name in rdc_amd.__all__


def test_tensor_arguments_are_checked_before_the_library():
    """Comm methods take the wide pairs as int64 [..., 2] with an explicit
    value="float64" | "int64" and MAXLOC / MINLOC only; everything else is a
    TypeError raised before any library call (the handle here is null)."""
    torch = pytest.importorskip("torch")
    import rdc_amd
    c = rdc_amd.Comm()
    ok = torch.zeros(5, 2, dtype=torch.int64)
    calls = [lambda t, op, **kw: c.allreduce(t, op, **kw),
             lambda t, op, **kw: c.reduce_scatter(t, op, **kw),
             lambda t, op, **kw: c.reduce(t, op, 0, **kw),
             lambda t, op, **kw: c.scan(t, op, **kw),
             lambda t, op, **kw: c.allreduce_coalesced([t], op, **kw)]
    for call in calls:
        for op in (rdc_amd.Op.MAXLOC, rdc_amd.Op.MINLOC):
            for value in ("float64", "int64"):
                for bad in (torch.zeros(5, 2, dtype=torch.float64), torch.zeros(5, 2, dtype=torch.int32),
                            torch.zeros(5, 3, dtype=torch.int64), torch.zeros(10, dtype=torch.int64),
                            torch.zeros((), dtype=torch.int64)):
                    with pytest.raises(TypeError):
                        call(bad, op, value=value)
                with pytest.raises(ValueError):  # a host tensor gets as far as the device check, not further
                    call(ok, op, value=value)
            with pytest.raises(TypeError):  # value= is required
                call(ok, op)
            for value in ("float32", "int32", "double", 16):
                with pytest.raises(TypeError):
                    call(ok, op, value=value)
        with pytest.raises(TypeError):
            call(ok, rdc_amd.Op.SUM, value="float64")


def test_pack_and_unpack_pairs16():
    torch = pytest.importorskip("torch")
    import rdc_amd
    v = torch.tensor([[1.0 + 2.0 ** -40, -0.0], [float("nan"), 1e300]], dtype=torch.float64)
    i = torch.tensor([[1 << 40, -1], [0, -2 ** 63]], dtype=torch.int64)
    p = rdc_amd.pack_pairs16(v, i)
    assert p.dtype == torch.int64 and tuple(p.shape) == (2, 2, 2) and p.is_contiguous()
    as_np = p.numpy().reshape(-1, 2).copy().view(W.F64_I64).reshape(-1)
    assert as_np["value"].tobytes() == v.numpy().tobytes() and list(as_np["index"]) == [1 << 40, -1, 0, -2 ** 63]
    v2, i2 = rdc_amd.unpack_pairs16(p, "float64")
    assert v2.numpy().tobytes() == v.numpy().tobytes() and i2.tolist() == i.tolist()
    vi = torch.tensor([1 << 32, -2 ** 63], dtype=torch.int64)
    v3, i3 = rdc_amd.unpack_pairs16(rdc_amd.pack_pairs16(vi, torch.tensor([1, 2], dtype=torch.int32)), value="int64")
    assert v3.tolist() == [1 << 32, -2 ** 63] and i3.tolist() == [1, 2] and i3.dtype == torch.int64
    for bad in (v.float(), vi.int()):
        with pytest.raises(TypeError):
            rdc_amd.pack_pairs16(bad, torch.zeros(bad.shape, dtype=torch.int64))
    with pytest.raises(ValueError):
        rdc_amd.pack_pairs16(v, i[0])
    for bad, value in ((p.int(), "int64"), (p[..., :1], "int64"), (p, "float32"), (p, None)):
        with pytest.raises(TypeError):
            rdc_amd.unpack_pairs16(bad, value)


# --------------------------------------------------------- kernel resources --
@pytest.fixture(scope="module")
def wide_kernels():
    from tests.test_kernel_resources import LIB, READELF, kernel_metadata
    if not os.path.exists(LIB):
        pytest.skip("librdc_amd.so not built")
    if not os.path.exists(READELF):
        pytest.skip("llvm-readelf not available")
    return {k: v for k, v in kernel_metadata(LIB).items() if "pair_f64_t" in k or "pair_i64_t" in k}


def test_wide_loc_kernels_present_without_scratch_below_256_vgprs(wide_kernels):
    """Every family of test_loc_plan.FAMILIES is instantiated for MaxLoc /
    MinLoc (template arguments Li4 / Li5) x both wide pair types, has no
    private segment and stays below 256 VGPRs (k_svc<OP, T, 16, 256, true>
    through SvcWaves, as for the 8-byte pairs)."""
    from tests.test_loc_plan import FAMILIES
    assert len(FAMILIES) == 10
    for family in FAMILIES:
        found = {k: v for k, v in wide_kernels.items() if re.search(r"\d+%sI" % family, k)}
        for op in (4, 5):
            for t in ("pair_f64_t", "pair_i64_t"):
                assert any("ILi%dENS_10%s" % (op, t) in k for k in found), (family, op, t, sorted(found))
    assert not {k: v for k, v in wide_kernels.items() if v[0] != 0}
    assert not {k: v for k, v in wide_kernels.items() if v[1] >= 256}
