"""CPU: MaxLoc / MinLoc over (value, index) pairs without a GPU — the numpy
restatement (tests/loc_ref.py) tied to the oracle's orders, the rule table
through include/rdc.h's host reducer, the C ABI's sizes and refusals, the
Python surface's argument checks, and the loc kernels' register budgets."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from tests import loc_ref as L
from tests.conftest import ROOT

INC = os.path.join(ROOT, "include")
SRC = os.path.join(ROOT, "tests", "cpp", "loc_reducer.cc")


# ------------------------------------------------------------- order check --
@pytest.mark.parametrize("n", [2, 3, 5, 8])
@pytest.mark.parametrize("op", [L.OP_MAX, L.OP_MIN])
def test_restated_orders_equal_the_oracle_with_plain_max_min(n, op):
    """The ring and tree folds of loc_ref, run with plain Max / Min on float32
    inputs holding NaN, +-0 and +-inf, give the oracle's bits: Max / Min keep a
    NaN or a zero's sign depending on the operand order, so this pins it."""
    rng = np.random.default_rng(4100 + 10 * n + op)
    special = np.array([np.nan, 0.0, -0.0, np.inf, -np.inf, 1.5, -2.0], dtype=np.float32)
    for count in (1, n - 1, n + 1, 257):
        xs = [special[rng.integers(0, special.size, count)] for _ in range(n)]
        want_ring = O.expected_allreduce(xs, O.DT_FLOAT32, op)
        want_tree = O.expected_tree(xs, O.DT_FLOAT32, op)
        assert L.ring(xs, op).tobytes() == want_ring.tobytes(), (n, op, count)
        assert L.tree(xs, op).tobytes() == want_tree.tobytes(), (n, op, count)
    assert np.isnan(want_ring).any() and (want_ring == 0).any()


def test_generated_inputs_cover_the_tie_kinds():
    for dtype in (L.DT_F32_I32, L.DT_I32_I32):
        for fold in (L.ring, L.tree, L.scan):
            st = L.new_stats()
            fold(L.gen_inputs(7, 3, 64, dtype), L.OP_MAXLOC, stats=st)
            L.assert_covers_ties(st, dtype, fold.__name__)


# -------------------------------------------------------------- rule check --
@pytest.fixture(scope="module")
def loc_reducer_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("loc") / "loc_reducer")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-I", INC, SRC, "-o", exe,
                           "-L", os.path.join(ROOT, "rdc_amd"), "-lrdc_amd",
                           "-Wl,-rpath," + os.path.join(ROOT, "rdc_amd")])
    return exe


@pytest.mark.parametrize("dtype", [L.DT_F32_I32, L.DT_I32_I32])
def test_rule_table_host_reducer_and_restatement(loc_reducer_exe, tmp_path, dtype):
    """op::Reducer<op::MaxLoc / MinLoc, ValueIndex<V>> and loc_ref.apply both
    give the table's results, byte for byte (NaN payloads and zero signs
    included: the rule moves whole elements)."""
    dst, src, want_max, want_min = L.table_arrays(dtype)
    names = [row[0] for row in L.rule_table(dtype)]
    for need in ("greater", "less", "equal value, lower index", "equal value, higher index",
                 "equal value, equal index"):
        assert need in names
    assert any("NaN" in s for s in names) == (dtype == L.DT_F32_I32)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(dst.tobytes() + src.tobytes())
    for opname, op, want in (("maxloc", L.OP_MAXLOC, want_max), ("minloc", L.OP_MINLOC, want_min)):
        assert L.apply(op, dst, src).tobytes() == want.tobytes(), opname
        subprocess.check_call([loc_reducer_exe, opname, "f32" if dtype == L.DT_F32_I32 else "i32", fin, fout])
        got = np.fromfile(fout, dtype=L.NP_DTYPE[dtype])
        for k, name in enumerate(names):
            assert got[k].tobytes() == want[k].tobytes(), (opname, name, got[k], want[k])


@pytest.mark.parametrize("bad", [1, 2])
def test_mismatched_op_and_element_type_do_not_compile(tmp_path, bad):
    """Allreduce<op::Sum, ValueIndex<float>> (1) and Allreduce<op::MaxLoc, float> (2)."""
    p = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-I", INC, "-DBAD=%d" % bad, SRC],
                       capture_output=True, text=True)
    assert p.returncode != 0
    assert "rdc::ValueIndex<V> elements" in p.stderr, p.stderr[-2000:]


# --------------------------------------------------------------------- ABI --
def test_pair_dtypes_are_eight_bytes_in_the_plan_entries():
    from rdc_amd._lib import _LIB
    for dtype in (12, 13):
        a, b = (ctypes.c_uint64 * 5)(), (ctypes.c_uint64 * 5)()
        assert _LIB.RdcPlanHbmBytes(3, 1001, dtype, 2, a) == 0, _LIB.RdcGetLastError()
        assert _LIB.RdcPlanHbmBytes(3, 1001, 4, 2, b) == 0
        assert list(a) == list(b) and a[0] > 0
        assert _LIB.RdcPlanScanBytes(3, 1, 1001, dtype, a) == 0, _LIB.RdcGetLastError()
        assert _LIB.RdcPlanScanBytes(3, 1, 1001, 4, b) == 0
        assert list(a) == list(b) and a[0] > 0
    assert _LIB.RdcPlanScanBytes(3, 1, 1001, 14, a) != 0


def valid(dtype, op):
    if dtype in (12, 13) or op in (4, 5):
        return dtype in (12, 13) and op in (4, 5)
    return not (op == 3 and dtype in (6, 7, 10, 11))


def test_refusal_matrix_of_dtypes_and_ops():
    """Every op 0..5 against every dtype 0..13 through RdcPlanScan and
    RdcPlanReduceTo: MAXLOC / MINLOC go with the pair dtypes only and the pair
    dtypes with them only; a refusal on that ground names the dtype and the op."""
    from rdc_amd._lib import _LIB
    npieces = ctypes.c_int()
    nvalid = 0
    for dtype in range(14):
        for op in range(6):
            rcs = [_LIB.RdcPlanScan(3, 1, 1001, dtype, op, 0, 0, 0, None, 0, ctypes.byref(npieces)),
                   _LIB.RdcPlanReduceTo(3, 1, 0, 1001, dtype, op, 0, 0, 0, None, 0, ctypes.byref(npieces))]
            err = _LIB.RdcGetLastError().decode()
            if valid(dtype, op):
                assert rcs == [0, 0], (dtype, op, err)
                nvalid += 1
                continue
            assert rcs[0] != 0 and rcs[1] != 0, (dtype, op)
            if dtype in (12, 13) or op in (4, 5):
                assert "(dtype, op) = (%d, %d)" % (dtype, op) in err and "MAXLOC" in err, (dtype, op, err)
    assert nvalid == 12 * 4 - 4 + 4
    # unknown codes: as before
    assert _LIB.RdcPlanScan(3, 1, 1001, 99, 0, 0, 0, 0, None, 0, ctypes.byref(npieces)) != 0
    assert b"bad dtype 99" in _LIB.RdcGetLastError()
    assert _LIB.RdcPlanScan(3, 1, 1001, 12, 6, 0, 0, 0, None, 0, ctypes.byref(npieces)) != 0
    assert b"bad op 6" in _LIB.RdcGetLastError()


def test_world_of_one_still_refuses_a_bad_pair():
    """RdcAllreduce validates before its world-size-1 return: no GPU needed."""
    from rdc_amd._lib import _LIB
    x = np.zeros(4, dtype=np.float32)
    assert _LIB.RdcReduce(None, None, 0, 6, 4, None) != 0
    assert b"(dtype, op) = (6, 4)" in _LIB.RdcGetLastError()
    assert _LIB.RdcReduce(None, None, 0, 12, 2, None) != 0
    assert b"(dtype, op) = (12, 2)" in _LIB.RdcGetLastError()
    assert _LIB.RdcFill(None, 0, 12, 1, 0, None) != 0
    assert b"pair dtype 12" in _LIB.RdcGetLastError()
    del x


# ---------------------------------------------------------- Python surface --
def test_python_constants_and_structured_dtypes():
    import rdc_amd
    assert int(rdc_amd.Op.MAXLOC) == 4 and int(rdc_amd.Op.MINLOC) == 5
    for dt, code, vkind in ((rdc_amd.F32_I32, 12, "f"), (rdc_amd.I32_I32, 13, "i")):
        assert rdc_amd.DTYPE_ENUM__[dt] == code
        assert dt.itemsize == 8 and dt.names == ("value", "index")
        assert dt.fields["value"][1] == 0 and dt.fields["index"][1] == 4
        assert dt.fields["value"][0].kind == vkind and dt.fields["value"][0].itemsize == 4
        assert dt.fields["index"][0] == np.dtype(np.int32)
    assert rdc_amd.F32_I32 == L.F32_I32 and rdc_amd.I32_I32 == L.I32_I32


def test_tensor_arguments_are_checked_before_the_library():
    """Comm methods take pairs as int32 [..., 2] with MAXLOC / MINLOC only;
    everything else is a TypeError raised before any library call (the handle
    here is null: a call would fail differently)."""
    torch = pytest.importorskip("torch")
    import rdc_amd
    c = rdc_amd.Comm()
    ok = torch.zeros(5, 2, dtype=torch.int32)
    calls = [lambda t, op, **kw: c.allreduce(t, op, **kw),
             lambda t, op, **kw: c.reduce_scatter(t, op, **kw),
             lambda t, op, **kw: c.reduce(t, op, 0, **kw),
             lambda t, op, **kw: c.scan(t, op, **kw),
             lambda t, op, **kw: c.allreduce_coalesced([t], op, **kw)]
    for call in calls:
        for op in (rdc_amd.Op.MAXLOC, rdc_amd.Op.MINLOC):
            for bad in (torch.zeros(5, 2, dtype=torch.float32), torch.zeros(5, 2, dtype=torch.int64),
                        torch.zeros(5, 3, dtype=torch.int32), torch.zeros(10, dtype=torch.int32),
                        torch.zeros((), dtype=torch.int32)):
                with pytest.raises(TypeError):
                    call(bad, op)
            with pytest.raises(TypeError):
                call(ok, op, value="float64")
            with pytest.raises(ValueError):  # a host tensor gets as far as the device check, not further
                call(ok, op, value="int32")
        with pytest.raises(TypeError):
            call(ok, rdc_amd.Op.SUM, value="float32")


def test_pack_and_unpack_pairs():
    torch = pytest.importorskip("torch")
    import rdc_amd
    v = torch.tensor([[1.5, -0.0], [float("nan"), 2.0]], dtype=torch.float32)
    i = torch.tensor([[3, -1], [0, 7]], dtype=torch.int64)
    p = rdc_amd.pack_pairs(v, i)
    assert p.dtype == torch.int32 and tuple(p.shape) == (2, 2, 2) and p.is_contiguous()
    as_np = p.numpy().reshape(-1, 2).copy().view(L.F32_I32).reshape(-1)
    assert as_np["value"].tobytes() == v.numpy().tobytes() and list(as_np["index"]) == [3, -1, 0, 7]
    v2, i2 = rdc_amd.unpack_pairs(p)
    assert v2.numpy().tobytes() == v.numpy().tobytes() and i2.tolist() == [[3, -1], [0, 7]]
    vi = torch.tensor([5, -2 ** 31], dtype=torch.int32)
    v3, i3 = rdc_amd.unpack_pairs(rdc_amd.pack_pairs(vi, torch.tensor([1, 2])), value="int32")
    assert v3.tolist() == [5, -2 ** 31] and i3.tolist() == [1, 2]
    with pytest.raises(TypeError):
        rdc_amd.pack_pairs(v.double(), i)
    with pytest.raises(TypeError):
        rdc_amd.unpack_pairs(p.float())


# --------------------------------------------------------- kernel resources --
FAMILIES = ["k_reduce", "k_mesh", "k_ring", "k_oneshot", "k_tree", "k_direct", "k_rscatter", "k_rooted", "k_scan",
            "k_svc"]


@pytest.fixture(scope="module")
def loc_kernels():
    from tests.test_kernel_resources import LIB, READELF, kernel_metadata
    if not os.path.exists(LIB):
        pytest.skip("librdc_amd.so not built")
    if not os.path.exists(READELF):
        pytest.skip("llvm-readelf not available")
    return {k: v for k, v in kernel_metadata(LIB).items() if "pair_f32_t" in k or "pair_i32_t" in k}


@pytest.mark.parametrize("family", FAMILIES)
def test_loc_kernels_present_without_scratch_below_256_vgprs(loc_kernels, family):
    """Every family is instantiated for MaxLoc / MinLoc (template arguments
    Li4 / Li5) x both pair types, has no private segment and stays below 256
    VGPRs.

    k_svc<OP, T, 16, 256, true> (the opt-in host exchange at more than 8 ranks,
    one resident 256-thread block) is compiled for two waves per SIMD for the
    pair types (rdc_kernels_impl.h SvcWaves): 245 VGPRs, where the compiler
    left to itself takes 306, as it does for every other element type."""
    found = {k: v for k, v in loc_kernels.items() if re.search(r"\d+%sI" % family, k)}
    for op in (4, 5):
        for t in ("pair_f32_t", "pair_i32_t"):
            assert any("ILi%dENS_10%s" % (op, t) in k for k in found), (family, op, t, sorted(found))
    assert not {k: v for k, v in found.items() if v[0] != 0}
    assert not {k: v for k, v in found.items() if v[1] >= 256}
