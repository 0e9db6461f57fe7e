"""Reduce-scatter without a GPU: the chunk map (RdcPlanSplit), the launches of
the scratch schedule (RdcPlanReduceScatter), the byte model
(RdcPlanReduceScatterBytes), the ABI's argument checks and world-size-1
behaviour, the built kernels' resources and the C++ header.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from tests.conftest import ROOT
from tests.test_capi import run_py
from tests.test_kernel_resources import LIB, READELF, kernel_metadata
from tests.test_plan import WORDS, layout, plan


def split_range(count, n, rank):
    from rdc_amd._lib import _LIB
    lo, hi = ctypes.c_uint64(), ctypes.c_uint64()
    assert _LIB.RdcPlanSplit(count, n, rank, ctypes.byref(lo), ctypes.byref(hi)) == 0, _LIB.RdcGetLastError()
    return lo.value, hi.value


@pytest.mark.parametrize("n", range(1, 17))
def test_plan_split_is_the_oracles(n):
    import rdc_amd
    for count in (0, 1, n - 1, n, n + 1, 1001, (1 << 31) + 5):
        want = [tuple(int(x) for x in be) for be in O.split(count, n)]
        assert [split_range(count, n, r) for r in range(n)] == want, (n, count)
        assert [rdc_amd.split_range(count, n, r) for r in range(n)] == want


def test_plan_split_rejects_bad_arguments():
    from rdc_amd._lib import _LIB
    lo, hi = ctypes.c_uint64(), ctypes.c_uint64()
    for n, rank in ((0, 0), (17, 0), (4, 4), (4, -1)):
        assert _LIB.RdcPlanSplit(10, n, rank, ctypes.byref(lo), ctypes.byref(hi)) != 0
    assert _LIB.RdcPlanSplit(10, 2, 0, None, ctypes.byref(hi)) != 0


def rs_plan(n, count, dtype, scratch, tile=0, max_blocks=256):
    from rdc_amd._lib import _LIB
    npieces = ctypes.c_int()
    rc = _LIB.RdcPlanReduceScatter(n, count, dtype, scratch, tile, max_blocks, None, 0, ctypes.byref(npieces))
    assert rc == 0, _LIB.RdcGetLastError()
    k = npieces.value
    buf = (ctypes.c_uint64 * (WORDS * max(1, k)))()
    assert _LIB.RdcPlanReduceScatter(n, count, dtype, scratch, tile, max_blocks, buf, k, ctypes.byref(npieces)) == 0
    arr = np.frombuffer(buf, dtype=np.uint64).reshape(max(1, k), WORDS)[:k]
    return [dict(tile=int(row[0]), nb=(int(row[1]), int(row[2]), int(row[3])),
                 off=[int(x) for x in row[4:4 + n]], len=[int(x) for x in row[20:20 + n]],
                 mis=[int(x) for x in row[36:36 + n]], tiles=[int(x) for x in row[52:52 + n]]) for row in arr]


SCRATCH = 16 << 20


@pytest.mark.parametrize("n", [2, 3, 8])
@pytest.mark.parametrize("dt", [O.DT_INT8, O.DT_FLOAT32, O.DT_FLOAT64])
def test_plan_reduce_scatter_is_the_mesh_plan_without_a_gather_role(n, dt):
    esz = np.dtype(O.NP_DTYPE[dt]).itemsize
    slot = layout(n, SCRATCH)["slot"]
    big = (2 * slot // esz + 5) * n + 1      # every chunk needs three slots' worth of pieces
    for count in (1, 5, 4099, big):
        for max_blocks in (256, 24, 2, 1):
            pieces = rs_plan(n, count, dt, SCRATCH, max_blocks=max_blocks)
            mesh = plan(n, count, dt, SCRATCH, algo=2, max_blocks=max_blocks)
            assert len(pieces) == len(mesh) and (count != big or len(pieces) == 3)
            nxt = [b * esz for b, _ in O.split(count, n)]
            for p, q in zip(pieces, mesh):
                nb_s, nb_r, nb_g = p["nb"]
                assert nb_g == 0 and nb_s >= 1 and nb_r >= 1, p["nb"]
                assert nb_s + nb_r <= max(2, max_blocks)
                tmax = max(p["tiles"])
                assert nb_s <= (n - 1) * tmax and nb_r <= tmax    # no block without an item
                for key in ("tile", "off", "len", "mis", "tiles"):
                    assert p[key] == q[key], (n, count, key)
                for c in range(n):
                    if p["len"][c]:
                        assert p["off"][c] == nxt[c]
                        nxt[c] += p["len"][c]
            assert nxt == [e * esz for _, e in O.split(count, n)]     # each chunk covered exactly once


def test_plan_reduce_scatter_splits_the_grid_one_to_two():
    """Enough tiles for every block: the default 4 : 8 role split gives the
    scatter a third of the grid and the reduce role the rest."""
    (p,) = rs_plan(8, 1 << 28, O.DT_FLOAT32, 0, tile=64 << 10, max_blocks=240)
    assert p["nb"] == (80, 160, 0)


def test_plan_reduce_scatter_empty_and_world1():
    assert rs_plan(4, 0, O.DT_FLOAT32, 0) == []
    assert rs_plan(1, 100, O.DT_FLOAT32, 0) == []


def model(fn, n, count, dtype, algo):
    from rdc_amd._lib import _LIB
    out = (ctypes.c_uint64 * 5)()
    assert getattr(_LIB, fn)(n, count, dtype, algo, out) == 0, _LIB.RdcGetLastError()
    return dict(zip(("read_max", "write_max", "read_sum", "write_sum", "egress_max"), [int(x) for x in out]))


@pytest.mark.parametrize("n", [2, 3, 8])
def test_reduce_scatter_byte_model_closed_forms(n):
    count, dt, esz = 1000003, O.DT_FLOAT32, 4
    assert count % n
    lens = [(e - b) * esz for b, e in O.split(count, n)]
    S = count * esz
    # mesh: the scatter loads every other chunk and stores it remotely; the
    # fold loads n x chunk r and stores chunk r
    m = model("RdcPlanReduceScatterBytes", n, count, dt, 2)
    rd = [S - l + n * l for l in lens]
    wr = [S - l + l for l in lens]
    assert m == dict(read_max=max(rd), write_max=max(wr), read_sum=sum(rd), write_sum=sum(wr),
                     egress_max=max(S - l for l in lens))
    # direct: n x chunk r loaded, chunk r stored; the peers load the rest of this rank's buffer
    d = model("RdcPlanReduceScatterBytes", n, count, dt, 6)
    assert d == dict(read_max=n * max(lens), write_max=max(lens), read_sum=n * S, write_sum=S,
                     egress_max=max(S - l for l in lens))
    full = model("RdcPlanHbmBytes", n, count, dt, 6)
    assert d["read_max"] + d["write_max"] < full["read_max"] + full["write_max"]
    from rdc_amd._lib import _LIB
    out = (ctypes.c_uint64 * 5)()
    for algo in (0, 1, 3, 4, 5):
        assert _LIB.RdcPlanReduceScatterBytes(n, count, dt, algo, out) != 0


def test_world_size_one_and_argument_errors():
    out = run_py(r'''
import ctypes, numpy as np, rdc_amd as r
from rdc_amd._lib import _LIB
buf = np.arange(7, dtype=np.float32)
p = buf.ctypes.data_as(ctypes.c_void_p)
assert _LIB.RdcReduceScatter(p, 7, 6, 2) != 0 and b"RdcInit" in _LIB.RdcGetLastError()
r.init([])
assert r.get_world_size() == 1
assert _LIB.RdcReduceScatter(p, 7, 6, 2) == 0 and np.array_equal(buf, np.arange(7, dtype=np.float32))
assert _LIB.RdcReduceScatter(p, 0, 6, 2) == 0
assert _LIB.RdcReduceScatter(p, 7, 6, 3) != 0 and b"BITOR" in _LIB.RdcGetLastError()
assert _LIB.RdcReduceScatter(p, 7, 99, 2) != 0 and b"dtype" in _LIB.RdcGetLastError()
assert _LIB.RdcReduceScatterOn(None, p, 7, 6, 2) != 0
a = np.arange(6, dtype=np.int32).reshape(2, 3)
v = r.reduce_scatter(a, r.Op.MAX)
assert v.shape == (6,) and np.shares_memory(v, a) and np.array_equal(a.ravel(), np.arange(6))
assert r.split_range(6, 1, 0) == (0, 6)
# the schedules a reduce-scatter does not have are refused by name, before the communicator is looked at
for algo in (1, 3, 4, 5, 7, -1):
    assert _LIB.RdcCommReduceScatter(None, p, 7, 6, 2, algo, None) != 0
    assert ("algo %d" % algo).encode() in _LIB.RdcGetLastError(), _LIB.RdcGetLastError()
assert _LIB.RdcCommReduceScatter(None, p, 7, 6, 2, 2, None) != 0
assert b"algo" not in _LIB.RdcGetLastError()
r.finalize()
print("OK")
''')
    assert "OK" in out


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(LIB):
        pytest.skip("librdc_amd.so not built")
    if not os.path.exists(READELF):
        pytest.skip("llvm-readelf not available")
    return kernel_metadata(LIB)


@pytest.mark.parametrize("family", ["k_rscatterI", "k_rscatter_directI"])
def test_reduce_scatter_kernels_resources(kernels, family):
    """4 ops x 10 element types (BITOR: integers only) x 2 widths: no scratch,
    two waves per SIMD (below 256 VGPRs), like the allreduce's kernels."""
    fam = {k: v for k, v in kernels.items() if family in k}
    assert len(fam) >= 40, len(fam)
    assert not {k: v for k, v in fam.items() if v[0] != 0}
    assert not {k: v for k, v in fam.items() if v[1] >= 256}


def test_cpp_reduce_scatter_compiles_and_runs_at_world_one():
    src = os.path.join(ROOT, "tests", "cpp", "reduce_scatter.cc")
    exe = os.path.join("/tmp", "rdc_reduce_scatter_%d" % os.getpid())
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
                           "-L", os.path.join(ROOT, "rdc_amd"), "-lrdc_amd",
                           "-Wl,-rpath," + os.path.join(ROOT, "rdc_amd")])
    try:
        p = subprocess.run([exe, "7"], env=dict(os.environ, RDC_WORLD_SIZE="1"), capture_output=True, text=True,
                           timeout=60)
    finally:
        os.unlink(exe)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "reduce-scatter OK (world 1, N 7)" in p.stdout
