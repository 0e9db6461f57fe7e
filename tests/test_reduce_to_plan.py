"""The rooted reduce (ReduceTo) without a GPU: the launches of its schedule
(RdcPlanReduceTo), the byte model (RdcPlanReduceToBytes), the ABI's argument
checks and world-size-1 behaviour, the built kernels' resources and the C++
header.
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

SCRATCH = 16 << 20
DT_OF_ESZ = {1: O.DT_INT8, 2: O.DT_FLOAT16, 4: O.DT_FLOAT32, 8: O.DT_FLOAT64}


def rt_plan(n, rank, root, count, dtype, scratch=SCRATCH, tile=0, max_blocks=256, op=O.OP_SUM):
    from rdc_amd._lib import _LIB
    npieces = ctypes.c_int()
    rc = _LIB.RdcPlanReduceTo(n, rank, root, count, dtype, op, scratch, tile, max_blocks, None, 0,
                              ctypes.byref(npieces))
    assert rc == 0, _LIB.RdcGetLastError()
    k = npieces.value
    buf = (ctypes.c_uint64 * (WORDS * max(1, k)))()
    assert _LIB.RdcPlanReduceTo(n, rank, root, count, dtype, op, scratch, tile, max_blocks, buf, k,
                                ctypes.byref(npieces)) == 0
    arr = np.frombuffer(buf, dtype=np.uint64).reshape(max(1, k), WORDS)[:k]
    return [dict(tile=int(row[0]), nb=(int(row[1]), int(row[2]), int(row[3])),
                 off=[int(x) for x in row[4:4 + n]], len=[int(x) for x in row[20:20 + n]],
                 mis=[int(x) for x in row[36:36 + n]], tiles=[int(x) for x in row[52:52 + n]]) for row in arr]


def roots_of(n):
    return sorted({0, n // 2, n - 1})


@pytest.mark.parametrize("esz", [1, 2, 4, 8])
@pytest.mark.parametrize("n", [2, 3, 4, 5, 6, 7, 8, 16])
def test_plan_reduce_to_cuts_like_the_mesh_on_every_rank_and_root(n, esz):
    """The pieces are the mesh allreduce's whatever the rank and the root; only
    the roles differ.  The grid bound: a rank that runs k roles needs k blocks,
    so the grid is at most max(max_blocks, k) — k = 3 on the root, 2 elsewhere
    (max_blocks = 2 cannot hold the root's three roles; the reduce-scatter's
    plan has the same floor of one block per role)."""
    dt = DT_OF_ESZ[esz]
    for count in (1, n - 1, 7, 1001, 4099, (1 << 22) + 3):
        for max_blocks in (256, 2, 3, 5):
            mesh = plan(n, count, dt, SCRATCH, algo=2, max_blocks=max_blocks)
            assert mesh
            for root in roots_of(n):
                for rank in range(n):
                    pieces = rt_plan(n, rank, root, count, dt, max_blocks=max_blocks)
                    assert len(pieces) == len(mesh)
                    for p, q in zip(pieces, mesh):
                        for key in ("tile", "off", "len", "mis", "tiles"):
                            assert p[key] == q[key], (n, count, rank, root, key)
                        nb_s, nb_r, nb_g = p["nb"]
                        tmax = max(p["tiles"])
                        assert tmax >= 1
                        assert (nb_g == 0) == (rank != root), (rank, root, p["nb"])
                        # every role with items has a block, none has more blocks than items
                        assert 1 <= nb_s <= (n - 1) * tmax and 1 <= nb_r <= tmax, p["nb"]
                        if rank == root:
                            assert 1 <= nb_g <= (n - 1) * tmax, p["nb"]
                        roles = 3 if rank == root else 2
                        assert nb_s + nb_r + nb_g <= max(max_blocks, roles), (max_blocks, p["nb"])


@pytest.mark.parametrize("n", [2, 3, 8])
def test_plan_reduce_to_multi_piece_tiles_each_chunk_exactly(n):
    dt, esz = O.DT_FLOAT32, 4
    slot = layout(n, SCRATCH)["slot"]
    count = (2 * slot // esz + 5) * n + 1      # every chunk needs three slots' worth of pieces
    for rank, root in ((0, 0), (n - 1, 0), (0, n - 1)):
        pieces = rt_plan(n, rank, root, count, dt)
        assert len(pieces) == 3
        nxt = [b * esz for b, _ in O.split(count, n)]
        for p in pieces:
            for c in range(n):
                assert p["len"][c] <= slot
                if p["len"][c]:
                    assert p["off"][c] == nxt[c]
                    nxt[c] += p["len"][c]
                assert p["tiles"][c] == -(-p["len"][c] // p["tile"])
        assert nxt == [e * esz for _, e in O.split(count, n)]


def test_plan_reduce_to_empty_and_world1():
    assert rt_plan(4, 1, 2, 0, O.DT_FLOAT32) == []
    assert rt_plan(1, 0, 0, 100, O.DT_FLOAT32) == []


def rt_bytes(n, rank, root, count, dtype):
    from rdc_amd._lib import _LIB
    out = (ctypes.c_uint64 * 5)()
    assert _LIB.RdcPlanReduceToBytes(n, rank, root, count, dtype, out) == 0, _LIB.RdcGetLastError()
    return dict(zip(("read_max", "write_max", "read_sum", "write_sum", "egress_max"), [int(x) for x in out]))


@pytest.mark.parametrize("n", [2, 3, 8, 16])
def test_reduce_to_byte_model_closed_forms(n):
    from rdc_amd._lib import _LIB
    dt, esz = O.DT_FLOAT32, 4
    for count in (n, 1001, 1000003):
        lens = [int(e - b) * esz for b, e in O.split(count, n)]
        S = count * esz
        for root in roots_of(n):
            rd, wr, eg = [], [], []
            for r, own in enumerate(lens):
                others = S - own
                # scatter: the other chunks loaded and stored remotely; fold: n copies of the own chunk loaded
                rd.append(others + n * own + (others if r == root else 0))   # root: + its AG slots
                # the result: remote off the root; on the root local, plus the gathered chunks
                wr.append(others + own + (others if r == root else 0))
                eg.append(others + (0 if r == root else own))
                assert rt_bytes(n, r, root, count, dt) == dict(read_max=rd[r], write_max=wr[r], read_sum=rd[r],
                                                               write_sum=wr[r], egress_max=eg[r]), (n, root, r)
            total = rt_bytes(n, -1, root, count, dt)
            assert total == dict(read_max=max(rd), write_max=max(wr), read_sum=sum(rd), write_sum=sum(wr),
                                 egress_max=max(eg))
            full = (ctypes.c_uint64 * 5)()
            assert _LIB.RdcPlanHbmBytes(n, count, dt, 2, full) == 0
            assert sum(wr) < int(full[3]), (n, count, root, sum(wr), int(full[3]))
            assert sum(rd) < int(full[2])


def test_plan_reduce_to_refusals():
    from rdc_amd._lib import _LIB
    k = ctypes.c_int()
    out = (ctypes.c_uint64 * 5)()
    for n, rank, root in ((4, 0, 4), (4, 0, -1), (2, 0, 2), (16, 3, 16), (1, 0, 1)):
        assert _LIB.RdcPlanReduceTo(n, rank, root, 100, O.DT_FLOAT32, O.OP_SUM, 0, 0, 0, None, 0, ctypes.byref(k)) != 0
        assert b"root" in _LIB.RdcGetLastError()
        assert _LIB.RdcPlanReduceToBytes(n, rank, root, 100, O.DT_FLOAT32, out) != 0
        assert b"root" in _LIB.RdcGetLastError()
    for n, rank in ((4, 4), (4, -1), (0, 0), (17, 0)):
        assert _LIB.RdcPlanReduceTo(n, rank, 0, 100, O.DT_FLOAT32, O.OP_SUM, 0, 0, 0, None, 0, ctypes.byref(k)) != 0
    assert _LIB.RdcPlanReduceTo(4, 0, 0, 100, 99, O.OP_SUM, 0, 0, 0, None, 0, ctypes.byref(k)) != 0
    assert b"dtype" in _LIB.RdcGetLastError()
    assert _LIB.RdcPlanReduceTo(4, 0, 0, 100, O.DT_FLOAT32, O.OP_BITOR, 0, 0, 0, None, 0, ctypes.byref(k)) != 0
    assert b"BITOR" in _LIB.RdcGetLastError()
    assert _LIB.RdcPlanReduceTo(4, 0, 0, 100, O.DT_FLOAT32, 7, 0, 0, 0, None, 0, ctypes.byref(k)) != 0
    assert _LIB.RdcPlanReduceToBytes(4, 0, 0, 100, 99, out) != 0


def test_world_size_one_and_argument_errors():
    out = run_py(r'''
import ctypes, numpy as np, rdc_amd as r
from rdc_amd._lib import _LIB
assert "reduce" in r.__all__
buf = np.arange(7, dtype=np.float32)
p = buf.ctypes.data_as(ctypes.c_void_p)
assert _LIB.RdcReduceTo(p, 7, 6, 2, 0) != 0 and b"RdcInit" in _LIB.RdcGetLastError()
r.init([])
assert r.get_world_size() == 1
assert _LIB.RdcReduceTo(p, 7, 6, 2, 0) == 0 and np.array_equal(buf, np.arange(7, dtype=np.float32))
assert _LIB.RdcReduceTo(p, 0, 6, 2, 0) == 0
for root in (1, -1):
    assert _LIB.RdcReduceTo(p, 7, 6, 2, root) != 0 and b"root" in _LIB.RdcGetLastError()
assert _LIB.RdcReduceTo(p, 7, 6, 3, 0) != 0 and b"BITOR" in _LIB.RdcGetLastError()
assert _LIB.RdcReduceTo(p, 7, 99, 2, 0) != 0 and b"dtype" in _LIB.RdcGetLastError()
assert _LIB.RdcReduceToOn(None, p, 7, 6, 2, 0) != 0
assert _LIB.RdcCommReduceTo(None, p, 7, 6, 2, 0, None) != 0
a = np.arange(6, dtype=np.int32).reshape(2, 3)
assert r.reduce(a, r.Op.MAX, 0) is a and np.array_equal(a.ravel(), np.arange(6))
try:
    r.reduce(a, r.Op.MAX, 1)
    raise SystemExit("root 1 of 1 accepted")
except r.RdcError as e:
    assert "root" in str(e)
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


def test_rooted_kernels_resources(kernels):
    """4 ops x 10 element types (BITOR: integers only) x 2 widths: no scratch,
    two waves per SIMD (below 256 VGPRs), like the allreduce's kernels."""
    fam = {k: v for k, v in kernels.items() if "k_rootedI" in k}
    assert len(fam) >= 40, len(fam)
    assert not {k: v for k, v in fam.items() if v[0] != 0}
    assert not {k: v for k, v in fam.items() if v[1] >= 256}


def test_cpp_reduce_to_compiles_and_runs_at_world_one():
    src = os.path.join(ROOT, "tests", "cpp", "reduce_to.cc")
    exe = os.path.join("/tmp", "rdc_reduce_to_%d" % os.getpid())
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
                           "-L", os.path.join(ROOT, "rdc_amd"), "-lrdc_amd",
                           "-Wl,-rpath," + os.path.join(ROOT, "rdc_amd")])
    try:
        p = subprocess.run([exe, "7", "0"], env=dict(os.environ, RDC_WORLD_SIZE="1"), capture_output=True, text=True,
                           timeout=60)
    finally:
        os.unlink(exe)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "reduce-to OK (world 1, N 7, root 0)" in p.stdout
