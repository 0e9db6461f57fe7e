"""GPU: MaxLoc / MinLoc over (value, index) pairs on the device path, byte for
byte against the numpy restatement tests/loc_ref.py (ring, tree and scan
orders; tests/test_loc_plan.py ties those to the oracle).

Inputs come from loc_ref.gen_inputs: five values (NaN, -0, +0 among the f32
ones, INT32_MIN among the i32 ones) and four indexes, so ranks collide in value
and in index; every test that claims ties first asserts on the expected data
that an element decided by the index rule, a full tie and (f32) a NaN first
operand are present.

* single-process groups of 2 and 3 (RdcCommInitAll on GPU 0), created once;
* multi-process: 4 and 8 processes on GPU 0, tests/mp_loc_worker.py;
* C++ through the launcher: tests/cpp/loc.cc.
"""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import loc_ref as L
from tests.conftest import ROOT
from tests.test_gpu_reduce_scatter import launch_counters, make_group, run_mp

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

WORKER = os.path.join(ROOT, "tests", "mp_loc_worker.py")
DTYPES = [L.DT_F32_I32, L.DT_I32_I32]
OPS = [L.OP_MAXLOC, L.OP_MINLOC]
ALGOS = {"ring": 1, "mesh": 2, "mesh_pull": 5, "oneshot": 3, "tree": 4, "auto": 0}
TILE = 8192  # pairs in one 64 KiB tile
GUARD = 4096
SENTINEL = 0xA5


class Groups(object):
    """The groups of 3 and of 2, each created at its first use and in that
    order, as in the other GPU test modules: every rank's stream needs a
    hardware queue of its own, and a group made while no other
    group's streams are still unused gets them."""

    def __init__(self):
        self.made = {}

    def get(self, n):
        if n not in self.made:
            comms = make_group(n, {3: 24 << 20, 2: 16 << 20}[n])
            # the default threshold: every size takes the ring order unless algo 4 asks for the tree's
            assert comms[0].get_param("rdc_reduce_ring_mincount") < 8
            self.made[n] = comms
        return self.made[n]

    def items(self):
        for n in (3, 2):
            yield n, self.get(n)

    def __getitem__(self, n):
        return self.get(n)


@pytest.fixture(scope="module")
def groups():
    g = Groups()
    yield g
    for comms in g.made.values():
        for c in comms:
            c.destroy()


def ar_counts(n):
    return sorted({1, n - 1, n, n + 1, 2, 3, 4097, TILE - 1, TILE, TILE + 1, 200003})


@functools.lru_cache(maxsize=None)
def case(n, dtype, op, count):
    """(inputs, ring result, tree result, fold statistics of both), computed once per shape."""
    xs = L.gen_inputs(9000 + 100 * n + dtype, n, count, dtype)
    st = L.new_stats()
    ring, tree = L.ring(xs, op, st), L.tree(xs, op, st)
    for a in xs + [ring, tree]:
        a.setflags(write=False)
    return xs, ring, tree, st


def guarded(x, pad):
    """uint8 ROCm tensor: GUARD sentinel bytes, pad more, x's bytes, GUARD sentinel bytes
    (torch allocations are 256-B aligned, so pad is the buffer's address mod 16)."""
    raw = np.frombuffer(x.tobytes(), dtype=np.uint8)
    host = np.full(2 * GUARD + pad + raw.size, SENTINEL, dtype=np.uint8)
    host[GUARD + pad: GUARD + pad + raw.size] = raw
    t = torch.from_numpy(host).cuda()
    assert (t.data_ptr() + GUARD) % 16 == 0
    return t, GUARD + pad, raw.size


def back(buf):
    """The buffer's bytes; the sentinels around it must be untouched."""
    t, lo, nbytes = buf
    host = t.cpu().numpy()
    assert (host[:lo] == SENTINEL).all() and (host[lo + nbytes:] == SENTINEL).all(), "guard bytes changed"
    return host[lo: lo + nbytes].tobytes()


def launch_all(comms, fn):
    """fn(rank, stream pointer) -> rc on every rank's own stream, then every rank's check."""
    from rdc_amd._lib import _LIB
    torch.cuda.synchronize()
    for r in range(len(comms)):
        rc = fn(r, ctypes.c_void_p(comms.streams[r].cuda_stream))
        assert rc == 0, _LIB.RdcGetLastError()
    for r in range(len(comms)):
        comms[r].check(ctypes.c_void_p(comms.streams[r].cuda_stream))


def dptr(buf):
    return ctypes.c_void_p(buf[0].data_ptr() + buf[1])


@pytest.mark.parametrize("algo", list(ALGOS))
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_group_allreduce_every_schedule(groups, dtype, op, algo):
    """Groups of 2 and 3, every count at a 16-B aligned base and at base + 8 (the
    element-wise head / tail paths): every rank holds loc_ref's bytes, the ring
    order's for every schedule but the tree."""
    from rdc_amd._lib import _LIB
    for n, comms in groups.items():
        for count in ar_counts(n):
            xs, ring, tree, st = case(n, dtype, op, count)
            if count >= 4097:
                L.assert_covers_ties(st, dtype, (n, count))
            want = (tree if algo == "tree" else ring).tobytes()
            for pad in (0, 8):
                bufs = [guarded(x, pad) for x in xs]
                launch_all(comms, lambda r, sp: _LIB.RdcCommAllreduceEx(comms[r].handle, dptr(bufs[r]), count, dtype,
                                                                        op, ALGOS[algo], sp))
                for r in range(n):
                    assert back(bufs[r]) == want, (n, dtype, op, algo, count, pad, "rank", r)


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_group_reduce_scatter_reduce_to_scan(groups, dtype, op):
    """The same inputs through the other collectives: reduce-scatter (bytes
    outside the chunk untouched), ReduceTo (roots 0 and n-1, non-roots
    untouched), Scan and Exscan (rank 0 untouched)."""
    from rdc_amd._lib import _LIB
    for n, comms in groups.items():
        for count in (1, n + 1, TILE + 1, 200003):
            xs, ring, _, st = case(n, dtype, op, count)
            if count >= TILE:
                L.assert_covers_ties(st, dtype, (n, count))
            pad = 8 if count % 2 else 0
            bufs = [guarded(x, pad) for x in xs]
            launch_all(comms, lambda r, sp: _LIB.RdcCommReduceScatter(comms[r].handle, dptr(bufs[r]), count, dtype,
                                                                      op, 0, sp))
            want = L.reduce_scatter(xs, op)
            for r in range(n):
                assert back(bufs[r]) == want[r].tobytes(), ("reduce-scatter", n, count, r)
            for root in (0, n - 1):
                bufs = [guarded(x, pad) for x in xs]
                launch_all(comms, lambda r, sp: _LIB.RdcCommReduceTo(comms[r].handle, dptr(bufs[r]), count, dtype,
                                                                     op, root, sp))
                for r in range(n):
                    assert back(bufs[r]) == (ring if r == root else xs[r]).tobytes(), ("reduce", n, count, root, r)
            for exclusive in (0, 1):
                sst = L.new_stats()
                want = L.scan(xs, op, bool(exclusive), sst)
                if count >= TILE:
                    L.assert_covers_ties(sst, dtype, ("scan", n, count))
                bufs = [guarded(x, pad) for x in xs]
                launch_all(comms, lambda r, sp: _LIB.RdcCommScan(comms[r].handle, dptr(bufs[r]), count, dtype, op,
                                                                 exclusive, sp))
                for r in range(n):
                    assert back(bufs[r]) == want[r].tobytes(), ("scan", n, count, exclusive, r)


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_group_coalesced_allreduce(groups, dtype, op):
    """Five buckets of mixed counts, each its own allocation, some at base + 8:
    one allreduce per bucket, byte for byte."""
    from rdc_amd._lib import _LIB
    for n, comms in groups.items():
        counts = [1, n + 1, TILE + 1, 200003, 3]
        cases = [case(n, dtype, op, k) for k in counts]
        pads = [0, 8, 8, 0, 8]
        bufs = [[guarded(cases[b][0][r], pads[b]) for b in range(5)] for r in range(n)]

        def call(r, sp):
            arr = (ctypes.c_void_p * 5)(*[bufs[r][b][0].data_ptr() + bufs[r][b][1] for b in range(5)])
            cnt = (ctypes.c_size_t * 5)(*counts)
            return _LIB.RdcCommAllreduceCoalesced(comms[r].handle, arr, cnt, 5, dtype, op, 0, sp)
        launch_all(comms, call)
        for r in range(n):
            for b in range(5):
                assert back(bufs[r][b]) == cases[b][1].tobytes(), (n, "bucket", b, "rank", r)


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_rdc_reduce_local(dtype, op):
    """RdcReduce (dst = OP(dst, src) on one GPU) at an 8-byte-offset base: the
    rule table and random colliding data, counts 1, 3 and 100003."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rdc_amd._lib import _LIB
    tdst, tsrc, want_max, want_min = L.table_arrays(dtype)
    sets = [(tdst, tsrc, want_max if op == L.OP_MAXLOC else want_min)]
    for count in (1, 3, 100003):
        d, s = L.gen_inputs(9500 + count + dtype, 2, count, dtype)
        st = L.new_stats()
        sets.append((d, s, L.apply(op, d, s, st)))
        if count > 3:
            L.assert_covers_ties(st, dtype, count)
    for d, s, want in sets:
        for spad in (8, 0):  # src congruent with dst mod 16 (16-B lanes after a head), then not (element-wise)
            db, sb = guarded(d, 8), guarded(s, spad)
            torch.cuda.synchronize()
            assert _LIB.RdcReduce(dptr(db), dptr(sb), d.size, dtype, op, None) == 0, _LIB.RdcGetLastError()
            torch.cuda.synchronize()
            assert back(db) == want.tobytes(), (d.size, spad)
            assert back(sb) == s.tobytes()


def test_group_refusals_launch_nothing(groups):
    """float32 with MAXLOC, F32_I32 with SUM and a 4-byte aligned pair buffer
    are refused before a launch: the launch counter stays."""
    from rdc_amd._lib import _LIB
    comms = groups[2]
    t = torch.zeros(256, dtype=torch.uint8, device="cuda")
    before = launch_counters(comms)
    for dtype, op, off, msg in ((6, 4, 0, b"(dtype, op) = (6, 4)"), (12, 2, 0, b"(dtype, op) = (12, 2)"),
                                (13, 0, 0, b"(dtype, op) = (13, 0)"), (12, 4, 4, b"not aligned"),
                                (13, 5, 12, b"not aligned")):
        p = ctypes.c_void_p(t.data_ptr() + off)
        assert _LIB.RdcCommAllreduce(comms[0].handle, p, 8, dtype, op, None) != 0, (dtype, op, off)
        assert msg in _LIB.RdcGetLastError(), _LIB.RdcGetLastError()
        assert _LIB.RdcCommScan(comms[0].handle, p, 8, dtype, op, 0, None) != 0
        assert _LIB.RdcCommReduceTo(comms[0].handle, p, 8, dtype, op, 0, None) != 0
        assert _LIB.RdcCommReduceScatter(comms[0].handle, p, 8, dtype, op, 0, None) != 0
    assert _LIB.RdcFill(ctypes.c_void_p(t.data_ptr()), 8, 12, 1, 0, None) != 0
    assert _LIB.RdcReduce(ctypes.c_void_p(t.data_ptr() + 4), ctypes.c_void_p(t.data_ptr() + 64), 4, 12, 4, None) != 0
    assert launch_counters(comms) == before


def mp_cases(env_name):
    """Small counts (at most 1 Mi pairs).  "direct": RDC_DIRECT_BYTES=256K, so a
    1 MiB automatic allreduce takes the registered-buffer schedule; "tree":
    rdc_reduce_ring_mincount=64K, so buffers of at most 64 KiB take the tree order."""
    s = 0x10C000
    if env_name == "direct":
        return {"RDC_DIRECT_BYTES": "256K"}, [
            {"kind": "dev", "count": 1001, "dtype": 12, "op": 4, "seed": s + 1},                       # auto, small
            {"kind": "dev", "count": (1 << 17) + 2, "dtype": 12, "op": 4, "seed": s + 2, "direct": True},  # auto -> direct
            {"kind": "dev", "count": (1 << 17) + 3, "dtype": 13, "op": 5, "seed": s + 3, "pad": 8, "direct": True},
            {"kind": "host", "count": 4099, "dtype": 12, "op": 5, "seed": s + 4},                      # the service
            {"kind": "host", "count": 70001, "dtype": 13, "op": 4, "seed": s + 5},                     # zero-copy
            {"kind": "host", "count": (3 << 17) + 5, "dtype": 12, "op": 4, "seed": s + 6},             # 3 MiB: pieces
            {"kind": "py_struct", "count": 20011, "dtype": 12, "op": 4, "seed": s + 7},
            {"kind": "py_tensor", "count": 20011, "dtype": 13, "op": 5, "seed": s + 8},
            {"kind": "py_tensor", "count": 1 << 20, "dtype": 12, "op": 5, "seed": s + 9},
        ]
    return {"rdc_reduce_ring_mincount": "64K"}, [
        {"kind": "dev", "count": 8192, "dtype": 12, "op": 4, "seed": s + 11},     # 64 KiB: the tree order
        {"kind": "dev", "count": 8193, "dtype": 12, "op": 4, "seed": s + 12},     # one pair more: the ring order
        {"kind": "dev", "count": 5, "dtype": 13, "op": 5, "seed": s + 13, "pad": 8},
        {"kind": "host", "count": 4099, "dtype": 13, "op": 4, "seed": s + 14},    # the service, tree order
        {"kind": "host", "count": 70001, "dtype": 12, "op": 5, "seed": s + 15},   # zero-copy, ring order
    ]


@pytest.mark.parametrize("env_name", ["direct", "tree"])
@pytest.mark.parametrize("world", [4, 8])
def test_mp_allreduce(world, env_name):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    env, cases = mp_cases(env_name)
    mincount = (64 << 10) if env_name == "tree" else 1
    tmp = run_mp(world, cases, worker=WORKER, timeout=300, env_extra=env)
    covered = L.new_stats()
    for i, c in enumerate(cases):
        xs = L.gen_inputs(c["seed"], world, c["count"], c["dtype"])
        fold = L.tree if c["count"] * 8 <= mincount else L.ring
        want = fold(xs, c["op"], covered).tobytes()
        for r in range(world):
            got = np.load(os.path.join(tmp, "case%d_rank%d.npy" % (i, r)))
            info = json.load(open(os.path.join(tmp, "case%d_rank%d.json" % (i, r))))
            assert got.tobytes() == want, (env_name, i, c, "rank", r)
            if c.get("direct"):
                assert info["launch"][5] == 6, (i, info)
            if c["kind"] == "py_struct":
                assert info["dtype_kept"] and "not aligned" in info["misaligned"], info
            if c["kind"] == "py_tensor":
                assert info["returns_its_argument"], info
    L.assert_covers_ties(covered, L.DT_F32_I32, env_name)


@pytest.mark.parametrize("world", [2, 3])
def test_cpp_maxloc_equals_the_host_custom_reducer(world, tmp_path):
    """tests/cpp/loc.cc: Allreduce<op::MaxLoc / MinLoc> on a device buffer
    against rdc::Reducer<ValueIndex<float>, f> on a host copy, byte for byte."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    exe = str(tmp_path / "loc")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "loc.cc"), "-o", exe,
                           "-L", os.path.join(ROOT, "rdc_amd"), "-lrdc_amd", "-L", os.path.join(rocm, "lib"),
                           "-lamdhip64", "-Wl,-rpath," + os.path.join(ROOT, "rdc_amd"),
                           "-Wl,-rpath," + os.path.join(rocm, "lib")])
    env = dict(os.environ, RDC_SCRATCH_BYTES="64M")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "-m", "rdc_amd.launcher", "-n", str(world), "--gpus", "1", exe, "100003"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    for r in range(world):
        assert "rank %d: maxloc and minloc OK (world %d, N 100003)" % (r, world) in p.stdout, p.stdout
