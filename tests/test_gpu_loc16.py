"""GPU: MaxLoc / MinLoc over the 16-byte (value, index) pairs — dtype 16
{double, int64} and 17 {int64, int64} — on the device path, byte for byte
against tests/loc16_ref.py (loc_ref's rule and ring, tree and scan orders).

Inputs come from loc16_ref.gen_inputs: values and indexes that a 32-bit or
float32 shortcut gets wrong (doubles equal as float32, differences in the high
dword only, a set top bit of the low dword, INT64_MIN / MAX, NaN, +-0, +-inf
against +-max).  Every test that claims them first asserts on the expected
data, at counts of 2049 and more, that an element decided by the index rule, a
full tie, (f64) a NaN first operand, and elements decided by the upper 32 bits
of the value and of the index are present.

One 64 KiB tile holds 4096 of these pairs.  An element is one 16-byte vector,
so buffers sit on 16-byte boundaries (base + 8 is refused) with guard bytes
around them.

* single-process groups of 2 and 3 (RdcCommInitAll on GPU 0), created once;
* multi-process: 2, 4 and 8 processes on GPU 0, tests/mp_loc16_worker.py;
* C++ through the launcher: tests/cpp/loc16.cc.
"""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import loc16_ref as W
from tests import loc_ref as L
from tests.conftest import ROOT
from tests.test_gpu_ops import OwnStream
from tests.test_gpu_reduce_scatter import Group, launch_counters, run_mp

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

WORKER = os.path.join(ROOT, "tests", "mp_loc16_worker.py")
DTYPES = [W.DT_F64_I64, W.DT_I64_I64]
OPS = [W.OP_MAXLOC, W.OP_MINLOC]
ALGOS = {"ring": 1, "mesh": 2, "mesh_pull": 5, "oneshot": 3, "tree": 4, "auto": 0}
TILE = 4096  # pairs in one 64 KiB tile
ESZ = 16
GUARD = 4096
SENTINEL = 0xA5
COVER = 2049  # counts from here on must hold every kind of element (module docstring)


class Groups(object):
    """The groups of 3 and of 2, each created at its first use and in that
    order, as in tests/test_gpu_loc.py: every rank's stream needs a hardware
    queue of its own.  The streams are this module's own HIP
    streams (tests/test_gpu_ops.py OwnStream), destroyed with the module:
    drawing from torch's stream pool would change which pool streams, and so
    which hardware queues, every later module's groups land on."""

    def __init__(self):
        self.made = {}
        self.hip = ctypes.CDLL("libamdhip64.so")

    def get(self, n):
        if n not in self.made:
            if not torch.cuda.is_available():
                pytest.skip("no GPU")
            import rdc_amd
            comms = Group(rdc_amd.init_group([0] * n, scratch_bytes={3: 24 << 20, 2: 16 << 20}[n]))
            comms.streams = [OwnStream(self.hip) for _ in range(n)]
            # the default threshold: every size takes the ring order unless algo 4 asks for the tree's
            assert comms[0].get_param("rdc_reduce_ring_mincount") < 16
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
    torch.cuda.synchronize()
    for comms in g.made.values():
        for c in comms:
            c.destroy()
        for st in comms.streams:
            st.destroy()


def ar_counts(n):
    return sorted({1, 2, 3, n - 1, n, n + 1, 2049, TILE - 1, TILE, TILE + 1, 100003})


@functools.lru_cache(maxsize=None)
def case(n, dtype, op, count):
    """(inputs, ring result, tree result, fold statistics of both), computed once per shape."""
    xs = W.gen_inputs(16000 + 100 * n + dtype, n, count, dtype)
    st = W.new_stats()
    ring, tree = W.ring(xs, op, st), W.tree(xs, op, st)
    for a in xs + [ring, tree]:
        a.setflags(write=False)
    return xs, ring, tree, st


def guarded(x, pad=0):
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
    """Groups of 2 and 3, every count: every rank holds loc16_ref's bytes, the
    ring order's for every schedule but the tree."""
    from rdc_amd._lib import _LIB
    for n, comms in groups.items():
        for count in ar_counts(n):
            xs, ring, tree, st = case(n, dtype, op, count)
            if count >= COVER:
                W.assert_covers(st, dtype, (n, count))
            want = (tree if algo == "tree" else ring).tobytes()
            bufs = [guarded(x) for x in xs]
            launch_all(comms, lambda r, sp: _LIB.RdcCommAllreduceEx(comms[r].handle, dptr(bufs[r]), count, dtype,
                                                                    op, ALGOS[algo], sp))
            for r in range(n):
                assert back(bufs[r]) == want, (n, dtype, op, algo, count, "rank", r)


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_group_reduce_scatter_reduce_to_scan(groups, dtype, op):
    """The same inputs through the other collectives: reduce-scatter (bytes
    outside the chunk untouched), ReduceTo (roots 0 and n-1, non-roots
    untouched), Scan and Exscan (rank 0 untouched)."""
    from rdc_amd._lib import _LIB
    for n, comms in groups.items():
        for count in (1, n + 1, TILE + 1, 100003):
            xs, ring, _, st = case(n, dtype, op, count)
            if count >= COVER:
                W.assert_covers(st, dtype, (n, count))
            bufs = [guarded(x) for x in xs]
            launch_all(comms, lambda r, sp: _LIB.RdcCommReduceScatter(comms[r].handle, dptr(bufs[r]), count, dtype,
                                                                      op, 0, sp))
            want = W.reduce_scatter(xs, op)
            for r in range(n):
                assert back(bufs[r]) == want[r].tobytes(), ("reduce-scatter", n, count, r)
            for root in (0, n - 1):
                bufs = [guarded(x) for x in xs]
                launch_all(comms, lambda r, sp: _LIB.RdcCommReduceTo(comms[r].handle, dptr(bufs[r]), count, dtype,
                                                                     op, root, sp))
                for r in range(n):
                    assert back(bufs[r]) == (ring if r == root else xs[r]).tobytes(), ("reduce", n, count, root, r)
            for exclusive in (0, 1):
                sst = W.new_stats()
                want = W.scan(xs, op, bool(exclusive), sst)
                if count >= COVER:
                    W.assert_covers(sst, dtype, ("scan", n, count))
                bufs = [guarded(x) for x in xs]
                launch_all(comms, lambda r, sp: _LIB.RdcCommScan(comms[r].handle, dptr(bufs[r]), count, dtype, op,
                                                                 exclusive, sp))
                for r in range(n):
                    assert back(bufs[r]) == want[r].tobytes(), ("scan", n, count, exclusive, r)


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_group_coalesced_allreduce(groups, dtype, op):
    """One list mixing the allreduce's counts, each bucket its own allocation:
    one allreduce per bucket, byte for byte."""
    from rdc_amd._lib import _LIB
    for n, comms in groups.items():
        counts = ar_counts(n)
        nb = len(counts)
        cases = [case(n, dtype, op, k) for k in counts]
        bufs = [[guarded(cases[b][0][r]) for b in range(nb)] for r in range(n)]

        def call(r, sp):
            arr = (ctypes.c_void_p * nb)(*[bufs[r][b][0].data_ptr() + bufs[r][b][1] for b in range(nb)])
            cnt = (ctypes.c_size_t * nb)(*counts)
            return _LIB.RdcCommAllreduceCoalesced(comms[r].handle, arr, cnt, nb, dtype, op, 0, sp)
        launch_all(comms, call)
        for r in range(n):
            for b in range(nb):
                assert back(bufs[r][b]) == cases[b][1].tobytes(), (n, "bucket", b, counts[b], "rank", r)


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_rdc_reduce_local(dtype, op):
    """RdcReduce (dst = OP(dst, src) on one GPU): the rule table and generated
    colliding data, counts 1, 3, 2049 and 100003."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rdc_amd._lib import _LIB
    tdst, tsrc, want_max, want_min = W.table_arrays(dtype)
    sets = [(tdst, tsrc, want_max if op == W.OP_MAXLOC else want_min)]
    for count in (1, 3, 2049, 100003):
        d, s = W.gen_inputs(16500 + count + dtype, 2, count, dtype)
        st = W.new_stats()
        sets.append((d, s, W.apply(op, d, s, st)))
        if count >= COVER:
            W.assert_covers(st, dtype, count)
    for d, s, want in sets:
        db, sb = guarded(d), guarded(s)
        torch.cuda.synchronize()
        assert _LIB.RdcReduce(dptr(db), dptr(sb), d.size, dtype, op, None) == 0, _LIB.RdcGetLastError()
        torch.cuda.synchronize()
        assert back(db) == want.tobytes(), d.size
        assert back(sb) == s.tobytes()


def test_group_refusals_launch_nothing(groups):
    """A wide pair buffer at base + 8 is refused by every entry point, as are
    float64 with MAXLOC and the wide pairs with SUM: the launch counter stays."""
    from rdc_amd._lib import _LIB
    comms = groups[2]
    t = torch.zeros(1024, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 16 == 0
    before = launch_counters(comms)
    h = comms[0].handle
    for dtype, op, off, msg in ((7, 4, 0, b"(dtype, op) = (7, 4)"), (16, 2, 0, b"(dtype, op) = (16, 2)"),
                                (17, 0, 0, b"(dtype, op) = (17, 0)"), (16, 4, 8, b"not aligned"),
                                (17, 5, 8, b"not aligned"), (16, 5, 24, b"not aligned")):
        p = ctypes.c_void_p(t.data_ptr() + off)
        arr, cnt = (ctypes.c_void_p * 1)(p.value), (ctypes.c_size_t * 1)(8)
        calls = {"allreduce": lambda: _LIB.RdcCommAllreduce(h, p, 8, dtype, op, None),
                 "allreduce ex": lambda: _LIB.RdcCommAllreduceEx(h, p, 8, dtype, op, 2, None),
                 "scan": lambda: _LIB.RdcCommScan(h, p, 8, dtype, op, 0, None),
                 "exscan": lambda: _LIB.RdcCommScan(h, p, 8, dtype, op, 1, None),
                 "reduce to": lambda: _LIB.RdcCommReduceTo(h, p, 8, dtype, op, 0, None),
                 "reduce-scatter": lambda: _LIB.RdcCommReduceScatter(h, p, 8, dtype, op, 0, None),
                 "coalesced": lambda: _LIB.RdcCommAllreduceCoalesced(h, arr, cnt, 1, dtype, op, 0, None),
                 "allreduce on": lambda: _LIB.RdcAllreduceOn(h, p, 8, dtype, op),
                 "reduce": lambda: _LIB.RdcReduce(p, ctypes.c_void_p(t.data_ptr() + 512), 8, dtype, op, None)}
        for name, call in calls.items():
            assert call() != 0, (name, dtype, op, off)
            assert msg in _LIB.RdcGetLastError(), (name, _LIB.RdcGetLastError())
    # a misaligned source is refused too
    assert _LIB.RdcReduce(ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(t.data_ptr() + 520), 8, 16, 4, None) != 0
    for dtype in DTYPES:
        assert _LIB.RdcFill(ctypes.c_void_p(t.data_ptr()), 8, dtype, 1, 0, None) != 0
        assert b"pair dtype %d" % dtype in _LIB.RdcGetLastError()
    assert launch_counters(comms) == before
    assert not t.any().item()


def test_three_launches_back_to_back_on_one_stream(groups):
    """F64_I64 allreduce (mesh), F32_I32 scan, I64_I64 allreduce (one-shot) on
    each rank's stream without a host synchronisation in between: all three
    results exact (the element size changes from launch to launch; the scratch
    slots are shared)."""
    from rdc_amd._lib import _LIB
    for n, comms in groups.items():
        count = TILE + 1
        a_in, a_ring, _, _ = case(n, W.DT_F64_I64, W.OP_MAXLOC, count)
        b_in = L.gen_inputs(16700 + n, n, count, L.DT_F32_I32)
        b_want = L.scan(b_in, L.OP_MINLOC)
        c_in, c_ring, _, _ = case(n, W.DT_I64_I64, W.OP_MINLOC, count)
        A, B, C = [guarded(x) for x in a_in], [guarded(x) for x in b_in], [guarded(x) for x in c_in]

        def three(r, sp):
            h = comms[r].handle
            return (_LIB.RdcCommAllreduceEx(h, dptr(A[r]), count, W.DT_F64_I64, W.OP_MAXLOC, ALGOS["mesh"], sp)
                    or _LIB.RdcCommScan(h, dptr(B[r]), count, L.DT_F32_I32, L.OP_MINLOC, 0, sp)
                    or _LIB.RdcCommAllreduceEx(h, dptr(C[r]), count, W.DT_I64_I64, W.OP_MINLOC, ALGOS["oneshot"], sp))
        launch_all(comms, three)
        for r in range(n):
            assert back(A[r]) == a_ring.tobytes(), (n, "mesh F64_I64", r)
            assert back(B[r]) == b_want[r].tobytes(), (n, "scan F32_I32", r)
            assert back(C[r]) == c_ring.tobytes(), (n, "one-shot I64_I64", r)


# ------------------------------------------------------------ multi-process --
def mp_cases(env_name, world):
    """Small counts.  "direct": RDC_DIRECT_BYTES=256K, so a 1 MiB automatic
    allreduce takes the registered-buffer schedule; "tree":
    rdc_reduce_ring_mincount=64K, so buffers of at most 64 KiB (4096 pairs)
    take the tree order.  Each holds a count of 2049 or more that the world
    size does not divide, and count n - 1."""
    s = 0x10C160
    if env_name == "direct":
        return {"RDC_DIRECT_BYTES": "256K"}, [
            {"kind": "dev", "count": world - 1, "dtype": 16, "op": 4, "seed": s + 1},
            {"kind": "dev", "count": (1 << 16) + 3, "dtype": 16, "op": 4, "seed": s + 2, "direct": True},
            {"kind": "dev", "count": (1 << 16) + 5, "dtype": 17, "op": 5, "seed": s + 3, "direct": True},
            {"kind": "py_struct", "count": 20011, "dtype": 16, "op": 4, "seed": s + 4},
            {"kind": "py_tensor", "count": 20011, "dtype": 17, "op": 5, "seed": s + 5},
        ]
    return {"rdc_reduce_ring_mincount": "64K"}, [
        {"kind": "dev", "count": 4095, "dtype": 16, "op": 4, "seed": s + 11},     # just below 64 KiB: the tree order
        {"kind": "dev", "count": 4096, "dtype": 17, "op": 5, "seed": s + 12},     # 64 KiB: the tree order
        {"kind": "dev", "count": 4097, "dtype": 16, "op": 5, "seed": s + 13},     # one pair more: the ring order
        {"kind": "dev", "count": world - 1, "dtype": 17, "op": 4, "seed": s + 14},
        {"kind": "host", "count": 2051, "dtype": 16, "op": 4, "seed": s + 15},    # the service, tree order
    ]


def check_mp(world, cases, tmp, mincount, what):
    covered = {d: W.new_stats() for d in DTYPES}
    for i, c in enumerate(cases):
        xs = W.gen_inputs(c["seed"], world, c["count"], c["dtype"])
        fold = W.tree if c["count"] * ESZ <= mincount else W.ring
        want = fold(xs, c["op"], covered[c["dtype"]] if c["count"] >= COVER else None).tobytes()
        for r in range(world):
            got = np.load(os.path.join(tmp, "case%d_rank%d.npy" % (i, r)))
            info = json.load(open(os.path.join(tmp, "case%d_rank%d.json" % (i, r))))
            assert got.tobytes() == want, (what, i, c, "rank", r)
            if c.get("direct"):
                assert info["launch"][5] == 6, (i, info)
            if c["kind"] in ("dev", "host"):
                assert info["guard_kept"], (i, info)
            if c["kind"] == "py_struct":
                assert info["dtype_kept"] and "not aligned" in info["misaligned"], info
            if c["kind"] == "py_tensor":
                assert info["returns_its_argument"], info
    return covered


@pytest.mark.parametrize("env_name", ["direct", "tree"])
@pytest.mark.parametrize("world", [4, 8])
def test_mp_allreduce(world, env_name):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    env, cases = mp_cases(env_name, world)
    assert any(c["count"] >= COVER and c["count"] % world for c in cases)
    tmp = run_mp(world, cases, worker=WORKER, timeout=300, env_extra=env)
    covered = check_mp(world, cases, tmp, (64 << 10) if env_name == "tree" else 1, env_name)
    W.assert_covers(covered[W.DT_F64_I64], W.DT_F64_I64, env_name)


def test_mp_host_buffers_take_every_host_path():
    """Host buffers of 64 B, 64 KiB, 64 KiB + 16, 1 MiB + 16 and 16 MiB + 16
    through RdcAllreduceOn at 2 processes: the resident service (up to 64 KiB),
    the zero-copy path (up to 1 MiB) and the pipelined pieces above, each at
    least once, with guard bytes around every host buffer."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    s = 0x10C16A0
    sizes = [64, 64 << 10, (64 << 10) + 16, (1 << 20) + 16, (16 << 20) + 16]
    cases = [{"kind": "host", "count": b // ESZ, "dtype": DTYPES[i % 2], "op": OPS[(i // 2) % 2], "seed": s + i}
             for i, b in enumerate(sizes)]
    tmp = run_mp(2, cases, worker=WORKER, timeout=300)
    covered = check_mp(2, cases, tmp, 1, "host")
    for d in DTYPES:
        W.assert_covers(covered[d], d, "host")


@pytest.mark.parametrize("world", [2, 3])
def test_cpp_maxloc_equals_the_host_custom_reducer(world, tmp_path):
    """tests/cpp/loc16.cc: Allreduce<op::MaxLoc / MinLoc> on a device buffer of
    ValueIndex<double> against rdc::Reducer<ValueIndex<double>, f> on a host
    copy, byte for byte."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    exe = str(tmp_path / "loc16")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "loc16.cc"), "-o", exe,
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
        assert "rank %d: maxloc16 and minloc16 OK (world %d, N 100003)" % (r, world) in p.stdout, p.stdout
