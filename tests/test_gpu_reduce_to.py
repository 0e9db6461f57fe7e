"""GPU parity of the rooted reduce (RdcCommReduceTo / RdcReduceTo; MPI_Reduce)
against the CPU oracle: on the root every element holds the bits of the ring
allreduce, and on every other rank every byte of the buffer still holds that
rank's own input.  Every device buffer sits between 4 KiB of sentinel bytes,
which no rank may change.

* single-process groups (k_rooted): n communicators on GPU 0, one stream each,
  created once per module;
* multi-process: n processes on GPU 0, tests/mp_reduce_to_worker.py.
"""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O
from tests.conftest import ROOT
from tests.gpu_util import VALID, rand_input, same_bits
from tests.test_gpu_reduce_scatter import (expected_rs, last_launch, launch_counters, load, make_group,  # noqa: F401
                                           run_mp)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

WORKER = os.path.join(ROOT, "tests", "mp_reduce_to_worker.py")
GUARD = 4096
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def group3():
    g = make_group(3, 24 << 20)
    yield g
    for c in g:
        c.destroy()


@pytest.fixture(scope="module")
def group2():
    g = make_group(2, 16 << 20)
    yield g
    for c in g:
        c.destroy()


def expected_rt(inputs, dtype, op, root):
    """Per rank: the ring allreduce on the root, the rank's own input elsewhere."""
    full = O.expected_allreduce(inputs, dtype, op)
    return [full if r == root else np.ascontiguousarray(x) for r, x in enumerate(inputs)]


def guarded(x, pad_bytes):
    """uint8 ROCm tensor: GUARD sentinel bytes, pad_bytes more, x's bytes, GUARD sentinel bytes."""
    raw = np.frombuffer(np.ascontiguousarray(x).tobytes(), dtype=np.uint8)
    host = np.full(2 * GUARD + pad_bytes + raw.size, SENTINEL, dtype=np.uint8)
    host[GUARD + pad_bytes: GUARD + pad_bytes + raw.size] = raw
    return torch.from_numpy(host).cuda(), GUARD + pad_bytes, raw.size


def assert_rt(bufs, inputs, dtype, op, root, what):
    """The root holds the reduction, every other rank its input byte for byte,
    and no sentinel byte around any buffer changed."""
    want = expected_rt(inputs, dtype, op, root)
    for r, (t, lo, nbytes) in enumerate(bufs):
        host = t.cpu().numpy()
        assert (host[:lo] == SENTINEL).all() and (host[lo + nbytes:] == SENTINEL).all(), (what, "guards of rank", r)
        got = np.frombuffer(host[lo: lo + nbytes].tobytes(), dtype=O.NP_DTYPE[dtype])
        if r == root:
            assert same_bits(got, want[r], dtype), (what, "the root's result")
        else:
            assert got.tobytes() == want[r].tobytes(), (what, "buffer of non-root rank", r)


def run_group_rt(comms, inputs, dtype, op, root, pads=None):
    """Launch every rank's rooted reduce on its own stream; the guarded buffers back."""
    from rdc_amd._lib import _LIB
    n = len(comms)
    count = inputs[0].size
    pads = pads or [0] * n
    esz = np.dtype(O.NP_DTYPE[dtype]).itemsize
    bufs = [guarded(x, p * esz) for x, p in zip(inputs, pads)]
    torch.cuda.synchronize()
    for r in range(n):
        rc = _LIB.RdcCommReduceTo(comms[r].handle, ctypes.c_void_p(bufs[r][0].data_ptr() + bufs[r][1]), count, dtype,
                                  op, root, ctypes.c_void_p(comms.streams[r].cuda_stream))
        assert rc == 0, _LIB.RdcGetLastError()
    for r in range(n):
        comms[r].check(ctypes.c_void_p(comms.streams[r].cuda_stream))
    return bufs


def assert_roles(comms, root):
    """RdcCommLastLaunch: mesh algo, gather blocks on the root only."""
    for r, c in enumerate(comms):
        ll = last_launch(c)
        assert ll[5] == 2 and ll[1] >= 1 and ll[2] >= 1 and ll[0] == ll[1] + ll[2] + ll[3], (r, ll)
        assert (ll[3] >= 1) if r == root else (ll[3] == 0), (r, root, ll)


@pytest.mark.parametrize("dtype,op", VALID)
def test_group3_all_types(group3, dtype, op):
    """Counts below n (empty chunks, also the root's own), chunk boundaries off
    16 B, buffers at rank-dependent offsets (pads 1, 0, 3 elements: the
    element-wise fold) and vector heads and tails, the root cycling."""
    rng = np.random.default_rng(277 + dtype * 8 + op)
    for k, count in enumerate((1, 2, 5, 1001, 4099)):
        root = (k + 1) % 3   # counts 1 and 2: the root's own chunk is empty
        inputs = [rand_input(rng, count, dtype) for _ in range(3)]
        bufs = run_group_rt(group3, inputs, dtype, op, root, pads=[1, 0, 3])
        assert_rt(bufs, inputs, dtype, op, root, (dtype, op, count, root))
        assert_roles(group3, root)


def test_group3_every_root_at_every_count(group3):
    """fp32 sum: each count of the type sweep with each of the three roots."""
    rng = np.random.default_rng(278)
    for count in (1, 2, 5, 1001, 4099):
        for root in range(3):
            inputs = [rand_input(rng, count, O.DT_FLOAT32) for _ in range(3)]
            bufs = run_group_rt(group3, inputs, O.DT_FLOAT32, O.OP_SUM, root, pads=[1, 0, 3])
            assert_rt(bufs, inputs, O.DT_FLOAT32, O.OP_SUM, root, (count, root))
            assert_roles(group3, root)


@pytest.mark.parametrize("root", [0, 1])
def test_group_multi_piece(group2, root):
    """A chunk larger than a scratch slot goes through several launches."""
    rng = np.random.default_rng(279 + root)
    count = (6 << 20) // 4 * 3 + 7   # 18 MiB fp32 > 2 x 4 MiB slots
    inputs = [rng.standard_normal(count).astype(np.float32) for _ in range(2)]
    bufs = run_group_rt(group2, inputs, O.DT_FLOAT32, O.OP_SUM, root, pads=[0, 5])
    assert_rt(bufs, inputs, O.DT_FLOAT32, O.OP_SUM, root, ("multi-piece", root))
    assert_roles(group2, root)


@pytest.mark.parametrize("s16,r16,grid,tile", [(1, 14, 0, 0), (7, 1, 24, 64 << 10)])
def test_group_tuned_shapes_stay_exact(group3, s16, r16, grid, tile):
    rng = np.random.default_rng(s16 * 100 + r16 + 1)
    try:
        for c in group3:
            c.tune(s16, r16, grid, tile)
        for root in (2, 0):
            inputs = [rng.standard_normal(300007).astype(np.float32) for _ in range(3)]
            bufs = run_group_rt(group3, inputs, O.DT_FLOAT32, O.OP_SUM, root, pads=[0, 1, 2])
            assert_rt(bufs, inputs, O.DT_FLOAT32, O.OP_SUM, root, (s16, r16, grid, tile, root))
            assert_roles(group3, root)
            for c in group3:
                ll = last_launch(c)
                assert (grid == 0 or ll[0] <= grid) and (tile == 0 or ll[4] == tile), ll
    finally:
        for c in group3:
            c.tune()


@pytest.mark.parametrize("dtype,op", [(O.DT_FLOAT32, O.OP_SUM), (O.DT_INT64, O.OP_MAX)])
def test_group3_reduce_then_broadcast_is_the_allreduce(group3, dtype, op):
    from rdc_amd._lib import _LIB
    rng = np.random.default_rng(280 + dtype)
    count = 70001
    esz = np.dtype(O.NP_DTYPE[dtype]).itemsize
    want = None
    for root in (1, 2):
        inputs = [rand_input(rng, count, dtype) for _ in range(3)]
        bufs = [guarded(x, 0) for x in inputs]
        torch.cuda.synchronize()
        for r in range(3):
            sp = ctypes.c_void_p(group3.streams[r].cuda_stream)
            p = ctypes.c_void_p(bufs[r][0].data_ptr() + bufs[r][1])
            assert _LIB.RdcCommReduceTo(group3[r].handle, p, count, dtype, op, root, sp) == 0, _LIB.RdcGetLastError()
            assert _LIB.RdcCommBroadcast(group3[r].handle, p, count * esz, root, sp) == 0, _LIB.RdcGetLastError()
        ring = [np.ascontiguousarray(x).copy() for x in inputs]
        O.allreduce_ring(ring, dtype, op)
        want = O.expected_allreduce(inputs, dtype, op)
        for r in range(3):
            group3[r].check(ctypes.c_void_p(group3.streams[r].cuda_stream))
            t, lo, nbytes = bufs[r]
            host = t.cpu().numpy()
            got = np.frombuffer(host[lo: lo + nbytes].tobytes(), dtype=O.NP_DTYPE[dtype])
            assert same_bits(got, want, dtype) and same_bits(got, ring[r], dtype), (root, r)
            assert (host[:lo] == SENTINEL).all() and (host[lo + nbytes:] == SENTINEL).all(), (root, r)


def test_group_refusals_launch_nothing(group3):
    from rdc_amd._lib import _LIB
    t = torch.zeros(64 + 4, dtype=torch.float32, device="cuda")
    p = ctypes.c_void_p(t.data_ptr())
    before = launch_counters(group3)
    for root, word in ((-1, b"root"), (3, b"root")):
        for c in group3:
            assert _LIB.RdcCommReduceTo(c.handle, p, 64, O.DT_FLOAT32, O.OP_SUM, root, None) != 0
            assert word in _LIB.RdcGetLastError(), _LIB.RdcGetLastError()
    c = group3[0]
    assert _LIB.RdcCommReduceTo(c.handle, p, 64, O.DT_FLOAT32, O.OP_BITOR, 0, None) != 0
    assert b"unsupported" in _LIB.RdcGetLastError()
    assert _LIB.RdcCommReduceTo(c.handle, p, 64, 99, O.OP_SUM, 0, None) != 0
    assert _LIB.RdcCommReduceTo(c.handle, ctypes.c_void_p(t.data_ptr() + 2), 64, O.DT_FLOAT32, O.OP_SUM, 0, None) != 0
    assert b"aligned" in _LIB.RdcGetLastError()
    assert _LIB.RdcCommReduceTo(c.handle, None, 64, O.DT_FLOAT32, O.OP_SUM, 0, None) != 0
    assert b"null" in _LIB.RdcGetLastError()
    # count 0 succeeds and consumes no launch number
    for c in group3:
        assert _LIB.RdcCommReduceTo(c.handle, None, 0, O.DT_FLOAT32, O.OP_SUM, 1, None) == 0
    torch.cuda.synchronize()
    assert launch_counters(group3) == before
    # and the group still works
    rng = np.random.default_rng(281)
    inputs = [rand_input(rng, 1001, O.DT_FLOAT32) for _ in range(3)]
    assert_rt(run_group_rt(group3, inputs, O.DT_FLOAT32, O.OP_SUM, 1), inputs, O.DT_FLOAT32, O.OP_SUM, 1, "after")
    after = launch_counters(group3)
    assert after == [b + 1 for b in before], (before, after)


def test_group_graph_capture_replay(group2):
    """A captured rooted reduce replays with fresh inputs (the launch numbers
    live on the device); eager allreduces and an eager rooted reduce with the
    other root interleave with the replays, in poison mode."""
    import rdc_amd
    from rdc_amd._lib import _LIB
    from tests.gpu_util import from_dev, ptr, to_dev
    rng = np.random.default_rng(282)
    count, root = 300007, 1
    for c in group2:
        c.set_poison(True)
    try:
        ts = [torch.zeros(count, dtype=torch.float32, device="cuda") for _ in range(2)]
        graphs = []
        torch.cuda.synchronize()
        for r in range(2):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=group2.streams[r], capture_error_mode="thread_local"):
                group2[r].reduce(ts[r], rdc_amd.Op.SUM, root, stream=ctypes.c_void_p(group2.streams[r].cuda_stream))
            graphs.append(g)
        assert_roles(group2, root)
        torch.cuda.synchronize()

        def replay(tag):
            xs = [rng.standard_normal(count).astype(np.float32) for _ in range(2)]
            for r in range(2):
                ts[r].copy_(torch.from_numpy(xs[r]))
            torch.cuda.synchronize()
            for r in range(2):
                with torch.cuda.stream(group2.streams[r]):
                    graphs[r].replay()
            for r in range(2):
                group2[r].check(ctypes.c_void_p(group2.streams[r].cuda_stream))
            want = expected_rt(xs, O.DT_FLOAT32, O.OP_SUM, root)
            for r in range(2):
                assert ts[r].cpu().numpy().tobytes() == want[r].tobytes(), (tag, r)

        for it in range(4):
            replay(("replay", it))
        ctr = launch_counters(group2)
        assert ctr[0] == ctr[1], ("launch counters differ after the replays", ctr)
        for eager_algo in (2, 1, 0):
            xs = [rng.standard_normal(1001).astype(np.float32) for _ in range(2)]
            bufs = [to_dev(x) for x in xs]
            torch.cuda.synchronize()
            for r in range(2):
                assert _LIB.RdcCommAllreduceEx(group2[r].handle, ptr(bufs[r]), 1001, O.DT_FLOAT32, O.OP_SUM, eager_algo,
                                               ctypes.c_void_p(group2.streams[r].cuda_stream)) == 0
            want = O.expected_allreduce(xs, O.DT_FLOAT32, O.OP_SUM)
            for r in range(2):
                group2[r].check(ctypes.c_void_p(group2.streams[r].cuda_stream))
                assert from_dev(bufs[r], 0, 1001, O.DT_FLOAT32).tobytes() == want.tobytes(), (eager_algo, r)
        xs = [rng.standard_normal(1001).astype(np.float32) for _ in range(2)]
        assert_rt(run_group_rt(group2, xs, O.DT_FLOAT32, O.OP_SUM, 0), xs, O.DT_FLOAT32, O.OP_SUM, 0, "eager, root 0")
        for it in range(2):
            replay(("after eager", it))
        ctr = launch_counters(group2)
        assert ctr[0] == ctr[1], ("launch counters differ", ctr)
    finally:
        for c in group2:
            c.set_poison(False)


# --------------------------------------------------------------- multi-process
CHAIN = [("rt", 0), ("ar", 1), ("rt", 1), ("rt", 2), ("ar", 2), ("rt", 0), ("ar", 3), ("rt", 1), ("ar", 3), ("rt", 2),
         ("ar", 4), ("rt", 0), ("ar", 5), ("rt", 1), ("ar", 0), ("rt", 2), ("bc", 1), ("rt", 0), ("rs", 2), ("rt", 1),
         ("a2a", 0), ("rt", 2), ("ag", 0), ("rt", 0)]


def test_mp_back_to_back_launches_in_poison_mode():
    """The slot-reuse argument: a rooted reduce writes the
    root's AG slots only after folding the root's contribution of the same
    launch, and ends only after every peer's launch did.  24 launches on one
    int32 buffer without a host sync, consumed scratch poisoned: rooted reduces
    with rotating roots between allreduces of every schedule, a broadcast, a
    reduce-scatter, an all-to-all and an allgather; two rooted reduces back to
    back, a one-shot directly before and directly after one.  The buffer is
    refilled before each step and summed into an accumulator after it."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    world, count, seed = 3, 50001, 0x5EED7200
    case = {"kind": "chain", "count": count, "steps": CHAIN, "seed": seed}
    tmp = run_mp(world, [case], worker=WORKER)
    acc = [np.zeros(count, dtype=np.int32) for _ in range(world)]
    chunks = [(int(b), int(e)) for b, e in O.split(count, world)]
    m = count // world
    for k, (what, arg) in enumerate(CHAIN):
        xs = [O.fill(count, O.DT_INT32, seed + k, r) for r in range(world)]
        if what == "rt":
            step = expected_rt(xs, O.DT_INT32, O.OP_SUM, arg)
        elif what == "rs":
            step = expected_rs(xs, O.DT_INT32, O.OP_SUM)
        elif what == "ar":
            step = [x.copy() for x in xs]
            (O.allreduce_tree if arg == 4 else O.allreduce_ring)(step, O.DT_INT32, O.OP_SUM)
        elif what == "bc":
            step = [xs[arg]] * world
        elif what == "a2a":
            step = []
            for r in range(world):
                y = np.zeros(count, dtype=np.int32)
                for p in range(world):
                    y[p * m: (p + 1) * m] = xs[p][r * m: (r + 1) * m]
                step.append(y)
        else:  # allgather of the Split chunks, in place
            y = np.concatenate([xs[c][b:e] for c, (b, e) in enumerate(chunks)])
            step = [y] * world
        for r in range(world):
            O.reducer(np.ascontiguousarray(step[r]), acc[r], O.DT_INT32, O.OP_SUM)
    for r in range(world):
        got, _ = load(tmp, 0, r, O.DT_INT32)
        assert got.tobytes() == acc[r].tobytes(), r


def test_mp_host_buffer_and_python_surface():
    """RdcReduceTo on an ndarray inside a larger array of sentinel bytes, root 1:
    the root holds the result, the non-root array and every guard byte are
    untouched.  rdc_amd.reduce and Comm.reduce on tensors."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    world, count = 2, 100003
    cases = [{"kind": "host", "count": count, "op": 2, "root": 1},
             {"kind": "py", "count": count, "op": 2, "root": 0, "module": True, "seed": 0x5EED7300},
             {"kind": "py", "count": count, "op": 0, "root": 1, "seed": 0x5EED7400}]
    tmp = run_mp(world, cases, worker=WORKER)
    for i, c in enumerate(cases):
        inputs = [O.fill(count, O.DT_FLOAT32, c.get("seed", 0x5EED0000), r) for r in range(world)]
        want = expected_rt(inputs, O.DT_FLOAT32, c["op"], c["root"])
        for r in range(world):
            backing = np.load(os.path.join(tmp, "case%d_rank%d.npy" % (i, r)))
            info = json.load(open(os.path.join(tmp, "case%d_rank%d.json" % (i, r))))
            assert backing.size == count * 4 + 2 * GUARD
            assert (backing[:GUARD] == SENTINEL).all() and (backing[GUARD + count * 4:] == SENTINEL).all(), (i, r)
            got = np.frombuffer(backing[GUARD: GUARD + count * 4].tobytes(), dtype=np.float32)
            if r == c["root"]:
                assert same_bits(got, want[r], O.DT_FLOAT32), (i, r)
            else:
                assert got.tobytes() == want[r].tobytes(), (i, r)
            assert info["returns_its_argument"], (i, r)
            ll = info["launch"]
            assert ll[5] == 2 and ((ll[3] >= 1) if r == c["root"] else (ll[3] == 0)), (i, r, ll)


@pytest.mark.parametrize("world,root", [(2, 1), (3, 0)])
def test_cpp_reduce_to_through_the_launcher(world, root, tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    exe = str(tmp_path / "reduce_to")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "reduce_to.cc"), "-o", exe,
                           "-L", os.path.join(ROOT, "rdc_amd"), "-lrdc_amd",
                           "-Wl,-rpath," + os.path.join(ROOT, "rdc_amd")])
    env = dict(os.environ, RDC_SCRATCH_BYTES="64M")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "-m", "rdc_amd.launcher", "-n", str(world), "--gpus", "1", exe, "100003",
                        str(root)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    for r in range(world):
        assert "rank %d: reduce-to OK (world %d, N 100003, root %d)" % (r, world, root) in p.stdout, p.stdout
