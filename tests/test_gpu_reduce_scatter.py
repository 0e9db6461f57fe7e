"""GPU parity of the in-place reduce-scatter (RdcCommReduceScatter /
RdcReduceScatter; the reference's TryReduceScatterRing,
communicator_collective.cc:115-182) against the CPU oracle: on rank r chunk r
of utils::Split(0, count, n) holds the bits of the ring allreduce, and every
byte outside it still holds rank r's own input.

* single-process groups (the scratch schedule, k_rscatter): n communicators on
  GPU 0, one stream each, created once per module;
* multi-process (the registered-buffer schedule too, k_rscatter_direct): n
  processes on GPU 0, tests/mp_rs_worker.py.
"""
import ctypes
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import pytest

from oracle import oracle as O
from tests.conftest import ROOT, free_port
from tests.gpu_util import VALID, from_dev, ptr, rand_input, same_bits, to_dev

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

WORKER = os.path.join(ROOT, "tests", "mp_rs_worker.py")


class Group(list):
    streams = None


def make_group(n, scratch):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import rdc_amd
    g = Group(rdc_amd.init_group([0] * n, scratch_bytes=scratch))
    g.streams = [torch.cuda.Stream() for _ in range(n)]  # one per rank for the whole module
    return g


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


def expected_rs(inputs, dtype, op):
    """Per rank: its input with chunk r replaced by the ring allreduce's chunk r."""
    full = O.expected_allreduce(inputs, dtype, op)
    out = []
    for r, (b, e) in enumerate(O.split(inputs[0].size, len(inputs))):
        x = np.ascontiguousarray(inputs[r]).copy()
        x[b:e] = full[b:e]
        out.append(x)
    return out


def assert_rs(got, want, inputs, dtype, what):
    """The chunk holds the reduction and the rest is unchanged, rank by rank."""
    n = len(want)
    for r, (b, e) in enumerate(O.split(want[0].size, n)):
        assert same_bits(got[r][b:e], want[r][b:e], dtype), (what, "chunk of rank", r)
        assert got[r][:b].tobytes() == inputs[r][:b].tobytes() and got[r][e:].tobytes() == inputs[r][e:].tobytes(), \
            (what, "bytes outside the chunk of rank", r)


def run_group_rs(comms, inputs, dtype, op, algo, pads=None):
    """Launch every rank's reduce-scatter on its own stream; the whole buffers back."""
    from rdc_amd._lib import _LIB
    n = len(comms)
    count = inputs[0].size
    pads = pads or [0] * n
    esz = np.dtype(O.NP_DTYPE[dtype]).itemsize
    bufs = [to_dev(x, p * esz) for x, p in zip(inputs, pads)]
    torch.cuda.synchronize()
    for r in range(n):
        rc = _LIB.RdcCommReduceScatter(comms[r].handle, ptr(bufs[r], pads[r] * esz), count, dtype, op, algo,
                                       ctypes.c_void_p(comms.streams[r].cuda_stream))
        assert rc == 0, _LIB.RdcGetLastError()
    for r in range(n):
        comms[r].check(ctypes.c_void_p(comms.streams[r].cuda_stream))
    return [from_dev(bufs[r], pads[r] * esz, count, dtype) for r in range(n)]


def last_launch(comm):
    from rdc_amd._lib import _LIB
    ll = (ctypes.c_uint64 * 6)()
    assert _LIB.RdcCommLastLaunch(comm.handle, ll) == 0
    return [int(x) for x in ll]


@pytest.mark.parametrize("dtype,op", VALID)
def test_group3_mesh_all_types(group3, dtype, op):
    """Counts below n (empty chunks), chunk boundaries off 16 B, and buffers at
    rank-dependent offsets (pads 1, 0, 3 elements: the element-wise fold)."""
    rng = np.random.default_rng(177 + dtype * 8 + op)
    for count in (1, 2, 5, 1001, 4099):
        inputs = [rand_input(rng, count, dtype) for _ in range(3)]
        got = run_group_rs(group3, inputs, dtype, op, 2, pads=[1, 0, 3])
        assert_rs(got, expected_rs(inputs, dtype, op), inputs, dtype, (dtype, op, count))
        ll = last_launch(group3[0])
        assert ll[5] == 2 and ll[3] == 0 and ll[1] >= 1 and ll[2] >= 1 and ll[0] == ll[1] + ll[2], ll


def test_group3_auto_is_the_mesh(group3):
    """algo 0 in a single-process group: direct is not eligible there."""
    rng = np.random.default_rng(178)
    for count in (5, 70001):
        inputs = [rand_input(rng, count, O.DT_FLOAT32) for _ in range(3)]
        auto = run_group_rs(group3, inputs, O.DT_FLOAT32, O.OP_SUM, 0)
        assert last_launch(group3[1])[5] == 2
        mesh = run_group_rs(group3, inputs, O.DT_FLOAT32, O.OP_SUM, 2)
        assert_rs(auto, expected_rs(inputs, O.DT_FLOAT32, O.OP_SUM), inputs, O.DT_FLOAT32, count)
        for r in range(3):
            assert auto[r].tobytes() == mesh[r].tobytes()
    # explicit direct falls back to the mesh the same way
    got = run_group_rs(group3, inputs, O.DT_FLOAT32, O.OP_SUM, 6)
    assert last_launch(group3[2])[5] == 2
    assert_rs(got, expected_rs(inputs, O.DT_FLOAT32, O.OP_SUM), inputs, O.DT_FLOAT32, "algo 6")


def test_group_rejects_schedules_it_does_not_have(group2):
    from rdc_amd._lib import _LIB
    t = torch.zeros(64, dtype=torch.float32, device="cuda")
    for algo in (1, 3, 4, 5):
        assert _LIB.RdcCommReduceScatter(group2[0].handle, ptr(t), 64, O.DT_FLOAT32, O.OP_SUM, algo, None) != 0
        assert ("algo %d" % algo).encode() in _LIB.RdcGetLastError()
    assert _LIB.RdcCommReduceScatter(group2[0].handle, ptr(t), 64, O.DT_FLOAT32, O.OP_BITOR, 2, None) != 0


def test_group_multi_piece(group2):
    """A chunk larger than a scratch slot goes through several launches."""
    rng = np.random.default_rng(179)
    count = (6 << 20) // 4 * 3 + 7   # 18 MiB fp32 > 2 x 4 MiB slots
    inputs = [rng.standard_normal(count).astype(np.float32) for _ in range(2)]
    got = run_group_rs(group2, inputs, O.DT_FLOAT32, O.OP_SUM, 2, pads=[0, 5])
    assert_rs(got, expected_rs(inputs, O.DT_FLOAT32, O.OP_SUM), inputs, O.DT_FLOAT32, "multi-piece")


@pytest.mark.parametrize("s16,r16,grid,tile", [(1, 14, 0, 0), (7, 1, 24, 64 << 10)])
def test_group_tuned_shapes_stay_exact(group3, s16, r16, grid, tile):
    rng = np.random.default_rng(s16 * 100 + r16)
    try:
        for c in group3:
            c.tune(s16, r16, grid, tile)
        inputs = [rng.standard_normal(300007).astype(np.float32) for _ in range(3)]
        got = run_group_rs(group3, inputs, O.DT_FLOAT32, O.OP_SUM, 2, pads=[0, 1, 2])
        assert_rs(got, expected_rs(inputs, O.DT_FLOAT32, O.OP_SUM), inputs, O.DT_FLOAT32, (s16, r16, grid, tile))
        ll = last_launch(group3[0])
        assert ll[3] == 0 and (grid == 0 or ll[0] <= grid) and (tile == 0 or ll[4] == tile), ll
    finally:
        for c in group3:
            c.tune()


@pytest.mark.parametrize("dtype,op", [(O.DT_FLOAT32, O.OP_SUM), (O.DT_INT64, O.OP_MAX)])
def test_group3_reduce_scatter_then_allgather_is_the_allreduce(group3, dtype, op):
    from rdc_amd._lib import _LIB
    rng = np.random.default_rng(180 + dtype)
    count = 70001
    esz = np.dtype(O.NP_DTYPE[dtype]).itemsize
    inputs = [rand_input(rng, count, dtype) for _ in range(3)]
    bufs = [to_dev(x) for x in inputs]
    chunks = O.split(count, 3)
    torch.cuda.synchronize()
    for r in range(3):
        sp = ctypes.c_void_p(group3.streams[r].cuda_stream)
        assert _LIB.RdcCommReduceScatter(group3[r].handle, ptr(bufs[r]), count, dtype, op, 2, sp) == 0
        ptrs = (ctypes.c_void_p * 3)(*[bufs[r].data_ptr() + int(b) * esz for b, _ in chunks])
        sizes = (ctypes.c_size_t * 3)(*[int(e - b) * esz for b, e in chunks])
        assert _LIB.RdcCommAllgather(group3[r].handle, ptrs, sizes, sp) == 0, _LIB.RdcGetLastError()
    want = O.expected_allreduce(inputs, dtype, op)
    for r in range(3):
        group3[r].check(ctypes.c_void_p(group3.streams[r].cuda_stream))
        assert same_bits(from_dev(bufs[r], 0, count, dtype), want, dtype), r


def launch_counters(comms):
    from rdc_amd._lib import _LIB
    out = []
    for c in comms:
        v = ctypes.c_uint64()
        assert _LIB.RdcCommLaunchCounter(c.handle, ctypes.byref(v)) == 0, _LIB.RdcGetLastError()
        out.append(v.value)
    return out


@pytest.mark.parametrize("algo", ["mesh", "auto"])
def test_group_graph_capture_replay(group2, algo):
    """A captured reduce-scatter replays with fresh inputs (the launch numbers
    live on the device), eager allreduces and an eager reduce-scatter interleave
    with the replays, in poison mode; a captured algo 0 takes the mesh."""
    import rdc_amd
    from rdc_amd._lib import _LIB
    rng = np.random.default_rng(181)
    count = 300007
    for c in group2:
        c.set_poison(True)
    try:
        ts = [torch.zeros(count, dtype=torch.float32, device="cuda") for _ in range(2)]
        graphs = []
        torch.cuda.synchronize()
        for r in range(2):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=group2.streams[r], capture_error_mode="thread_local"):
                group2[r].reduce_scatter(ts[r], rdc_amd.Op.SUM, algo=algo,
                                         stream=ctypes.c_void_p(group2.streams[r].cuda_stream))
            graphs.append(g)
            assert last_launch(group2[r])[5] == 2
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
            assert_rs([t.cpu().numpy() for t in ts], expected_rs(xs, O.DT_FLOAT32, O.OP_SUM), xs, O.DT_FLOAT32, tag)

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
        got = run_group_rs(group2, xs, O.DT_FLOAT32, O.OP_SUM, 2)
        assert_rs(got, expected_rs(xs, O.DT_FLOAT32, O.OP_SUM), xs, O.DT_FLOAT32, "eager reduce-scatter")
        for it in range(2):
            replay(("after eager", it))
        ctr = launch_counters(group2)
        assert ctr[0] == ctr[1], ("launch counters differ", ctr)
    finally:
        for c in group2:
            c.set_poison(False)


def test_missing_peer_times_out_instead_of_hanging():
    """Rank 1 never joins: rank 0's reduce blocks give up after RDC_TIMEOUT,
    the end-of-launch wait for the peers' done words gives up with them, and
    RdcCommCheck reports the failure."""
    import rdc_amd
    from rdc_amd._lib import _LIB, RdcError
    assert _LIB.RdcSetParam(b"RDC_TIMEOUT", b"1") == 0
    try:
        g = make_group(2, 8 << 20)
    finally:
        assert _LIB.RdcSetParam(b"RDC_TIMEOUT", b"30") == 0
    try:
        t = torch.ones(100003, dtype=torch.float32, device="cuda")
        sp = ctypes.c_void_p(g.streams[0].cuda_stream)
        torch.cuda.synchronize()
        t0 = time.time()
        g[0].reduce_scatter(t, rdc_amd.Op.SUM, algo="mesh", stream=sp)
        with pytest.raises(RdcError, match="timed out"):
            g[0].check(sp)
        assert time.time() - t0 < 20
    finally:
        for c in g:
            c.destroy()


# --------------------------------------------------------------- multi-process
def run_mp(world, cases, worker=WORKER, timeout=240, env_extra=None):
    tmp = tempfile.mkdtemp(prefix="rdc_rs_")
    cf = os.path.join(tmp, "cases.json")
    with open(cf, "w") as f:
        json.dump(cases, f)
    port = free_port()
    env = dict(os.environ)
    env.update({"RDC_DEVICE": "0", "RDC_SCRATCH_BYTES": "64M"})
    env.update(env_extra or {})
    # every rank on GPU 0: the hardware-queue budget rdc_amd.launcher applies
    # to workers that share a GPU
    from rdc_amd.launcher import hw_queues_per_process, queues_over_budget
    q = hw_queues_per_process(world)
    if (q is not None and not env.get("RDC_TEST_KEEP_QUEUES")
            and queues_over_budget(env.get("GPU_MAX_HW_QUEUES"), q)):
        env["GPU_MAX_HW_QUEUES"] = str(q)
    procs = [subprocess.Popen([sys.executable, worker, str(r), str(world), str(port), tmp, cf], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(world)]
    outs = []
    deadline = time.time() + timeout
    for p in procs:
        try:
            out, _ = p.communicate(timeout=max(1.0, deadline - time.time()))
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            tails = []
            for r, q in enumerate(procs):  # what every rank printed before the kill
                try:
                    o, _ = q.communicate(timeout=10)
                    tails.append("rank %d:\n%s" % (r, o.decode(errors="replace")[-1500:]))
                except Exception:  # noqa: BLE001
                    tails.append("rank %d: (no output)" % r)
            raise AssertionError("multi-process run timed out after %.0f s\n%s" % (timeout, "\n".join(tails)))
        outs.append(out.decode(errors="replace"))
    failed = [r for r, p in enumerate(procs) if p.returncode != 0]
    assert not failed, "\n".join("rank %d failed (rc %d):\n%s" % (r, procs[r].returncode, outs[r][-1500:])
                                  for r in failed)
    return tmp


def load(tmp, i, r, dtype):
    got = np.load(os.path.join(tmp, "case%d_rank%d.npy" % (i, r)))
    info = json.load(open(os.path.join(tmp, "case%d_rank%d.json" % (i, r))))
    return np.frombuffer(got.tobytes(), dtype=O.NP_DTYPE[dtype]), info


def check_rs_case(tmp, i, c, world):
    """One "rs" case of a run: every rank's chunk and the bytes around it; returns the ranks' info."""
    dt = c["dtype"]
    inputs = [O.fill(c["count"], dt, c.get("seed", 0x5EED0000), r) for r in range(world)]
    loaded = [load(tmp, i, r, dt) for r in range(world)]
    assert_rs([g for g, _ in loaded], expected_rs(inputs, dt, c["op"]), inputs, dt, (i, c))
    return [info for _, info in loaded]


@pytest.mark.parametrize("world", [2, 3])
def test_mp_direct(world):
    """algo 6 between registered buffers: one small tile with head and tail, a
    buffer at an offset equal on every rank, several tiles, bytes; buffers
    that differ mod 16 fall back to the mesh on every rank; and a buffer whose
    lines the local L2s hold before the call, read back through a kernel."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cases = [
        {"kind": "rs", "count": 1001, "dtype": 6, "op": 2, "algo": 6},
        {"kind": "rs", "count": (1 << 20) + 3, "dtype": 10, "op": 0, "algo": 6, "pad": 6},
        {"kind": "rs", "count": 3 << 20, "dtype": 7, "op": 1, "algo": 6},
        {"kind": "rs", "count": 77777, "dtype": 1, "op": 3, "algo": 6},
        {"kind": "rs", "count": 262147, "dtype": 6, "op": 2, "algo": 6, "warm_l2": True, "seed": 0x5EEDF100},
        {"kind": "rs", "count": 100003, "dtype": 6, "op": 2, "algo": 6, "pad_per_rank": 4},
    ]
    tmp = run_mp(world, cases)
    for i, c in enumerate(cases):
        infos = check_rs_case(tmp, i, c, world)
        for info in infos:
            ll = info["launch"]
            assert ll[3] == 0, (i, ll)
            if "pad_per_rank" in c:
                assert ll[5] == 2 and ll[1] >= 1 and ll[2] >= 1, (i, ll)
                assert info["direct_fallback"] == info["direct_fallback_before"] + 1, (i, info)
            else:
                assert ll[5] == 6, (i, ll)
                assert info["direct_fallback"] == info["direct_fallback_before"], (i, info)
            assert info["direct_calls"] == info["direct_calls_before"] + 1, (i, info)
        assert len({info["direct_fallback"] for info in infos}) == 1, (i, infos)


def test_mp_auto_picks_direct_from_the_threshold():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cases = [{"kind": "rs", "count": 1 << 20, "dtype": 6, "op": 2, "algo": 0},
             {"kind": "rs", "count": 1000, "dtype": 6, "op": 2, "algo": 0}]
    results = {}
    for direct_bytes, want in (("1M", 6), ("0", 2)):
        tmp = run_mp(2, cases, env_extra={"RDC_DIRECT_BYTES": direct_bytes})
        infos = check_rs_case(tmp, 0, cases[0], 2)
        assert [info["launch"][5] for info in infos] == [want, want], (direct_bytes, infos)
        small = check_rs_case(tmp, 1, cases[1], 2)       # 4 KB: below the threshold, the mesh
        assert [info["launch"][5] for info in small] == [2, 2], (direct_bytes, small)
        results[direct_bytes] = [load(tmp, 0, r, 6)[0].tobytes() for r in range(2)]
    assert results["1M"] == results["0"]


CHAIN = [("rs", 2), ("ar", 1), ("rs", 2), ("rs", 2), ("ar", 2), ("rs", 2), ("ar", 3), ("rs", 2), ("ar", 4), ("rs", 2),
         ("ar", 5), ("rs", 2), ("bc", 1), ("rs", 2), ("ar", 0), ("rs", 0)]


def test_mp_back_to_back_launches_in_poison_mode():
    """The slot-reuse argument: a reduce-scatter's launch ends
    only after every peer's did, so whatever launch follows may rewrite the
    scratch slots at once.  16 launches on one int32 buffer without a host
    sync, consumed scratch poisoned: reduce-scatters between allreduces of
    every schedule, a broadcast, and another reduce-scatter; the buffer is
    refilled before each step and summed into an accumulator after it."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    world, count, seed = 3, 50001, 0x5EED7000
    case = {"kind": "chain", "count": count, "dtype": 2, "steps": CHAIN, "seed": seed}
    tmp = run_mp(world, [case])
    acc = [np.zeros(count, dtype=np.int32) for _ in range(world)]
    for k, (what, arg) in enumerate(CHAIN):
        xs = [O.fill(count, O.DT_INT32, seed + k, r) for r in range(world)]
        if what == "rs":
            step = expected_rs(xs, O.DT_INT32, O.OP_SUM)
        elif what == "ar":
            step = [x.copy() for x in xs]
            (O.allreduce_tree if arg == 4 else O.allreduce_ring)(step, O.DT_INT32, O.OP_SUM)
        else:
            step = [xs[arg]] * world
        for r in range(world):
            O.reducer(np.ascontiguousarray(step[r]), acc[r], O.DT_INT32, O.OP_SUM)
    for r in range(world):
        got, _ = load(tmp, 0, r, O.DT_INT32)
        assert got.tobytes() == acc[r].tobytes(), r


def test_mp_direct_then_scratch_schedules_on_one_buffer():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    world, count, dt, op = 3, 300007, O.DT_FLOAT32, O.OP_SUM
    steps = [("rs", 6), ("ar", 2), ("rs", 2), ("ar", 6)]
    tmp = run_mp(world, [{"kind": "algo_chain", "count": count, "dtype": dt, "op": op, "steps": steps}])
    state = [O.fill(count, dt, 0x5EED0000, r) for r in range(world)]
    for what, _ in steps:
        if what == "rs":
            state = expected_rs(state, dt, op)
        else:
            O.allreduce_ring(state, dt, op)
    for r in range(world):
        got, info = load(tmp, 0, r, dt)
        assert same_bits(got, state[r], dt), r
        assert info["direct_calls"] == info["direct_calls_before"] + 2, info
        assert info["direct_fallback"] == info["direct_fallback_before"], info


def test_mp_host_buffer_and_python_surface():
    """RdcReduceScatter on an ndarray inside a larger array of sentinel bytes:
    only the chunk is written.  Comm.reduce_scatter returns the view
    split_range names."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    world, count = 2, 100003
    cases = [{"kind": "host", "count": count, "dtype": 6, "op": 2},
             {"kind": "py", "count": count, "dtype": 6, "op": 2, "seed": 0x5EED7100}]
    tmp = run_mp(world, cases)
    chunks = [(int(b), int(e)) for b, e in O.split(count, world)]
    inputs = [O.fill(count, 6, 0x5EED0000, r) for r in range(world)]
    want = expected_rs(inputs, 6, 2)
    for r in range(world):
        backing = np.load(os.path.join(tmp, "case0_rank%d.npy" % r))
        info = json.load(open(os.path.join(tmp, "case0_rank%d.json" % r)))
        guard = (backing.size - count * 4) // 2
        assert guard == 4096 and (backing[:guard] == 0xA5).all() and (backing[guard + count * 4:] == 0xA5).all()
        got = np.frombuffer(backing[guard: guard + count * 4].tobytes(), dtype=np.float32)
        assert_rs([got if q == r else want[q] for q in range(world)], want, inputs, 6, ("host", r))
        assert info["view"] == [chunks[r][0], chunks[r][1] - chunks[r][0]], info
    infos = check_rs_case(tmp, 1, cases[1], world)
    for r, info in enumerate(infos):
        assert info["split_range"] == list(chunks[r]), info
        assert info["view"] == [chunks[r][0], chunks[r][1] - chunks[r][0]] and info["view_bytes_ok"], info
