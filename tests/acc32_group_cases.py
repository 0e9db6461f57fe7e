"""The single-process-group cases of the float32-accumulated Sum
(RdcCommAllreduceAcc32 / RdcCommReduceScatterAcc32 / RdcCommReduceToAcc32)
against the numpy restatement of its rule (tests/acc32_ref.py), bit for bit:
n communicators on GPU 0, one stream each, created once.  Every buffer sits
between 4 KiB of sentinel bytes which no rank may change; a reduce-scatter
leaves every byte outside chunk `rank` as passed, a rooted reduce every
non-root buffer.

pytest does not collect this file (its name is no test_*.py):
tests/test_gpu_acc32.py runs it once, in a process of its own, and reports
every case.  The ranks of a single-process group must each sit on a hardware
queue of their own, and which queue a stream gets depends on how many streams
the process has made before.  In the suite's process the streams of this file
would come first, and the groups that later modules create (some make a fresh
group per case) would get other queues than they get today: with these cases
in front, tests/test_gpu_allreduce.py::test_group_coalesced_mesh_unit_table
put both ranks of one of its groups on one queue and timed out.  In a process
of their own the cases change nothing for any other module, and they take the
three streams of group3 first, then the two of group2: with group2 first, two
ranks of group3 shared a queue.
"""
import ctypes

import numpy as np
import pytest

from oracle import oracle as O
from tests import acc32_ref as A
from tests import ops_ref
from tests.gpu_util import same_bits
from tests.test_gpu_reduce_scatter import last_launch, launch_counters, make_group
from tests.test_gpu_reduce_to import SENTINEL, guarded

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

F16, BF = O.DT_FLOAT16, O.DT_BFLOAT16


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


def group_of(request, n):
    """The module's group of n ranks, created at its first use.  The tests
    below take n = 3 first: ranks of one process must each sit on a hardware
    queue of their own (tests/test_gpu_allreduce.py), and the three streams of
    group3 get three fresh queues only while the process has opened no others."""
    return request.getfixturevalue("group%d" % n)


def expected(which, inputs, dtype, root=0):
    """Per rank, what the collective leaves in the buffer."""
    if which == "ar":
        return [A.allreduce(inputs, dtype)] * len(inputs)
    if which == "rs":
        return A.reduce_scatter(inputs, dtype)
    return A.reduce_to(inputs, dtype, root)


def launch(comms, which, bufs, count, dtype, root=0):
    from rdc_amd._lib import _LIB
    for r, (t, lo, _) in enumerate(bufs):
        p = ctypes.c_void_p(t.data_ptr() + lo)
        sp = ctypes.c_void_p(comms.streams[r].cuda_stream)
        if which == "ar":
            rc = _LIB.RdcCommAllreduceAcc32(comms[r].handle, p, count, dtype, sp)
        elif which == "rs":
            rc = _LIB.RdcCommReduceScatterAcc32(comms[r].handle, p, count, dtype, sp)
        else:
            rc = _LIB.RdcCommReduceToAcc32(comms[r].handle, p, count, dtype, root, sp)
        assert rc == 0, _LIB.RdcGetLastError()


def run_group(comms, which, inputs, dtype, root=0, pad_bytes=None):
    """Every rank's collective on its own stream; the guarded buffers back."""
    n = len(comms)
    bufs = [guarded(x, p) for x, p in zip(inputs, pad_bytes or [0] * n)]
    torch.cuda.synchronize()
    launch(comms, which, bufs, inputs[0].size, dtype, root)
    for r in range(n):
        comms[r].check(ctypes.c_void_p(comms.streams[r].cuda_stream))
    return bufs


def assert_result(which, bufs, inputs, want, dtype, root, what):
    """The rule's bits where the collective defines them, the caller's bytes
    everywhere else, and no sentinel byte changed."""
    n = len(inputs)
    chunks = O.split(inputs[0].size, n)
    for r, (t, lo, nbytes) in enumerate(bufs):
        host = t.cpu().numpy()
        assert (host[:lo] == SENTINEL).all() and (host[lo + nbytes:] == SENTINEL).all(), (what, "guards of rank", r)
        got = np.frombuffer(host[lo: lo + nbytes].tobytes(), dtype=O.NP_DTYPE[dtype])
        if which == "ar" or (which == "rt" and r == root):
            assert same_bits(got, want[r], dtype), (what, "result of rank", r)
        elif which == "rs":
            b, e = chunks[r]
            assert same_bits(got[b:e], want[r][b:e], dtype), (what, "chunk of rank", r)
            assert got[:b].tobytes() == inputs[r][:b].tobytes() and got[e:].tobytes() == inputs[r][e:].tobytes(), \
                (what, "bytes outside the chunk of rank", r)
        else:
            assert got.tobytes() == inputs[r].tobytes(), (what, "buffer of non-root rank", r)


def check_all(comms, inputs, dtype, what, pad_bytes=None, roots=None):
    """allreduce, reduce-scatter and the rooted reduce to each root on one set
    of inputs (the reference is computed once)."""
    n = len(comms)
    full = A.allreduce(inputs, dtype)
    ops_ref.assert_finite(full, dtype, what)
    rs = A.reduce_scatter(inputs, dtype)
    assert_result("ar", run_group(comms, "ar", inputs, dtype, 0, pad_bytes), inputs, [full] * n, dtype, 0,
                  (what, "ar"))
    assert_result("rs", run_group(comms, "rs", inputs, dtype, 0, pad_bytes), inputs, rs, dtype, 0, (what, "rs"))
    for root in (range(n) if roots is None else roots):
        want = [full if r == root else inputs[r] for r in range(n)]
        assert_result("rt", run_group(comms, "rt", inputs, dtype, root, pad_bytes), inputs, want, dtype, root,
                      (what, "rt", root))


# buffer offsets in bytes, per rank: aligned; 2 and 6 (the element-wise own ^ slot
# fold, heads and tails) mixed with aligned ranks; all at 16
OFFSETS = {2: [(0, 0), (2, 6), (6, 0), (16, 16)], 3: [(0, 0, 0), (2, 6, 0), (6, 2, 16), (16, 16, 16)]}


@pytest.mark.parametrize("dtype", A.DTYPES)
@pytest.mark.parametrize("n", [3, 2])
def test_group_counts_offsets_and_roots(request, n, dtype):
    """Counts 1 and n - 1 (empty chunks), 7, 1001 and 100003 (several tiles) at
    every offset set, all three collectives, every root."""
    comms = group_of(request, n)
    for k, count in enumerate((1, n - 1, 7, 1001, 100003)):
        inputs = A.gen_inputs(3100 + 10 * n + k + dtype, n, count, dtype)
        for pads in OFFSETS[n]:
            check_all(comms, inputs, dtype, (n, dtype, count, pads), pad_bytes=list(pads))


@pytest.mark.parametrize("dtype", A.DTYPES)
def test_group3_is_not_the_per_hop_sum(group3, dtype):
    """The data of the sweep above tell the rule from the ordinary Sum (the
    condition tests/test_acc32_plan.py checks for the generator), and the
    ordinary Sum on the same inputs still gives the oracle's per-hop bits."""
    from rdc_amd._lib import _LIB
    inputs = A.gen_inputs(3200 + dtype, 3, 100003, dtype)
    want = A.allreduce(inputs, dtype)
    ring = [np.array(x, copy=True) for x in inputs]
    O.allreduce_ring(ring, dtype, O.OP_SUM)
    assert (want.view(np.uint16) != ring[0].view(np.uint16)).mean() >= 0.02
    bufs = [guarded(x, 0) for x in inputs]
    torch.cuda.synchronize()
    for r in range(3):
        assert _LIB.RdcCommAllreduceEx(group3[r].handle, ctypes.c_void_p(bufs[r][0].data_ptr() + bufs[r][1]), 100003,
                                       dtype, O.OP_SUM, 2, ctypes.c_void_p(group3.streams[r].cuda_stream)) == 0
    for r in range(3):
        group3[r].check(ctypes.c_void_p(group3.streams[r].cuda_stream))
    assert_result("ar", bufs, inputs, ring, dtype, 0, "ordinary Sum")
    sibling = [last_launch(c) for c in group3]
    assert_result("ar", run_group(group3, "ar", inputs, dtype), inputs, [want] * 3, dtype, 0, "acc32")
    # RdcCommLastLaunch reports what the mesh sibling reports
    assert [last_launch(c) for c in group3] == sibling


@pytest.mark.parametrize("dtype", A.DTYPES)
def test_group3_order_table(group3, dtype):
    """The crafted cancellation rows: a fold in any other order fails here
    (tests/test_acc32_plan.py shows it on the CPU)."""
    for count, pads in ((None, (0, 0, 0)), (1001, (2, 0, 6))):
        check_all(group3, A.order_table(3, dtype, count=count), dtype, ("order table", dtype, count),
                  pad_bytes=list(pads))


@pytest.mark.parametrize("dtype", A.DTYPES)
@pytest.mark.parametrize("n", [3, 2])
def test_group_specials(request, n, dtype):
    """+-0, +-inf, inf - inf (a NaN), subnormals of both formats, the largest
    finite values, on the vector path and the element-wise one."""
    comms = group_of(request, n)
    inputs = A.specials(n, dtype)
    full = A.allreduce(inputs, dtype)
    assert ops_ref.is_nan(full, dtype).any() and ops_ref.is_inf(full, dtype).any()
    for pads in ([0] * n, [2] + [0] * (n - 1)):
        for which, root in (("ar", 0), ("rs", 0), ("rt", n - 1)):
            bufs = run_group(comms, which, inputs, dtype, root, pads)
            assert_result(which, bufs, inputs, expected(which, inputs, dtype, root), dtype, root,
                          ("specials", n, dtype, which, pads))


@pytest.mark.parametrize("which,dtype,root", [("ar", F16, 0), ("rs", BF, 0), ("rt", BF, 1)])
def test_group_multi_piece(group2, which, dtype, root):
    """A chunk larger than a scratch slot goes through several launches."""
    count = (6 << 20) // 2 * 3 + 7   # 18 MiB > 2 x 4 MiB slots
    inputs = A.gen_inputs(3300 + dtype, 2, count, dtype)
    before = launch_counters(group2)
    bufs = run_group(group2, which, inputs, dtype, root, [0, 6])
    after = launch_counters(group2)
    assert after[0] - before[0] >= 2 and after[0] == after[1], (before, after)
    assert_result(which, bufs, inputs, expected(which, inputs, dtype, root), dtype, root, ("multi-piece", which))


@pytest.mark.parametrize("s16,r16,grid,tile", [(1, 14, 0, 0), (7, 1, 24, 64 << 10)])
def test_group_tuned_shapes_stay_exact(group3, s16, r16, grid, tile):
    try:
        for c in group3:
            c.tune(s16, r16, grid, tile)
        for dtype in A.DTYPES:
            inputs = A.gen_inputs(3400 + s16 + dtype, 3, 300007, dtype)
            full = A.allreduce(inputs, dtype)
            for which, root in (("ar", 0), ("rs", 0), ("rt", 2)):
                want = {"ar": [full] * 3, "rs": A.reduce_scatter(inputs, dtype),
                        "rt": [full if r == root else inputs[r] for r in range(3)]}[which]
                bufs = run_group(group3, which, inputs, dtype, root, [0, 2, 4])
                assert_result(which, bufs, inputs, want, dtype, root, (s16, r16, grid, tile, which, dtype))
                for c in group3:
                    ll = last_launch(c)
                    assert ll[5] == 2 and (grid == 0 or ll[0] <= grid) and (tile == 0 or ll[4] == tile), ll
    finally:
        for c in group3:
            c.tune()


def test_group_refusals_launch_nothing(group3):
    from rdc_amd._lib import _LIB
    inputs = A.gen_inputs(3500, 3, 1001, BF)
    bufs = [guarded(x, 0) for x in inputs]
    torch.cuda.synchronize()
    before = launch_counters(group3)
    for r, c in enumerate(group3):
        p = ctypes.c_void_p(bufs[r][0].data_ptr() + bufs[r][1])
        for dt in list(range(10)) + [12, 13, 16, 17, 99]:
            for rc in (_LIB.RdcCommAllreduceAcc32(c.handle, p, 1001, dt, None),
                       _LIB.RdcCommReduceScatterAcc32(c.handle, p, 1001, dt, None),
                       _LIB.RdcCommReduceToAcc32(c.handle, p, 1001, dt, 0, None)):
                assert rc != 0
            assert _LIB.RdcGetLastError() == \
                ("rdc: float32-accumulated Sum needs float16 or bfloat16, got dtype %d" % dt).encode()
        for root in (-1, 3):
            assert _LIB.RdcCommReduceToAcc32(c.handle, p, 1001, BF, root, None) != 0
            assert b"root" in _LIB.RdcGetLastError()
        odd = ctypes.c_void_p(p.value + 1)
        assert _LIB.RdcCommAllreduceAcc32(c.handle, odd, 1000, BF, None) != 0 and b"aligned" in _LIB.RdcGetLastError()
        assert _LIB.RdcCommReduceScatterAcc32(c.handle, odd, 1000, F16, None) != 0
        assert _LIB.RdcCommReduceToAcc32(c.handle, odd, 1000, F16, 0, None) != 0
        assert _LIB.RdcCommAllreduceAcc32(c.handle, None, 1001, BF, None) != 0 and b"null" in _LIB.RdcGetLastError()
        # count 0 succeeds and consumes no launch number
        assert _LIB.RdcCommAllreduceAcc32(c.handle, None, 0, BF, None) == 0
        assert _LIB.RdcCommReduceScatterAcc32(c.handle, p, 0, F16, None) == 0
        assert _LIB.RdcCommReduceToAcc32(c.handle, None, 0, BF, 2, None) == 0
    torch.cuda.synchronize()
    assert launch_counters(group3) == before
    # an ordinary Sum on the same buffers afterwards still gives the oracle's bits
    for r in range(3):
        assert _LIB.RdcCommAllreduceEx(group3[r].handle, ctypes.c_void_p(bufs[r][0].data_ptr() + bufs[r][1]), 1001, BF,
                                       O.OP_SUM, 0, ctypes.c_void_p(group3.streams[r].cuda_stream)) == 0
    for r in range(3):
        group3[r].check(ctypes.c_void_p(group3.streams[r].cuda_stream))
    assert_result("ar", bufs, inputs, [O.expected_allreduce(inputs, BF, O.OP_SUM)] * 3, BF, 0, "Sum after refusals")
    after = launch_counters(group3)
    assert after == [b + 1 for b in before], (before, after)


def test_group_graph_capture_replay(group2):
    """A captured RdcCommAllreduceAcc32 replays with fresh inputs (the launch
    numbers live on the device); an eager ordinary Sum interleaves."""
    import rdc_amd
    count = 300007
    ts = [torch.zeros(count, dtype=torch.bfloat16, device="cuda") for _ in range(2)]
    graphs = []
    torch.cuda.synchronize()
    for r in range(2):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=group2.streams[r], capture_error_mode="thread_local"):
            group2[r].allreduce(ts[r], rdc_amd.Op.SUM, stream=ctypes.c_void_p(group2.streams[r].cuda_stream),
                                accumulate="float32")
        graphs.append(g)
    torch.cuda.synchronize()

    def replay(tag):
        xs = A.gen_inputs(3600 + tag, 2, count, BF)
        for r in range(2):
            ts[r].view(torch.int16).copy_(torch.from_numpy(xs[r].view(np.int16)))
        torch.cuda.synchronize()
        for r in range(2):
            with torch.cuda.stream(group2.streams[r]):
                graphs[r].replay()
        for r in range(2):
            group2[r].check(ctypes.c_void_p(group2.streams[r].cuda_stream))
        want = A.allreduce(xs, BF)
        for r in range(2):
            got = ts[r].view(torch.int16).cpu().numpy().view(np.uint16)
            assert same_bits(got, want, BF), (tag, r)

    for it in range(3):
        replay(it)
    xs = A.gen_inputs(3650, 2, 1001, F16)
    for algo in (2, 0):
        from rdc_amd._lib import _LIB
        bufs = [guarded(x, 0) for x in xs]
        torch.cuda.synchronize()
        for r in range(2):
            assert _LIB.RdcCommAllreduceEx(group2[r].handle, ctypes.c_void_p(bufs[r][0].data_ptr() + bufs[r][1]), 1001,
                                           F16, O.OP_SUM, algo, ctypes.c_void_p(group2.streams[r].cuda_stream)) == 0
        for r in range(2):
            group2[r].check(ctypes.c_void_p(group2.streams[r].cuda_stream))
        # two ranks: the ordinary Sum and the rule are the same bits
        assert_result("ar", bufs, xs, [A.allreduce(xs, F16)] * 2, F16, 0, ("eager Sum", algo))
    replay(9)
    ctr = launch_counters(group2)
    assert ctr[0] == ctr[1], ("launch counters differ", ctr)


