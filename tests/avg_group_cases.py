"""The single-process-group cases of Avg, the mean across ranks
(RdcCommAllreduceAvg / RdcCommReduceScatterAvg / RdcCommReduceToAvg) against
the numpy restatement of its rule (tests/avg_ref.py), bit for bit, for float32,
float64, float16 and bfloat16: n communicators on GPU 0, one stream each,
created once.  Every buffer sits between 4 KiB of sentinel bytes which no rank
may change; a reduce-scatter leaves every byte outside chunk `rank` as passed,
a rooted reduce every non-root buffer.

pytest does not collect this file (its name is no test_*.py):
tests/test_gpu_avg.py runs it once, in a process of its own, and reports every
case, for the reason tests/acc32_group_cases.py gives (which hardware queue a
stream gets depends on how many streams the process made before).  The cases
take the three streams of group3 first, then the two of group2.
"""
import ctypes

import numpy as np
import pytest

from oracle import oracle as O
from tests import avg_ref as A
from tests import ops_ref
from tests.gpu_util import same_bits
from tests.test_gpu_reduce_scatter import last_launch, launch_counters, make_group
from tests.test_gpu_reduce_to import SENTINEL, guarded

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

F32, F64, F16, BF = A.F32, A.F64, A.F16, A.BF


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
            rc = _LIB.RdcCommAllreduceAvg(comms[r].handle, p, count, dtype, sp)
        elif which == "rs":
            rc = _LIB.RdcCommReduceScatterAvg(comms[r].handle, p, count, dtype, sp)
        else:
            rc = _LIB.RdcCommReduceToAvg(comms[r].handle, p, count, dtype, root, sp)
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


# buffer offsets in bytes, per rank, by element size: aligned; one element and
# 2 / 6 bytes off 16-byte alignment (the element-wise own ^ slot fold, heads
# and tails) mixed with aligned ranks; all at 16.  float32 / float64 buffers
# must stay aligned to their element: 4 / 12 and 8 bytes there
OFFSETS = {2: {2: [(0, 0), (2, 6), (6, 0), (16, 16)], 3: [(0, 0, 0), (2, 6, 0), (6, 2, 16), (16, 16, 16)]},
           4: {2: [(0, 0), (4, 12), (12, 0), (16, 16)], 3: [(0, 0, 0), (4, 12, 0), (12, 4, 16), (16, 16, 16)]},
           8: {2: [(0, 0), (8, 8), (8, 0), (16, 16)], 3: [(0, 0, 0), (8, 8, 0), (8, 0, 16), (16, 16, 16)]}}


def pads_of(dtype, n, k):
    """offset set k of OFFSETS for this dtype's element size"""
    return list(OFFSETS[A.ESIZE[dtype]][n][k])


@pytest.mark.parametrize("dtype", A.DTYPES)
@pytest.mark.parametrize("n", [3, 2])
def test_group_counts_offsets_and_roots(request, n, dtype):
    """Counts 0, 1 and n - 1 (empty chunks), 7, 1001 and 65537 (several tiles)
    at every offset set, all three collectives, every root."""
    comms = group_of(request, n)
    for k, count in enumerate((0, 1, n - 1, 7, 1001, 65537)):
        inputs = A.gen_inputs(4100 + 10 * n + k + dtype, n, count, dtype)
        for j in range(4):
            pads = pads_of(dtype, n, j)
            check_all(comms, inputs, dtype, (n, dtype, count, pads), pad_bytes=pads)


@pytest.mark.parametrize("dtype", A.DTYPES)
def test_group3_is_not_sum_then_divide(group3, dtype):
    """The generator's data tell the rule from what a caller did before (the
    condition tests/test_avg_plan.py checks): the sum rounded to 16 bits and
    divided in a second pass, or, for float32 / float64, the sum multiplied by
    a rounded 1 / 3.  The mesh Sum on the same inputs still gives the oracle's
    bits, and RdcCommLastLaunch reports for Avg what it reports for that Sum."""
    from rdc_amd._lib import _LIB
    inputs = A.gen_inputs(4200 + dtype, 3, 65537, dtype)
    want = A.allreduce(inputs, dtype)
    other = A.sum_times_reciprocal(inputs, dtype) if dtype in A.WIDE else A.sum_round_then_divide(inputs, dtype)
    assert (A.bits(want, dtype) != A.bits(other, dtype)).mean() >= 0.01
    ring = [np.array(x, copy=True) for x in inputs]
    O.allreduce_ring(ring, dtype, O.OP_SUM)
    bufs = [guarded(x, 0) for x in inputs]
    torch.cuda.synchronize()
    for r in range(3):
        assert _LIB.RdcCommAllreduceEx(group3[r].handle, ctypes.c_void_p(bufs[r][0].data_ptr() + bufs[r][1]), 65537,
                                       dtype, O.OP_SUM, 2, ctypes.c_void_p(group3.streams[r].cuda_stream)) == 0
    for r in range(3):
        group3[r].check(ctypes.c_void_p(group3.streams[r].cuda_stream))
    assert_result("ar", bufs, inputs, ring, dtype, 0, "ordinary Sum")
    sibling = [last_launch(c) for c in group3]
    assert_result("ar", run_group(group3, "ar", inputs, dtype), inputs, [want] * 3, dtype, 0, "avg")
    assert [last_launch(c) for c in group3] == sibling and sibling[0][5] == 2


@pytest.mark.parametrize("dtype", A.DTYPES)
def test_group3_order_table(group3, dtype):
    """The crafted cancellation rows: a fold in any other order fails here
    (tests/test_avg_plan.py shows it on the CPU)."""
    for count, k in ((None, 0), (1001, 2)):
        check_all(group3, A.order_table(3, dtype, count=count), dtype, ("order table", dtype, count),
                  pad_bytes=pads_of(dtype, 3, k))


@pytest.mark.parametrize("dtype", A.DTYPES)
@pytest.mark.parametrize("n", [3, 2])
def test_group_specials(request, n, dtype):
    """+-0, +-inf, inf - inf (a NaN), subnormals of the format, the largest
    finite values and the float16 row whose Sum overflows while its mean does
    not, on the vector path and the element-wise one."""
    comms = group_of(request, n)
    inputs = A.specials(n, dtype)
    full = A.allreduce(inputs, dtype)
    assert ops_ref.is_nan(full, dtype).any() and ops_ref.is_inf(full, dtype).any()
    if dtype == F16:   # 40000.0 on every rank: the mean is 40000.0, not inf
        assert (full[-(n + 1):] == np.float16(40000.0)).all()
    for pads in ([0] * n, [A.ESIZE[dtype]] + [0] * (n - 1)):
        for which, root in (("ar", 0), ("rs", 0), ("rt", n - 1)):
            bufs = run_group(comms, which, inputs, dtype, root, pads)
            assert_result(which, bufs, inputs, expected(which, inputs, dtype, root), dtype, root,
                          ("specials", n, dtype, which, pads))


@pytest.mark.parametrize("which,dtype,root", [("ar", F32, 0), ("rs", BF, 0), ("rt", F64, 1), ("ar", F16, 0)])
def test_group_multi_piece(group2, which, dtype, root):
    """A chunk larger than a scratch slot goes through several launches."""
    count = (18 << 20) // A.ESIZE[dtype] + 7   # 18 MiB > 2 x 4 MiB slots
    inputs = A.gen_inputs(4300 + dtype, 2, count, dtype)
    before = launch_counters(group2)
    bufs = run_group(group2, which, inputs, dtype, root, [0, A.ESIZE[dtype]])
    after = launch_counters(group2)
    assert after[0] - before[0] >= 2 and after[0] == after[1], (before, after)
    assert_result(which, bufs, inputs, expected(which, inputs, dtype, root), dtype, root, ("multi-piece", which))


@pytest.mark.parametrize("s16,r16,grid,tile", [(1, 14, 0, 0), (7, 1, 24, 64 << 10)])
def test_group_tuned_shapes_stay_exact(group3, s16, r16, grid, tile):
    try:
        for c in group3:
            c.tune(s16, r16, grid, tile)
        for dtype in A.DTYPES:
            inputs = A.gen_inputs(4400 + s16 + dtype, 3, 100003, dtype)
            full = A.allreduce(inputs, dtype)
            for which, root in (("ar", 0), ("rs", 0), ("rt", 2)):
                want = {"ar": [full] * 3, "rs": A.reduce_scatter(inputs, dtype),
                        "rt": [full if r == root else inputs[r] for r in range(3)]}[which]
                bufs = run_group(group3, which, inputs, dtype, root, pads_of(dtype, 3, 2))
                assert_result(which, bufs, inputs, want, dtype, root, (s16, r16, grid, tile, which, dtype))
                for c in group3:
                    ll = last_launch(c)
                    assert ll[5] == 2 and (grid == 0 or ll[0] <= grid) and (tile == 0 or ll[4] == tile), ll
    finally:
        for c in group3:
            c.tune()


def test_group_refusals_launch_nothing(group3):
    from rdc_amd._lib import _LIB
    inputs = A.gen_inputs(4500, 3, 1001, BF)
    bufs = [guarded(x, 0) for x in inputs]
    torch.cuda.synchronize()
    before = launch_counters(group3)
    for r, c in enumerate(group3):
        p = ctypes.c_void_p(bufs[r][0].data_ptr() + bufs[r][1])
        for dt in [0, 1, 2, 3, 4, 5, 8, 9, 12, 13, 14, 15, 16, 17, 99, -1]:
            for rc in (_LIB.RdcCommAllreduceAvg(c.handle, p, 1001, dt, None),
                       _LIB.RdcCommReduceScatterAvg(c.handle, p, 1001, dt, None),
                       _LIB.RdcCommReduceToAvg(c.handle, p, 1001, dt, 0, None)):
                assert rc != 0
            assert _LIB.RdcGetLastError() == \
                ("rdc: Avg takes float32, float64, float16 or bfloat16, got dtype %d" % dt).encode()
        for root in (-1, 3):
            assert _LIB.RdcCommReduceToAvg(c.handle, p, 1001, BF, root, None) != 0
            assert b"root" in _LIB.RdcGetLastError()
        odd = ctypes.c_void_p(p.value + 1)
        assert _LIB.RdcCommAllreduceAvg(c.handle, odd, 1000, BF, None) != 0 and b"aligned" in _LIB.RdcGetLastError()
        assert _LIB.RdcCommReduceScatterAvg(c.handle, odd, 1000, F16, None) != 0
        assert _LIB.RdcCommReduceToAvg(c.handle, odd, 1000, F16, 0, None) != 0
        odd4 = ctypes.c_void_p(p.value + 2)   # element-aligned for 16 bits, not for float32 / float64
        assert _LIB.RdcCommAllreduceAvg(c.handle, odd4, 100, F32, None) != 0 and b"aligned" in _LIB.RdcGetLastError()
        assert _LIB.RdcCommReduceToAvg(c.handle, ctypes.c_void_p(p.value + 4), 100, F64, 0, None) != 0
        assert _LIB.RdcCommAllreduceAvg(c.handle, None, 1001, BF, None) != 0 and b"null" in _LIB.RdcGetLastError()
        # count 0 succeeds and consumes no launch number
        assert _LIB.RdcCommAllreduceAvg(c.handle, None, 0, BF, None) == 0
        assert _LIB.RdcCommReduceScatterAvg(c.handle, p, 0, F16, None) == 0
        assert _LIB.RdcCommReduceToAvg(c.handle, None, 0, BF, 2, None) == 0
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
    """One captured graph per rank holding RdcCommAllreduceAvg,
    RdcCommReduceScatterAvg and RdcCommReduceToAvg on three tensors replays
    with fresh inputs (the launch numbers live on the device); an eager
    ordinary Sum interleaves."""
    import rdc_amd
    from rdc_amd._lib import _LIB
    count, root = 100003, 1
    tdt = {F32: torch.float32, BF: torch.bfloat16}
    for dtype in (F32, BF):
        ts = [[torch.zeros(count, dtype=tdt[dtype], device="cuda") for _ in range(3)] for _ in range(2)]
        graphs = []
        torch.cuda.synchronize()
        for r in range(2):
            g = torch.cuda.CUDAGraph()
            sp = ctypes.c_void_p(group2.streams[r].cuda_stream)
            with torch.cuda.graph(g, stream=group2.streams[r], capture_error_mode="thread_local"):
                group2[r].allreduce(ts[r][0], rdc_amd.Op.SUM, stream=sp, average=True)
                group2[r].reduce_scatter(ts[r][1], rdc_amd.Op.SUM, stream=sp, average=True)
                group2[r].reduce(ts[r][2], rdc_amd.Op.SUM, root, stream=sp, average=True)
            graphs.append(g)
        torch.cuda.synchronize()

        def replay(tag):
            xs = A.gen_inputs(4600 + tag + dtype, 2, count, dtype)
            raw = np.int32 if dtype == F32 else np.int16
            for r in range(2):
                for t in ts[r]:
                    t.view(torch.int32 if dtype == F32 else torch.int16).copy_(torch.from_numpy(xs[r].view(raw)))
            torch.cuda.synchronize()
            for r in range(2):
                with torch.cuda.stream(group2.streams[r]):
                    graphs[r].replay()
            for r in range(2):
                group2[r].check(ctypes.c_void_p(group2.streams[r].cuda_stream))
            full = A.allreduce(xs, dtype)
            want = {0: [full] * 2, 1: A.reduce_scatter(xs, dtype), 2: A.reduce_to(xs, dtype, root)}
            for r in range(2):
                for k in range(3):
                    got = ts[r][k].view(torch.int32 if dtype == F32 else torch.int16).cpu().numpy().view(xs[r].dtype)
                    assert same_bits(got, want[k][r], dtype), (tag, dtype, r, k)

        for it in range(2):
            replay(it)
        xs = A.gen_inputs(4650, 2, 1001, F32)
        bufs = [guarded(x, 0) for x in xs]
        torch.cuda.synchronize()
        for r in range(2):
            assert _LIB.RdcCommAllreduceEx(group2[r].handle, ctypes.c_void_p(bufs[r][0].data_ptr() + bufs[r][1]), 1001,
                                           F32, O.OP_SUM, 0, ctypes.c_void_p(group2.streams[r].cuda_stream)) == 0
        for r in range(2):
            group2[r].check(ctypes.c_void_p(group2.streams[r].cuda_stream))
        assert_result("ar", bufs, xs, [O.expected_allreduce(xs, F32, O.OP_SUM)] * 2, F32, 0, "eager Sum")
        replay(9)
        ctr = launch_counters(group2)
        assert ctr[0] == ctr[1], ("launch counters differ", ctr)
