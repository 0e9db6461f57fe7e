"""GPU: Prod / BitAND / BitXOR (ops 8 / 9 / 10) on the device path, bit for bit
against the numpy restatement tests/ops_ref.py (ring, tree and scan orders;
tests/test_ops_plan.py ties those to the oracle).

Float inputs of the collective tests come from ops_ref.gen_input: random signs,
magnitudes in [0.5, 2) with full random mantissas, so a product of 8 stays
finite and every step rounds; each such test asserts that its expected data
holds no NaN and no inf, because gpu_util.same_bits treats any two NaNs as
equal.  Integer inputs are full range.

* RdcReduce: every (dtype, op), the whole domain of the byte product and of
  the half-precision products against 16 fixed factors;
* single-process groups of 2 and 3 (RdcCommInitAll on GPU 0), created once;
* multi-process: 4 and 8 processes on GPU 0, tests/mp_ops_worker.py;
* C++ through the launcher: tests/cpp/ops.cc.
"""
import ctypes
import functools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O
from tests import ops_ref as R
from tests.conftest import ROOT
from tests.gpu_util import from_dev, ptr, same_bits, to_dev
from tests.test_gpu_loc import back, dptr, guarded, launch_all
from tests.test_gpu_reduce_scatter import Group, launch_counters, run_mp

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

WORKER = os.path.join(ROOT, "tests", "mp_ops_worker.py")
ALGOS = {"ring": 1, "mesh": 2, "mesh_pull": 5, "oneshot": 3, "tree": 4, "auto": 0}
COUNTS = (1001, 100003)  # head / tail elements, the 16-B body, uneven Split chunks; several tiles at the larger
IDS = ["dt%d-op%d" % p for p in R.NEW_VALID]


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rdc_amd._lib import _LIB
    return _LIB


class OwnStream(object):
    """A HIP stream of this module's own, with the one attribute the helpers
    read.  torch.cuda.Stream() hands out the streams of a fixed pool in turn,
    and the other GPU test modules take their ranks' streams from it: a module
    that drew from the pool too would change which pool streams, with the
    hardware queues those were given at their first use, every later module's
    groups land on (the ranks of a group need a queue each).
    These streams are destroyed with the module, which returns their queues."""

    def __init__(self, hip):
        p = ctypes.c_void_p()
        assert hip.hipStreamCreate(ctypes.byref(p)) == 0
        self.hip, self.cuda_stream = hip, p.value

    def destroy(self):
        assert self.hip.hipStreamDestroy(ctypes.c_void_p(self.cuda_stream)) == 0


class Groups(object):
    """The groups of 3 and of 2, each created at its first use and in that
    order, as in the other GPU test modules, each rank on a stream of its own."""

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
    torch.cuda.synchronize()
    for comms in g.made.values():
        for c in comms:
            c.destroy()
        for st in comms.streams:
            st.destroy()


def esize(dtype):
    return np.dtype(O.NP_DTYPE[dtype]).itemsize


def equal(got_bytes, want, dtype):
    got = np.frombuffer(got_bytes, dtype=want.dtype)
    return same_bits(got, want, dtype)


@functools.lru_cache(maxsize=None)
def case(n, dtype, op, count):
    """(inputs, ring result, tree result), computed once per shape and left
    unchanged; float results hold no NaN and no inf."""
    xs = R.gen_inputs(7000 + 1000 * n + 16 * dtype + op, n, count, dtype)
    ring, tree = R.ring(xs, op, dtype), R.tree(xs, op, dtype)
    R.assert_finite(ring, dtype, (n, dtype, op, count))
    R.assert_finite(tree, dtype, (n, dtype, op, count))
    for a in xs + [ring, tree]:
        a.setflags(write=False)
    return xs, ring, tree


def run_reduce(lib, d, s, dtype, op, pd, ps):
    """RdcReduce on dst / src at byte offsets pd / ps; returns the new dst."""
    td, ts = to_dev(d, pd), to_dev(s, ps)
    assert lib.RdcReduce(ptr(td, pd), ptr(ts, ps), d.size, dtype, op, None) == 0, lib.RdcGetLastError()
    torch.cuda.synchronize()
    assert from_dev(ts, ps, s.size, dtype).tobytes() == s.tobytes()
    return from_dev(td, pd, d.size, dtype)


# ------------------------------------------------------------- 1. RdcReduce --
@pytest.mark.parametrize("dtype,op", R.NEW_VALID, ids=IDS)
def test_reduce_every_dtype_and_op(lib, dtype, op):
    """count 1001, dst and src at congruent and at incongruent misaligned
    offsets (the 16-B body after a head, then the element-wise path)."""
    rng = np.random.default_rng(1700 + 16 * dtype + op)
    d, s = R.gen_input(rng, 1001, dtype), R.gen_input(rng, 1001, dtype)
    want = R.apply(op, d, s, dtype)
    R.assert_finite(want, dtype)
    e = esize(dtype)
    for pd, ps in ((0, 0), (4 * e, 4 * e), (2 * e, 6 * e)):
        got = run_reduce(lib, d, s, dtype, op, pd, ps)
        assert same_bits(got, want, dtype), (dtype, op, pd, ps)


@pytest.mark.parametrize("dtype", [O.DT_INT8, O.DT_UINT8])
def test_reduce_byte_product_whole_domain(lib, dtype):
    """All 65,536 (d, s) byte pairs in one 64 KiB call (the four-lanes-per-dword
    product's whole domain), 16-B body and, at offset 3, head and tail too."""
    npd = O.NP_DTYPE[dtype]
    g = np.arange(256, dtype=np.uint8).view(npd)
    d, s = np.repeat(g, 256), np.tile(g, 256)
    want = R.apply(R.OP_PROD, d, s, dtype)
    assert want.view(np.uint8).tolist() == [(a * b) & 0xFF for a in range(256) for b in range(256)]
    for pad in (0, 3):
        got = run_reduce(lib, d, s, dtype, R.OP_PROD, pad, pad)
        assert got.tobytes() == want.tobytes(), (dtype, pad)


def half_factors(dtype):
    """16 fixed factors, as bits: 1, -1, 1 + ulp, -(1 + ulp), the largest value
    below 1, 0.75, 3, the largest finite, the smallest normal, the smallest
    subnormal, 2^-7, +0, -0, +inf, -inf and one quiet NaN."""
    if dtype == O.DT_FLOAT16:
        return np.array([0x3C00, 0xBC00, 0x3C01, 0xBC01, 0x3BFF, 0x3A00, 0x4200, 0x7BFF, 0x0400, 0x0001, 0x2000,
                         0x0000, 0x8000, 0x7C00, 0xFC00, 0x7E00], dtype=np.uint16)
    return np.array([0x3F80, 0xBF80, 0x3F81, 0xBF81, 0x3F7F, 0x3F40, 0x4040, 0x7F7F, 0x0080, 0x0001, 0x3C00,
                     0x0000, 0x8000, 0x7F80, 0xFF80, 0x7FC0], dtype=np.uint16)


@pytest.mark.parametrize("dtype", [O.DT_BFLOAT16, O.DT_FLOAT16])
def test_reduce_half_product_every_bit_pattern(lib, dtype):
    """Every one of the 65,536 bit patterns as d against 16 fixed factors
    (half_factors), 1 Mi elements, with same_bits: overflow to inf, underflow
    into subnormals and to zero, the sign of zero, inf x 0 and NaN in either
    operand.

    NaN share of the reference, computed on the CPU: 6.61 % for bfloat16 and
    9.18 % for float16.  It cannot be below 2 % with these cases: one factor in
    16 is a NaN (6.25 % of the elements by itself), and 254 (bfloat16) / 2046
    (float16, 3.1 %) of the 65,536 patterns of d are NaNs.  What is asserted
    instead, so that same_bits cannot hide anything but a payload: every NaN of
    the reference comes from a NaN operand or from inf x 0, those are all of
    them, the share of NaNs that no NaN operand explains (inf x 0) is below
    2 % (it is 0.0008 %), and same_bits itself requires the device's NaNs to
    sit at exactly the reference's positions."""
    f = half_factors(dtype)
    d16, s16 = np.tile(np.arange(65536, dtype=np.uint16), 16), np.repeat(f, 65536)
    npd = O.NP_DTYPE[dtype]
    d, s = d16.view(npd), s16.view(npd)
    want = R.apply(R.OP_PROD, d, s, dtype)
    nan_in = R.is_nan(d, dtype) | R.is_nan(s, dtype)
    zero = lambda a: (a.view(np.uint16) & 0x7FFF) == 0  # noqa: E731
    inf_zero = (R.is_inf(d, dtype) & zero(s)) | (zero(d) & R.is_inf(s, dtype))
    nan_out = R.is_nan(want, dtype)
    assert np.array_equal(nan_out, nan_in | inf_zero)
    assert (nan_out & ~nan_in).mean() < 0.02
    print("NaN share of the reference: %.4f %%, without a NaN operand: %.4f %%"
          % (100 * nan_out.mean(), 100 * (nan_out & ~nan_in).mean()))
    w16 = want.view(np.uint16)
    assert R.is_inf(want[~R.is_inf(d, dtype) & ~R.is_inf(s, dtype)], dtype).any()      # overflow
    sub = (w16 & 0x7FFF) < (0x0400 if dtype == O.DT_FLOAT16 else 0x0080)
    assert (sub & ((w16 & 0x7FFF) != 0) & ~zero(d)).any() and (sub & zero(want) & ~zero(d) & ~zero(s)).any()
    assert (w16 == 0x8000).any() and (w16 == 0).any()
    for pad in (0, 6):
        got = run_reduce(lib, d, s, dtype, R.OP_PROD, pad, pad)
        assert same_bits(got, want, dtype), (dtype, pad)


def wide_special(dtype):
    """4096 random pairs of wide magnitude plus a table of explicit cases."""
    npd = np.dtype(O.NP_DTYPE[dtype])
    fi = np.finfo(npd)
    rng = np.random.default_rng(4242 + dtype)
    span = 30 if dtype == O.DT_FLOAT32 else 250
    d = (rng.standard_normal(4096) * 10.0 ** rng.integers(-span, span, 4096)).astype(npd)
    s = (rng.standard_normal(4096) * 10.0 ** rng.integers(-span, span, 4096)).astype(npd)
    one, sub = npd.type(1), fi.smallest_subnormal
    table = [
        (fi.tiny, 0.5),                 # 0: a subnormal result, exact
        (sub * 3, 0.5),                 # 1: 1.5 units of the least subnormal: a tie, to even (2 units)
        (sub, 0.5),                     # 2: half a unit: a tie, to even (zero)
        (one + fi.eps, 1.5),            # 3: 1.5 + 1.5 eps: a tie, to even (up, 1.5 + 2 eps)
        (one + 3 * fi.eps, 1.5),        # 4: 1.5 + 4.5 eps: a tie, to even (down, 1.5 + 4 eps)
        (one + fi.eps, one + fi.eps),   # 5: 1 + 2 eps + eps^2 rounds down
        (fi.max, 2.0), (fi.max, -2.0),  # 6, 7: overflow to +-inf
        (fi.max, one + fi.eps),         # 8: overflow by rounding
        (-0.0, 5.0), (0.0, -5.0), (-0.0, -0.0),       # 9, 10, 11: the sign of zero
        (np.inf, 0.0), (np.nan, 1.0), (1.0, np.nan),  # 12, 13, 14: the only NaN results
        (np.inf, -1.0), (fi.tiny, fi.tiny),           # 15, 16: -inf; underflow to +0
    ]
    td = np.array([a for a, _ in table], dtype=npd)
    ts = np.array([b for _, b in table], dtype=npd)
    return np.concatenate([d, td]), np.concatenate([s, ts]), len(table)


@pytest.mark.parametrize("dtype", [O.DT_FLOAT32, O.DT_FLOAT64])
def test_reduce_float_product_wide_and_special(lib, dtype):
    """4096 random pairs of wide magnitude (results from subnormal to inf) and
    the table of wide_special: subnormal results, exact ties, overflow, the
    sign of zero.  NaN share of the reference: 3 elements of 4113, 0.07 %
    (asserted below 2 %)."""
    d, s, ntable = wide_special(dtype)
    want = R.apply(R.OP_PROD, d, s, dtype)
    assert np.isnan(want).mean() < 0.02 and np.isnan(want).sum() == 3
    t = want[-ntable:]
    fi = np.finfo(want.dtype)
    sub, eps = fi.smallest_subnormal, fi.eps
    assert t[0] == fi.tiny / 2 and t[1] == sub * 2 and t[2] == 0 and t[3] == 1.5 + 2 * eps and t[4] == 1.5 + 4 * eps
    assert t[5] == 1 + 2 * eps and t[6] == np.inf and t[7] == -np.inf and t[8] == np.inf
    assert t[9] == 0 and np.signbit(t[9]) and np.signbit(t[10]) and t[11] == 0 and not np.signbit(t[11])
    assert np.isnan(t[12:15]).all() and t[15] == -np.inf and t[16] == 0 and not np.signbit(t[16])
    assert ((np.abs(want[:4096]) < fi.tiny) & (want[:4096] != 0)).any() and np.isinf(want[:4096]).any()
    e = esize(dtype)
    for pd, ps in ((0, 0), (e, e), (e, 0)):
        got = run_reduce(lib, d, s, dtype, R.OP_PROD, pd, ps)
        assert same_bits(got, want, dtype), (dtype, pd, ps)


# ---------------------------------------------------------------- 2. groups --
@pytest.mark.parametrize("dtype,op", R.NEW_VALID, ids=IDS)
def test_group_allreduce_every_schedule(groups, dtype, op):
    """Groups of 2 and 3, both counts, every schedule the group reaches: every
    rank holds ops_ref's bits, the ring order's for every schedule but the
    tree.  float32 Prod at n = 3 also differs from a left-to-right product, so
    the test shows the order and not only the operator."""
    from rdc_amd._lib import _LIB
    e = esize(dtype)
    for n, comms in groups.items():
        for count in COUNTS:
            xs, ring, tree = case(n, dtype, op, count)
            if dtype == O.DT_FLOAT32 and op == R.OP_PROD and n == 3:
                assert (ring != R.left_to_right(list(xs), op, dtype)).any()
                assert (ring != tree).any()
            for algo, code in ALGOS.items():
                want = tree if algo == "tree" else ring
                pad = e if algo in ("ring", "oneshot") else 0  # base + one element: head and tail paths
                bufs = [guarded(x, pad) for x in xs]
                launch_all(comms, lambda r, sp: _LIB.RdcCommAllreduceEx(comms[r].handle, dptr(bufs[r]), count, dtype,
                                                                        op, code, sp))
                for r in range(n):
                    assert equal(back(bufs[r]), want, dtype), (n, dtype, op, algo, count, "rank", r)


@pytest.mark.parametrize("dtype,op", R.NEW_VALID, ids=IDS)
def test_group_reduce_scatter_reduce_to_scan(groups, dtype, op):
    """The same inputs through reduce-scatter (the rest of the buffer
    untouched), ReduceTo at a non-zero root (non-roots untouched), Scan and
    Exscan (rank 0 untouched)."""
    from rdc_amd._lib import _LIB
    e = esize(dtype)
    for n, comms in groups.items():
        for count in COUNTS:
            xs, ring, _ = case(n, dtype, op, count)
            pad = e if count % 2 else 0
            bufs = [guarded(x, pad) for x in xs]
            launch_all(comms, lambda r, sp: _LIB.RdcCommReduceScatter(comms[r].handle, dptr(bufs[r]), count, dtype,
                                                                      op, 0, sp))
            want = R.reduce_scatter(list(xs), op, dtype)
            for r in range(n):
                assert equal(back(bufs[r]), want[r], dtype), ("reduce-scatter", n, count, r)
            root = n - 1
            bufs = [guarded(x, pad) for x in xs]
            launch_all(comms, lambda r, sp: _LIB.RdcCommReduceTo(comms[r].handle, dptr(bufs[r]), count, dtype,
                                                                 op, root, sp))
            for r in range(n):
                assert equal(back(bufs[r]), ring if r == root else xs[r], dtype), ("reduce", n, count, root, r)
            for exclusive in (0, 1):
                want = R.scan(list(xs), op, bool(exclusive), dtype)
                for w in want:
                    R.assert_finite(w, dtype)
                bufs = [guarded(x, pad) for x in xs]
                launch_all(comms, lambda r, sp: _LIB.RdcCommScan(comms[r].handle, dptr(bufs[r]), count, dtype, op,
                                                                 exclusive, sp))
                for r in range(n):
                    assert equal(back(bufs[r]), want[r], dtype), ("scan", n, count, exclusive, r)


@pytest.mark.parametrize("dtype,op", R.NEW_VALID, ids=IDS)
def test_group_coalesced_allreduce(groups, dtype, op):
    """Five buffers of mixed small counts, each its own allocation, some at
    base + one element: one allreduce per buffer, bit for bit."""
    from rdc_amd._lib import _LIB
    e = esize(dtype)
    for n, comms in groups.items():
        counts = [1, n + 1, 1001, 4099, 3]
        cases = [case(n, dtype, op, k) for k in counts]
        pads = [0, e, e, 0, e]
        bufs = [[guarded(cases[b][0][r], pads[b]) for b in range(5)] for r in range(n)]

        def call(r, sp):
            arr = (ctypes.c_void_p * 5)(*[bufs[r][b][0].data_ptr() + bufs[r][b][1] for b in range(5)])
            cnt = (ctypes.c_size_t * 5)(*counts)
            return _LIB.RdcCommAllreduceCoalesced(comms[r].handle, arr, cnt, 5, dtype, op, 0, sp)
        launch_all(comms, call)
        for r in range(n):
            for b in range(5):
                assert equal(back(bufs[r][b]), cases[b][1], dtype), (n, "buffer", b, "rank", r)


# --------------------------------------------------------- 4. known answers --
def test_group_known_answers(groups):
    """Answers a reader can check by hand: XOR of one buffer on an even world
    is all zeros, BitAND of ~(1 << rank) clears exactly the low n bits, and an
    int32 Prod of rank + 1 is n!."""
    from rdc_amd._lib import _LIB
    count = 1001
    for n, comms in groups.items():
        same = (np.arange(count, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)).astype(np.uint32)
        sets = [(O.DT_UINT32, R.OP_BITAND, [np.full(count, ~(1 << r) & 0xFFFFFFFF, dtype=np.uint32) for r in range(n)],
                 np.full(count, 0xFFFFFFFF & ~((1 << n) - 1), dtype=np.uint32)),
                (O.DT_INT32, R.OP_PROD, [np.full(count, r + 1, dtype=np.int32) for r in range(n)],
                 np.full(count, math.factorial(n), dtype=np.int32)),
                (O.DT_UINT32, R.OP_BITXOR, [same] * n, np.zeros(count, dtype=np.uint32) if n % 2 == 0 else same)]
        for dtype, op, xs, want in sets:
            bufs = [guarded(x, 0) for x in xs]
            launch_all(comms, lambda r, sp: _LIB.RdcCommAllreduceEx(comms[r].handle, dptr(bufs[r]), count, dtype,
                                                                    op, 0, sp))
            for r in range(n):
                assert back(bufs[r]) == want.tobytes(), (n, dtype, op, r)


# -------------------------------------------------------------- 5. refusals --
def test_group_refusals_launch_nothing(groups):
    """A float dtype with BITXOR / BITAND and a pair dtype with PROD are
    refused before a launch: the launch counter stays."""
    from rdc_amd._lib import _LIB
    comms = groups[2]
    t = torch.zeros(256, dtype=torch.uint8, device="cuda")
    before = launch_counters(comms)
    p = ctypes.c_void_p(t.data_ptr())
    for dtype, op in ((6, 10), (11, 9), (12, 8), (13, 10), (2, 6), (6, 7), (2, 11)):
        # the communicator entries refuse by (dtype, op), as they do a float with BITOR
        assert _LIB.RdcCommAllreduce(comms[0].handle, p, 8, dtype, op, None) != 0, (dtype, op)
        assert b"unsupported (dtype, op) = (%d, %d)" % (dtype, op) in _LIB.RdcGetLastError(), _LIB.RdcGetLastError()
        assert _LIB.RdcCommScan(comms[0].handle, p, 8, dtype, op, 0, None) != 0
        assert _LIB.RdcCommReduceTo(comms[0].handle, p, 8, dtype, op, 0, None) != 0
        assert _LIB.RdcCommReduceScatter(comms[0].handle, p, 8, dtype, op, 0, None) != 0
        assert _LIB.RdcReduce(p, ctypes.c_void_p(t.data_ptr() + 64), 8, dtype, op, None) != 0
    assert launch_counters(comms) == before


# --------------------------------------------------------- 3. multi-process --
MP_OPS = [(O.DT_FLOAT32, R.OP_PROD), (O.DT_INT8, R.OP_PROD), (O.DT_UINT32, R.OP_BITAND), (O.DT_INT64, R.OP_BITXOR)]


def mp_cases(env_name):
    """"direct": RDC_DIRECT_BYTES=256K, so a 1 MiB automatic allreduce takes the
    registered-buffer schedule; host buffers of 4 KiB, 512 KiB and 2 MiB take
    the service, the zero-copy path and the pipelined pieces.  "tree":
    rdc_reduce_ring_mincount=64K, so buffers of at most 64 KiB take the tree
    order."""
    s = 0x0B5000
    cases = []
    if env_name == "direct":
        for k, (dt, op) in enumerate(MP_OPS):
            e = esize(dt)
            cases += [
                {"kind": "dev", "count": 1001, "dtype": dt, "op": op, "seed": s + 10 * k + 1, "pad": e},  # auto, small
                {"kind": "dev", "count": (1 << 20) // e + 1, "dtype": dt, "op": op, "seed": s + 10 * k + 2,
                 "direct": True},                                                                   # auto -> direct
            ]
        for k, ((dt, op), nbytes) in enumerate(zip(MP_OPS, (4 << 10, 512 << 10, 2 << 20, 4 << 10))):
            cases.append({"kind": "host", "count": nbytes // esize(dt), "dtype": dt, "op": op, "seed": s + 100 + k})
        cases += [
            {"kind": "host", "count": (512 << 10) // 4, "dtype": O.DT_FLOAT32, "op": R.OP_PROD, "seed": s + 110},
            {"kind": "host", "count": (2 << 20) // 8, "dtype": O.DT_INT64, "op": R.OP_BITXOR, "seed": s + 111},
            {"kind": "py_bf16", "count": 20011, "dtype": O.DT_BFLOAT16, "op": R.OP_PROD, "seed": s + 120},
            {"kind": "py_array", "count": 4099, "dtype": O.DT_FLOAT64, "op": R.OP_PROD, "seed": s + 121},
            {"kind": "dev", "count": 1001, "dtype": O.DT_UINT32, "op": R.OP_BITXOR, "known": "xor_same"},
            {"kind": "dev", "count": 1001, "dtype": O.DT_UINT32, "op": R.OP_BITAND, "known": "and_clear"},
            {"kind": "dev", "count": 1001, "dtype": O.DT_INT32, "op": R.OP_PROD, "known": "factorial"},
        ]
        return {"RDC_DIRECT_BYTES": "256K"}, cases
    for k, (dt, op) in enumerate(MP_OPS):
        e = esize(dt)
        cases += [
            {"kind": "dev", "count": (64 << 10) // e, "dtype": dt, "op": op, "seed": s + 200 + 10 * k},      # the tree order
            {"kind": "dev", "count": (64 << 10) // e + 1, "dtype": dt, "op": op, "seed": s + 201 + 10 * k},  # the ring order
        ]
    cases.append({"kind": "host", "count": 1024, "dtype": O.DT_FLOAT32, "op": R.OP_PROD, "seed": s + 250})  # service, tree
    return {"rdc_reduce_ring_mincount": "64K"}, cases


@pytest.mark.parametrize("env_name", ["direct", "tree"])
@pytest.mark.parametrize("world", [4, 8])
def test_mp_allreduce(world, env_name):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tests.mp_ops_worker import known_input
    env, cases = mp_cases(env_name)
    mincount = (64 << 10) if env_name == "tree" else 1
    tmp = run_mp(world, cases, worker=WORKER, timeout=300, env_extra=env)
    for i, c in enumerate(cases):
        dtype, op, count = c["dtype"], c["op"], c["count"]
        if "known" in c:
            xs = [known_input(c["known"], r, count) for r in range(world)]
            want = {"xor_same": np.zeros(count, dtype=np.uint32),
                    "and_clear": np.full(count, 0xFFFFFFFF & ~((1 << world) - 1), dtype=np.uint32),
                    "factorial": np.full(count, math.factorial(world), dtype=np.int32)}[c["known"]]
            assert R.ring(xs, op, dtype).tobytes() == want.tobytes()
        else:
            xs = R.gen_inputs(c["seed"], world, count, dtype)
            fold = R.tree if count * esize(dtype) <= mincount else R.ring
            want = fold(xs, op, dtype)
            R.assert_finite(want, dtype, c)
        for r in range(world):
            got = np.load(os.path.join(tmp, "case%d_rank%d.npy" % (i, r)))
            info = json.load(open(os.path.join(tmp, "case%d_rank%d.json" % (i, r))))
            assert equal(got.tobytes(), want, dtype), (env_name, i, c, "rank", r)
            if c.get("direct"):
                assert info["launch"][5] == 6, (i, info)
            if c["kind"] == "py_bf16":
                assert info["returns_its_argument"], info
            if c["kind"] == "py_array":
                assert info["dtype_kept"], info


# ------------------------------------------------------------------- 6. C++ --
@pytest.mark.parametrize("world", [2, 3])
def test_cpp_prod_and_bitxor_equal_the_host_custom_reducer(world, tmp_path):
    """tests/cpp/ops.cc: Allreduce<op::Prod>(float*) and Allreduce<op::BitXOR>
    (uint32_t*) on a device buffer against rdc::Reducer<T, f> with `dst *= src`
    / `dst ^= src` on a host copy, byte for byte."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    exe = str(tmp_path / "ops")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "ops.cc"), "-o", exe,
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
        assert "rank %d: prod and bitxor OK (world %d, N 100003)" % (r, world) in p.stdout, p.stdout
