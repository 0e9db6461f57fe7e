"""GPU tests of the all-to-all (RdcCommAlltoall / RdcCommAlltoallv, k_alltoall).
The expected bytes are index arithmetic in numpy alone: segment p of rank r's
send buffer lands in segment r of rank p's receive buffer,
    want[p][roff_p[r] : roff_p[r] + L] = send_r[soff_r[p] : soff_r[p] + L],
compared exactly.  Receive buffers are pre-filled with 0xA5 and sit between two
4 KiB guards of 0xA5: every byte outside the receive segments must still be
0xA5, and every send buffer must equal its input afterwards.

* single-process groups: n communicators on GPU 0, one stream each;
* multi-process: n processes on GPU 0, tests/mp_a2a_worker.py.
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
from tests.gpu_util import from_dev, ptr, same_bits, to_dev
from tests.mp_a2a_worker import GUARD, SENTINEL, offsets, row_col
from tests.test_gpu_reduce_scatter import Group, assert_rs, expected_rs, last_launch, launch_counters, run_mp

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

WORKER = os.path.join(ROOT, "tests", "mp_a2a_worker.py")
SZ = ctypes.c_size_t
KIB16 = 16 << 10

# One stream per rank.  The kernels of a group's ranks wait for each other, so
# two streams of one group must never share a hardware queue (tests/conftest.py,
# at most 3 ranks per process at 4 queues).  Every group of this
# module therefore uses the same three streams, made in a row at first need:
# how many streams other groups made before has no say in where a group's land.
_STREAMS = []


def make_group(n, scratch):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import rdc_amd
    assert n <= 3
    while len(_STREAMS) < 3:
        _STREAMS.append(torch.cuda.Stream())
    g = Group(rdc_amd.init_group([0] * n, scratch_bytes=scratch))
    g.streams = _STREAMS[:n]
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


def stream(g, r):
    return ctypes.c_void_p(g.streams[r].cuda_stream)


def a2a_cap(n, scratch):
    from rdc_amd._lib import _LIB
    cap = ctypes.c_uint64()
    assert _LIB.RdcPlanAlltoallCap(n, scratch, ctypes.byref(cap)) == 0
    return cap.value


def asym_matrix(n, shift=0):
    """M[r][p] = bytes r -> p: asymmetric, with a zero row (rank 0 sends
    nothing), a zero column (rank n-1 receives nothing) and a 1-byte segment."""
    sizes = [1, 15, 17, 4097, 70001, 3 * 65536 + 5, KIB16, 100003]
    M = [[sizes[(3 * r + 5 * p + shift) % len(sizes)] for p in range(n)] for r in range(n)]
    M[0] = [0] * n
    for r in range(n):
        M[r][n - 1] = 0
    M[n - 1][0] = 1
    return M


def dense_matrix(n, shift=1):
    sizes = [5, 200001, 1, 33, KIB16 + 1, 65536, 99999, 7]
    M = [[sizes[(3 * r + 5 * p + shift) % len(sizes)] for p in range(n)] for r in range(n)]
    assert any(M[r][p] != M[p][r] for r in range(n) for p in range(n))
    return M


def expected(M, sends, soffs, roffs, rtotals):
    """want[p]: the receive buffer of rank p with its guards, by index arithmetic"""
    n = len(M)
    want = [np.full(rtotals[p] + 2 * GUARD, SENTINEL, np.uint8) for p in range(n)]
    for r in range(n):
        for p in range(n):
            L = M[r][p]
            want[p][GUARD + roffs[p][r]: GUARD + roffs[p][r] + L] = sends[r][soffs[r][p]: soffs[r][p] + L]
    return want


class Exchange(object):
    """Device buffers of one exchange over the length matrix M: per rank a send
    buffer (seeded numpy bytes) and a receive buffer of 0xA5 between two
    guards, at the address offsets sbase[r] / rbase[r] (bytes past an aligned
    allocation); segments sgap / rgap bytes apart, the first rfirst bytes in."""

    def __init__(self, M, rng, sgap=0, rgap=0, sbase=None, rbase=None, rfirst=0):
        n = self.n = len(M)
        self.M = M
        self.sbase, self.rbase = sbase or [0] * n, rbase or [0] * n
        self.slen, self.rlen, self.soff, self.roff, self.rtotal, self.sends = [], [], [], [], [], []
        for r in range(n):
            sl, rl = row_col(M, r)
            so, st = offsets(sl, sgap)
            ro, rt = offsets(rl, rgap, rfirst)
            self.slen.append(sl), self.rlen.append(rl), self.soff.append(so), self.roff.append(ro)
            self.rtotal.append(rt)
            self.sends.append(rng.integers(0, 256, st, dtype=np.uint8))
        self.dsend = [to_dev(self.sends[r], self.sbase[r]) for r in range(n)]
        self.drecv = [torch.full((self.rtotal[r] + 2 * GUARD + self.rbase[r] + 64,), SENTINEL, dtype=torch.uint8,
                                 device="cuda") for r in range(n)]

    def launch_v(self, g, r):
        from rdc_amd._lib import _LIB
        n = self.n
        rc = _LIB.RdcCommAlltoallv(g[r].handle, ptr(self.dsend[r], self.sbase[r]), (SZ * n)(*self.soff[r]),
                                   (SZ * n)(*self.slen[r]), ptr(self.drecv[r], self.rbase[r] + GUARD),
                                   (SZ * n)(*self.roff[r]), (SZ * n)(*self.rlen[r]), stream(g, r))
        assert rc == 0, _LIB.RdcGetLastError()

    def launch_equal(self, g, r):
        from rdc_amd._lib import _LIB
        rc = _LIB.RdcCommAlltoall(g[r].handle, ptr(self.dsend[r], self.sbase[r]),
                                  ptr(self.drecv[r], self.rbase[r] + GUARD), self.M[0][0], stream(g, r))
        assert rc == 0, _LIB.RdcGetLastError()

    def verify(self, what):
        want = expected(self.M, self.sends, self.soff, self.roff, self.rtotal)
        for r in range(self.n):
            got = self.drecv[r][self.rbase[r]: self.rbase[r] + want[r].size].cpu().numpy()
            if got.tobytes() != want[r].tobytes():
                bad = np.flatnonzero(got != want[r])
                raise AssertionError("%s: rank %d receive buffer differs at %d bytes, first at %d (guard %d)"
                                     % (what, r, bad.size, bad[0] - GUARD, GUARD))
            sent = self.dsend[r][self.sbase[r]: self.sbase[r] + self.sends[r].size].cpu().numpy()
            assert sent.tobytes() == self.sends[r].tobytes(), (what, "send buffer of rank", r)


def run_exchange(g, x, equal=False, what=None):
    torch.cuda.synchronize()
    for r in range(x.n):
        (x.launch_equal if equal else x.launch_v)(g, r)
    for r in range(x.n):
        g[r].check(stream(g, r))
    x.verify(what)


def equal_sizes(g):
    """0, 1 B, around 16 B, around 16 KiB, and 3 tiles + 5 B (the tile of a small
    equal split; the caller checks that the last size was cut by that tile)"""
    run_exchange(g, Exchange([[KIB16] * len(g)] * len(g), np.random.default_rng(1)), equal=True, what="probe")
    tile = last_launch(g[0])[4]
    return [0, 1, 15, 16, 17, KIB16 - 1, KIB16, KIB16 + 1, 3 * tile + 5]


# ------------------------------------------------------ 1. single-process groups
@pytest.mark.parametrize("n", [2, 3])
def test_group_equal_split_sizes(group2, group3, n):
    g = group2 if n == 2 else group3
    rng = np.random.default_rng(4100 + n)
    for per in equal_sizes(g):
        before = launch_counters(g)
        run_exchange(g, Exchange([[per] * n] * n, rng), equal=True, what=("equal", n, per))
        ll = last_launch(g[n - 1])
        assert launch_counters(g) == [b + (1 if per else 0) for b in before], per
        if per:
            assert ll[5] == 102 and ll[2] == 0 and ll[1] >= 1 and ll[3] >= 1 and ll[0] == ll[1] + ll[3], ll
            assert ll[4] % 256 == 0 and ll[4] >= KIB16
    assert per == 3 * ll[4] + 5, ("the last size is not 3 tiles + 5 B", per, ll)


@pytest.mark.parametrize("n", [2, 3])
def test_group_alltoallv_asymmetric_zero_row_zero_column_one_byte(group2, group3, n):
    g = group2 if n == 2 else group3
    rng = np.random.default_rng(4200 + n)
    for M in (asym_matrix(n), dense_matrix(n)):
        before = launch_counters(g)
        run_exchange(g, Exchange(M, rng, sgap=3, rgap=7), what=("alltoallv", n, M))
        assert launch_counters(g) == [b + 1 for b in before]
    # every length zero: still one launch on every rank, nothing written
    before = launch_counters(g)
    run_exchange(g, Exchange([[0] * n] * n, rng), what="all zero")
    assert launch_counters(g) == [b + 1 for b in before]


@pytest.mark.parametrize("n", [2, 3])
def test_group_alltoallv_misaligned_bases(group2, group3, n):
    """send and receive bases 1, 0 and 3 bytes past an aligned address, receive
    offsets no multiples of 16: the 16-B path, every word path and the byte
    path of block_copy on both the push and the land side"""
    g = group2 if n == 2 else group3
    rng = np.random.default_rng(4300 + n)
    base = [1, 0, 3][:n]
    for M in (asym_matrix(n), dense_matrix(n)):
        for sgap, rgap, rfirst in ((3, 7, 5), (2, 4, 8), (0, 16, 0), (8, 2, 2)):
            run_exchange(g, Exchange(M, rng, sgap=sgap, rgap=rgap, sbase=base,
                                     rbase=base if rfirst in (5, 8) else base[::-1], rfirst=rfirst),
                         what=("misaligned", n, sgap, rgap, rfirst))


# ------------------------------------------------------------- 2. multi-piece
def test_group_multi_piece_and_capacity_refusal():
    from rdc_amd._lib import _LIB
    scratch = 1 << 20                      # 256 KiB slots at n = 2
    g = make_group(2, scratch)
    try:
        cap = a2a_cap(2, scratch)
        assert 200 << 10 < cap < 256 << 10
        rng = np.random.default_rng(4400)
        per = cap * 5 // 2
        before = launch_counters(g)
        run_exchange(g, Exchange([[per] * 2] * 2, rng), equal=True, what="2.5 x cap")
        assert launch_counters(g) == [b + 3 for b in before]
        # one segment of cap + 1 bytes: refused on the rank that sees it, nothing launched
        x = Exchange([[5, cap + 1], [7, 9]], rng)
        before = launch_counters(g)
        n = 2
        for r in range(2):
            rc = _LIB.RdcCommAlltoallv(g[r].handle, ptr(x.dsend[r]), (SZ * n)(*x.soff[r]), (SZ * n)(*x.slen[r]),
                                       ptr(x.drecv[r], GUARD), (SZ * n)(*x.roff[r]), (SZ * n)(*x.rlen[r]), stream(g, r))
            assert rc != 0 and b"longer than one launch" in _LIB.RdcGetLastError(), _LIB.RdcGetLastError()
        assert launch_counters(g) == before
        for r in range(2):
            assert bool((x.drecv[r] == SENTINEL).all())
        # exactly cap still goes
        run_exchange(g, Exchange([[5, cap], [cap - 1, 9]], rng), what="cap")
    finally:
        for c in g:
            c.destroy()


# -------------------------------------------------------------- 3. slot reuse
def test_group3_back_to_back_without_host_sync(group3):
    """64 alltoalls on every rank's stream with no host sync between them: a
    push may overwrite a slot only after its reader's previous launch ended
    (the done-word gate), or an earlier call's receive buffer shows later bytes"""
    rng = np.random.default_rng(4500)
    xs = [Exchange([[40001 + 16 * k] * 3] * 3, rng) for k in range(64)]
    torch.cuda.synchronize()
    for x in xs:
        for r in range(3):
            x.launch_equal(group3, r)
    for r in range(3):
        group3[r].check(stream(group3, r))
    for k, x in enumerate(xs):
        x.verify(("back to back", k))


# --------------------------------------------------------------- 4. the chain
def test_group3_chain_with_every_launch_kind_in_poison_mode(group3):
    """alltoallv, mesh allreduce, alltoall, ring allreduce, broadcast, alltoallv,
    allgather, one-shot allreduce, alltoall, reduce-scatter, alltoall, and the
    one-shot / empty alltoallv / mesh or ring triples — no host sync, consumed
    scratch poisoned: every predecessor / successor pair of DESIGN.md 4.2's
    new row."""
    from rdc_amd._lib import _LIB
    g, n = group3, 3
    rng = np.random.default_rng(4600)
    dt, op = O.DT_FLOAT32, O.OP_SUM
    # ... then the pairs that hide a one-shot from the launch after it: one-shot, an
    # alltoallv in which nobody sends anything, mesh; one-shot, an alltoallv in
    # which rank 0 neither sends nor receives, ring (push block 0's gate)
    idle0 = dense_matrix(n)
    idle0[0] = [0] * n
    for r in range(n):
        idle0[r][0] = 0
    steps = ["a2av", ("ar", 2, 300007), "a2a", ("ar", 1, 70001), "bc", "a2av", "ag", ("ar", 3, 1001), "a2a", "rs",
             "a2a", ("ar", 3, 4099), ("a2avm", [[0] * n] * n), ("ar", 2, 100003), ("ar", 3, 4099), ("a2avm", idle0),
             ("ar", 1, 100003)]
    for c in g:
        c.set_poison(True)
    try:
        state = []
        for k, s in enumerate(steps):
            if s == "a2av":
                state.append(Exchange(asym_matrix(n, k) if k else dense_matrix(n), rng, sgap=3, rgap=7, rfirst=1))
            elif s[0] == "a2avm":
                state.append(Exchange(s[1], rng, sgap=3, rgap=7, rfirst=1))
            elif s == "a2a":
                state.append(Exchange([[100003 + k] * n] * n, rng))
            elif s in ("bc", "ag"):
                sizes = [(1 << 20) + 5] * n if s == "bc" else [70001, 7, 200003]
                data = [rng.integers(0, 256, sz, dtype=np.uint8) for sz in sizes]
                if s == "bc":
                    bufs = [to_dev(data[r]) for r in range(n)]
                else:
                    bufs = [[to_dev(data[c] if c == r else np.zeros(sizes[c], np.uint8)) for c in range(n)]
                            for r in range(n)]
                state.append((data, bufs))
            else:
                count = s[2] if s != "rs" else 50001
                inputs = [rng.standard_normal(count).astype(np.float32) for _ in range(n)]
                state.append((inputs, [to_dev(x) for x in inputs]))
        torch.cuda.synchronize()
        for s, st in zip(steps, state):
            for r in range(n):
                sp = stream(g, r)
                if s == "a2av" or s[0] == "a2avm":
                    st.launch_v(g, r)
                elif s == "a2a":
                    st.launch_equal(g, r)
                elif s == "bc":
                    assert _LIB.RdcCommBroadcast(g[r].handle, ptr(st[1][r]), st[0][0].size, 1, sp) == 0
                elif s == "ag":
                    ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in st[1][r]])
                    assert _LIB.RdcCommAllgather(g[r].handle, ptrs, (SZ * n)(*[d.size for d in st[0]]), sp) == 0
                elif s == "rs":
                    assert _LIB.RdcCommReduceScatter(g[r].handle, ptr(st[1][r]), st[0][0].size, dt, op, 2, sp) == 0
                else:
                    assert _LIB.RdcCommAllreduceEx(g[r].handle, ptr(st[1][r]), s[2], dt, op, s[1], sp) == 0, \
                        _LIB.RdcGetLastError()
        for r in range(n):
            g[r].check(stream(g, r))
        for k, (s, st) in enumerate(zip(steps, state)):
            if s in ("a2av", "a2a") or s[0] == "a2avm":
                st.verify(("chain step", k, s))
            elif s == "bc":
                for r in range(n):
                    assert from_dev(st[1][r], 0, st[0][1].size, O.DT_UINT8).tobytes() == st[0][1].tobytes(), (k, r)
            elif s == "ag":
                for r in range(n):
                    for c in range(n):
                        assert from_dev(st[1][r][c], 0, st[0][c].size, O.DT_UINT8).tobytes() == st[0][c].tobytes(), \
                            (k, r, c)
            elif s == "rs":
                got = [from_dev(st[1][r], 0, st[0][0].size, dt) for r in range(n)]
                assert_rs(got, expected_rs(st[0], dt, op), st[0], dt, ("chain step", k))
            else:
                want = O.expected_allreduce(st[0], dt, op)
                for r in range(n):
                    assert same_bits(from_dev(st[1][r], 0, s[2], dt), want, dt), ("chain step", k, s, r)
    finally:
        for c in g:
            c.set_poison(False)


# ------------------------------------------------------- 5. launch counter
def test_group2_launch_counter_across_two_to_the_32():
    """A fresh group (every hand-off flag still 0) with the counter just below
    2^32: the equal-split sizes and the alltoallv matrices stay exact, one count
    per launch.  As in test_group_launch_counter_far_past_zeroed_flags an
    allreduce is the first launch after the jump: the pushes gate on the peers'
    done words of the PREVIOUS launch, which RdcCommSetLaunchCounter does not
    write (a counter only ever advances by launches, and each one writes them)."""
    from rdc_amd._lib import _LIB
    g = make_group(2, 16 << 20)
    try:
        start = (1 << 32) - 3
        for c in g:
            assert _LIB.RdcCommSetLaunchCounter(c.handle, start) == 0, _LIB.RdcGetLastError()
        rng = np.random.default_rng(4700)
        xs = [rng.standard_normal(1001).astype(np.float32) for _ in range(2)]
        bufs = [to_dev(x) for x in xs]
        torch.cuda.synchronize()
        for r in range(2):
            assert _LIB.RdcCommAllreduceEx(g[r].handle, ptr(bufs[r]), 1001, O.DT_FLOAT32, O.OP_SUM, 2, stream(g, r)) == 0
        for r in range(2):
            g[r].check(stream(g, r))
            assert same_bits(from_dev(bufs[r], 0, 1001, O.DT_FLOAT32),
                             O.expected_allreduce(xs, O.DT_FLOAT32, O.OP_SUM), O.DT_FLOAT32)
        launches = 1
        for per in (0, 1, 15, 16, 17, KIB16 - 1, KIB16, KIB16 + 1, 3 * 65536 + 5):
            run_exchange(g, Exchange([[per] * 2] * 2, rng), equal=True, what=("counter", per))
            launches += 1 if per else 0
            assert launch_counters(g) == [start + launches] * 2
        for M in (asym_matrix(2), dense_matrix(2)):
            run_exchange(g, Exchange(M, rng, sgap=3, rgap=7), what=("counter", M))
            launches += 1
        assert launch_counters(g) == [start + launches] * 2 and start + launches > 1 << 32
    finally:
        for c in g:
            c.destroy()


# ------------------------------------------------------------ 6. multi-process
def check_mp_case(tmp, i, c, world):
    seed = c.get("seed", 0x5EEDA2A0)
    if "M" in c:
        M, sgap, rgap = c["M"], c.get("sgap", 0), c.get("rgap", 0)
    else:
        M, sgap, rgap = [[c["bytes"]] * world for _ in range(world)], 0, 0
    soffs, roffs, rtotals, sends = [], [], [], []
    for r in range(world):
        sl, rl = row_col(M, r)
        so, st = offsets(sl, sgap)
        ro, rt = offsets(rl, rgap)
        soffs.append(so), roffs.append(ro), rtotals.append(rt)
        sends.append(O.fill(st, O.DT_UINT8, seed, r))
    want = expected(M, sends, soffs, roffs, rtotals)
    for r in range(world):
        z = np.load(os.path.join(tmp, "case%d_rank%d.npz" % (i, r)))
        assert z["recv"].tobytes() == want[r].tobytes(), (i, c["kind"], "receive buffer of rank", r)
        assert z["send"].tobytes() == sends[r].tobytes(), (i, c["kind"], "send buffer of rank", r)
        info = json.load(open(os.path.join(tmp, "case%d_rank%d.json" % (i, r))))
        if c["kind"] in ("a2a", "a2av", "py"):
            assert info["launch"][5] == 102 and info["launch"][2] == 0, info


def mp_matrix(n, unit=1):
    """the asymmetric matrix scaled to n ranks (multiples of `unit` bytes)"""
    return [[x * unit for x in row] for row in asym_matrix(n)]


@pytest.mark.parametrize("world", [2, 4, 5, 8])
def test_mp_alltoall(world):
    """n processes on GPU 0 (never more than 8 at once; the launcher's queue
    rule applies inside run_mp): the equal split at 100003 B per peer, the
    asymmetric matrix scaled to n, Comm.all_to_all / all_to_all_v on tensors
    and the blocking entry on numpy arrays."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cases = [
        {"kind": "a2a", "bytes": 100003},
        {"kind": "a2av", "M": mp_matrix(world), "sgap": 3, "rgap": 7, "seed": 0x5EEDA2A1},
        {"kind": "py", "bytes": 40000, "seed": 0x5EEDA2A2},
        {"kind": "py", "bytes": 40004, "seed": 0x5EEDA2A6, "module": True},
        {"kind": "py", "M": mp_matrix(world, 4), "sgap": 4, "rgap": 12, "seed": 0x5EEDA2A3},
        {"kind": "py", "M": mp_matrix(world, 4), "sgap": 8, "rgap": 4, "seed": 0x5EEDA2A7, "module": True},
        {"kind": "host", "bytes": 100003, "seed": 0x5EEDA2A4},
        {"kind": "host", "M": mp_matrix(world), "sgap": 1, "rgap": 5, "seed": 0x5EEDA2A5},
    ]
    tmp = run_mp(world, cases, worker=WORKER)
    for i, c in enumerate(cases):
        check_mp_case(tmp, i, c, world)


# --------------------------------------------------------------------- 7. fuzz
def fuzz_case(seed):
    """seed -> (n, rng, matrix, gaps and address offsets): lengths in [0, 300 KiB], a fifth of them 0"""
    rng = np.random.default_rng(4800 + seed)
    n = 2 + seed % 4
    M = [[int(rng.integers(0, (300 << 10) + 1)) if rng.random() < 0.8 else 0 for _ in range(n)] for _ in range(n)]
    kw = dict(sgap=int(rng.integers(0, 40)), rgap=int(rng.integers(0, 40)),
              sbase=[int(b) for b in rng.integers(0, 16, n)], rbase=[int(b) for b in rng.integers(0, 16, n)])
    return n, rng, M, kw


def test_fuzz_groups_of_two_and_three(group2, group3):
    """the seeded matrices at n = 2 and 3 (a single process drives one stream
    per rank, and more than three would share hardware queues): random
    displacements with gaps, random address offsets"""
    for seed in range(20):
        n, rng, M, kw = fuzz_case(seed)
        if n <= 3:
            run_exchange(group2 if n == 2 else group3, Exchange(M, rng, rfirst=int(rng.integers(0, 64)), **kw),
                         what=("fuzz", seed, n))


@pytest.mark.parametrize("world", [4, 5])
def test_fuzz_processes_of_four_and_five(world):
    """the seeded matrices at n = 4 and 5, one process per rank"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cases = []
    for seed in range(20):
        n, _, M, kw = fuzz_case(seed)
        if n == world:
            cases.append(dict(kind="a2av", M=M, seed=0x5EEDF000 + seed, **kw))
    assert len(cases) == 5
    tmp = run_mp(world, cases, worker=WORKER)
    for i, c in enumerate(cases):
        check_mp_case(tmp, i, c, world)


# ---------------------------------------------------------------------- 8. C++
@pytest.mark.parametrize("world", [2, 3])
def test_cpp_alltoall_through_the_launcher(world, tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    exe = str(tmp_path / "alltoall")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "alltoall.cc"), "-o", exe,
                           "-L", os.path.join(ROOT, "rdc_amd"), "-lrdc_amd",
                           "-Wl,-rpath," + os.path.join(ROOT, "rdc_amd")])
    env = dict(os.environ, RDC_SCRATCH_BYTES="64M")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "-m", "rdc_amd.launcher", "-n", str(world), "--gpus", "1", exe, "100003"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    for r in range(world):
        assert "rank %d: all-to-all OK (world %d, N 100003)" % (r, world) in p.stdout, p.stdout
