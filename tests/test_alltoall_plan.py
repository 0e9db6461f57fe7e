"""All-to-all without a GPU: the plan each rank makes from its row and column
of the size matrix (RdcPlanAlltoall) — sender and receiver must cut every pair
alike —, the launch capacity (RdcPlanAlltoallCap), the byte model
(RdcPlanAlltoallBytes), the refusals and world-size-1 behaviour of the ABI, the
built kernel's resources and the C++ header.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.test_capi import run_py
from tests.test_kernel_resources import LIB, READELF, kernel_metadata
from tests.test_plan import layout

MIN_TILE = 16 << 10


def a2a_cap(n, scratch):
    from rdc_amd._lib import _LIB
    cap = ctypes.c_uint64()
    assert _LIB.RdcPlanAlltoallCap(n, scratch, ctypes.byref(cap)) == 0, _LIB.RdcGetLastError()
    return cap.value


def a2a_plan(n, rank, send_len, recv_len, scratch=0, tile=0, max_blocks=256, equal_len=0):
    from rdc_amd._lib import _LIB
    out = (ctypes.c_uint64 * 36)()
    sl = (ctypes.c_uint64 * 16)(*send_len)
    rl = (ctypes.c_uint64 * 16)(*recv_len)
    rc = _LIB.RdcPlanAlltoall(n, rank, sl, rl, scratch, tile, max_blocks, equal_len, out)
    assert rc == 0, _LIB.RdcGetLastError()
    return dict(tile=int(out[0]), nb_push=int(out[1]), nb_land=int(out[2]),
                out_tiles=[int(x) for x in out[4:4 + n]], in_tiles=[int(x) for x in out[20:20 + n]])


def matrix_plans(n, M, **kw):
    """every rank's plan of the exchange with length matrix M[r][p] (r -> p)"""
    return [a2a_plan(n, r, [M[r][p] for p in range(n)], [M[p][r] for p in range(n)], **kw) for r in range(n)]


@pytest.mark.parametrize("scratch", [1 << 20, 24 << 20, 0])
@pytest.mark.parametrize("n", range(2, 17))
def test_sender_and_receiver_cut_every_pair_alike(n, scratch):
    cap = a2a_cap(n, scratch)
    L = layout(n, scratch)
    rng = np.random.RandomState(1000 * n + (scratch >> 20))
    for trial, (tile, max_blocks) in enumerate(((0, 256), (0, 6), (48 << 10, 32), (0, 1))):
        t = a2a_plan(n, 0, [0] * n, [0] * n, scratch, tile, max_blocks)["tile"]
        pool = [min(x, cap) for x in (0, 0, 1, t - 1, t, t + 1, 3 * t + 5, cap - 1, cap)]
        M = [[int(pool[rng.randint(len(pool))]) if rng.rand() < 0.7 else int(rng.randint(0, cap + 1))
              for _ in range(n)] for _ in range(n)]
        M[rng.randint(n)] = [0] * n                         # a zero row
        c0 = rng.randint(n)
        for r in range(n):
            M[r][c0] = 0                                    # a zero column
        plans = matrix_plans(n, M, scratch=scratch, tile=tile, max_blocks=max_blocks)
        assert len({p["tile"] for p in plans}) == 1, "tile_bytes differs between ranks"
        assert plans[0]["tile"] == t and t % 256 == 0 and t >= MIN_TILE
        for r in range(n):
            for p in range(n):
                want = -(-M[r][p] // t)
                if r != p:
                    assert plans[r]["out_tiles"][p] == plans[p]["in_tiles"][r] == want, (n, r, p, M[r][p])
                else:
                    assert plans[r]["out_tiles"][r] == 0 and plans[r]["in_tiles"][r] == want
                # every planned tile lies inside the slot, and has a flag of its own
                assert M[r][p] <= cap <= L["slot"] - 256 and (want == 0 or (want - 1) * t < M[r][p])
                assert want <= L["max_tiles"]
            assert plans[r]["nb_push"] >= 1 and plans[r]["nb_land"] >= 1
            assert plans[r]["nb_push"] + plans[r]["nb_land"] <= max(2, max_blocks)


@pytest.mark.parametrize("n", [2, 3, 8, 16])
@pytest.mark.parametrize("scratch", [1 << 20, 16 << 20, 24 << 20, 0])
def test_capacity_is_the_allgathers_piece(n, scratch):
    L = layout(n, scratch)
    cap = a2a_cap(n, scratch)
    assert cap == (L["slot"] - 256) // 256 * 256          # PlanAllgather's per-piece capacity
    # the finest tiling of the longest segment still fits the flag row
    p = a2a_plan(n, 0, [cap] * n, [cap] * n, scratch, MIN_TILE, 256)
    assert p["tile"] == MIN_TILE and max(p["out_tiles"] + p["in_tiles"]) <= L["max_tiles"]
    assert (max(p["in_tiles"]) - 1) * p["tile"] < cap


def test_equal_split_tile_follows_the_bytes_per_peer_only():
    """the equal split may size its tile by bytes_per_peer (every rank knows it):
    one push item per push block inside [64 KiB, 1 MiB]; alltoallv never does"""
    n, G = 4, 64
    for per, want in ((1, 64 << 10), (1 << 20, 98304 + 0), (64 << 20, 1 << 20)):
        plans = [a2a_plan(n, r, [per] * n, [per] * n, 0, 0, G, equal_len=per) for r in range(n)]
        assert len({p["tile"] for p in plans}) == 1
        t = plans[0]["tile"]
        assert 64 << 10 <= t <= 1 << 20 and t % 256 == 0
        assert t == max(64 << 10, min(1 << 20, -(-(per * (n - 1) // (G // 2)) // 256) * 256)) == want
        assert a2a_plan(n, 0, [per] * n, [per] * n, 0, 0, G)["tile"] == 64 << 10


def test_all_zero_plan_is_still_one_launch_with_both_roles():
    for n in (2, 5, 16):
        for r in range(n):
            p = a2a_plan(n, r, [0] * n, [0] * n)
            assert p["nb_push"] == 1 and p["nb_land"] == 1 and p["tile"] >= MIN_TILE
            assert p["out_tiles"] == [0] * n and p["in_tiles"] == [0] * n


def test_roles_hold_no_block_without_an_item():
    t = 64 << 10
    p = a2a_plan(3, 1, [t, 5, 2 * t + 1], [1, 5, 0], max_blocks=256)
    assert p["out_tiles"] == [1, 0, 3] and p["in_tiles"] == [1, 1, 0]
    assert p["nb_push"] == 2 * 3 and p["nb_land"] == 3 * 1       # (n-1) x most outgoing, n x most incoming tiles
    p = a2a_plan(3, 1, [40 * t] * 3, [40 * t] * 3, max_blocks=10)
    assert (p["nb_push"], p["nb_land"]) == (5, 5)


def test_byte_model_three_rank_hand_count():
    from rdc_amd._lib import _LIB
    #            to 0  to 1  to 2
    M = [[7, 100, 0],        # from 0
         [3000, 11, 5],      # from 1
         [1, 64, 900]]       # from 2
    for r in range(3):
        send = M[r]
        recv = [M[p][r] for p in range(3)]
        out = (ctypes.c_uint64 * 5)()
        assert _LIB.RdcPlanAlltoallBytes(3, r, (ctypes.c_uint64 * 3)(*send), (ctypes.c_uint64 * 3)(*recv), out) == 0
        got = [int(x) for x in out]
        own = M[r][r]
        push = sum(send) - own           # read from the send buffer, written into the peers' slots
        land = sum(recv) - own           # read from this rank's slots, written into the receive buffer
        reads, writes = (push + own) + land, push + (land + own)
        assert got == [reads, writes, reads, writes, push], (r, got)
    assert [int(x) for x in out] == [0 + 5 + 900 + 1 + 64, 1 + 64 + 0 + 5 + 900, 970, 970, 65]  # rank 2, by hand
    assert _LIB.RdcPlanAlltoallBytes(3, 3, (ctypes.c_uint64 * 3)(), (ctypes.c_uint64 * 3)(), out) != 0


def test_world_size_one_copies_and_refusals():
    out = run_py(r'''
import ctypes, numpy as np, rdc_amd as r
from rdc_amd._lib import _LIB
sz = ctypes.c_size_t
def arr(*v): return (sz * len(v))(*v)
def ptr(a, off=0): return ctypes.c_void_p(a.ctypes.data + off)
src = np.arange(100, dtype=np.uint8)
dst = np.full(100, 0xA5, np.uint8)
assert _LIB.RdcAlltoall(ptr(src), ptr(dst), 10) != 0 and b"RdcInit" in _LIB.RdcGetLastError()
r.init([])
assert r.get_world_size() == 1
cap = ctypes.c_uint64()
assert _LIB.RdcPlanAlltoallCap(1, 0, ctypes.byref(cap)) == 0 and cap.value > 0
# world size 1: the own-segment copy only, every other byte as it was
assert _LIB.RdcAlltoallv(ptr(src), arr(20), arr(30), ptr(dst), arr(5), arr(30)) == 0, _LIB.RdcGetLastError()
want = np.full(100, 0xA5, np.uint8); want[5:35] = np.arange(20, 50)
assert np.array_equal(dst, want) and np.array_equal(src, np.arange(100, dtype=np.uint8))
dst[:] = 0xA5
assert _LIB.RdcAlltoall(ptr(src), ptr(dst), 60) == 0
want = np.full(100, 0xA5, np.uint8); want[:60] = np.arange(60)
assert np.array_equal(dst, want)
# zero bytes: legal, null pointers included
assert _LIB.RdcAlltoallv(None, arr(0), arr(0), None, arr(0), arr(0)) == 0
assert _LIB.RdcAlltoall(None, None, 0) == 0
before = dst.copy()
def refused(rc, word):
    assert rc != 0 and word in _LIB.RdcGetLastError(), _LIB.RdcGetLastError()
    assert np.array_equal(dst, before)
# a null pointer with a non-zero length
refused(_LIB.RdcAlltoallv(None, arr(0), arr(4), ptr(dst), arr(0), arr(4)), b"null send")
refused(_LIB.RdcAlltoallv(ptr(src), arr(0), arr(4), None, arr(0), arr(4)), b"null receive")
refused(_LIB.RdcAlltoall(None, ptr(dst), 4), b"null send")
refused(_LIB.RdcAlltoallv(ptr(src), None, arr(4), ptr(dst), arr(0), arr(4)), b"null offset")
# overlapping send and receive ranges (in place is not supported)
refused(_LIB.RdcAlltoallv(ptr(dst), arr(0), arr(10), ptr(dst), arr(9), arr(10)), b"overlap")
refused(_LIB.RdcAlltoall(ptr(dst), ptr(dst, 3), 8), b"overlap")
assert _LIB.RdcAlltoallv(ptr(dst), arr(0), arr(10), ptr(dst), arr(10), arr(10)) == 0    # adjacent is fine
dst[:] = before
# the own segment has one length
refused(_LIB.RdcAlltoallv(ptr(src), arr(0), arr(4), ptr(dst), arr(0), arr(5)), b"two lengths")
# a segment longer than one launch carries
big = np.zeros(cap.value + 1, np.uint8); big2 = np.zeros(cap.value + 1, np.uint8)
refused(_LIB.RdcAlltoallv(ptr(big), arr(0), arr(cap.value + 1), ptr(big2), arr(0), arr(cap.value + 1)), b"longer than one launch")
assert _LIB.RdcAlltoallv(ptr(big), arr(0), arr(cap.value), ptr(big2), arr(0), arr(cap.value)) == 0
# ... which the equal split cuts itself
big[:] = np.arange(big.size) % 251
assert _LIB.RdcAlltoall(ptr(big), ptr(big2), big.size) == 0 and np.array_equal(big, big2)
# the device entry points refuse the same way (nothing is launched at world size 1)
c = r.new_comm("a2a")
refused(_LIB.RdcCommAlltoallv(c.handle, ptr(dst), arr(0), arr(10), ptr(dst), arr(9), arr(10), None), b"overlap")
refused(_LIB.RdcCommAlltoall(c.handle, None, ptr(dst), 4, None), b"null send")
assert _LIB.RdcCommAlltoallv(None, ptr(src), arr(0), arr(4), ptr(dst), arr(0), arr(4), None) != 0
# the Python surface on numpy arrays
a = np.arange(12, dtype=np.int32); b = np.full(12, -1, np.int32)
assert r.all_to_all(a, b) is b and np.array_equal(a, b)
b[:] = -1
assert r.all_to_all_v(a, [5], b, [5], send_displs=[2], recv_displs=[6]) is b
assert np.array_equal(b, [-1] * 6 + [2, 3, 4, 5, 6] + [-1])
b[:] = -1
assert c.all_to_all_v(a, [3], b, [3]) is b and np.array_equal(b, [0, 1, 2] + [-1] * 9)
assert c.all_to_all(a, b) is b and np.array_equal(a, b)
for bad in (lambda: r.all_to_all_v(a, [13], b, [13]), lambda: r.all_to_all_v(a, [1, 2], b, [1]),
            lambda: r.all_to_all(a, b[:6])):
    try:
        bad()
    except ValueError:
        pass
    else:
        raise AssertionError("not refused")
r.finalize()
print("OK")
''')
    assert "OK" in out


def test_alltoall_kernel_resources():
    """one operator-independent instantiation, no scratch, below 128 VGPRs"""
    if not os.path.exists(LIB):
        pytest.skip("librdc_amd.so not built")
    if not os.path.exists(READELF):
        pytest.skip("llvm-readelf not available")
    fam = {k: v for k, v in kernel_metadata(LIB).items() if "k_alltoall" in k}
    assert len(fam) == 1, fam
    (scratch, vgprs), = [v[:2] for v in fam.values()]
    assert scratch == 0 and vgprs < 128, fam


def test_cpp_alltoall_compiles_and_runs_at_world_one(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "alltoall.cc")
    exe = str(tmp_path / "alltoall")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
                           "-L", os.path.join(ROOT, "rdc_amd"), "-lrdc_amd",
                           "-Wl,-rpath," + os.path.join(ROOT, "rdc_amd")])
    p = subprocess.run([exe, "7"], env=dict(os.environ, RDC_WORLD_SIZE="1"), capture_output=True, text=True,
                       timeout=60, cwd=str(tmp_path))
    assert p.returncode == 0, p.stdout + p.stderr
    assert "all-to-all OK (world 1, N 7)" in p.stdout
