"""The prefix reduction across ranks (Scan / Exscan) without a GPU: the launches
of its schedule (RdcPlanScan), the byte model (RdcPlanScanBytes) and the
argument checks of both.
"""
import ctypes

import numpy as np
import pytest

from oracle import oracle as O
from tests.test_plan import WORDS, layout

SCRATCH = 16 << 20
DT_OF_ESZ = {1: O.DT_INT8, 2: O.DT_FLOAT16, 4: O.DT_FLOAT32, 8: O.DT_FLOAT64}


def scan_plan(n, rank, count, dtype, scratch=SCRATCH, tile=0, max_blocks=256, op=O.OP_SUM):
    from rdc_amd._lib import _LIB
    npieces = ctypes.c_int()
    rc = _LIB.RdcPlanScan(n, rank, count, dtype, op, scratch, tile, max_blocks, None, 0, ctypes.byref(npieces))
    assert rc == 0, _LIB.RdcGetLastError()
    k = npieces.value
    buf = (ctypes.c_uint64 * (WORDS * max(1, k)))()
    assert _LIB.RdcPlanScan(n, rank, count, dtype, op, scratch, tile, max_blocks, buf, k, ctypes.byref(npieces)) == 0
    arr = np.frombuffer(buf, dtype=np.uint64).reshape(max(1, k), WORDS)[:k]
    return [dict(tile=int(row[0]), grid=int(row[1]), nb=(int(row[2]), int(row[3])), off=int(row[4]), len=int(row[20]),
                 mis=int(row[36]), tiles=int(row[52]), rest=[int(x) for x in row[5:20]] + [int(x) for x in row[21:36]])
            for row in arr]


def slot_cap(n, scratch):
    """The all-to-all's per-launch capacity: round_down(slot_bytes - 256, 256)."""
    return (layout(n, scratch)["slot"] - 256) // 256 * 256


@pytest.mark.parametrize("esz", [1, 2, 4, 8])
@pytest.mark.parametrize("n", [2, 3, 8, 16])
def test_pieces_tile_the_buffer_and_fit_a_slot_and_a_flag_row(n, esz):
    dt = DT_OF_ESZ[esz]
    for scratch in (1 << 20, SCRATCH):
        L = layout(n, scratch)
        cap = slot_cap(n, scratch)
        for count in (1, 2, 15, 1001, 4099, (1 << 20) + 1, (18 << 20) // esz + 7):
            for tile, max_blocks in ((0, 256), (0, 2), (256, 2), (64 << 10, 24), (1 << 20, 5)):
                pieces = scan_plan(n, 0, count, dt, scratch, tile, max_blocks)
                assert pieces
                pos = 0
                for p in pieces:
                    assert p["off"] == pos and p["len"] > 0 and p["len"] % esz == 0, (count, tile, p)
                    pos += p["len"]
                    assert p["len"] <= cap, ("a piece exceeds one slot", p, cap)
                    assert p["tile"] % 256 == 0 and p["tile"] > 0
                    assert p["tiles"] == -(-p["len"] // p["tile"])
                    assert p["tiles"] <= L["max_tiles"], ("a piece exceeds the flag row", p, L)
                    assert 1 <= p["grid"] <= min(p["tiles"], max_blocks)
                    assert p["grid"] == min(p["tiles"], max_blocks)
                    assert p["mis"] == 0 and p["nb"] == (0, 0) and not any(p["rest"])
                    if tile:
                        assert p["tile"] == tile
                    else:
                        assert (64 << 10) <= p["tile"] <= (1 << 20)
                    # every piece but the last is full
                    if p is not pieces[-1]:
                        assert p["len"] == min(cap, L["max_tiles"] * p["tile"]) if tile else p["len"] == cap
                assert pos == count * esz, "the pieces do not cover the buffer"


def test_a_small_configured_tile_is_kept_and_bounds_the_piece():
    """RdcCommTune(max_blocks=2, tile_bytes=256): 4099 fp32 elements are 65
    tiles over 2 blocks; a buffer of more than max_tiles x 256 bytes is cut."""
    (p,) = scan_plan(3, 1, 4099, O.DT_FLOAT32, SCRATCH, 256, 2)
    assert (p["tile"], p["tiles"], p["grid"], p["len"]) == (256, 65, 2, 16396)
    L = layout(2, SCRATCH)
    count = (L["max_tiles"] * 256 * 2 + 260) // 4
    pieces = scan_plan(2, 0, count, O.DT_FLOAT32, SCRATCH, 256, 2)
    assert [q["len"] for q in pieces] == [L["max_tiles"] * 256, L["max_tiles"] * 256, 260]
    assert all(q["tiles"] <= L["max_tiles"] for q in pieces)


def test_multi_piece_of_the_gpu_test():
    """18 MiB + 7 elements of fp32 on 2 ranks with 16 MiB of scratch: several launches."""
    pieces = scan_plan(2, 0, (18 << 20) // 4 + 7, O.DT_FLOAT32, 16 << 20)
    assert len(pieces) >= 2
    assert sum(p["len"] for p in pieces) == (18 << 20) + 28


@pytest.mark.parametrize("n", [2, 3, 8])
def test_the_plan_does_not_depend_on_the_rank(n):
    for count in (1, 4099, (1 << 22) + 3, (40 << 20) + 1):
        for tile, max_blocks in ((0, 256), (512, 3), (0, 7)):
            ref = scan_plan(n, 0, count, O.DT_FLOAT32, SCRATCH, tile, max_blocks)
            for rank in range(1, n):
                assert scan_plan(n, rank, count, O.DT_FLOAT32, SCRATCH, tile, max_blocks) == ref, (count, rank)


def test_world_size_one_and_count_zero_plan_nothing():
    assert scan_plan(1, 0, 1001, O.DT_FLOAT32) == []
    assert scan_plan(3, 2, 0, O.DT_FLOAT32) == []


def scan_bytes(n, rank, count, dtype):
    from rdc_amd._lib import _LIB
    out = (ctypes.c_uint64 * 5)()
    assert _LIB.RdcPlanScanBytes(n, rank, count, dtype, out) == 0, _LIB.RdcGetLastError()
    return [int(x) for x in out]


@pytest.mark.parametrize("n", [2, 3, 8])
def test_byte_model_matches_the_table(n):
    """rank 0: loads S, stores S remote; 0 < r < n-1: loads 2 S, stores 2 S, one
    remote; rank n-1: loads 2 S, stores S."""
    for dt, esz in ((O.DT_INT8, 1), (O.DT_FLOAT32, 4), (O.DT_FLOAT64, 8)):
        for count in (1, 4099, (1 << 22) + 3):
            S = count * esz
            rd_sum = wr_sum = 0
            for r in range(n):
                rd = S if r == 0 else 2 * S
                wr = S if r in (0, n - 1) else 2 * S
                eg = 0 if r == n - 1 else S
                assert scan_bytes(n, r, count, dt) == [rd, wr, rd, wr, eg], (n, r, count)
                rd_sum += rd
                wr_sum += wr
            assert scan_bytes(n, -1, count, dt) == [2 * S, 2 * S if n > 2 else S, rd_sum, wr_sum, S]
    assert scan_bytes(1, 0, 1001, O.DT_FLOAT32) == [0] * 5
    assert scan_bytes(n, 0, 0, O.DT_FLOAT32) == [0] * 5


def test_bad_arguments_are_refused():
    from rdc_amd._lib import _LIB
    k = ctypes.c_int()
    out = (ctypes.c_uint64 * 5)()

    def refused(*args):
        return _LIB.RdcPlanScan(*args, None, 0, ctypes.byref(k)) != 0

    assert refused(3, 3, 100, O.DT_FLOAT32, O.OP_SUM, SCRATCH, 0, 256)       # rank outside [0, n)
    assert refused(3, -1, 100, O.DT_FLOAT32, O.OP_SUM, SCRATCH, 0, 256)
    assert refused(0, 0, 100, O.DT_FLOAT32, O.OP_SUM, SCRATCH, 0, 256)       # no ranks
    assert refused(17, 0, 100, O.DT_FLOAT32, O.OP_SUM, SCRATCH, 0, 256)
    assert refused(3, 0, 100, O.DT_FLOAT32, O.OP_BITOR, SCRATCH, 0, 256)     # unsupported (dtype, op)
    assert b"BITOR" in _LIB.RdcGetLastError(), _LIB.RdcGetLastError()
    assert refused(3, 0, 100, 99, O.OP_SUM, SCRATCH, 0, 256)
    assert refused(3, 0, 100, O.DT_FLOAT32, 9, SCRATCH, 0, 256)
    assert refused(3, 0, 100, O.DT_FLOAT32, O.OP_SUM, SCRATCH, 100, 256)     # tile not a multiple of 256
    assert _LIB.RdcPlanScan(3, 0, 100, O.DT_FLOAT32, O.OP_SUM, SCRATCH, 0, 256, None, 0, None) != 0
    assert _LIB.RdcPlanScanBytes(3, 3, 100, O.DT_FLOAT32, out) != 0
    assert _LIB.RdcPlanScanBytes(0, 0, 100, O.DT_FLOAT32, out) != 0
    assert _LIB.RdcPlanScanBytes(3, 0, 100, 99, out) != 0
    assert _LIB.RdcPlanScanBytes(3, 0, 100, O.DT_FLOAT32, None) != 0
