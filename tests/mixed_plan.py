"""Seeded plan of a mixed-collective chain (tests/mp_mixed_worker.py) and its
expected output computed with the CPU oracle (tests/test_gpu_mixed.py; the
plan itself is checked on CPU in tests/test_plan.py)."""
import random

import numpy as np

ESZ = {0: 1, 1: 1, 2: 4, 3: 4, 4: 8, 5: 8, 6: 4, 7: 8, 8: 8, 9: 8, 10: 2, 11: 2}
# (dtype, op) pairs with reference semantics (BitOR only on integers)
PAIRS = [(6, 2), (6, 0), (7, 2), (2, 2), (2, 3), (10, 2), (11, 2), (4, 1), (1, 0)]


def make_plan(seed, nops, world):
    rng = random.Random(seed)
    plan = []
    for k in range(nops):
        kind = rng.choice(["allreduce", "allreduce", "bcast", "allgather", "coalesced", "host"])
        s = 0x5EED0000 + 1000 * k
        if kind == "allreduce":
            dt, op = rng.choice(PAIRS)
            count = rng.choice([1, 7, 1000, 4099, 65536 + 3, 300001])
            plan.append({"kind": kind, "count": count, "dtype": dt, "op": op, "algo": rng.choice([0, 1, 2, 3]),
                         "seed": s})
        elif kind == "bcast":
            plan.append({"kind": kind, "bytes": rng.choice([1, 100, 4096, 100003, 1 << 20, 3 << 20]),
                         "root": rng.randrange(world), "seed": s})
        elif kind == "allgather":
            plan.append({"kind": kind, "sizes": [rng.choice([0, 3, 64, 5000, 70001]) for _ in range(world)],
                         "seed": s})
        elif kind == "host":  # synchronous, host buffer: the small-allreduce service or the launch path
            dt, op = rng.choice(PAIRS)
            plan.append({"kind": kind, "count": rng.choice([1, 7, 1000, 4099, 16384, 20000]), "dtype": dt, "op": op,
                         "seed": s})
        else:
            dt, op = rng.choice([(6, 2), (2, 0), (10, 2)])
            nb = rng.randint(2, 9)
            plan.append({"kind": kind, "counts": [rng.choice([0, 1, 5, 1024, 33333, 131072]) for _ in range(nb)],
                         "dtype": dt, "op": op, "algo": rng.choice([0, 0, 1, 2, 3]), "seed": s})
    return plan


def output_bytes(plan):
    """Total bytes of every op's outputs, in the worker's order."""
    tot = 0
    for op in plan:
        if op["kind"] in ("allreduce", "host"):
            tot += op["count"] * ESZ[op["dtype"]]
        elif op["kind"] == "bcast":
            tot += op["bytes"]
        elif op["kind"] == "allgather":
            tot += sum(op["sizes"])
        else:
            tot += sum(op["counts"]) * ESZ[op["dtype"]]
    return tot


def expected(plan, world):
    """Concatenated bytes every rank must hold after the chain (allreduce and
    broadcast results are identical everywhere, and allgather lands every
    rank's data everywhere)."""
    from oracle import oracle as O
    parts = []
    for op in plan:
        kind = op["kind"]
        if kind in ("allreduce", "host"):
            xs = [O.fill(op["count"], op["dtype"], op["seed"], r) for r in range(world)]
            parts.append(np.frombuffer(O.expected_allreduce(xs, op["dtype"], op["op"]).tobytes(), np.uint8))
        elif kind == "bcast":
            parts.append(np.frombuffer(O.fill(op["bytes"], 1, op["seed"], op["root"]).tobytes(), np.uint8))
        elif kind == "allgather":
            for r, s in enumerate(op["sizes"]):
                parts.append(np.frombuffer(O.fill(s, 1, op["seed"], r).tobytes(), np.uint8))
        else:
            for b, c in enumerate(op["counts"]):
                xs = [O.fill(c, op["dtype"], op["seed"] + b, r) for r in range(world)]
                parts.append(np.frombuffer(O.expected_allreduce(xs, op["dtype"], op["op"]).tobytes(), np.uint8))
    return np.concatenate(parts) if parts else np.zeros(0, np.uint8)


# ---------------------------------------------------------------------------
# The covering chain: every ordered pair of launch kinds, once each.
#
# LAUNCH_KINDS names what a device-buffer call can leave behind as the
# predecessor on the shared channel (RDC_KIND_* in rdc_common.h): the five
# forced allreduce schedules, the registered-buffer schedule taken by an
# automatic allreduce above RDC_DIRECT_BYTES (the test sets 256K), broadcast,
# allgather, a coalesced list, and the four newer kernels with both forms of
# the all-to-all and both modes of the scan.
LAUNCH_KINDS = ("mesh", "ring", "mesh_pull", "oneshot", "tree", "direct", "bcast", "allgather", "coalesced",
                "rscatter", "alltoall", "alltoallv", "rooted", "scan", "exscan")
ALLREDUCE_ALGO = {"mesh": 2, "ring": 1, "mesh_pull": 5, "oneshot": 3, "tree": 4, "direct": 0}
# the algo RdcCommLastLaunch must report after the call (6: the direct schedule)
RECORDED_ALGO = {"mesh": 2, "ring": 1, "mesh_pull": 5, "oneshot": 3, "tree": 4, "direct": 6}
REDUCING = ("mesh", "ring", "mesh_pull", "oneshot", "tree", "direct", "coalesced", "rscatter", "rooted", "scan",
            "exscan")
COVER_ESZ = dict(ESZ)
COVER_ESZ.update({12: 8, 13: 8})
# PAIRS, then fp32 / fp16 / int8 Prod, uint32 BitAND, uint64 BitXOR
COVER_PAIRS = PAIRS + [(6, 8), (10, 8), (0, 8), (3, 9), (5, 10)]
# the MaxLoc / MinLoc (value, index) pairs: kinds that reduce only
LOC_PAIRS = [(12, 4), (13, 5)]
COVER_COUNTS = (1, 7, 1001, 4099, 65536 + 3, 300001)
COALESCED_COUNTS = (0, 1, 5, 1024, 33333, 65536 + 3)
A2AV_LENGTHS = (1, 15, 17, 4097, 16384, 70001, 100003, 3 * 65536 + 5)
COVER_SCRATCH = 64 << 20     # RDC_SCRATCH_BYTES of the GPU test
DIRECT_BUFFER = 1 << 20      # a `direct` step: this many bytes plus one element
RING_MINCOUNT = 1            # the default rdc_reduce_ring_mincount, in bytes
SENTINEL = 0xA5              # what an all-to-all's receive buffer holds outside its segments


def alltoall_cap(world, scratch=COVER_SCRATCH):
    """RdcPlanAlltoallCap: the longest segment one all-to-all launch carries."""
    import ctypes
    from rdc_amd._lib import _LIB
    cap = ctypes.c_uint64()
    assert _LIB.RdcPlanAlltoallCap(world, scratch, ctypes.byref(cap)) == 0
    return int(cap.value)


def euler_walk(rng, kinds):
    """Hierholzer's algorithm on the complete directed graph over `kinds`,
    self-loops included, the edge lists shuffled by rng: a closed walk of
    len(kinds)^2 + 1 nodes in which every ordered pair is adjacent once."""
    adj = {}
    for k in kinds:
        adj[k] = list(kinds)
        rng.shuffle(adj[k])
    stack, walk = [rng.choice(list(kinds))], []
    while stack:
        v = stack[-1]
        if adj[v]:
            stack.append(adj[v].pop())
        else:
            walk.append(stack.pop())
    walk.reverse()
    return walk


def _a2av_matrix(rng, world, cap):
    """M[r][p] = bytes r -> p.  One matrix in eight is all zeros; about one in
    four has a rank that neither sends nor receives."""
    if rng.randrange(8) == 0:
        return [[0] * world for _ in range(world)]
    M = [[min(cap, rng.choice(A2AV_LENGTHS) + rng.randrange(16)) if rng.random() < 0.75 else 0
          for _ in range(world)] for _ in range(world)]
    if rng.randrange(4) == 0:
        idle = rng.randrange(world)
        M[idle] = [0] * world
        for r in range(world):
            M[r][idle] = 0
    return M


def a2av_layout(M, sgap, rgap):
    """Per rank: (send offsets, send lengths, send bytes, receive offsets,
    receive lengths); and the receive buffer's size, the same on every rank
    (the largest), so that the blob's layout does not depend on the rank."""
    n = len(M)
    rows = []
    for r in range(n):
        slen, rlen = [M[r][p] for p in range(n)], [M[p][r] for p in range(n)]
        soff, at = [], 0
        for l in slen:
            soff.append(at)
            at += l + sgap
        stotal = at
        roff, at = [], 0
        for l in rlen:
            roff.append(at)
            at += l + rgap
        rows.append((soff, slen, stotal, roff, rlen, at))
    rtotal = max(row[5] for row in rows)
    return [row[:5] for row in rows], rtotal


def make_cover_plan(seed, world, host_every=8):
    """The walk of euler_walk with per-step parameters, and after every
    host_every-th launch one synchronous host-buffer allreduce (kind "host":
    not a node of the walk).  Every step carries "out", the bytes of its
    outputs in the blob, equal on every rank."""
    rng = random.Random(seed)
    cap = alltoall_cap(world)
    plan = []
    for k, kind in enumerate(euler_walk(rng, LAUNCH_KINDS)):
        dt, op = rng.choice(COVER_PAIRS + LOC_PAIRS if kind in REDUCING else COVER_PAIRS)
        esz = COVER_ESZ[dt]
        count = rng.choice(COVER_COUNTS)
        step = {"kind": kind, "dtype": dt, "op": op, "count": count, "off": rng.randrange(2),
                "seed": 0xC0FE0000 + 1000 * k}
        if kind in ALLREDUCE_ALGO:
            if kind == "direct":
                step["count"] = count = DIRECT_BUFFER // esz + 1
            elif kind != "tree" and count * esz <= RING_MINCOUNT:
                # a buffer of at most rdc_reduce_ring_mincount bytes takes the tree order whatever
                # the algo: two elements, so that the step stays a launch of its own kind
                step["count"] = count = 2
            step["algo"] = ALLREDUCE_ALGO[kind]
            step["out"] = count * esz
        elif kind in ("rscatter", "scan", "exscan"):
            step["out"] = count * esz
        elif kind == "rooted":
            step["root"] = rng.randrange(world)
            step["out"] = count * esz
        elif kind == "bcast":
            step["root"] = rng.randrange(world)
            step["out"] = count * esz
        elif kind == "allgather":
            step["sizes"] = [rng.choice([0, 3, 64, count * esz]) for _ in range(world)]
            step["out"] = sum(step["sizes"])
        elif kind == "coalesced":
            nb = rng.randint(2, 6)
            # two live buckets at least: a list with one runs as a plain allreduce, an empty one not at all
            step["counts"] = [rng.choice(COALESCED_COUNTS[1:] if b < 2 else COALESCED_COUNTS) for b in range(nb)]
            step["algo"] = rng.choice([0, 1, 2, 5])
            step["out"] = sum(step["counts"]) * esz
        elif kind == "alltoall":
            step["bytes"] = min(cap, count * esz)
            step["out"] = world * step["bytes"]
        elif kind == "alltoallv":
            step["M"] = _a2av_matrix(rng, world, cap)
            step["sgap"], step["rgap"] = rng.randrange(1, 9), rng.randrange(1, 9)
            step["out"] = a2av_layout(step["M"], step["sgap"], step["rgap"])[1]
        else:
            raise ValueError(kind)
        plan.append(step)
        if (k + 1) % host_every == 0:
            dt, op = rng.choice(PAIRS)
            n = rng.randint(1, 20000)
            plan.append({"kind": "host", "dtype": dt, "op": op, "count": n, "seed": 0xC0FE0000 + 1000 * k + 500,
                         "out": n * COVER_ESZ[dt]})
    return plan


def cover_offsets(plan):
    """Byte offset of every step's outputs in the blob; the last entry is the
    blob's size."""
    offs = [0]
    for step in plan:
        offs.append(offs[-1] + step["out"])
    return offs


def is_float_step(step):
    return step["kind"] in REDUCING + ("host",) and step["dtype"] in (6, 7, 10, 11)


def cover_inputs(step, world, seed=None, count=None):
    """Per-rank inputs of a reducing step: the oracle's generator (the bits
    RdcFill writes) for the reference (dtype, op) pairs and the integer ops,
    ops_ref's finite factors for a floating-point Prod, loc_ref's for pairs."""
    from oracle import oracle as O
    dt, op = step["dtype"], step["op"]
    seed = step["seed"] if seed is None else seed
    count = step["count"] if count is None else count
    if dt in (12, 13):
        from tests import loc_ref
        return loc_ref.gen_inputs(seed, world, count, dt)
    if op == 8 and dt in O.FLOAT_DTYPES:
        from tests import ops_ref
        return ops_ref.gen_inputs(seed, world, count, dt)
    return [O.fill(count, dt, seed, r) for r in range(world)]


def uses_fill(step):
    """True where cover_inputs is the oracle's generator, which RdcFill restates on the device."""
    return not (step["dtype"] in (12, 13) or (step["op"] == 8 and step["dtype"] in (6, 7, 10, 11)))


def _fold(order, xs, dt, op, exclusive=False):
    """The project's pinned references: the oracle for the reference ops'
    ring and tree orders, tests/ops_ref.py for ops 8 / 9 / 10 and for the
    scan and reduce-scatter of every op, tests/loc_ref.py for the pairs."""
    from oracle import oracle as O
    from tests import loc_ref, ops_ref
    if dt in (12, 13):
        if order == "scan":
            return loc_ref.scan(xs, op, exclusive)
        return {"ring": loc_ref.ring, "tree": loc_ref.tree, "rscatter": loc_ref.reduce_scatter}[order](xs, op)
    if order == "scan":
        return ops_ref.scan(xs, op, exclusive, dt)
    if order == "rscatter":
        return ops_ref.reduce_scatter(xs, op, dt)
    if op in (8, 9, 10):
        return {"ring": ops_ref.ring, "tree": ops_ref.tree}[order](xs, op, dt)
    return {"ring": O.expected_allreduce, "tree": O.expected_tree}[order](xs, dt, op)


def _u8(a):
    return np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8)


def expected_step(step, world):
    """Per rank, the bytes of the step's outputs in the worker's order."""
    from oracle import oracle as O
    from tests import ops_ref
    kind = step["kind"]
    dt, op = step["dtype"], step["op"]

    def checked(a):
        if is_float_step(step):  # the blob is compared as bytes: a NaN would still compare, but none is meant
            ops_ref.assert_finite(a, dt, step)
        return _u8(a)

    if kind in ALLREDUCE_ALGO or kind == "host":
        xs = cover_inputs(step, world)
        return [checked(_fold("tree" if kind == "tree" else "ring", xs, dt, op))] * world
    if kind == "coalesced":
        parts = [checked(_fold("ring", cover_inputs(step, world, step["seed"] + b, c), dt, op))
                 for b, c in enumerate(step["counts"])]
        return [np.concatenate(parts)] * world
    if kind == "rscatter":
        return [checked(a) for a in _fold("rscatter", cover_inputs(step, world), dt, op)]
    if kind == "rooted":
        xs = cover_inputs(step, world)
        full = checked(_fold("ring", xs, dt, op))
        return [full if r == step["root"] else _u8(xs[r]) for r in range(world)]
    if kind in ("scan", "exscan"):
        return [checked(a) for a in _fold("scan", cover_inputs(step, world), dt, op, kind == "exscan")]
    if kind == "bcast":
        return [_u8(O.fill(step["out"], 1, step["seed"], step["root"]))] * world
    if kind == "allgather":
        return [np.concatenate([_u8(O.fill(s, 1, step["seed"], r)) for r, s in enumerate(step["sizes"])])] * world
    if kind == "alltoall":
        b = step["bytes"]
        sends = [O.fill(world * b, 1, step["seed"], r) for r in range(world)]
        return [np.concatenate([sends[r][p * b: (p + 1) * b] for r in range(world)]) for p in range(world)]
    if kind == "alltoallv":
        rows, rtotal = a2av_layout(step["M"], step["sgap"], step["rgap"])
        sends = [O.fill(rows[r][2], 1, step["seed"], r) for r in range(world)]
        want = [np.full(rtotal, SENTINEL, np.uint8) for _ in range(world)]
        for r in range(world):
            for p in range(world):
                ln = step["M"][r][p]
                want[p][rows[p][3][r]: rows[p][3][r] + ln] = sends[r][rows[r][0][p]: rows[r][0][p] + ln]
        return want
    raise ValueError(kind)


def expected_cover(plan, world):
    """Per rank, the concatenated bytes it must hold after the chain (a blob
    per rank: reduce-scatter, rooted reduce, scan and all-to-all leave
    different bytes on different ranks).  Asserts that no floating-point
    step's expected data holds a NaN or an inf."""
    parts = [[] for _ in range(world)]
    for step in plan:
        outs = expected_step(step, world)
        for r in range(world):
            assert outs[r].size == step["out"], (step, r, outs[r].size)
            parts[r].append(outs[r])
    return [np.concatenate(p) for p in parts]


def describe(step):
    """A step's kind and parameters on one line (a length matrix in full)."""
    return "%s %s" % (step["kind"], ", ".join("%s=%s" % (k, step[k]) for k in sorted(step) if k not in ("kind", "out")))


def first_mismatch(plan, got, want):
    """None, or (step index, first differing byte inside the step, number of
    differing bytes in the step) of the first step whose bytes differ."""
    if got.tobytes() == want.tobytes():
        return None
    first = int(np.flatnonzero(got != want)[0])
    offs = cover_offsets(plan)
    for k in range(len(plan)):
        if offs[k] <= first < offs[k + 1]:
            bad = int((got[offs[k]: offs[k + 1]] != want[offs[k]: offs[k + 1]]).sum())
            return k, first - offs[k], bad
    raise AssertionError("byte %d outside the blob" % first)


def mismatch_report(plan, rank, got, want):
    """None, or the message for rank's blob: the step, its predecessor (the
    launch before it, host calls skipped), the rank and the byte."""
    hit = first_mismatch(plan, got, want)
    if hit is None:
        return None
    k, byte, bad = hit
    prev = [j for j in range(k) if plan[j]["kind"] != "host"]
    return ("step %d [%s] after step %s [%s]: rank %d differs at %d of %d bytes, first at byte %d of the step"
            % (k, describe(plan[k]), prev[-1] if prev else "-", describe(plan[prev[-1]]) if prev else "none",
               rank, bad, plan[k]["out"], byte))
