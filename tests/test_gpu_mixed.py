"""GPU: randomized chains mixing every collective kind and schedule on one
communicator, stream-ordered with no host synchronisation between launches
(tests/mp_mixed_worker.py), as 3 and 4 processes on GPU 0 — exercises the
cross-launch protocol (one-shot slot halves and post-one-shot gates,
broadcast/allgather done-word gates, forwarded broadcasts, unit-table
coalesced launches) the way a training step interleaves them.  Every op's
output is checked bit-exactly against the CPU oracle.  The covering chain
(test_cover_chain_every_adjacent_pair) runs every ordered pair of the 15
launch kinds back to back once, the newer kernels, dtypes and ops included."""
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import pytest

from tests.conftest import ROOT, free_port
from tests.mixed_plan import expected, make_plan

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.mark.parametrize("world,seed", [(3, 11), (4, 12), (3, 13)])
def test_mixed_collective_chain(world, seed):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    nops = 40
    tmp = tempfile.mkdtemp(prefix="rdc_mixed_")
    port = free_port()
    env = dict(os.environ, RDC_DEVICE="0", RDC_NBLOCKS="32", RDC_SCRATCH_BYTES="64M")
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "mp_mixed_worker.py"), str(r), str(world),
                               str(port), tmp, str(seed), str(nops)], env=env, stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for r in range(world)]
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=150)[0])
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
    report = "\n".join("--- rank %d rc=%s\n%s" % (r, p.returncode, o[-2000:]) for r, (p, o) in enumerate(zip(procs, outs)))
    for p in procs:
        assert p.returncode == 0, report
    want = expected(make_plan(seed, nops, world), world)
    for r in range(world):
        got = np.load(os.path.join(tmp, "mixed_rank%d.npy" % r))
        assert got.size == want.size, (r, got.size, want.size)
        if got.tobytes() != want.tobytes():
            bad = np.nonzero(got != want)[0]
            raise AssertionError("rank %d: %d bytes differ, first at %d" % (r, bad.size, bad[0]))


# The chain above gives 40 launches 150 s, nearly all of it allowance for
# starting the ranks (imports, the rendezvous, the channel's self-check).  The
# covering chain starts as many ranks once and then issues 226 launches and 28
# host calls of at most 2.4 MB each, a few seconds of GPU time (measured: the
# ranks of a case run 3 s in all), so the same allowance holds.  Every
# device-side wait is bounded by RDC_TIMEOUT (tests/conftest.py: 30 s): a rank
# that hangs reports an error long before this, and a hit timeout is a hang.
COVER_TIMEOUT = 150


@pytest.mark.parametrize("world,seed,poison", [(3, 21, 1), (4, 22, 1), (3, 23, 0)])
def test_cover_chain_every_adjacent_pair(world, seed, poison):
    """tests/mixed_plan.make_cover_plan: a seeded Eulerian circuit over the 15
    launch kinds, so every ordered pair (predecessor, successor) of DESIGN.md
    4.2's table runs back to back exactly once, at sizes, dtypes, ops and
    offsets drawn per step, on one stream with no host synchronisation, with
    synchronous host-buffer allreduces in between.  Every rank's outputs are
    compared byte for byte with the pinned references, and a mismatch names
    the step and its predecessor."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tests.mixed_plan import RECORDED_ALGO, describe, expected_cover, make_cover_plan, mismatch_report
    tmp = tempfile.mkdtemp(prefix="rdc_cover_")
    port = free_port()
    env = dict(os.environ, RDC_DEVICE="0", RDC_NBLOCKS="32", RDC_SCRATCH_BYTES="64M", RDC_DIRECT_BYTES="256K")
    t0 = time.time()
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "mp_mixed_worker.py"), str(r), str(world),
                               str(port), tmp, str(seed), str(poison), "cover"], env=env, stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for r in range(world)]
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=COVER_TIMEOUT)[0])
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
    print("cover chain world %d seed %d poison %d: ranks ran %.1f s" % (world, seed, poison, time.time() - t0))
    report = "\n".join("--- rank %d rc=%s\n%s" % (r, p.returncode, o[-2000:]) for r, (p, o) in enumerate(zip(procs, outs)))
    for p in procs:
        assert p.returncode == 0, report
    plan = make_cover_plan(seed, world)
    want = expected_cover(plan, world)
    for r in range(world):
        got = np.load(os.path.join(tmp, "cover_rank%d.npy" % r))
        assert got.size == want[r].size, (r, got.size, want[r].size)
        msg = mismatch_report(plan, r, got, want[r])
        if msg:
            raise AssertionError(msg)
    for r in range(world):
        info = json.load(open(os.path.join(tmp, "cover_rank%d.json" % r)))
        for k, step in enumerate(plan):
            if step["kind"] not in RECORDED_ALGO:
                continue
            algo = info["algos"][str(k)]
            if step["kind"] == "direct" and algo != 6:
                raise AssertionError("step %d [%s] on rank %d fell back to algo %d: direct_fallback %d, "
                                     "direct_fail_reason %d" % (k, describe(step), r, algo, info["direct_fallback"],
                                                                info["direct_fail_reason"]))
            assert algo == RECORDED_ALGO[step["kind"]], (k, describe(step), "rank", r, "recorded algo", algo)
