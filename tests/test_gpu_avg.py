"""GPU parity of Avg, the mean across ranks of float32 / float64 / float16 /
bfloat16 buffers (RdcCommAllreduceAvg / RdcCommReduceScatterAvg /
RdcCommReduceToAvg and the blocking entries) against the numpy restatement of
its rule (tests/avg_ref.py), bit for bit.  Every buffer sits between 4 KiB of sentinel
bytes which no rank may change; a reduce-scatter leaves every byte outside
chunk `rank` as passed, a rooted reduce every non-root buffer.

* single-process groups: tests/avg_group_cases.py, run once in a process of
  its own (tests/acc32_group_cases.py says why), every case of it reported here;
* multi-process: n processes on GPU 0, tests/mp_avg_worker.py (n = 12 runs
  the 16-rank instantiations).
"""
import json
import os
import subprocess
import sys
import xml.etree.ElementTree as ET

import numpy as np
import pytest

from oracle import oracle as O
from tests import acc32_ref
from tests import avg_ref as A
from tests import ops_ref
from tests.conftest import ROOT
from tests.gpu_util import same_bits
from tests.test_gpu_reduce_scatter import run_mp
from tests.test_gpu_reduce_to import GUARD, SENTINEL

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

WORKER = os.path.join(ROOT, "tests", "mp_avg_worker.py")
GROUP_CASES_FILE = os.path.join(ROOT, "tests", "avg_group_cases.py")
F32, F64, F16, BF = A.F32, A.F64, A.F16, A.BF

# ------------------------------------------------------- single-process groups
GROUP_CASES = (
    ["test_group_counts_offsets_and_roots[%d-%d]" % (n, dt) for n in (3, 2) for dt in A.DTYPES] +
    ["test_group3_is_not_sum_then_divide[%d]" % dt for dt in A.DTYPES] +
    ["test_group3_order_table[%d]" % dt for dt in A.DTYPES] +
    ["test_group_specials[%d-%d]" % (n, dt) for n in (3, 2) for dt in A.DTYPES] +
    ["test_group_multi_piece[ar-6-0]", "test_group_multi_piece[rs-11-0]", "test_group_multi_piece[rt-7-1]",
     "test_group_multi_piece[ar-10-0]",
     "test_group_tuned_shapes_stay_exact[1-14-0-0]", "test_group_tuned_shapes_stay_exact[7-1-24-65536]",
     "test_group_refusals_launch_nothing", "test_group_graph_capture_replay"])


@pytest.fixture(scope="module")
def group_report(tmp_path_factory):
    """{case: None if it passed, else what went wrong}, from one run of
    tests/avg_group_cases.py in a child process.  The run stops at the first
    failure: a case after it is reported as not run."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    xml = str(tmp_path_factory.mktemp("avg_groups") / "report.xml")
    p = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                        "--junitxml", xml, GROUP_CASES_FILE], cwd=ROOT, capture_output=True, text=True, timeout=600)
    tail = (p.stdout[-3000:] + p.stderr[-2000:])
    assert os.path.exists(xml), "the group cases did not run:\n" + tail
    report = {}
    for tc in ET.parse(xml).getroot().iter("testcase"):
        bad = [e for e in tc if e.tag in ("failure", "error", "skipped")]
        report[tc.get("name")] = None if not bad else "%s: %s" % (bad[0].tag, (bad[0].text or bad[0].get("message") or "")[-3000:])
    return report, tail


@pytest.mark.parametrize("case", GROUP_CASES)
def test_group(group_report, case):
    report, tail = group_report
    assert case in report, "not run (an earlier case failed, or the run ended):\n" + tail
    assert report[case] is None, report[case]


def test_group_cases_are_all_listed(group_report):
    assert sorted(group_report[0]) == sorted(GROUP_CASES)


# --------------------------------------------------------------- multi-process
def unguard(backing, count, dtype, pad=0):
    """The payload of a saved guarded buffer; asserts its sentinels."""
    lo, nb = GUARD + pad, count * A.ESIZE[dtype]
    assert backing.size == nb + 2 * GUARD + pad
    assert (backing[:lo] == SENTINEL).all() and (backing[lo + nb:] == SENTINEL).all(), "guard bytes changed"
    return np.frombuffer(backing[lo: lo + nb].tobytes(), dtype=O.NP_DTYPE[dtype])


def case_inputs(c, world):
    if c.get("data") == "order":
        return A.order_table(world, c["dtype"], count=c["count"])
    return A.gen_inputs(c.get("seed", 0x5EEDB000), world, c["count"], c["dtype"])


def assert_rank(which, got, r, inputs, full, dtype, root, what):
    """One rank's payload after collective `which`."""
    mine = inputs[r]
    if which in ("ar", "sum", "acc32") or (which == "rt" and r == root):
        assert same_bits(got, full, dtype), (what, "result of rank", r)
    elif which == "rs":
        b, e = O.split(mine.size, len(inputs))[r]
        assert same_bits(got[b:e], full[b:e], dtype), (what, "chunk of rank", r)
        assert got[:b].tobytes() == mine[:b].tobytes() and got[e:].tobytes() == mine[e:].tobytes(), \
            (what, "bytes outside the chunk of rank", r)
    else:
        assert got.tobytes() == mine.tobytes(), (what, "buffer of non-root rank", r)


BIG = (1 << 20) + 5


@pytest.mark.parametrize("world", [4, 5, 8, 12])
def test_mp_collectives(world):
    """n = 4, 5, 8: the 8-rank instantiations; n = 12: the 16-rank ones.  1001
    and 1 Mi + 5 elements, the generator's data and the order table; all three
    collectives and all four dtypes in every world."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cases = [
        {"kind": "coll", "which": "ar", "count": 1001, "dtype": F16, "pad": 2},
        {"kind": "coll", "which": "ar", "count": 1001, "dtype": F64, "data": "order", "pad": 8},
        {"kind": "coll", "which": "rs", "count": 1001, "dtype": BF, "pad": 6},
        {"kind": "coll", "which": "rt", "count": 1001, "dtype": F32, "data": "order", "root": world - 1, "pad": 4},
        {"kind": "coll", "which": "ar", "count": BIG, "dtype": F32, "seed": 0x5EEDB100},
        {"kind": "coll", "which": "ar", "count": BIG, "dtype": BF, "data": "order"},
        {"kind": "coll", "which": "rs", "count": BIG, "dtype": F64, "seed": 0x5EEDB200},
        {"kind": "coll", "which": "rt", "count": BIG, "dtype": F16, "data": "order", "root": 1, "pad": 2},
    ]
    tmp = run_mp(world, cases, worker=WORKER)
    for i, c in enumerate(cases):
        inputs = case_inputs(c, world)
        full = A.allreduce(inputs, c["dtype"])
        ops_ref.assert_finite(full, c["dtype"], (world, i))
        for r in range(world):
            backing = np.load(os.path.join(tmp, "case%d_rank%d.npy" % (i, r)))
            info = json.load(open(os.path.join(tmp, "case%d_rank%d.json" % (i, r))))
            got = unguard(backing, c["count"], c["dtype"], c.get("pad", 0))
            assert_rank(c["which"], got, r, inputs, full, c["dtype"], c.get("root", 0), (world, i, c))
            assert info["launch"][5] == 2, info


CHAIN = [("ar", 0), ("sum", 0), ("acc32", 0), ("rs", 0), ("rt", 2)]


@pytest.mark.parametrize("world,dtype", [(4, BF), (5, F16)])
def test_mp_back_to_back_in_poison_mode(world, dtype):
    """avg allreduce -> ordinary Sum allreduce -> acc32 allreduce -> avg
    reduce-scatter -> avg rooted reduce with no host sync between them,
    consumed scratch poisoned: the siblings' slot-reuse argument holds for the
    fold with the division."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    count = 50001
    case = {"kind": "chain", "count": count, "dtype": dtype, "steps": CHAIN, "seed": 0x5EEDB300}
    tmp = run_mp(world, [case], worker=WORKER)
    inputs = case_inputs(case, world)
    want = {"avg": A.allreduce(inputs, dtype), "sum": ops_ref.ring(inputs, ops_ref.OP_SUM, dtype),
            "acc32": acc32_ref.allreduce(inputs, dtype)}
    for v in want.values():
        ops_ref.assert_finite(v, dtype)
    for r in range(world):
        backing = np.load(os.path.join(tmp, "case0_rank%d.npy" % r))
        for k, (which, root) in enumerate(CHAIN):
            got = unguard(backing[k], count, dtype)
            assert_rank(which, got, r, inputs, want.get(which, want["avg"]), dtype, root, (world, k, which))


def test_mp_host_buffers_and_python_surface():
    """The six blocking entries on guarded host arrays; numpy float32 /
    float64 / float16 and torch tensors of all four dtypes through
    rdc_amd.allreduce / reduce_scatter / reduce and the Comm methods with
    average=True (and accumulate="float32" on 16-bit data)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    world, count, root = 3, 50001, 1
    cases = [{"kind": "host", "count": count, "dtype": BF, "root": root, "seed": 0x5EEDB400},
             {"kind": "host", "count": count, "dtype": F16, "root": root, "data": "order"},
             {"kind": "host", "count": count, "dtype": F32, "root": root, "seed": 0x5EEDB410},
             {"kind": "host", "count": count, "dtype": F64, "root": root, "data": "order"}] + \
            [{"kind": "py", "count": count, "dtype": dt, "root": root, "seed": 0x5EEDB500 + dt} for dt in A.DTYPES]
    tmp = run_mp(world, cases, worker=WORKER)
    host_steps = ["ar", "rs", "rt", "ar", "rs", "rt"]
    py_np = ["ar", "ar", "rt", "rs"]
    py_torch = ["ar", "ar", "rs", "rs", "rt", "rt"]
    for i, c in enumerate(cases):
        dtype = c["dtype"]
        inputs = case_inputs(c, world)
        full = A.allreduce(inputs, dtype)
        steps = host_steps if c["kind"] == "host" else (py_np if dtype != BF else []) + py_torch
        for r in range(world):
            backing = np.load(os.path.join(tmp, "case%d_rank%d.npy" % (i, r)))
            info = json.load(open(os.path.join(tmp, "case%d_rank%d.json" % (i, r))))
            assert backing.shape[0] == len(steps)
            for k, which in enumerate(steps):
                assert_rank(which, unguard(backing[k], count, dtype), r, inputs, full, dtype, root, (i, r, k, which))
            if c["kind"] == "py":
                assert all(info["flags"]) and len(info["flags"]) == len(steps), info


@pytest.mark.parametrize("world,root", [(2, 1), (4, 0)])
def test_cpp_avg_through_the_launcher(world, root, tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    exe = str(tmp_path / "avg")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "avg.cc"), "-o", exe,
                           "-L", os.path.join(ROOT, "rdc_amd"), "-lrdc_amd",
                           "-Wl,-rpath," + os.path.join(ROOT, "rdc_amd")])
    env = dict(os.environ, RDC_SCRATCH_BYTES="64M")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "-m", "rdc_amd.launcher", "-n", str(world), "--gpus", "1", exe, "100003",
                        str(root)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    for r in range(world):
        assert "rank %d: avg OK (world %d, N 100003, root %d)" % (r, world, root) in p.stdout, p.stdout
