"""Randomized stress of mixed collective chains (tests/mp_mixed_worker.py) at
2-5 processes on GPU 0, 80 ops per run, every output checked bit-exactly
against the CPU oracle.  python tests/stress_mixed.py (on the GPU box).

--cover runs the covering chain instead (tests/mixed_plan.make_cover_plan:
every ordered pair of launch kinds once per run) over a range of seeds,
worlds 2-5 in turn, poison mode on every other seed:
python tests/stress_mixed.py --cover --seeds 100 108"""
import argparse, os, subprocess, sys, tempfile
import numpy as np
sys.path.insert(0, os.getcwd())
from tests.mixed_plan import expected, expected_cover, make_cover_plan, make_plan, mismatch_report
from tests.conftest import free_port
ap = argparse.ArgumentParser()
ap.add_argument("--cover", action="store_true", help="the covering chain over --seeds")
ap.add_argument("--seeds", type=int, nargs=2, default=[100, 108], metavar=("FIRST", "END"),
                help="--cover: seeds FIRST .. END-1")
args = ap.parse_args()
if args.cover:
    runs = [(2 + k % 4, seed) for k, seed in enumerate(range(*args.seeds))]
else:
    runs = [(2, 21), (3, 22), (4, 23), (5, 24), (3, 25), (4, 26), (2, 27), (5, 28)]
fails = 0
for world, seed in runs:
    nops = 80
    tmp = tempfile.mkdtemp()
    port = free_port()
    env = dict(os.environ, RDC_DEVICE="0", RDC_NBLOCKS="24", RDC_SCRATCH_BYTES="64M")
    tail = [str(seed), str(nops)]
    if args.cover:
        env["RDC_DIRECT_BYTES"] = "256K"
        tail = [str(seed), str(seed % 2), "cover"]
    ps = [subprocess.Popen([sys.executable, "tests/mp_mixed_worker.py", str(r), str(world), str(port), tmp] + tail,
                           env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(world)]
    try:
        outs = [p.communicate(timeout=300)[0] for p in ps]
    except subprocess.TimeoutExpired:
        for p in ps: p.kill()
        raise
    ok = all(p.returncode == 0 for p in ps)
    if ok and args.cover:
        plan = make_cover_plan(seed, world)
        want = expected_cover(plan, world)
        for r in range(world):
            msg = mismatch_report(plan, r, np.load(os.path.join(tmp, "cover_rank%d.npy" % r)), want[r])
            if msg:
                ok = False
                print(msg)
    elif ok:
        want = expected(make_plan(seed, nops, world), world)
        for r in range(world):
            got = np.load(os.path.join(tmp, "mixed_rank%d.npy" % r))
            if got.tobytes() != want.tobytes():
                ok = False
    print("world %d seed %d: %s" % (world, seed, "OK" if ok else "FAIL"), flush=True)
    if not ok:
        fails += 1
        for o in outs: print(o[-1500:])
sys.exit(1 if fails else 0)
