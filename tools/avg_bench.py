#!/usr/bin/env python
"""Cost of Avg (the mean across ranks, divided inside the allreduce) against
the sum a caller divides afterwards.

Per dtype (float32, bfloat16) and size (MiB per rank), on the "main"
communicator and the process's current stream, three forms in alternating
rounds:

  a  avg       RdcCommAllreduceAvg
  b  sum       the sibling without the division: RdcCommAllreduceEx(float32,
               SUM, algo 2: the mesh) / RdcCommAllreduceAcc32(bfloat16)
  c  sum_div   b followed by tensor.div_(n) on the same stream: what a caller
               does today (one more launch, one more read and write of the
               buffer)

A round's time is the slowest rank's wall time per call over `calls` calls
enqueued back to back and ended by a device synchronise; the figure is the
median over the rounds, with the min and max next to it.  Every form is warmed
at every size, and the buffer is refilled before each round.  a_over_c and
a_minus_b_ms come from the medians.  The ranks share one GPU: no xGMI link is
timed.

    python -m rdc_amd.launcher -n N --gpus 1 python tools/avg_bench.py [sizes_MiB] [calls] [rounds] [out.json]
"""
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BF16, F32, SUM = 11, 6, 2


def main():
    sizes = [float(x) for x in (sys.argv[1] if len(sys.argv) > 1 else "1,16,256").replace("/", ",").split(",")]
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    out_path = sys.argv[4] if len(sys.argv) > 4 else None
    import torch
    import rdc_amd
    from rdc_amd._lib import _LIB, check_call
    if not torch.cuda.is_available():
        raise SystemExit("avg_bench needs a GPU")
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")) % torch.cuda.device_count())
    rdc_amd.init([])
    rank, world = rdc_amd.get_rank(), rdc_amd.get_world_size()
    comm = rdc_amd.get_comm("main")
    sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def slowest(t):
        return float(rdc_amd.allreduce(np.array([t], dtype=np.float64), rdc_amd.Op.MAX)[0])

    out = {}
    for name, code, tdt, esz in (("float32", F32, torch.float32, 4), ("bfloat16", BF16, torch.bfloat16, 2)):
        big = int(max(sizes) * (1 << 20)) // esz
        g = torch.Generator(device="cuda")
        g.manual_seed(0xA76 + rank)
        src = torch.randn(big, dtype=torch.float32, device="cuda", generator=g).to(tdt)
        buf = torch.empty_like(src)
        p = ctypes.c_void_p(buf.data_ptr())
        rows = {}
        for mib in sizes:
            n = int(mib * (1 << 20)) // esz

            def avg():
                check_call(_LIB.RdcCommAllreduceAvg(comm.handle, p, n, code, sp))

            def plain():
                if code == F32:
                    check_call(_LIB.RdcCommAllreduceEx(comm.handle, p, n, F32, SUM, 2, sp))
                else:
                    check_call(_LIB.RdcCommAllreduceAcc32(comm.handle, p, n, BF16, sp))

            def sum_div():
                plain()
                buf[:n].div_(world)

            forms = (("avg", avg), ("sum", plain), ("sum_div", sum_div))

            def timed(fn):
                buf[:n].copy_(src[:n])
                torch.cuda.synchronize()
                rdc_amd.barrier()
                t0 = time.perf_counter()
                for _ in range(calls):
                    fn()
                torch.cuda.synchronize()
                return slowest((time.perf_counter() - t0) / calls)

            for _, fn in forms:   # warm every form at this size
                buf[:n].copy_(src[:n])
                for _ in range(2):
                    fn()
            comm.check(sp)
            ts = {}
            for _ in range(rounds):
                for form, fn in forms:
                    ts.setdefault(form, []).append(timed(fn))
            comm.check(sp)
            row = {}
            for form, v in ts.items():
                v.sort()
                row[form] = {"ms": round(v[len(v) // 2] * 1e3, 4), "min": round(v[0] * 1e3, 4),
                             "max": round(v[-1] * 1e3, 4)}
            row["a_over_c"] = round(row["avg"]["ms"] / row["sum_div"]["ms"], 3)
            row["a_minus_b_ms"] = round(row["avg"]["ms"] - row["sum"]["ms"], 4)
            rows["%g MiB" % mib] = row
        out[name] = rows
        del src, buf
    if rank == 0:
        line = json.dumps({"avg_bench_ms_per_call": out, "world": world, "calls": calls, "rounds": rounds,
                           "ranks_share_gpu": True})
        print(line, flush=True)
        if out_path:
            os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
            open(out_path, "w").write(line + "\n")
    rdc_amd.barrier()
    rdc_amd.finalize()


if __name__ == "__main__":
    main()
