#!/usr/bin/env python
"""Cost and accuracy of the float32-accumulated Sum on bfloat16 buffers.

Per size (MiB of bfloat16 per rank), on the "main" communicator and the
process's current stream, three forms in alternating rounds:

  a  sum_mesh   RdcCommAllreduceEx(bf16, SUM, algo 2): the ordinary Sum on the
                same schedule, rounding at every hop (the baseline)
  b  acc32      RdcCommAllreduceAcc32: float32 accumulator, one rounding
  c  upcast     what a caller did before it existed: cast the buffer to
                float32, automatic float32 Sum allreduce, cast back (two extra
                passes over memory and twice the bytes exchanged)

A round's time is the slowest rank's wall time per call over `calls` calls
enqueued back to back and ended by a device synchronise; the figure is the
median over the rounds, with the min and max next to it.  Every form is warmed
at every size, and the buffer is refilled before each round (repeated in-place
sums grow).  b_over_a and b_over_c are ratios of the medians.

The error report runs a and b once on a fixed seeded input (exponents
2^-20 .. 2^20, full mantissas, 1 Mi elements) and gives the largest and the
mean error of every element against the float64 sum of the ranks' values, in
bfloat16 ulps of that sum.

    python -m rdc_amd.launcher -n N --gpus 1 python tools/acc32_bench.py [sizes_MiB] [calls] [rounds] [out.json]
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
ERR_COUNT = 1 << 20


def gen_bf16(seed, rank, count):
    """bfloat16 bits: random sign, exponent field 107..147, 7 random mantissa bits."""
    rng = np.random.default_rng([seed, rank])
    return ((rng.integers(0, 2, count).astype(np.uint16) << 15) | (rng.integers(107, 148, count).astype(np.uint16) << 7) |
            rng.integers(0, 128, count).astype(np.uint16)).astype(np.uint16)


def bf16_to_f64(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def main():
    sizes = [float(x) for x in (sys.argv[1] if len(sys.argv) > 1 else "1,16,256").replace("/", ",").split(",")]
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    out_path = sys.argv[4] if len(sys.argv) > 4 else None
    import torch
    import rdc_amd
    from rdc_amd._lib import _LIB, check_call
    if not torch.cuda.is_available():
        raise SystemExit("acc32_bench needs a GPU")
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")) % torch.cuda.device_count())
    rdc_amd.init([])
    rank, world = rdc_amd.get_rank(), rdc_amd.get_world_size()
    comm = rdc_amd.get_comm("main")
    sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def slowest(t):
        return float(rdc_amd.allreduce(np.array([t], dtype=np.float64), rdc_amd.Op.MAX)[0])

    big = int(max(max(sizes) * (1 << 20) // 2, ERR_COUNT))
    src = torch.from_numpy(gen_bf16(0xACC32, rank, big).view(np.int16)).cuda().view(torch.bfloat16)
    buf = torch.empty_like(src)
    wide = torch.empty(big, dtype=torch.float32, device="cuda")
    p, q = ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(wide.data_ptr())

    # ---- error against the float64 sum, forms a and b
    errors = {}
    xs = [bf16_to_f64(gen_bf16(0xACC32, r, big)[:ERR_COUNT]) for r in range(world)]
    exact = np.sum(xs, axis=0)
    with np.errstate(divide="ignore"):
        ulp = np.exp2(np.floor(np.log2(np.abs(exact))) - 7)
    ok = exact != 0
    for name, run in (("sum_mesh", lambda: _LIB.RdcCommAllreduceEx(comm.handle, p, ERR_COUNT, BF16, SUM, 2, sp)),
                      ("acc32", lambda: _LIB.RdcCommAllreduceAcc32(comm.handle, p, ERR_COUNT, BF16, sp))):
        buf.copy_(src)
        check_call(run())
        comm.check(sp)
        got = bf16_to_f64(buf[:ERR_COUNT].view(torch.int16).cpu().numpy().view(np.uint16))
        e = np.abs(got - exact)[ok] / ulp[ok]
        errors[name] = {"max_ulp": round(float(e.max()), 3), "mean_ulp": round(float(e.mean()), 4)}

    # ---- time
    out = {}
    for mib in sizes:
        n = int(mib * (1 << 20)) // 2

        def sum_mesh():
            check_call(_LIB.RdcCommAllreduceEx(comm.handle, p, n, BF16, SUM, 2, sp))

        def acc32():
            check_call(_LIB.RdcCommAllreduceAcc32(comm.handle, p, n, BF16, sp))

        def upcast():
            wide[:n].copy_(buf[:n])
            check_call(_LIB.RdcCommAllreduceEx(comm.handle, q, n, F32, SUM, 0, sp))
            buf[:n].copy_(wide[:n])

        forms = (("sum_mesh", sum_mesh), ("acc32", acc32), ("upcast", upcast))

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
            for name, fn in forms:
                ts.setdefault(name, []).append(timed(fn))
        comm.check(sp)
        row = {}
        for name, v in ts.items():
            v.sort()
            row[name] = {"ms": round(v[len(v) // 2] * 1e3, 4), "min": round(v[0] * 1e3, 4), "max": round(v[-1] * 1e3, 4)}
        row["b_over_a"] = round(row["acc32"]["ms"] / row["sum_mesh"]["ms"], 3)
        row["b_over_c"] = round(row["acc32"]["ms"] / row["upcast"]["ms"], 3)
        ll = (ctypes.c_uint64 * 6)()
        acc32()
        check_call(_LIB.RdcCommLastLaunch(comm.handle, ll))
        comm.check(sp)
        row["acc32_grid_scatter_reduce_gather_tile"] = [int(x) for x in ll[:5]]
        out["%g MiB" % mib] = row
    if rank == 0:
        line = json.dumps({"acc32_bench_ms_per_call": out, "error_vs_float64_sum_bf16_ulps": errors, "world": world,
                           "dtype": "bfloat16", "calls": calls, "rounds": rounds, "ranks_share_gpu": True,
                           "error_elements": ERR_COUNT})
        print(line, flush=True)
        if out_path:
            os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
            open(out_path, "w").write(line + "\n")
    rdc_amd.barrier()
    rdc_amd.finalize()


if __name__ == "__main__":
    main()
