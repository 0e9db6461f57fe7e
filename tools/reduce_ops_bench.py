"""RdcReduce (k_reduce) on large buffers: every listed (dtype, op) against Sum
of the same dtype and bytes, timed in one run with one method.

    python tools/reduce_ops_bench.py [--lib PATH] [--mib 1024] [--rounds 9] [--reps 10] [--only prod_i8,...]

Per dtype the forms alternate: `rounds` rounds of `reps` back-to-back calls per
form, HIP events around each round, after one untimed round.  Sum moves the same
bytes through the same kernel body and is memory-bound, so it is the yardstick:
each form's median ms per call is reported with its min / max over the rounds
and as a ratio to Sum's median, beside Sum's own min / max.  Timing does not
depend on the values; floats multiply by 1 so that they stay finite.
--lib loads another build of librdc_amd.so (the generic-loop variant of a
packed reduce16, for an A/B).  One JSON line.
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SUM, PROD, BITAND, BITXOR = 2, 8, 9, 10
# name -> (dtype code, torch dtype name, operators timed beside Sum)
FORMS = [("i8", 0, "int8", [PROD]), ("u8", 1, "uint8", [PROD, BITAND, BITXOR]), ("f16", 10, "float16", [PROD]),
         ("bf16", 11, "bfloat16", [PROD]), ("i32", 2, "int32", [PROD]), ("f32", 6, "float32", [PROD]),
         ("i64", 4, "int64", [PROD]), ("u64", 5, "int64", [BITAND, BITXOR]), ("f64", 7, "float64", [PROD])]
OPNAME = {SUM: "sum", PROD: "prod", BITAND: "bitand", BITXOR: "bitxor"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(ROOT, "rdc_amd", "librdc_amd.so"))
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    import torch
    lib = ctypes.CDLL(a.lib)
    lib.RdcReduce.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int,
                              ctypes.c_void_p]
    lib.RdcGetLastError.restype = ctypes.c_char_p
    nbytes = a.mib << 20
    only = set(x for x in a.only.split(",") if x)
    out = {"lib": os.path.basename(a.lib), "bytes": nbytes, "moved_bytes_per_call": 3 * nbytes, "rounds": a.rounds,
           "reps_per_round": a.reps, "forms": {}}
    for name, code, tname, ops in FORMS:
        if only and name not in only:
            continue
        tdt = getattr(torch, tname)
        count = nbytes // torch.empty(0, dtype=tdt).element_size()
        dst = torch.ones(count, dtype=tdt, device="cuda")
        src = torch.ones(count, dtype=tdt, device="cuda")
        if not tdt.is_floating_point:
            src.view(torch.uint8).random_(0, 256)
            dst.view(torch.uint8).random_(0, 256)
        ms = {op: [] for op in [SUM] + ops}
        for rnd in range(a.rounds + 1):
            for op in [SUM] + ops:
                if tdt.is_floating_point and op == SUM:
                    dst.fill_(1)  # keep sums finite too (not timed)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(a.reps):
                    rc = lib.RdcReduce(dst.data_ptr(), src.data_ptr(), count, code, op, None)
                    if rc != 0:
                        raise RuntimeError(lib.RdcGetLastError())
                e1.record()
                torch.cuda.synchronize()
                if rnd > 0:
                    ms[op].append(e0.elapsed_time(e1) / a.reps)
        base = sorted(ms[SUM])[len(ms[SUM]) // 2]
        for op, v in ms.items():
            v.sort()
            med = v[len(v) // 2]
            out["forms"]["%s_%s" % (OPNAME[op], name)] = {
                "median_ms": round(med, 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4),
                "TB_per_s": round(3 * nbytes / med / 1e9, 3), "over_sum_median": round(med / base, 4)}
        del dst, src
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
