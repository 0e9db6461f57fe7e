"""One rank of a multi-process run of Avg, the mean across ranks (spawned by
tests/test_gpu_avg.py).

argv: rank world port outdir cases_json.  Every case builds this rank's input
with tests/avg_ref.py (the generator or the order table, by seed / rank),
runs the collectives of its kind and saves what the parent checks against the
numpy restatement of the rule to outdir/case<i>_rank<r>.npy, plus
case<i>_rank<r>.json (the last launch).  Every buffer sits between GUARD
sentinel bytes, which are saved with it.
"""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SENTINEL = 0xA5
GUARD = 4096


def main():
    rank, world, port, outdir, cases = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5]
    cases = json.loads(open(cases).read())
    import torch
    import rdc_amd
    from rdc_amd._lib import _LIB, check_call
    from tests import avg_ref as A
    device = int(os.environ.get("RDC_DEVICE", "0"))
    rdc_amd.init(["RDC_RANK=%d" % rank, "RDC_WORLD_SIZE=%d" % world, "RDC_TRACKER_PORT=%d" % port,
                  "RDC_TRACKER_URI=127.0.0.1", "RDC_DEVICE=%d" % device])
    torch.cuda.set_device(device)
    comm = rdc_amd.get_comm("main")
    sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def last_launch():
        ll = (ctypes.c_uint64 * 6)()
        check_call(_LIB.RdcCommLastLaunch(comm.handle, ll))
        return [int(x) for x in ll]

    def my_input(c):
        if c.get("data") == "order":
            return A.order_table(world, c["dtype"], count=c["count"])[rank]
        return A.gen_rank(c.get("seed", 0x5EEDB000), rank, c["count"], c["dtype"])

    def host_guarded(x, pad=0):
        """(backing bytes, the view of x inside them)"""
        raw = np.ascontiguousarray(x).view(np.uint8)
        backing = np.full(raw.size + 2 * GUARD + pad, SENTINEL, dtype=np.uint8)
        backing[GUARD + pad: GUARD + pad + raw.size] = raw
        return backing, backing[GUARD + pad: GUARD + pad + raw.size].view(x.dtype)

    def dev_guarded(x, pad=0):
        backing, _ = host_guarded(x, pad)
        t = torch.from_numpy(backing).cuda()
        return t, ctypes.c_void_p(t.data_ptr() + GUARD + pad)

    def run(which, p, count, dtype, root):
        if which == "ar":
            check_call(_LIB.RdcCommAllreduceAvg(comm.handle, p, count, dtype, sp))
        elif which == "rs":
            check_call(_LIB.RdcCommReduceScatterAvg(comm.handle, p, count, dtype, sp))
        elif which == "rt":
            check_call(_LIB.RdcCommReduceToAvg(comm.handle, p, count, dtype, root, sp))
        elif which == "acc32":   # the float32-accumulated Sum (16-bit dtypes)
            check_call(_LIB.RdcCommAllreduceAcc32(comm.handle, p, count, dtype, sp))
        elif which == "sum":   # the ordinary Sum, automatic schedule
            check_call(_LIB.RdcCommAllreduceEx(comm.handle, p, count, dtype, 2, 0, sp))
        else:
            raise ValueError(which)

    for i, c in enumerate(cases):
        kind, count, dtype = c["kind"], c["count"], c["dtype"]
        info = {}
        x = my_input(c)
        if kind == "coll":
            t, p = dev_guarded(x, c.get("pad", 0))
            run(c["which"], p, count, dtype, c.get("root", 0))
            comm.check(sp)
            out = t.cpu().numpy()
        elif kind == "chain":
            # one buffer per step, the same input in each; no host sync between the launches
            bufs = [dev_guarded(x) for _ in c["steps"]]
            torch.cuda.synchronize()
            comm.set_poison(True)
            for (which, root), (t, p) in zip(c["steps"], bufs):
                run(which, p, count, dtype, root)
            comm.check(sp)
            comm.set_poison(False)
            out = np.stack([t.cpu().numpy() for t, _ in bufs])
        elif kind == "host":
            # the three blocking entries on guarded host arrays ("main" and the handle's)
            outs = []
            for which, on in (("ar", False), ("rs", True), ("rt", False), ("ar", True), ("rs", False), ("rt", True)):
                backing, v = host_guarded(x)
                q = v.ctypes.data_as(ctypes.c_void_p)
                h = (comm.handle,) if on else ()
                name = {"ar": "RdcAllreduceAvg", "rs": "RdcReduceScatterAvg", "rt": "RdcReduceToAvg"}[which]
                args = h + (q, count, dtype) + ((c["root"],) if which == "rt" else ())
                check_call(getattr(_LIB, name + ("On" if on else ""))(*args))
                outs.append(backing)
            out = np.stack(outs)
        elif kind == "py":
            # the Python surface with average=True: numpy (float32 / float64 / float16) and torch
            # (all four), module functions and Comm methods; accumulate="float32" on 16-bit data
            outs = []
            flags = []
            root = c["root"]
            acc = "float32" if dtype in (10, 11) else None
            if dtype != 11:
                for f in (lambda a: rdc_amd.allreduce(a, rdc_amd.Op.SUM, average=True),
                          lambda a: comm.allreduce(a, rdc_amd.Op.SUM, accumulate=acc, average=True)):
                    backing, v = host_guarded(x)
                    got = f(v)
                    flags.append(got is not v and got.dtype == x.dtype)
                    outs.append(host_guarded(got)[0])
                backing, v = host_guarded(x)
                flags.append(rdc_amd.reduce(v, rdc_amd.Op.SUM, root, average=True) is v)
                outs.append(backing)
                backing, v = host_guarded(x)
                lo, hi = rdc_amd.split_range(count, world, rank)
                got = comm.reduce_scatter(v, rdc_amd.Op.SUM, average=True)
                flags.append(got.size == hi - lo and (got.size == 0 or got.ctypes.data == v[lo:hi].ctypes.data))
                outs.append(backing)
            tdt = {6: torch.float32, 7: torch.float64, 10: torch.float16, 11: torch.bfloat16}[dtype]
            nbytes = count * A.ESIZE[dtype]
            for f in (lambda a: rdc_amd.allreduce(a, rdc_amd.Op.SUM, average=True),
                      lambda a: comm.allreduce(a, rdc_amd.Op.SUM, algo="mesh", stream=sp, accumulate=acc, average=True),
                      lambda a: rdc_amd.reduce_scatter(a, rdc_amd.Op.SUM, average=True),
                      lambda a: comm.reduce_scatter(a, rdc_amd.Op.SUM, stream=sp, average=True),
                      lambda a: rdc_amd.reduce(a, rdc_amd.Op.SUM, root, accumulate=acc, average=True),
                      lambda a: comm.reduce(a, rdc_amd.Op.SUM, root, stream=sp, average=True)):
                t, _ = dev_guarded(x)
                a = t[GUARD: GUARD + nbytes].view(tdt)
                got = f(a)
                comm.check(sp)
                flags.append(got.dtype == tdt and got.data_ptr() >= a.data_ptr())
                outs.append(t.cpu().numpy())
            info["flags"] = [bool(v) for v in flags]
            out = np.stack(outs)
        else:
            raise ValueError(kind)
        info["launch"] = last_launch()
        np.save(os.path.join(outdir, "case%d_rank%d.npy" % (i, rank)), out)
        open(os.path.join(outdir, "case%d_rank%d.json" % (i, rank)), "w").write(json.dumps(info))
        print("rank %d case %d ok" % (rank, i), flush=True)
    rdc_amd.finalize()


if __name__ == "__main__":
    main()
