"""One rank of a multi-process scan run (spawned by tests/test_gpu_scan.py).

argv: rank world port outdir cases_json.  Every case fills its buffer on the
device (RdcFill, seed / rank), runs the collectives of its kind and saves what
the parent checks against the CPU oracle to outdir/case<i>_rank<r>.npy, plus
case<i>_rank<r>.json (the last launch).  Buffers are allocated once per case;
nothing here empties torch's cache.
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
ESZ = {0: 1, 1: 1, 2: 4, 3: 4, 4: 8, 5: 8, 6: 4, 7: 8, 8: 8, 9: 8, 10: 2, 11: 2}


def main():
    rank, world, port, outdir, cases = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5]
    cases = json.loads(open(cases).read())
    import torch
    import rdc_amd
    from rdc_amd._lib import _LIB, check_call
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

    for i, c in enumerate(cases):
        kind, count = c["kind"], c["count"]
        seed = c.get("seed", 0x5EED0000)
        info = {}
        if kind == "chain":
            # int32 sums on one buffer, no host sync between the launches: refill, collective, accumulate
            buf = torch.zeros(count, dtype=torch.int32, device="cuda")
            other = torch.zeros(count, dtype=torch.int32, device="cuda")   # the all-to-all's receive buffer
            acc = torch.zeros(count, dtype=torch.int32, device="cuda")
            p, q = ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(other.data_ptr())
            m = count // world
            bounds = [rdc_amd.split_range(count, world, r) for r in range(world)]
            ag_ptrs = (ctypes.c_void_p * world)(*[buf.data_ptr() + 4 * lo for lo, _ in bounds])
            ag_sizes = (ctypes.c_size_t * world)(*[4 * (hi - lo) for lo, hi in bounds])
            comm.set_poison(True)
            for k, (what, arg) in enumerate(c["steps"]):
                check_call(_LIB.RdcFill(p, count, 2, seed + k, rank, sp))
                res = p
                if what == "sc":
                    check_call(_LIB.RdcCommScan(comm.handle, p, count, 2, 2, arg, sp))
                elif what == "rt":
                    check_call(_LIB.RdcCommReduceTo(comm.handle, p, count, 2, 2, arg, sp))
                elif what == "ar":
                    check_call(_LIB.RdcCommAllreduceEx(comm.handle, p, count, 2, 2, arg, sp))
                elif what == "rs":
                    check_call(_LIB.RdcCommReduceScatter(comm.handle, p, count, 2, 2, arg, sp))
                elif what == "bc":
                    check_call(_LIB.RdcCommBroadcast(comm.handle, p, count * 4, arg, sp))
                elif what == "a2a":
                    check_call(_LIB.RdcCommAlltoall(comm.handle, p, q, m * 4, sp))
                    res = q
                elif what == "ag":
                    check_call(_LIB.RdcCommAllgather(comm.handle, ag_ptrs, ag_sizes, sp))
                else:
                    raise ValueError(what)
                check_call(_LIB.RdcReduce(ctypes.c_void_p(acc.data_ptr()), res, count, 2, 2, sp))
            comm.check(sp)
            comm.set_poison(False)
            out = acc.cpu().numpy().view(np.uint8)
        elif kind == "scan":
            # RdcCommScan of any dtype at an element offset (pads[rank]) inside sentinel bytes
            dtype, esz = c["dtype"], ESZ[c["dtype"]]
            lo, nbytes = GUARD + c["pads"][rank] * esz, count * esz
            t = torch.full((lo + nbytes + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
            x = ctypes.c_void_p(t.data_ptr() + lo)
            check_call(_LIB.RdcFill(x, count, dtype, seed, rank, sp))
            check_call(_LIB.RdcCommScan(comm.handle, x, count, dtype, c["op"], c["exclusive"], sp))
            comm.check(sp)
            out = t.cpu().numpy()
        elif kind == "host":
            # float32 ndarray inside a larger backing array of sentinel bytes
            nbytes = count * 4
            dev = torch.zeros(count, dtype=torch.float32, device="cuda")
            check_call(_LIB.RdcFill(ctypes.c_void_p(dev.data_ptr()), count, 6, seed, rank, sp))
            comm.check(sp)
            backing = np.full(nbytes + 2 * GUARD, SENTINEL, dtype=np.uint8)
            backing[GUARD: GUARD + nbytes] = dev.cpu().numpy().view(np.uint8)
            host = backing[GUARD: GUARD + nbytes].view(np.float32)
            ret = rdc_amd.scan(host, rdc_amd.Op(c["op"]), exclusive=bool(c["exclusive"]))
            info["returns_its_argument"] = ret is host
            out = backing
        elif kind == "py":
            # "module": rdc_amd.scan on torch's current stream, else Comm.scan
            t = torch.full((count + 2 * GUARD // 4,), float("nan"), dtype=torch.float32, device="cuda")
            t.view(torch.uint8).fill_(SENTINEL)
            x = t[GUARD // 4: GUARD // 4 + count]
            check_call(_LIB.RdcFill(ctypes.c_void_p(x.data_ptr()), count, 6, seed, rank, sp))
            if c.get("module"):
                ret = rdc_amd.scan(x, rdc_amd.Op(c["op"]), exclusive=bool(c["exclusive"]))
            else:
                ret = comm.scan(x, rdc_amd.Op(c["op"]), exclusive=bool(c["exclusive"]), stream=sp)
            comm.check(sp)
            info["returns_its_argument"] = ret is x
            out = t.view(torch.uint8).cpu().numpy()
        else:
            raise ValueError(kind)
        info["launch"] = last_launch()
        np.save(os.path.join(outdir, "case%d_rank%d.npy" % (i, rank)), out)
        open(os.path.join(outdir, "case%d_rank%d.json" % (i, rank)), "w").write(json.dumps(info))
        print("rank %d case %d ok" % (rank, i), flush=True)
    rdc_amd.finalize()


if __name__ == "__main__":
    main()
