"""One rank of a multi-process reduce-scatter run (spawned by
tests/test_gpu_reduce_scatter.py).

argv: rank world port outdir cases_json.  Every case fills its buffer on the
device (RdcFill, seed / rank), runs the collectives of its kind and saves the
WHOLE buffer to outdir/case<i>_rank<r>.npy — the parent checks this rank's
chunk against the CPU oracle and every other byte against the input — plus
case<i>_rank<r>.json: the last launch and the direct schedule's counters.
Buffers are allocated once per case; nothing here empties torch's cache.
"""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ESZ = {0: 1, 1: 1, 2: 4, 3: 4, 4: 8, 5: 8, 6: 4, 7: 8, 8: 8, 9: 8, 10: 2, 11: 2}
SENTINEL = 0xA5


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

    def stat(key):
        v = ctypes.c_uint64()
        check_call(_LIB.RdcCommGetParam(comm.handle, key.encode(), ctypes.byref(v)))
        return int(v.value)

    def last_launch():
        ll = (ctypes.c_uint64 * 6)()
        check_call(_LIB.RdcCommLastLaunch(comm.handle, ll))
        return [int(x) for x in ll]

    def rs(p, count, dtype, op, algo):
        check_call(_LIB.RdcCommReduceScatter(comm.handle, ctypes.c_void_p(p), count, dtype, op, algo, sp))

    def ar(p, count, dtype, op, algo):
        check_call(_LIB.RdcCommAllreduceEx(comm.handle, ctypes.c_void_p(p), count, dtype, op, algo, sp))

    for i, c in enumerate(cases):
        kind, count, dtype = c["kind"], c["count"], c["dtype"]
        pad = c.get("pad", 0) + rank * c.get("pad_per_rank", 0)
        nbytes = count * ESZ[dtype]
        buf = torch.zeros(nbytes + pad + 64, dtype=torch.uint8, device="cuda")
        p = buf.data_ptr() + pad
        seed = c.get("seed", 0x5EED0000)
        check_call(_LIB.RdcFill(ctypes.c_void_p(p), count, dtype, seed, rank, sp))
        info = {"direct_calls_before": stat("direct_calls"), "direct_fallback_before": stat("direct_fallback")}
        if kind == "rs":
            if c.get("warm_l2"):  # every XCD's L2 holds the buffer's lines before the owner's stores
                buf.sum()
            rs(p, count, dtype, c["op"], c.get("algo", 0))
            comm.check(sp)
            info["launch"] = last_launch()
            # warm_l2: the result read back by a copy KERNEL (through the L2s), not by a DMA copy
            out = (buf[pad: pad + nbytes].clone() if c.get("warm_l2") else buf[pad: pad + nbytes]).cpu().numpy()
        elif kind == "chain":
            # no host sync between the launches: refill, collective, accumulate
            comm.set_poison(True)
            acc = torch.zeros(count, dtype=torch.int32, device="cuda")
            for k, (what, arg) in enumerate(c["steps"]):
                check_call(_LIB.RdcFill(ctypes.c_void_p(p), count, 2, seed + k, rank, sp))
                if what == "rs":
                    rs(p, count, 2, 2, arg)
                elif what == "ar":
                    ar(p, count, 2, 2, arg)
                else:
                    check_call(_LIB.RdcCommBroadcast(comm.handle, ctypes.c_void_p(p), count * 4, arg, sp))
                check_call(_LIB.RdcReduce(ctypes.c_void_p(acc.data_ptr()), ctypes.c_void_p(p), count, 2, 2, sp))
            comm.check(sp)
            comm.set_poison(False)
            out = acc.cpu().numpy().view(np.uint8)
        elif kind == "algo_chain":
            # direct and scratch schedules on one buffer, stream-ordered
            for what, algo in c["steps"]:
                (rs if what == "rs" else ar)(p, count, dtype, c["op"], algo)
            comm.check(sp)
            out = buf[pad: pad + nbytes].cpu().numpy()
        elif kind == "host":
            # the buffer sits inside a larger backing array of sentinel bytes
            guard = 4096
            backing = np.full(nbytes + 2 * guard, SENTINEL, dtype=np.uint8)
            comm.check(sp)
            backing[guard: guard + nbytes] = buf[pad: pad + nbytes].cpu().numpy()
            host = backing[guard: guard + nbytes].view(np.float32)
            view = rdc_amd.reduce_scatter(host, rdc_amd.Op(c["op"]))
            info["view"] = [int(view.ctypes.data - host.ctypes.data) // ESZ[dtype], int(view.size)]
            out = backing
        elif kind == "py":
            t = buf[pad: pad + nbytes].view(torch.float32)
            view = comm.reduce_scatter(t, rdc_amd.Op(c["op"]), algo=c.get("algo", "auto"), stream=sp)
            comm.check(sp)
            info["view"] = [(view.data_ptr() - t.data_ptr()) // 4, view.numel()]
            info["split_range"] = list(rdc_amd.split_range(count, world, rank))
            info["view_bytes_ok"] = bool(view.cpu().numpy().tobytes() ==
                                         t[info["view"][0]: info["view"][0] + view.numel()].cpu().numpy().tobytes())
            out = buf[pad: pad + nbytes].cpu().numpy()
        else:
            raise ValueError(kind)
        info["direct_calls"] = stat("direct_calls")
        info["direct_fallback"] = stat("direct_fallback")
        np.save(os.path.join(outdir, "case%d_rank%d.npy" % (i, rank)), out)
        open(os.path.join(outdir, "case%d_rank%d.json" % (i, rank)), "w").write(json.dumps(info))
        del buf
        print("rank %d case %d ok" % (rank, i), flush=True)
    rdc_amd.finalize()


if __name__ == "__main__":
    main()
