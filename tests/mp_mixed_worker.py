"""One rank of a randomized mixed-collective chain (spawned by
tests/test_gpu_mixed.py): a seeded sequence of allreduce (every schedule),
broadcast (rotating roots, direct and forwarded), variable-size allgather and
coalesced allreduce launches on ONE communicator and ONE stream with no host
synchronisation in between, so consecutive launches of different kinds
overlap across ranks the way a training step issues them; synchronous
host-buffer allreduces (the small-allreduce service, or the launch path above
64 KiB) run in between while earlier launches may still be in flight.  Every op has its
own output buffers; all are saved at the end for the parent to check against
the CPU oracle.

argv: rank world port outdir seed nops

With a seventh value, `cover`, the rank runs the covering chain instead
(tests/mixed_plan.make_cover_plan: every ordered pair of launch kinds once);
the sixth value is then the poison switch (0 / 1), see main_cover.
"""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.mixed_plan import ESZ, make_plan  # noqa: E402


def main():
    rank, world, port, outdir = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    seed, nops = int(sys.argv[5]), int(sys.argv[6])
    import torch
    import rdc_amd
    from rdc_amd._lib import _LIB, check_call
    rdc_amd.init(["RDC_RANK=%d" % rank, "RDC_WORLD_SIZE=%d" % world, "RDC_TRACKER_PORT=%d" % port,
                  "RDC_TRACKER_URI=127.0.0.1", "RDC_DEVICE=0"])
    torch.cuda.set_device(0)
    comm = rdc_amd.get_comm("main")
    sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    keep = []

    def dev(nbytes):
        t = torch.zeros(max(nbytes, 1) + 64, dtype=torch.uint8, device="cuda")
        keep.append(t)
        return t

    outs = []
    for op in make_plan(seed, nops, world):
        kind = op["kind"]
        if kind == "allreduce":
            n, dt = op["count"], op["dtype"]
            t = dev(n * ESZ[dt])
            check_call(_LIB.RdcFill(ctypes.c_void_p(t.data_ptr()), n, dt, op["seed"], rank, sp))
            check_call(_LIB.RdcCommAllreduceEx(comm.handle, ctypes.c_void_p(t.data_ptr()), n, dt, op["op"],
                                               op["algo"], sp))
            outs.append((t, n * ESZ[dt]))
        elif kind == "host":
            from oracle import oracle as O  # the checker's generator (same bits as RdcFill)
            h = O.fill(op["count"], op["dtype"], op["seed"], rank).copy()
            check_call(_LIB.RdcAllreduce(ctypes.c_void_p(h.ctypes.data), op["count"], op["dtype"], op["op"], None, None))
            outs.append((h, h.nbytes))
        elif kind == "bcast":
            nb = op["bytes"]
            t = dev(nb)
            check_call(_LIB.RdcFill(ctypes.c_void_p(t.data_ptr()), nb, 1, op["seed"], rank, sp))
            check_call(_LIB.RdcCommBroadcast(comm.handle, ctypes.c_void_p(t.data_ptr()), nb, op["root"], sp))
            outs.append((t, nb))
        elif kind == "allgather":
            sizes = op["sizes"]
            ts = [dev(s) for s in sizes]
            check_call(_LIB.RdcFill(ctypes.c_void_p(ts[rank].data_ptr()), sizes[rank], 1, op["seed"], rank, sp))
            ptrs = (ctypes.c_void_p * world)(*[x.data_ptr() for x in ts])
            szs = (ctypes.c_size_t * world)(*sizes)
            check_call(_LIB.RdcCommAllgather(comm.handle, ptrs, szs, sp))
            outs.extend(zip(ts, sizes))
        else:
            counts, dt = op["counts"], op["dtype"]
            ts = [dev(c * ESZ[dt]) for c in counts]
            for b, (x, c) in enumerate(zip(ts, counts)):
                check_call(_LIB.RdcFill(ctypes.c_void_p(x.data_ptr()), c, dt, op["seed"] + b, rank, sp))
            ptrs = (ctypes.c_void_p * len(counts))(*[x.data_ptr() for x in ts])
            cnt = (ctypes.c_size_t * len(counts))(*counts)
            check_call(_LIB.RdcCommAllreduceCoalesced(comm.handle, ptrs, cnt, len(counts), dt, op["op"], op["algo"],
                                                      sp))
            outs.extend((x, c * ESZ[dt]) for x, c in zip(ts, counts))
    comm.check(sp)
    blob = np.concatenate([np.frombuffer(t.tobytes(), np.uint8) if isinstance(t, np.ndarray) else t[:nb].cpu().numpy()
                           for t, nb in outs]) if outs else np.zeros(0, np.uint8)
    np.save(os.path.join(outdir, "mixed_rank%d.npy" % rank), blob)
    print("rank %d: mixed OK" % rank, flush=True)
    rdc_amd.finalize()


def main_cover():
    """argv: rank world port outdir seed poison cover.  Every step's buffers
    are allocated and filled first; after one device synchronisation every
    launch goes onto the one stream with no host synchronisation up to the
    final check, except what the synchronous host-buffer calls do themselves.
    Saves cover_rank<r>.npy (the outputs of every step, concatenated in plan
    order) and cover_rank<r>.json (RdcCommLastLaunch's algo after every
    allreduce step, and the direct schedule's fallback counters)."""
    rank, world, port, outdir = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    seed, poison = int(sys.argv[5]), int(sys.argv[6])
    import json
    import torch
    import rdc_amd
    from rdc_amd._lib import _LIB, check_call
    from tests.mixed_plan import (ALLREDUCE_ALGO, COVER_ESZ, SENTINEL, a2av_layout, cover_inputs, make_cover_plan,
                                  uses_fill)
    rdc_amd.init(["RDC_RANK=%d" % rank, "RDC_WORLD_SIZE=%d" % world, "RDC_TRACKER_PORT=%d" % port,
                  "RDC_TRACKER_URI=127.0.0.1", "RDC_DEVICE=0"])
    torch.cuda.set_device(0)
    comm = rdc_amd.get_comm("main")
    sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    plan = make_cover_plan(seed, world)

    def dev(nbytes, off, value=0):
        """(tensor, address `off` bytes past its base) with room for nbytes"""
        t = torch.full((max(nbytes, 1) + off + 64,), value, dtype=torch.uint8, device="cuda")
        return t, t.data_ptr() + off

    def filled(step, off, count=None, sd=None):
        """a device buffer holding this rank's input of a reducing step"""
        dt = step["dtype"]
        count = step["count"] if count is None else count
        sd = step["seed"] if sd is None else sd
        nb = count * COVER_ESZ[dt]
        t, p = dev(nb, off)
        if uses_fill(step):
            check_call(_LIB.RdcFill(vp(p), count, dt, sd, rank, sp))
        elif nb:
            x = cover_inputs(step, world, sd, count)[rank]
            t[off: off + nb] = torch.from_numpy(np.frombuffer(x.tobytes(), np.uint8).copy()).cuda()
        return t, p, nb

    def bytes_filled(nbytes, off, sd):
        t, p = dev(nbytes, off)
        check_call(_LIB.RdcFill(vp(p), nbytes, 1, sd, rank, sp))
        return t, p

    calls, outs = [], []   # per step: a closure that launches it; (buffer, byte offset, bytes) of every output
    for step in plan:
        kind, dt, op = step["kind"], step["dtype"], step["op"]
        if kind == "host":
            from oracle import oracle as O  # the checker's generator
            h = O.fill(step["count"], dt, step["seed"], rank).copy()
            calls.append(lambda h=h, n=step["count"], dt=dt, op=op:
                         _LIB.RdcAllreduce(vp(h.ctypes.data), n, dt, op, None, None))
            outs.append((h, 0, h.nbytes))
            continue
        off = step["off"] * (COVER_ESZ[dt] if kind not in ("bcast", "allgather", "alltoall", "alltoallv") else 1)
        if kind in ALLREDUCE_ALGO:
            t, p, nb = filled(step, off)
            calls.append(lambda p=p, s=step: _LIB.RdcCommAllreduceEx(comm.handle, vp(p), s["count"], s["dtype"],
                                                                     s["op"], s["algo"], sp))
            outs.append((t, off, nb))
        elif kind == "rscatter":
            t, p, nb = filled(step, off)
            calls.append(lambda p=p, s=step: _LIB.RdcCommReduceScatter(comm.handle, vp(p), s["count"], s["dtype"],
                                                                       s["op"], 2, sp))
            outs.append((t, off, nb))
        elif kind == "rooted":
            t, p, nb = filled(step, off)
            calls.append(lambda p=p, s=step: _LIB.RdcCommReduceTo(comm.handle, vp(p), s["count"], s["dtype"],
                                                                  s["op"], s["root"], sp))
            outs.append((t, off, nb))
        elif kind in ("scan", "exscan"):
            t, p, nb = filled(step, off)
            calls.append(lambda p=p, s=step: _LIB.RdcCommScan(comm.handle, vp(p), s["count"], s["dtype"], s["op"],
                                                              int(s["kind"] == "exscan"), sp))
            outs.append((t, off, nb))
        elif kind == "coalesced":
            bufs = [filled(step, off, c, step["seed"] + b) for b, c in enumerate(step["counts"])]
            ptrs = (vp * len(bufs))(*[p for _, p, _ in bufs])
            cnt = (sz * len(bufs))(*step["counts"])
            calls.append(lambda ptrs=ptrs, cnt=cnt, s=step: _LIB.RdcCommAllreduceCoalesced(
                comm.handle, ptrs, cnt, len(s["counts"]), s["dtype"], s["op"], s["algo"], sp))
            outs.extend((t, off, nb) for t, _, nb in bufs)
        elif kind == "bcast":
            t, p = bytes_filled(step["out"], off, step["seed"])
            calls.append(lambda p=p, s=step: _LIB.RdcCommBroadcast(comm.handle, vp(p), s["out"], s["root"], sp))
            outs.append((t, off, step["out"]))
        elif kind == "allgather":
            sizes = step["sizes"]
            bufs = [bytes_filled(s, off, step["seed"]) if r == rank else dev(s, off) for r, s in enumerate(sizes)]
            ptrs = (vp * world)(*[p for _, p in bufs])
            szs = (sz * world)(*sizes)
            calls.append(lambda ptrs=ptrs, szs=szs: _LIB.RdcCommAllgather(comm.handle, ptrs, szs, sp))
            outs.extend((t, off, s) for (t, _), s in zip(bufs, sizes))
        elif kind == "alltoall":
            b = step["bytes"]
            st, ps = bytes_filled(world * b, off, step["seed"])
            rt, pr = dev(world * b, off, SENTINEL)
            calls.append(lambda ps=ps, pr=pr, b=b, st=st: _LIB.RdcCommAlltoall(comm.handle, vp(ps), vp(pr), b, sp))
            outs.append((rt, off, world * b))
        elif kind == "alltoallv":
            rows, rtotal = a2av_layout(step["M"], step["sgap"], step["rgap"])
            soff, slen, stotal, roff, rlen = rows[rank]
            st, ps = bytes_filled(stotal, off, step["seed"])
            rt, pr = dev(rtotal, off, SENTINEL)
            arrs = [(sz * world)(*a) for a in (soff, slen, roff, rlen)]
            calls.append(lambda ps=ps, pr=pr, a=arrs, st=st: _LIB.RdcCommAlltoallv(comm.handle, vp(ps), a[0], a[1],
                                                                                   vp(pr), a[2], a[3], sp))
            outs.append((rt, off, rtotal))
        else:
            raise ValueError(kind)
    torch.cuda.synchronize()
    if poison:
        comm.set_poison(True)
    algos = {}
    ll = (ctypes.c_uint64 * 6)()
    for k, (step, call) in enumerate(zip(plan, calls)):
        check_call(call())
        if step["kind"] in ALLREDUCE_ALGO:
            check_call(_LIB.RdcCommLastLaunch(comm.handle, ll))  # host-side: no synchronisation
            algos[k] = int(ll[5])
    comm.check(sp)
    blob = np.concatenate([np.frombuffer(t.tobytes(), np.uint8)[:nb] if isinstance(t, np.ndarray)
                           else t[off: off + nb].cpu().numpy() for t, off, nb in outs])
    np.save(os.path.join(outdir, "cover_rank%d.npy" % rank), blob)
    info = {"algos": algos, "direct_fallback": comm.get_param("direct_fallback"),
            "direct_fail_reason": comm.get_param("direct_fail_reason")}
    with open(os.path.join(outdir, "cover_rank%d.json" % rank), "w") as f:
        json.dump(info, f)
    print("rank %d: cover OK" % rank, flush=True)
    rdc_amd.finalize()


if __name__ == "__main__":
    if len(sys.argv) > 7 and sys.argv[7] == "cover":
        main_cover()
    else:
        main()
