"""One rank of a multi-process all-to-all run (spawned by
tests/test_gpu_alltoall.py).

argv: rank world port outdir cases_json.  Every case fills its send buffer on
the device (RdcFill, uint8, seed / rank), pre-fills the receive buffer and 4 KiB
guards around it with 0xA5, runs the exchange of its kind and saves
outdir/case<i>_rank<r>.npz: `recv` (guards included) and `send` (after the
call) — the parent builds the expected bytes with numpy alone — plus
case<i>_rank<r>.json with the last launch.  Kinds: "a2a" (RdcCommAlltoall),
"a2av" (RdcCommAlltoallv over the length matrix M, M[r][p] = bytes r -> p),
"py" (Comm.all_to_all / all_to_all_v on int32 tensors, or with "module" the
module-level rdc_amd.all_to_all / all_to_all_v), "host" (the blocking
entry on numpy arrays).
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


def offsets(lens, gap, first=0):
    """Displacements of consecutive segments `gap` bytes apart, the first at `first`."""
    out, at = [], first
    for l in lens:
        out.append(at)
        at += l + gap
    return out, at


def row_col(M, r):
    n = len(M)
    return [M[r][p] for p in range(n)], [M[p][r] for p in range(n)]


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
    sz = ctypes.c_size_t

    def last_launch():
        ll = (ctypes.c_uint64 * 6)()
        check_call(_LIB.RdcCommLastLaunch(comm.handle, ll))
        return [int(x) for x in ll]

    def filled(nbytes, seed, base):
        t = torch.zeros(nbytes + base + 64, dtype=torch.uint8, device="cuda")
        check_call(_LIB.RdcFill(ctypes.c_void_p(t.data_ptr() + base), nbytes, 1, seed, rank, sp))
        return t

    for i, c in enumerate(cases):
        kind, seed = c["kind"], c.get("seed", 0x5EEDA2A0)
        if kind in ("a2a", "py", "host") and "M" not in c:
            M = [[c["bytes"]] * world for _ in range(world)]
            sgap = rgap = 0
        else:
            M, sgap, rgap = c["M"], c.get("sgap", 0), c.get("rgap", 0)
        slen, rlen = row_col(M, rank)
        soff, stotal = offsets(slen, sgap)
        roff, rtotal = offsets(rlen, rgap)
        # "sbase" / "rbase": per-rank address offsets of the two buffers (a2av only)
        sb, rb = c.get("sbase", [0] * world)[rank], c.get("rbase", [0] * world)[rank]
        send = filled(stotal, seed, sb)[sb:]
        recv = torch.full((rb + rtotal + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")[rb:]
        rp = recv.data_ptr() + GUARD
        if kind == "a2a":
            check_call(_LIB.RdcCommAlltoall(comm.handle, ctypes.c_void_p(send.data_ptr()), ctypes.c_void_p(rp),
                                            c["bytes"], sp))
            comm.check(sp)
        elif kind == "a2av":
            check_call(_LIB.RdcCommAlltoallv(comm.handle, ctypes.c_void_p(send.data_ptr()), (sz * world)(*soff),
                                             (sz * world)(*slen), ctypes.c_void_p(rp), (sz * world)(*roff),
                                             (sz * world)(*rlen), sp))
            comm.check(sp)
        elif kind == "py":
            # counts and displacements in int32 elements (every length a multiple of 4)
            st, rt = send[:stotal].view(torch.int32), recv[GUARD: GUARD + rtotal].view(torch.int32)
            # "module": the module-level function (on "main"), else the Comm method
            if "M" in c:
                fn = rdc_amd.all_to_all_v if c.get("module") else comm.all_to_all_v
                out = fn(st, [l // 4 for l in slen], rt, [l // 4 for l in rlen], [o // 4 for o in soff],
                         [o // 4 for o in roff])
            else:
                out = (rdc_amd.all_to_all if c.get("module") else comm.all_to_all)(st, rt)
            assert out is rt
            comm.check(sp)
        elif kind == "host":
            comm.check(sp)
            hs = send[:stotal].cpu().numpy()
            hr = np.full(rtotal + 2 * GUARD, SENTINEL, np.uint8)
            if "M" in c:
                out = comm.all_to_all_v(hs, slen, hr[GUARD: GUARD + rtotal], rlen, soff, roff)
            else:
                out = rdc_amd.all_to_all(hs, hr[GUARD: GUARD + rtotal])
            assert np.shares_memory(out, hr)
            recv = torch.from_numpy(hr)
            send = torch.from_numpy(hs)
        else:
            raise ValueError(kind)
        np.savez(os.path.join(outdir, "case%d_rank%d.npz" % (i, rank)), recv=recv.cpu().numpy(),
                 send=send[:stotal].cpu().numpy())
        open(os.path.join(outdir, "case%d_rank%d.json" % (i, rank)), "w").write(json.dumps({"launch": last_launch()}))
        del send, recv
        print("rank %d case %d ok" % (rank, i), flush=True)
    rdc_amd.finalize()


if __name__ == "__main__":
    main()
