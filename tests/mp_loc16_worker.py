"""One rank of a multi-process run over the 16-byte MaxLoc / MinLoc pairs
(spawned by tests/test_gpu_loc16.py).

argv: rank world port outdir cases_json.  Every case takes this rank's input
from tests/loc16_ref.gen_inputs(seed, world, count, dtype)[rank] (uploaded:
RdcFill has no pattern for pairs), runs one allreduce of its kind and saves the
bytes to outdir/case<i>_rank<r>.npy plus case<i>_rank<r>.json (the last launch).
"""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ESZ = 16


def main():
    rank, world, port, outdir, cases = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5]
    cases = json.loads(open(cases).read())
    import torch
    import rdc_amd
    from rdc_amd._lib import _LIB, check_call
    from tests import loc16_ref as W
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
        kind, count, dtype, op = c["kind"], c["count"], c["dtype"], c["op"]
        x = W.gen_inputs(c["seed"], world, count, dtype)[rank]
        info = {}
        if kind == "dev":
            # RdcCommAllreduceEx on a device buffer with sentinel bytes after it
            t = torch.full((count * ESZ + 64,), 0xA5, dtype=torch.uint8, device="cuda")
            assert t.data_ptr() % 16 == 0
            t[: count * ESZ] = torch.from_numpy(np.frombuffer(x.tobytes(), dtype=np.uint8).copy()).cuda()
            torch.cuda.synchronize()
            check_call(_LIB.RdcCommAllreduceEx(comm.handle, ctypes.c_void_p(t.data_ptr()), count, dtype, op,
                                               c.get("algo", 0), sp))
            comm.check(sp)
            info["guard_kept"] = bool((t[count * ESZ:] == 0xA5).all().item())
            out = t[: count * ESZ].cpu().numpy()
        elif kind == "host":
            # the blocking entry on host memory through this communicator: the resident
            # service, the zero-copy path or the pipelined pieces, by size
            raw = np.full(count * ESZ + 48, 0xA5, dtype=np.uint8)
            o = (-raw.ctypes.data) % 16 + 16
            h = raw[o: o + count * ESZ]
            h[:] = np.frombuffer(x.tobytes(), dtype=np.uint8)
            check_call(_LIB.RdcAllreduceOn(comm.handle, ctypes.c_void_p(h.ctypes.data), count, dtype, op))
            info["guard_kept"] = bool((raw[:o] == 0xA5).all() and (raw[o + count * ESZ:] == 0xA5).all())
            out = h.copy()
        elif kind == "py_struct":
            # rdc_amd.allreduce on a structured array; an 8-byte aligned one is refused, never copied
            res = rdc_amd.allreduce(x, rdc_amd.Op(op))
            info["dtype_kept"] = res.dtype == x.dtype
            raw = np.zeros(8 * ESZ + 32, dtype=np.uint8)
            o = (8 - raw.ctypes.data) % 16
            mis = raw[o: o + 8 * ESZ].view(x.dtype)
            try:
                rdc_amd.allreduce(mis, rdc_amd.Op(op))
                info["misaligned"] = "accepted"
            except rdc_amd.RdcError as e:
                info["misaligned"] = str(e)
            out = np.frombuffer(res.tobytes(), dtype=np.uint8)
        elif kind == "py_tensor":
            # Comm.allreduce on an int64 tensor of pairs, value= naming the value type
            t = torch.from_numpy(np.frombuffer(x.tobytes(), dtype=np.int64).reshape(-1, 2).copy()).cuda()
            ret = comm.allreduce(t, rdc_amd.Op(op), value="float64" if dtype == 16 else "int64")
            comm.check(sp)
            info["returns_its_argument"] = ret is t
            out = np.frombuffer(t.cpu().numpy().tobytes(), dtype=np.uint8)
        else:
            raise ValueError(kind)
        info["launch"] = last_launch()
        np.save(os.path.join(outdir, "case%d_rank%d.npy" % (i, rank)), out)
        open(os.path.join(outdir, "case%d_rank%d.json" % (i, rank)), "w").write(json.dumps(info))
        print("rank %d case %d ok" % (rank, i), flush=True)
    rdc_amd.finalize()


if __name__ == "__main__":
    main()
