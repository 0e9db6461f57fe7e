"""One rank of a multi-process MaxLoc / MinLoc run (spawned by tests/test_gpu_loc.py).

argv: rank world port outdir cases_json.  Every case takes this rank's input
from tests/loc_ref.gen_inputs(seed, world, count, dtype)[rank] (uploaded: RdcFill
has no pattern for pairs), runs one allreduce of its kind and saves the bytes
to outdir/case<i>_rank<r>.npy plus case<i>_rank<r>.json (the last launch).
"""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    rank, world, port, outdir, cases = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5]
    cases = json.loads(open(cases).read())
    import torch
    import rdc_amd
    from rdc_amd._lib import _LIB, check_call
    from tests import loc_ref as L
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
        x = L.gen_inputs(c["seed"], world, count, dtype)[rank]
        info = {}
        if kind == "dev":
            # RdcCommAllreduceEx on a device buffer at a byte offset (the same on every rank)
            pad = c.get("pad", 0)
            t = torch.zeros(count * 8 + pad + 64, dtype=torch.uint8, device="cuda")
            t[pad: pad + count * 8] = torch.from_numpy(np.frombuffer(x.tobytes(), dtype=np.uint8).copy()).cuda()
            torch.cuda.synchronize()
            check_call(_LIB.RdcCommAllreduceEx(comm.handle, ctypes.c_void_p(t.data_ptr() + pad), count, dtype, op,
                                               c.get("algo", 0), sp))
            comm.check(sp)
            out = t[pad: pad + count * 8].cpu().numpy()
        elif kind == "host":
            # the blocking entry on host memory: the resident service, the zero-copy path or the pieces
            h = x.copy()
            check_call(_LIB.RdcAllreduce(ctypes.c_void_p(h.ctypes.data), count, dtype, op, None, None))
            out = np.frombuffer(h.tobytes(), dtype=np.uint8)
        elif kind == "py_struct":
            # rdc_amd.allreduce on a structured array; a 4-byte aligned one is refused, never copied
            res = rdc_amd.allreduce(x, rdc_amd.Op(op))
            info["dtype_kept"] = res.dtype == x.dtype
            raw = np.zeros(8 * 16 + 16, dtype=np.uint8)
            o = (4 - raw.ctypes.data) % 8
            mis = raw[o: o + 8 * 16].view(x.dtype)
            try:
                rdc_amd.allreduce(mis, rdc_amd.Op(op))
                info["misaligned"] = "accepted"
            except rdc_amd.RdcError as e:
                info["misaligned"] = str(e)
            out = np.frombuffer(res.tobytes(), dtype=np.uint8)
        elif kind == "py_tensor":
            # Comm.allreduce on an int32 tensor of pairs, value= naming the value type
            t = torch.from_numpy(np.frombuffer(x.tobytes(), dtype=np.int32).reshape(-1, 2).copy()).cuda()
            ret = comm.allreduce(t, rdc_amd.Op(op), value="float32" if dtype == 12 else "int32")
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
