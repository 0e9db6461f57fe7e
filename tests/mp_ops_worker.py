"""One rank of a multi-process Prod / BitAND / BitXOR run (spawned by tests/test_gpu_ops.py).

argv: rank world port outdir cases_json.  Every case takes this rank's input
from tests/ops_ref.gen_inputs(seed, world, count, dtype)[rank] — or, "known":
a value derived from the rank — uploads it, runs one allreduce of its kind and
saves the bytes to outdir/case<i>_rank<r>.npy plus case<i>_rank<r>.json (the
last launch).
"""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def known_input(name, rank, count):
    if name == "xor_same":      # the same buffer on every rank
        return (np.arange(count, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)).astype(np.uint32)
    if name == "and_clear":     # rank r clears bit r
        return np.full(count, ~(1 << rank) & 0xFFFFFFFF, dtype=np.uint32)
    if name == "factorial":     # the product of rank + 1
        return np.full(count, rank + 1, dtype=np.int32)
    raise ValueError(name)


def main():
    rank, world, port, outdir, cases = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5]
    cases = json.loads(open(cases).read())
    import torch
    import rdc_amd
    from rdc_amd._lib import _LIB, check_call
    from oracle import oracle as O
    from tests import ops_ref as R
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
        if "known" in c:
            x = known_input(c["known"], rank, count)
        else:
            x = R.gen_inputs(c["seed"], world, count, dtype)[rank]
        assert x.dtype == np.dtype(O.NP_DTYPE[dtype])
        nbytes = x.nbytes
        info = {}
        if kind == "dev":
            # RdcCommAllreduceEx on a device buffer at a byte offset (the same on every rank)
            pad = c.get("pad", 0)
            t = torch.zeros(nbytes + pad + 64, dtype=torch.uint8, device="cuda")
            t[pad: pad + nbytes] = torch.from_numpy(np.frombuffer(x.tobytes(), dtype=np.uint8).copy()).cuda()
            torch.cuda.synchronize()
            check_call(_LIB.RdcCommAllreduceEx(comm.handle, ctypes.c_void_p(t.data_ptr() + pad), count, dtype, op,
                                               c.get("algo", 0), sp))
            comm.check(sp)
            out = t[pad: pad + nbytes].cpu().numpy()
        elif kind == "host":
            # the blocking entry on host memory: the resident service, the zero-copy path or the pieces
            h = x.copy()
            check_call(_LIB.RdcAllreduce(ctypes.c_void_p(h.ctypes.data), count, dtype, op, None, None))
            out = np.frombuffer(h.tobytes(), dtype=np.uint8)
        elif kind == "py_array":
            # rdc_amd.allreduce on an ndarray with the new Op members
            res = rdc_amd.allreduce(x, rdc_amd.Op(op))
            info["dtype_kept"] = res.dtype == x.dtype
            out = np.frombuffer(res.tobytes(), dtype=np.uint8)
        elif kind == "py_bf16":
            # Comm.allreduce on a torch.bfloat16 tensor (x: its bits)
            t = torch.from_numpy(x.view(np.int16).copy()).cuda().view(torch.bfloat16)
            ret = comm.allreduce(t, rdc_amd.Op(op))
            comm.check(sp)
            info["returns_its_argument"] = ret is t
            out = np.frombuffer(t.view(torch.int16).cpu().numpy().tobytes(), dtype=np.uint8)
        else:
            raise ValueError(kind)
        info["launch"] = last_launch()
        np.save(os.path.join(outdir, "case%d_rank%d.npy" % (i, rank)), out)
        open(os.path.join(outdir, "case%d_rank%d.json" % (i, rank)), "w").write(json.dumps(info))
        print("rank %d case %d ok" % (rank, i), flush=True)
    rdc_amd.finalize()


if __name__ == "__main__":
    main()
