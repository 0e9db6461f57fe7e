#!/usr/bin/env python
"""Per-launch time of each allreduce schedule over a range of sizes, on the
communicator's own stream, max over ranks (the schedule-choice data for
RDC_ONESHOT_BYTES / RDC_DIRECT_BYTES).  fp32 sum; algo 0 = the automatic
choice (its schedule in auto_schedule), algo 1 = ring (reference
schedule), 2 = mesh, 3 = one-shot (skipped where it does not fit the slot
half), 5 = pull-mode mesh, 6 = direct (registered buffers).  SWEEP_ALGOS
(e.g. "0/1/6") picks the schedules.  Direct-schedule calls also report the
host side of their rendezvous per call (<name>_rendezvous_us: publish, map,
confirm; <name>_export_us: the export step alone; max over ranks).
SWEEP_COLLECTIVE=reduce_scatter times RdcCommReduceScatter instead, algos 0 / 2 /
6 (rs_auto, rs_mesh, rs_direct), and in the same run the allreduce's mesh and
direct schedules as the yardstick (allreduce_mesh, allreduce_direct); next to
the direct entry, rs_direct_hbm_fraction = the modelled HBM bytes (read + write,
the most of any rank) of the direct reduce-scatter over the direct allreduce's
(RdcPlanReduceScatterBytes / RdcPlanHbmBytes).
SWEEP_COLLECTIVE=alltoall times RdcCommAlltoall (sizes are MiB per PAIR) and the
same exchange written with Comm.isend / Comm.irecv on the same buffers, in
alternating rounds (SWEEP_ROUNDS, default 5): per form the median over rounds of
the slowest rank's time per call and the spread (max - min) / median.  The
collective is timed twice: "alltoall" = calls enqueued back to back, one
synchronise at the end (pipelined throughput per call), "alltoall_sync" = a
synchronise after every call, which is what the point-to-point form does (its
waits complete every call); "speedup" compares the two synchronised forms.  Next to
them the all-to-all's share of the HBM peak by RdcPlanAlltoallBytes (every
rank's bytes: the ranks share one GPU).
SWEEP_COLLECTIVE=reduce_to times RdcCommReduceTo (root 0) and, on the same
communicator and buffer, the mesh allreduce (algo 2) and the automatic
allreduce (algo 0: what a caller who needs the sum on one rank uses today), in
alternating rounds (SWEEP_ROUNDS, default 5), each form pipelined (<name>) and
synchronised per call (<name>_sync): the median over rounds of the slowest
rank's time per call and the spread.  Next to them reduce_to_bytes_ratio = the
rooted reduce's modelled HBM bytes (read + write, summed over the ranks) over
the mesh allreduce's (RdcPlanReduceToBytes / RdcPlanHbmBytes), and
reduce_to_hbm_fraction = those bytes per pipelined call over the HBM peak (the
ranks share one GPU).
SWEEP_COLLECTIVE=scan times RdcCommScan (inclusive) and, on the same
communicator and buffer, the same prefix built from what a caller had before it
(Comm.recv from rank r-1, RdcReduce, Comm.send to rank r+1: "composed") and the
ring allreduce (algo 1) of the same bytes as the scale, in alternating rounds
(SWEEP_ROUNDS, default 5).  The two collectives are timed pipelined (<name>) and
synchronised per call (<name>_sync); the composed form completes every call by
construction.  Per form the median over rounds of the slowest rank's time per
call and the spread.  Next to them scan_hbm_fraction = the scan's modelled HBM
bytes (RdcPlanScanBytes, read + write, summed over the ranks: they share one
GPU) per pipelined call over the HBM peak.
SWEEP_DTYPE / SWEEP_OP pick the element type and operator of the allreduce,
reduce_to and scan modes: f32 (default) / i64 / f32_i32 / f64_i64 and sum
(default) / max / maxloc.  SWEEP_DTYPE=f32_i32 (8-byte pairs) or f64_i64
(16-byte pairs) with SWEEP_OP=maxloc times MaxLoc over (value, index) pairs,
its inputs uploaded from numpy (RdcFill has no pattern for pairs);
SWEEP_DTYPE=i64 SWEEP_OP=max is their yardstick at the same byte sizes.

    python -m torch.distributed.run --nproc-per-node N tools/algo_sweep.py [sizes_MiB] [steps]
"""
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


HBM_PEAK = 8.0e12  # bytes / s, one MI355X

# element type and operator of the allreduce / reduce_to / scan modes
DT, ESZ = {"f32": (6, 4), "i64": (4, 8), "f32_i32": (12, 8), "f64_i64": (16, 16)}[os.environ.get("SWEEP_DTYPE", "f32")]
OP = {"sum": 2, "max": 0, "maxloc": 4}[os.environ.get("SWEEP_OP", "sum")]


def fill_input(buf, rank):
    """Synthetic input over the whole buffer: RdcFill, or for pairs an upload
    from numpy (values from a small set so that ranks tie, index = rank)."""
    import rdc_amd
    if DT not in (12, 16):
        from rdc_amd._lib import _LIB, check_call
        import torch
        check_call(_LIB.RdcFill(ctypes.c_void_p(buf.data_ptr()), buf.numel() * buf.element_size() // ESZ, DT,
                                0x5EED0000, rank, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return
    import numpy as np
    import torch
    rng = np.random.default_rng(0x5EED0000 + rank)
    x = np.empty(buf.numel() * buf.element_size() // ESZ, dtype=rdc_amd.F32_I32 if DT == 12 else rdc_amd.F64_I64)
    x["value"] = rng.integers(-4, 5, x.size).astype(x.dtype["value"])
    x["index"] = rank
    buf.view(torch.uint8).copy_(torch.from_numpy(x.view(np.uint8)))


def alltoall_sweep(sizes, steps, rank, world, comm, sp):
    """sizes: MiB per PAIR.  Per size, `rounds` rounds alternating the two forms
    on the same buffers; a round's time is the slowest rank's, the figure the
    median over rounds, the spread (max - min) / median."""
    import torch
    import torch.distributed as dist
    from rdc_amd._lib import _LIB, check_call
    rounds = int(os.environ.get("SWEEP_ROUNDS", "5"))
    big = int(max(sizes) * (1 << 20))
    send = torch.empty(world * big, dtype=torch.uint8, device="cuda")
    recv = torch.empty(world * big, dtype=torch.uint8, device="cuda")
    check_call(_LIB.RdcFill(ctypes.c_void_p(send.data_ptr()), world * big, 1, 0x5EED0000, rank, sp))
    out = {}
    for mib in sizes:
        nb = int(mib * (1 << 20))

        def a2a():
            check_call(_LIB.RdcCommAlltoall(comm.handle, ctypes.c_void_p(send.data_ptr()),
                                            ctypes.c_void_p(recv.data_ptr()), nb, sp))

        def p2p():  # the same exchange as a user of the parent commit writes it
            wcs = []
            for k in range(1, world):
                src, dst = (rank - k) % world, (rank + k) % world
                wcs.append(comm.irecv(recv[src * nb: (src + 1) * nb], src))
                wcs.append(comm.isend(send[dst * nb: (dst + 1) * nb], dst))
            recv[rank * nb: (rank + 1) * nb].copy_(send[rank * nb: (rank + 1) * nb])
            for w in wcs:
                w.wait()

        def timed(fn, n_steps):
            torch.cuda.synchronize()
            dist.barrier()
            t0 = time.perf_counter()
            for _ in range(n_steps):
                fn()
            torch.cuda.synchronize()
            t = torch.tensor([(time.perf_counter() - t0) / n_steps], dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            return float(t[0])

        def a2a_sync():  # one call at a time, as the point-to-point form completes every call
            a2a()
            torch.cuda.synchronize()

        n_a2a = max(steps, min(500, int(2e8 // max(nb * (world - 1), 1))))
        n_p2p = max(3, min(steps, int(5e7 // max(nb * (world - 1), 1))))
        for _ in range(3):
            a2a()
        p2p()
        comm.check(sp)
        ta, tsy, tp = [], [], []
        for _ in range(rounds):
            ta.append(timed(a2a, n_a2a))
            tsy.append(timed(a2a_sync, min(n_a2a, 100)))
            tp.append(timed(p2p, n_p2p))
        comm.check(sp)
        row = {}
        for name, ts in (("alltoall", ta), ("alltoall_sync", tsy), ("isend_irecv", tp)):
            ts.sort()
            med = ts[len(ts) // 2]
            row[name] = round(med * 1e3, 4)
            row[name + "_spread"] = round((ts[-1] - ts[0]) / med, 3)
        m = (ctypes.c_uint64 * 5)()
        lens = (ctypes.c_uint64 * 16)(*([nb] * world))
        check_call(_LIB.RdcPlanAlltoallBytes(world, rank, lens, lens, m))
        # every rank's modelled bytes share this GPU's HBM
        row["alltoall_hbm_fraction"] = round(world * (m[0] + m[1]) / (row["alltoall"] * 1e-3) / HBM_PEAK, 4)
        # like with like: both forms completing every call
        row["speedup"] = round(row["isend_irecv"] / row["alltoall_sync"], 2)
        ll = (ctypes.c_uint64 * 6)()
        check_call(_LIB.RdcCommLastLaunch(comm.handle, ll))
        row["grid_push_land_tile"] = [int(ll[0]), int(ll[1]), int(ll[3]), int(ll[4])]
        out["%g MiB" % mib] = row
    if rank == 0:
        print(json.dumps({"algo_sweep_ms_per_call": out, "world": world, "collective": "alltoall",
                          "size_is": "MiB per pair", "rounds": rounds, "ranks_share_gpu": True,
                          "hbm_peak_bytes_per_s": HBM_PEAK}), flush=True)


def reduce_to_sweep(sizes, steps, rank, world, comm, sp):
    """Per size, `rounds` rounds alternating the three forms on one buffer; a
    round's time is the slowest rank's, the figure the median over rounds."""
    import torch
    import torch.distributed as dist
    import rdc_amd
    from rdc_amd._lib import _LIB, check_call
    rounds = int(os.environ.get("SWEEP_ROUNDS", "5"))
    big = int(max(sizes) * (1 << 20))
    buf = torch.empty(big // 4, dtype=torch.float32, device="cuda")
    fill_input(buf, rank)
    p = ctypes.c_void_p(buf.data_ptr())
    out = {}
    for mib in sizes:
        nb = int(mib * (1 << 20))

        def rooted():
            check_call(_LIB.RdcCommReduceTo(comm.handle, p, nb // ESZ, DT, OP, 0, sp))

        def mesh():
            check_call(_LIB.RdcCommAllreduceEx(comm.handle, p, nb // ESZ, DT, OP, 2, sp))

        def auto():
            check_call(_LIB.RdcCommAllreduceEx(comm.handle, p, nb // ESZ, DT, OP, 0, sp))

        def timed(fn, n_steps, sync):
            torch.cuda.synchronize()
            dist.barrier()
            t0 = time.perf_counter()
            for _ in range(n_steps):
                fn()
                if sync:
                    torch.cuda.synchronize()
            torch.cuda.synchronize()
            t = torch.tensor([(time.perf_counter() - t0) / n_steps], dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            return float(t[0])

        forms = (("reduce_to", rooted), ("allreduce_mesh", mesh), ("allreduce_auto", auto))
        n_steps = max(steps, min(500, int(2e8 // max(nb, 1))))
        for _, fn in forms:
            for _ in range(3):
                fn()
        comm.check(sp)
        ts = {}
        ll = (ctypes.c_uint64 * 6)()
        for _ in range(rounds):
            for name, fn in forms:
                ts.setdefault(name, []).append(timed(fn, n_steps, False))
                ts.setdefault(name + "_sync", []).append(timed(fn, min(n_steps, 100), True))
        comm.check(sp)
        row = {}
        for name, v in ts.items():
            v.sort()
            med = v[len(v) // 2]
            row[name] = round(med * 1e3, 4)
            row[name + "_spread"] = round((v[-1] - v[0]) / med, 3)
        auto()
        check_call(_LIB.RdcCommLastLaunch(comm.handle, ll))
        row["auto_schedule"] = {1: "ring", 2: "mesh", 3: "oneshot", 4: "tree", 5: "mesh_pull",
                                6: "direct"}.get(int(ll[5]), int(ll[5]))
        rooted()
        check_call(_LIB.RdcCommLastLaunch(comm.handle, ll))
        comm.check(sp)
        row["root_grid_scatter_reduce_gather_tile"] = [int(x) for x in ll[:5]]
        m, full = (ctypes.c_uint64 * 5)(), (ctypes.c_uint64 * 5)()
        check_call(_LIB.RdcPlanReduceToBytes(world, -1, 0, nb // ESZ, DT, m))
        check_call(_LIB.RdcPlanHbmBytes(world, nb // ESZ, DT, 2, full))
        row["reduce_to_bytes_ratio"] = round((m[2] + m[3]) / float(full[2] + full[3]), 4)
        row["reduce_to_hbm_fraction"] = round((m[2] + m[3]) / (row["reduce_to"] * 1e-3) / HBM_PEAK, 4)
        row["speedup_vs_mesh"] = round(row["allreduce_mesh"] / row["reduce_to"], 3)
        row["speedup_vs_auto"] = round(row["allreduce_auto"] / row["reduce_to"], 3)
        row["speedup_vs_mesh_sync"] = round(row["allreduce_mesh_sync"] / row["reduce_to_sync"], 3)
        row["speedup_vs_auto_sync"] = round(row["allreduce_auto_sync"] / row["reduce_to_sync"], 3)
        out["%g MiB" % mib] = row
    if rank == 0:
        print(json.dumps({"algo_sweep_ms_per_call": out, "world": world, "collective": "reduce_to", "root": 0,
                          "rounds": rounds, "ranks_share_gpu": True, "hbm_peak_bytes_per_s": HBM_PEAK}), flush=True)


def scan_sweep(sizes, steps, rank, world, comm, sp):
    """Per size, `rounds` rounds alternating the three forms on one buffer; a
    round's time is the slowest rank's, the figure the median over rounds."""
    import torch
    import torch.distributed as dist
    import rdc_amd
    from rdc_amd._lib import _LIB, check_call
    rounds = int(os.environ.get("SWEEP_ROUNDS", "5"))
    big = int(max(sizes) * (1 << 20))
    buf = torch.empty(big // 4, dtype=torch.float32, device="cuda")
    tmp = torch.empty(big // 4, dtype=torch.float32, device="cuda")
    p, q = ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(tmp.data_ptr())
    out = {}
    for mib in sizes:
        nb = int(mib * (1 << 20))
        fill_input(buf, rank)   # sums of sums overflow after enough calls: fresh values per size

        def scan():
            check_call(_LIB.RdcCommScan(comm.handle, p, nb // ESZ, DT, OP, 0, sp))

        def ring():
            check_call(_LIB.RdcCommAllreduceEx(comm.handle, p, nb // ESZ, DT, OP, 1, sp))

        def composed():  # the same prefix as a user of the parent commit writes it
            if rank > 0:
                comm.recv(tmp[: nb // 4], rank - 1)
                check_call(_LIB.RdcReduce(p, q, nb // ESZ, DT, OP, sp))
            if rank < world - 1:
                comm.send(buf[: nb // 4], rank + 1)

        def timed(fn, n_steps, sync):
            torch.cuda.synchronize()
            dist.barrier()
            t0 = time.perf_counter()
            for _ in range(n_steps):
                fn()
                if sync:
                    torch.cuda.synchronize()
            torch.cuda.synchronize()
            t = torch.tensor([(time.perf_counter() - t0) / n_steps], dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            return float(t[0])

        n_steps = max(steps, min(500, int(2e8 // max(nb, 1))))
        n_comp = max(3, min(steps, int(5e7 // max(nb * (world - 1), 1))))
        for fn in (scan, ring):
            for _ in range(3):
                fn()
        composed()
        comm.check(sp)
        ts = {}
        for _ in range(rounds):
            for name, fn in (("scan", scan), ("allreduce_ring", ring)):
                ts.setdefault(name, []).append(timed(fn, n_steps, False))
                ts.setdefault(name + "_sync", []).append(timed(fn, min(n_steps, 100), True))
            ts.setdefault("composed", []).append(timed(composed, n_comp, True))
        comm.check(sp)
        row = {}
        for name, v in ts.items():
            v.sort()
            med = v[len(v) // 2]
            row[name] = round(med * 1e3, 4)
            row[name + "_spread"] = round((v[-1] - v[0]) / med, 3)
        ll = (ctypes.c_uint64 * 6)()
        scan()
        check_call(_LIB.RdcCommLastLaunch(comm.handle, ll))
        comm.check(sp)
        row["scan_grid_tile"] = [int(ll[0]), int(ll[4])]
        m = (ctypes.c_uint64 * 5)()
        check_call(_LIB.RdcPlanScanBytes(world, -1, nb // ESZ, DT, m))
        row["scan_hbm_fraction"] = round((m[2] + m[3]) / (row["scan"] * 1e-3) / HBM_PEAK, 4)
        row["speedup_vs_composed"] = round(row["composed"] / row["scan_sync"], 2)   # both complete every call
        row["scan_over_ring"] = round(row["scan"] / row["allreduce_ring"], 3)
        row["scan_over_ring_sync"] = round(row["scan_sync"] / row["allreduce_ring_sync"], 3)
        out["%g MiB" % mib] = row
    if rank == 0:
        print(json.dumps({"algo_sweep_ms_per_call": out, "world": world, "collective": "scan", "rounds": rounds,
                          "ranks_share_gpu": True, "hbm_peak_bytes_per_s": HBM_PEAK}), flush=True)


def main():
    sizes = [float(x) for x in (sys.argv[1] if len(sys.argv) > 1 else "1,4,16,64,256").replace("/", ",").split(",")]
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    import torch
    import torch.distributed as dist
    import rdc_amd
    from rdc_amd._lib import _LIB, check_call
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")) % torch.cuda.device_count())
    dist.init_process_group("gloo")
    rdc_amd.init([])
    comm = rdc_amd.get_comm("main")
    sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    if os.environ.get("SWEEP_COLLECTIVE", "allreduce") == "alltoall":
        alltoall_sweep(sizes, steps, rank, world, comm, sp)
        dist.barrier()
        rdc_amd.finalize()
        return
    if os.environ.get("SWEEP_COLLECTIVE", "allreduce") == "reduce_to":
        reduce_to_sweep(sizes, steps, rank, world, comm, sp)
        dist.barrier()
        rdc_amd.finalize()
        return
    if os.environ.get("SWEEP_COLLECTIVE", "allreduce") == "scan":
        scan_sweep(sizes, steps, rank, world, comm, sp)
        dist.barrier()
        rdc_amd.finalize()
        return
    half = ctypes.c_uint64()
    check_call(_LIB.RdcCommGetParam(comm.handle, b"slot_bytes", ctypes.byref(half)))
    big = int(max(sizes) * (1 << 20))
    buf = torch.empty(big // 4, dtype=torch.float32, device="cuda")
    fill_input(buf, rank)
    rs_mode = os.environ.get("SWEEP_COLLECTIVE", "allreduce") == "reduce_scatter"
    out = {}
    for mib in sizes:
        nb = int(mib * (1 << 20))
        row = {}
        if rs_mode:
            entries = [(True, 0, "rs_auto"), (True, 2, "rs_mesh"), (True, 6, "rs_direct"),
                       (False, 2, "allreduce_mesh"), (False, 6, "allreduce_direct")]
        else:
            entries = [(False, algo, name) for algo, name in ((0, "auto"), (1, "ring"), (2, "mesh"), (3, "oneshot"),
                                                              (5, "mesh_pull"), (6, "direct"))
                       if str(algo) in os.environ.get("SWEEP_ALGOS", "0/1/2/3").replace(",", "/").split("/")]
        for scatter, algo, name in entries:
            if algo == 3 and nb > half.value // 2:
                continue

            def one():
                if scatter:
                    check_call(_LIB.RdcCommReduceScatter(comm.handle, ctypes.c_void_p(buf.data_ptr()), nb // ESZ, DT, OP,
                                                         algo, sp))
                else:
                    check_call(_LIB.RdcCommAllreduceEx(comm.handle, ctypes.c_void_p(buf.data_ptr()), nb // ESZ, DT, OP,
                                                       algo, sp))

            def stats():
                r = {}
                for k in ("direct_calls", "direct_rendezvous_ns", "direct_export_ns"):
                    v = ctypes.c_uint64()
                    check_call(_LIB.RdcCommGetParam(comm.handle, k.encode(), ctypes.byref(v)))
                    r[k] = int(v.value)
                return r
            for _ in range(3):
                one()
            torch.cuda.synchronize()
            comm.check(sp)
            dist.barrier()
            n_steps = max(steps, int(2e8 // max(nb, 1)) if nb < (16 << 20) else steps)
            d0 = stats()
            t0 = time.perf_counter()
            for _ in range(n_steps):
                one()
            torch.cuda.synchronize()
            t = torch.tensor([(time.perf_counter() - t0) / n_steps], dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            comm.check(sp)
            row[name] = round(float(t[0]) * 1e3, 4)
            ll = (ctypes.c_uint64 * 6)()
            check_call(_LIB.RdcCommLastLaunch(comm.handle, ll))
            if algo == 0:  # the schedule the automatic choice launched
                row["rs_auto_schedule" if scatter else "auto_schedule"] = {1: "ring", 2: "mesh", 3: "oneshot", 4: "tree", 5: "mesh_pull",
                                        6: "direct"}.get(int(ll[5]), int(ll[5]))
            d1 = stats()
            if d1["direct_calls"] > d0["direct_calls"]:  # host side of the direct rendezvous, per call (max over ranks)
                nc = d1["direct_calls"] - d0["direct_calls"]
                v = torch.tensor([(d1["direct_rendezvous_ns"] - d0["direct_rendezvous_ns"]) / nc / 1e3,
                                  (d1["direct_export_ns"] - d0["direct_export_ns"]) / nc / 1e3], dtype=torch.float64)
                dist.all_reduce(v, op=dist.ReduceOp.MAX)
                row[name + "_rendezvous_us"] = round(float(v[0]), 2)
                row[name + "_export_us"] = round(float(v[1]), 2)
        if rs_mode:
            m, full = (ctypes.c_uint64 * 5)(), (ctypes.c_uint64 * 5)()
            check_call(_LIB.RdcPlanReduceScatterBytes(world, nb // ESZ, DT, 6, m))
            check_call(_LIB.RdcPlanHbmBytes(world, nb // ESZ, DT, 6, full))
            row["rs_direct_hbm_fraction"] = round((m[0] + m[1]) / float(full[0] + full[1]), 4)
        out["%g MiB" % mib] = row
    if rank == 0:
        print(json.dumps({"algo_sweep_ms_per_launch": out, "world": world,
                          "collective": "reduce_scatter" if rs_mode else "allreduce", "ranks_share_gpu": True,
                          "RDC_DIRECT_BYTES": os.environ.get("RDC_DIRECT_BYTES", "auto (default)")}), flush=True)
    dist.barrier()
    rdc_amd.finalize()


if __name__ == "__main__":
    main()
