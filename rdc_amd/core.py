"""rdc's Python surface (rdc/core.py) over the MI355X device path.

Same names, argument meaning and results as the reference module:
``init``, ``finalize``, ``get_rank``, ``get_world_size``, ``tracker_print``,
``get_processor_name``, ``broadcast`` (pickled objects), ``allreduce``
(ndarray copy semantics) and the ``Op`` enum (rdc/core.py:16-27).  The
reference binds ``_LIB.Rdc*`` symbols that were never implemented
(SURVEY.md §0 finding 3); here they are the C ABI of librdc_amd.so.

Device extension: ``allreduce`` also takes a ROCm ``torch.Tensor`` and then
reduces it in place on the GPU, stream-ordered on torch's current stream.
"""
import ctypes
import pickle
import sys
from enum import Enum

import numpy as np

from ._lib import _LIB, check_call


class Op(Enum):
    """Reduction operators = mpi::OpType (include/core/mpi.h:12-17)."""
    MAX = 0
    MIN = 1
    SUM = 2
    BITOR = 3
    # MI355X additions (MPI_MAXLOC / MPI_MINLOC) over (value, index) pairs
    # (F32_I32 / I32_I32): the greatest / least value and, among equal values,
    # the lowest index
    MAXLOC = 4
    MINLOC = 5
    # MI355X additions (MPI_PROD / MPI_BAND / MPI_BXOR); 6 and 7 are unassigned.
    # PROD: every arithmetic dtype (integers wrap; bf16: exact f32 product
    # rounded once); BITAND / BITXOR: integer dtypes only, as BITOR
    PROD = 8
    BITAND = 9
    BITXOR = 10

    def __int__(self):
        return self.value


# numpy dtype -> mpi::DataType (rdc/core.py:160-169 = include/core/mpi.h:19-30),
# plus the MI355X additions float16 = 10 (bfloat16 = 11 via torch only)
# (value, index) pairs of Op.MAXLOC / Op.MINLOC: 8 bytes, the value first.  An
# array of pairs must be 8-byte aligned (numpy guarantees it for its own
# allocations); one that is not gets the library's refusal, never a copy.
# Tensors: torch.int32 [..., 2] with value="float32" | "int32" (Comm.allreduce).
F32_I32 = np.dtype([("value", np.float32), ("index", np.int32)])
I32_I32 = np.dtype([("value", np.int32), ("index", np.int32)])
# the 16-byte pairs: a 64-bit index (it can number every element the library
# moves) and float64 / int64 values; arrays must be 16-byte aligned.
# Tensors: torch.int64 [..., 2] with an explicit value="float64" | "int64".
F64_I64 = np.dtype([("value", np.float64), ("index", np.int64)])
I64_I64 = np.dtype([("value", np.int64), ("index", np.int64)])

DTYPE_ENUM__ = {
    np.dtype("int8"): 0,
    np.dtype("uint8"): 1,
    np.dtype("int32"): 2,
    np.dtype("uint32"): 3,
    np.dtype("int64"): 4,
    np.dtype("uint64"): 5,
    np.dtype("float32"): 6,
    np.dtype("float64"): 7,
    np.dtype("float16"): 10,
    F32_I32: 12,
    I32_I32: 13,
    F64_I64: 16,
    I64_I64: 17,
}
_PAIR_DTYPES = (F32_I32, I32_I32, F64_I64, I64_I64)


def init(args=None, lib="standard", lib_dll=None):
    """Initialise rdc (RdcInit); ``args`` defaults to sys.argv (key=val pairs are parameters)."""
    del lib, lib_dll  # one backend: the MI355X device path
    if args is None:
        args = sys.argv
    enc = [a.encode() if isinstance(a, str) else bytes(a) for a in args]
    arr = (ctypes.c_char_p * max(1, len(enc)))()
    arr[: len(enc)] = enc
    check_call(_LIB.RdcInit(len(enc), arr))


def finalize():
    check_call(_LIB.RdcFinalize())


def get_rank():
    return _LIB.RdcGetRank()


def get_world_size():
    return _LIB.RdcGetWorldSize()


def is_distributed():
    return bool(_LIB.RdcIsDistributed())


def tracker_print(msg):
    if not isinstance(msg, str):
        msg = str(msg)
    check_call(_LIB.RdcTrackerPrint(msg.encode("utf-8")))


def get_processor_name():
    mxlen = 256
    length = ctypes.c_ulong()
    buf = ctypes.create_string_buffer(mxlen)
    check_call(_LIB.RdcGetProcessorName(buf, ctypes.byref(length), mxlen))
    return buf.value


def barrier():
    check_call(_LIB.RdcBarrier())


def broadcast(data, root):
    """Broadcast a picklable object from ``root`` (two RdcBroadcast calls:
    length, then payload — rdc/core.py:121-156)."""
    rank = get_rank()
    length = ctypes.c_ulong()
    payload = None
    if root == rank:
        if data is None:
            raise ValueError("need to pass in data when broadcasting")
        payload = pickle.dumps(data, protocol=pickle.HIGHEST_PROTOCOL)
        length.value = len(payload)
    check_call(_LIB.RdcBroadcast(ctypes.byref(length), ctypes.sizeof(ctypes.c_ulong), root))
    if root != rank:
        dptr = (ctypes.c_char * length.value)()
        check_call(_LIB.RdcBroadcast(ctypes.cast(dptr, ctypes.c_void_p), length.value, root))
        return pickle.loads(dptr.raw)
    src = ctypes.create_string_buffer(payload, len(payload))
    check_call(_LIB.RdcBroadcast(ctypes.cast(src, ctypes.c_void_p), length.value, root))
    return data


_PREPARE_T = ctypes.CFUNCTYPE(None, ctypes.c_void_p)


def _torch_dtype_enum(t):
    from . import device
    return device.dtype_enum(t.dtype)


def acc32_requested(accumulate, op, data):
    """True when ``accumulate="float32"`` selects the float32-accumulated Sum
    (RdcAllreduceAcc32 and its siblings: the owner of a chunk adds the ranks'
    16-bit values in binary32, in the ring order, and rounds once — the
    ordinary Sum rounds at every hop); False for ``None``.  The op must be
    Op.SUM and the data numpy.float16, torch.float16 or torch.bfloat16:
    anything else raises ValueError before the library is called."""
    if accumulate is None:
        return False
    if accumulate != "float32":
        raise ValueError("rdc_amd: accumulate must be None or \"float32\", got %r" % (accumulate,))
    if int(op) != Op.SUM.value:
        raise ValueError("rdc_amd: accumulate=\"float32\" goes with Op.SUM only")
    if isinstance(data, np.ndarray):
        ok = data.dtype == np.float16
    elif type(data).__module__.startswith("torch"):
        import torch
        ok = data.dtype in (torch.float16, torch.bfloat16)
    else:
        ok = False
    if not ok:
        raise ValueError("rdc_amd: accumulate=\"float32\" takes numpy.float16, torch.float16 or torch.bfloat16 data, "
                         "got %s" % (getattr(data, "dtype", type(data)),))
    return True


def average_requested(average, accumulate, op, data):
    """True when ``average=True`` selects Avg, the mean across ranks
    (RdcAllreduceAvg and its siblings: the owner of a chunk divides its
    ring-order sum by the world size before it stores — one launch, one
    rounding, and no float16 overflow that a later division cannot undo);
    False when ``average`` is false.  The op must be Op.SUM and the data
    float32, float64 or float16 (numpy or torch) or torch.bfloat16.  16-bit
    data always accumulate in float32, so ``accumulate`` may be ``None`` or
    ``"float32"`` there, with the same result; on float32 / float64 data
    ``accumulate`` stays refused (``acc32_requested``).  Anything else raises
    ValueError before the library is called."""
    if not average:
        return False
    if int(op) != Op.SUM.value:
        raise ValueError("rdc_amd: average=True goes with Op.SUM only")
    if isinstance(data, np.ndarray):
        ok = data.dtype in (np.float32, np.float64, np.float16)
    elif type(data).__module__.startswith("torch"):
        import torch
        ok = data.dtype in (torch.float32, torch.float64, torch.float16, torch.bfloat16)
    else:
        ok = False
    if not ok:
        raise ValueError("rdc_amd: average=True takes float32, float64 or float16 data (numpy or torch) or "
                         "torch.bfloat16, got %s" % (getattr(data, "dtype", type(data)),))
    if accumulate is not None:
        acc32_requested(accumulate, op, data)
    return True


def fold_requested(accumulate, average, op, data):
    """The mesh-family fold that ``accumulate=`` / ``average=`` select: ``"Avg"``
    (``average_requested``), ``"Acc32"`` (``acc32_requested``) or ``None`` for
    the ordinary reduction; ValueError as those two raise it."""
    if average_requested(average, accumulate, op, data):
        return "Avg"
    if acc32_requested(accumulate, op, data):
        return "Acc32"
    return None


def _fold_entry(name, fold, on):
    """The C entry of a blocking mesh-family fold: Rdc<name>Avg / Rdc<name>Acc32, ...On with a handle."""
    return getattr(_LIB, "Rdc" + name + fold + ("On" if on else ""))


def allreduce(data, op, prepare_fun=None, value=None, accumulate=None, average=False):
    """Allreduce across ranks.

    numpy.ndarray: returns the reduced, flattened array (a copy unless ravel
    gave a view of ``data`` — the reference's rule, rdc/core.py:196-217).
    torch.Tensor on a ROCm device: reduced in place on the GPU and returned.
    ``prepare_fun(data)``, if given, runs before the reduction.
    Op.MAXLOC / Op.MINLOC: a structured array of dtype F32_I32 / I32_I32 /
    F64_I64 / I64_I64, or an int32 / int64 tensor of pairs read as ``value``
    (Comm.allreduce).  ``accumulate="float32"`` (Op.SUM on float16 / bfloat16
    data only): the float32-accumulated Sum (``acc32_requested``).
    ``average=True`` (Op.SUM on floating data): the mean across ranks, divided
    where the result is produced (``average_requested``).
    """
    op = int(Op(op) if not isinstance(op, Op) else op)
    fold = fold_requested(accumulate, average, op, data)
    if type(data).__module__.startswith("torch"):
        from . import comm as _comm
        if prepare_fun is not None:
            prepare_fun(data)
        return _comm.get_comm("main").allreduce(data, op, value=None if fold else value, accumulate=accumulate,
                                                average=average)
    return host_allreduce(data, op, prepare_fun, fold=fold)


def host_allreduce(data, op, prepare_fun=None, comm=None, fold=None):
    """rdc/core.py:172-217 on a host ndarray: RdcAllreduce on "main", or
    RdcAllreduceOn on the communicator handle ``comm`` (``fold``, a
    ``fold_requested`` value: RdcAllreduceAcc32 / RdcAllreduceAvg, ...On with
    ``comm``, same copy rule)."""
    op = int(Op(op) if not isinstance(op, Op) else op)
    if not isinstance(data, np.ndarray):
        raise TypeError("allreduce only takes in numpy.ndarray or torch.Tensor")
    buf = data.ravel()
    misaligned_pairs = buf.dtype in _PAIR_DTYPES and buf.ctypes.data % buf.dtype.itemsize != 0
    if buf.base is data.base and not misaligned_pairs:  # those go to the library as they are: it refuses them
        buf = buf.copy()
    if buf.dtype not in DTYPE_ENUM__:
        raise TypeError("data type %s not supported" % str(buf.dtype))
    if not buf.flags.c_contiguous:
        buf = np.ascontiguousarray(buf)
    if fold:
        if prepare_fun is not None:
            prepare_fun(data)
        ptr = buf.ctypes.data_as(ctypes.c_void_p)
        if comm is not None:
            check_call(_fold_entry("Allreduce", fold, True)(comm, ptr, buf.size, DTYPE_ENUM__[buf.dtype]))
        else:
            check_call(_fold_entry("Allreduce", fold, False)(ptr, buf.size, DTYPE_ENUM__[buf.dtype]))
        return buf
    if comm is not None:
        if prepare_fun is not None:
            prepare_fun(data)
        check_call(_LIB.RdcAllreduceOn(comm, buf.ctypes.data_as(ctypes.c_void_p), buf.size,
                                       DTYPE_ENUM__[buf.dtype], op))
        return buf
    cb = None
    if prepare_fun is not None:
        cb = _PREPARE_T(lambda _arg: prepare_fun(data))
    check_call(_LIB.RdcAllreduce(buf.ctypes.data_as(ctypes.c_void_p), buf.size, DTYPE_ENUM__[buf.dtype], op,
                                 ctypes.cast(cb, ctypes.c_void_p) if cb is not None else None, None))
    return buf


def split_range(count, n, rank):
    """``(begin, end)``: the element range of chunk ``rank`` of
    utils::Split(0, count, n) (include/utils/utils.h:59-70, RdcPlanSplit) — the
    chunk a reduce-scatter leaves on that rank."""
    lo, hi = ctypes.c_uint64(), ctypes.c_uint64()
    check_call(_LIB.RdcPlanSplit(int(count), int(n), int(rank), ctypes.byref(lo), ctypes.byref(hi)))
    return lo.value, hi.value


def reduce_scatter(data, op, value=None, accumulate=None, average=False):
    """In-place reduce-scatter on the "main" communicator (RdcReduceScatter;
    TryReduceScatterRing, communicator_collective.cc:115-182): chunk
    ``get_rank()`` of ``split_range(data.size, get_world_size(), get_rank())``
    receives the reduction — the bits ``allreduce`` puts there — and every
    other element of ``data`` stays as passed.  A contiguous numpy.ndarray
    (synchronous) or a ROCm torch.Tensor (stream-ordered on torch's current
    stream); returns the flat view of this rank's chunk.
    ``accumulate="float32"``: the float32-accumulated Sum (``acc32_requested``);
    ``average=True``: the mean across ranks (``average_requested``)."""
    op = int(Op(op) if not isinstance(op, Op) else op)
    fold = fold_requested(accumulate, average, op, data)
    if type(data).__module__.startswith("torch"):
        from . import comm as _comm
        return _comm.get_comm("main").reduce_scatter(data, op, value=None if fold else value,
                                                     accumulate=accumulate, average=average)
    return host_reduce_scatter(data, op, fold=fold)


def host_reduce_scatter(data, op, comm=None, fold=None):
    """reduce_scatter of a host ndarray: RdcReduceScatter on "main", or
    RdcReduceScatterOn on the Comm ``comm`` (``fold``, a ``fold_requested``
    value: RdcReduceScatterAcc32 / RdcReduceScatterAvg, ...On with ``comm``)."""
    op = int(Op(op) if not isinstance(op, Op) else op)
    if not isinstance(data, np.ndarray) or not data.flags.c_contiguous:
        raise TypeError("reduce_scatter takes a contiguous numpy.ndarray or a torch.Tensor")
    if data.dtype not in DTYPE_ENUM__:
        raise TypeError("data type %s not supported" % str(data.dtype))
    ptr = data.ctypes.data_as(ctypes.c_void_p)
    if fold:
        if comm is not None:
            check_call(_fold_entry("ReduceScatter", fold, True)(comm.handle, ptr, data.size, DTYPE_ENUM__[data.dtype]))
            n, r = comm.world_size, comm.rank
        else:
            check_call(_fold_entry("ReduceScatter", fold, False)(ptr, data.size, DTYPE_ENUM__[data.dtype]))
            n, r = get_world_size(), get_rank()
    elif comm is not None:
        check_call(_LIB.RdcReduceScatterOn(comm.handle, ptr, data.size, DTYPE_ENUM__[data.dtype], op))
        n, r = comm.world_size, comm.rank
    else:
        check_call(_LIB.RdcReduceScatter(ptr, data.size, DTYPE_ENUM__[data.dtype], op))
        n, r = get_world_size(), get_rank()
    lo, hi = split_range(data.size, n, r)
    return data.reshape(-1)[lo:hi]


def all_to_all(send, recv):
    """Out-of-place all-to-all on the "main" communicator, equal split: part p
    of ``send`` lands in part ``get_rank()`` of rank p's ``recv``.  Contiguous
    numpy.ndarrays (synchronous, RdcAlltoall) or ROCm torch.Tensors
    (stream-ordered on torch's current stream) of equal size divisible by the
    world size; returns ``recv``."""
    if type(send).__module__.startswith("torch"):
        from . import comm as _comm
        return _comm.get_comm("main").all_to_all(send, recv)
    return host_all_to_all(send, recv)


def host_all_to_all(send, recv, comm=None):
    """all_to_all of host ndarrays: RdcAlltoall on "main", or RdcAlltoallOn on
    the Comm ``comm`` (any size: the library cuts the launches)."""
    from .comm import _a2a_equal_counts
    for a in (send, recv):
        if not isinstance(a, np.ndarray) or not a.flags.c_contiguous:
            raise TypeError("all_to_all takes contiguous numpy.ndarrays or torch.Tensors")
    if send.dtype != recv.dtype:
        raise TypeError("all_to_all needs one dtype")
    n = comm.world_size if comm is not None else get_world_size()
    nbytes = _a2a_equal_counts(send.size, recv.size, n)[0] * send.itemsize
    sp, rp = send.ctypes.data_as(ctypes.c_void_p), recv.ctypes.data_as(ctypes.c_void_p)
    if comm is not None:
        check_call(_LIB.RdcAlltoallOn(comm.handle, sp, rp, nbytes))
    else:
        check_call(_LIB.RdcAlltoall(sp, rp, nbytes))
    return recv


def all_to_all_v(send, send_counts, recv, recv_counts, send_displs=None, recv_displs=None):
    """All-to-all with per-peer counts on the "main" communicator
    (RdcAlltoallv), counts and displacements in elements, displacements
    defaulting to the prefix sums: ``send_counts[p]`` elements at
    ``send_displs[p]`` go to rank p, which receives them at its
    ``recv_displs[get_rank()]``.  numpy.ndarrays (synchronous) or ROCm
    torch.Tensors (stream-ordered); returns ``recv``."""
    if type(send).__module__.startswith("torch"):
        from . import comm as _comm
        return _comm.get_comm("main").all_to_all_v(send, send_counts, recv, recv_counts, send_displs, recv_displs)
    return host_all_to_all_v(send, send_counts, recv, recv_counts, send_displs, recv_displs)


def host_all_to_all_v(send, send_counts, recv, recv_counts, send_displs=None, recv_displs=None, comm=None):
    """all_to_all_v of host ndarrays: RdcAlltoallv on "main", or RdcAlltoallvOn
    on the Comm ``comm``."""
    from .comm import _a2a_bytes
    for a in (send, recv):
        if not isinstance(a, np.ndarray) or not a.flags.c_contiguous:
            raise TypeError("all_to_all takes contiguous numpy.ndarrays or torch.Tensors")
    if send.dtype != recv.dtype:
        raise TypeError("all_to_all needs one dtype")
    n = comm.world_size if comm is not None else get_world_size()
    so, sl, ro, rl = _a2a_bytes(n, send_counts, send_displs, recv_counts, recv_displs, send.itemsize, send.size,
                                recv.size)
    sp, rp = send.ctypes.data_as(ctypes.c_void_p), recv.ctypes.data_as(ctypes.c_void_p)
    if comm is not None:
        check_call(_LIB.RdcAlltoallvOn(comm.handle, sp, so, sl, rp, ro, rl))
    else:
        check_call(_LIB.RdcAlltoallv(sp, so, sl, rp, ro, rl))
    return recv


def reduce(data, op, root, value=None, accumulate=None, average=False):
    """In-place reduction to rank ``root`` on the "main" communicator
    (RdcReduceTo; MPI_Reduce): on ``root`` ``data`` receives the reduction —
    the bits ``allreduce`` puts there by the ring order, at every size — and
    on every other rank ``data`` stays exactly as passed.  ``root`` must be the
    same on every rank.  A contiguous numpy.ndarray (synchronous) or a ROCm
    torch.Tensor (stream-ordered on torch's current stream); returns ``data``.
    ``accumulate="float32"``: the float32-accumulated Sum (``acc32_requested``);
    ``average=True``: the mean across ranks (``average_requested``)."""
    op = int(Op(op) if not isinstance(op, Op) else op)
    fold = fold_requested(accumulate, average, op, data)
    if type(data).__module__.startswith("torch"):
        from . import comm as _comm
        return _comm.get_comm("main").reduce(data, op, root, value=None if fold else value, accumulate=accumulate,
                                             average=average)
    return host_reduce(data, op, root, fold=fold)


def host_reduce(data, op, root, comm=None, fold=None):
    """reduce of a host ndarray: RdcReduceTo on "main", or RdcReduceToOn on the
    Comm ``comm`` (``fold``, a ``fold_requested`` value: RdcReduceToAcc32 /
    RdcReduceToAvg / RdcReduceToAvgOn)."""
    op = int(Op(op) if not isinstance(op, Op) else op)
    if not isinstance(data, np.ndarray) or not data.flags.c_contiguous:
        raise TypeError("reduce takes a contiguous numpy.ndarray or a torch.Tensor")
    if data.dtype not in DTYPE_ENUM__:
        raise TypeError("data type %s not supported" % str(data.dtype))
    ptr = data.ctypes.data_as(ctypes.c_void_p)
    if fold:
        if comm is not None:
            check_call(_fold_entry("ReduceTo", fold, True)(comm.handle, ptr, data.size, DTYPE_ENUM__[data.dtype],
                                                           int(root)))
        else:
            check_call(_fold_entry("ReduceTo", fold, False)(ptr, data.size, DTYPE_ENUM__[data.dtype], int(root)))
    elif comm is not None:
        check_call(_LIB.RdcReduceToOn(comm.handle, ptr, data.size, DTYPE_ENUM__[data.dtype], op, int(root)))
    else:
        check_call(_LIB.RdcReduceTo(ptr, data.size, DTYPE_ENUM__[data.dtype], op, int(root)))
    return data


def scan(data, op, exclusive=False, value=None):
    """In-place prefix reduction across ranks on the "main" communicator
    (RdcScan; MPI_Scan, ``exclusive=True``: MPI_Exscan): rank r ends with the
    left fold of ranks 0..r (exclusive: 0..r-1, r > 0) in rank order, element
    by element; on rank 0 ``data`` stays exactly as passed.  A contiguous
    numpy.ndarray (synchronous) or a ROCm torch.Tensor (stream-ordered on
    torch's current stream); returns ``data``."""
    op = int(Op(op) if not isinstance(op, Op) else op)
    if type(data).__module__.startswith("torch"):
        from . import comm as _comm
        return _comm.get_comm("main").scan(data, op, exclusive, value=value)
    return host_scan(data, op, exclusive)


def host_scan(data, op, exclusive=False, comm=None):
    """scan of a host ndarray: RdcScan on "main", or RdcScanOn on the Comm
    ``comm``."""
    op = int(Op(op) if not isinstance(op, Op) else op)
    if not isinstance(data, np.ndarray) or not data.flags.c_contiguous:
        raise TypeError("scan takes a contiguous numpy.ndarray or a torch.Tensor")
    if data.dtype not in DTYPE_ENUM__:
        raise TypeError("data type %s not supported" % str(data.dtype))
    ptr = data.ctypes.data_as(ctypes.c_void_p)
    ex = 1 if exclusive else 0
    if comm is not None:
        check_call(_LIB.RdcScanOn(comm.handle, ptr, data.size, DTYPE_ENUM__[data.dtype], op, ex))
    else:
        check_call(_LIB.RdcScan(ptr, data.size, DTYPE_ENUM__[data.dtype], op, ex))
    return data


def allreduce_coalesced(arrays, op, value=None):
    """Bucketed allreduce of a list of arrays of one dtype, in place: the
    result of ``allreduce`` on each one (bit-identical), moved in fused device
    launches (RdcAllreduceCoalesced).  numpy arrays (contiguous) or ROCm
    tensors (stream-ordered on torch's current stream).  Returns the list."""
    op = int(Op(op) if not isinstance(op, Op) else op)
    if not arrays:
        return arrays
    if type(arrays[0]).__module__.startswith("torch"):
        from . import comm as _comm
        return _comm.get_comm("main").allreduce_coalesced(arrays, op, value=value)
    for a in arrays:
        if not isinstance(a, np.ndarray) or not a.flags.c_contiguous:
            raise TypeError("allreduce_coalesced takes contiguous numpy arrays")
        if a.dtype != arrays[0].dtype:
            raise TypeError("allreduce_coalesced needs one dtype")
    if arrays[0].dtype not in DTYPE_ENUM__:
        raise TypeError("data type %s not supported" % str(arrays[0].dtype))
    nb = len(arrays)
    ptrs = (ctypes.c_void_p * nb)(*[a.ctypes.data for a in arrays])
    counts = (ctypes.c_size_t * nb)(*[a.size for a in arrays])
    check_call(_LIB.RdcAllreduceCoalesced(ptrs, counts, nb, DTYPE_ENUM__[arrays[0].dtype], op))
    return arrays


def allgather(arrays):
    """Allgather of host arrays (rdc::Allgather, include/api.h:47-52): arrays[c]
    is pre-sized on every rank and arrays[get_rank()] holds this rank's data;
    on return every arrays[c] holds rank c's data.  In place; returns arrays."""
    n = get_world_size()
    if len(arrays) != n:
        raise ValueError("allgather needs one array per rank")
    for a in arrays:
        if not isinstance(a, np.ndarray) or not a.flags.c_contiguous:
            raise TypeError("allgather takes contiguous numpy arrays")
    ptrs = (ctypes.c_void_p * n)(*[a.ctypes.data for a in arrays])
    sizes = (ctypes.c_size_t * n)(*[a.nbytes for a in arrays])
    check_call(_LIB.RdcAllgather(ptrs, sizes))
    return arrays


def send(buf, dest):
    """rdc::Send on the main communicator (include/api.h:10, rdc-inl.h:53-62):
    blocking send of a Buffer / ndarray / bytes / ROCm tensor to rank ``dest``."""
    from .comm import get_comm
    get_comm("main").send(buf, dest)


def recv(buf, src):
    """rdc::Recv on the main communicator (include/api.h:11): blocking receive
    into ``buf`` from rank ``src``; returns ``buf``."""
    from .comm import get_comm
    return get_comm("main").recv(buf, src)
