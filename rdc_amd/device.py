"""Device-memory helpers: torch dtype mapping, op::Reducer on the GPU, and
the synthetic input generator (bit-identical to the CPU oracle's)."""
import ctypes

from ._lib import _LIB, check_call

_TORCH_ENUM = None


def dtype_enum(torch_dtype):
    global _TORCH_ENUM
    if _TORCH_ENUM is None:
        import torch
        m = {
            torch.int8: 0, torch.uint8: 1, torch.int32: 2, torch.int64: 4,
            torch.float32: 6, torch.float64: 7, torch.float16: 10, torch.bfloat16: 11,
        }
        for name, v in (("uint32", 3), ("uint64", 5)):
            if hasattr(torch, name):
                m[getattr(torch, name)] = v
        _TORCH_ENUM = m
    try:
        return _TORCH_ENUM[torch_dtype]
    except KeyError:
        raise TypeError("rdc_amd: dtype %s not supported" % torch_dtype)


def current_stream_ptr(device=None):
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _check_tensor(t):
    if not t.is_cuda:
        raise ValueError("rdc_amd: expected a tensor on a ROCm device")
    if not t.is_contiguous():
        raise ValueError("rdc_amd: tensor must be contiguous")


def reduce_(dst, src, op, stream=None):
    """dst = OP(dst, src) element-wise on the GPU (op::Reducer, include/core/mpi.h:113-120)."""
    _check_tensor(dst)
    _check_tensor(src)
    if dst.dtype != src.dtype or dst.numel() != src.numel():
        raise ValueError("rdc_amd: dst/src dtype or size mismatch")
    s = stream if stream is not None else current_stream_ptr(dst.device)
    check_call(_LIB.RdcReduce(ctypes.c_void_p(dst.data_ptr()), ctypes.c_void_p(src.data_ptr()), dst.numel(),
                              dtype_enum(dst.dtype), int(op), s))
    return dst


def fill_(t, seed, rank, stream=None):
    """Synthetic input u = splitmix64(seed ^ rank<<40 ^ i) mapped per dtype."""
    _check_tensor(t)
    s = stream if stream is not None else current_stream_ptr(t.device)
    check_call(_LIB.RdcFill(ctypes.c_void_p(t.data_ptr()), t.numel(), dtype_enum(t.dtype), seed, rank, s))
    return t


def pack_pairs(values, indices):
    """(value, index) pairs for Op.MAXLOC / Op.MINLOC as torch has no struct
    dtype: a contiguous ``torch.int32`` tensor of shape ``values.shape + (2,)``
    holding each value's bits (``values``: float32 or int32) and its index.
    Plain torch code, a convenience beside the hot path."""
    import torch
    if values.dtype not in (torch.float32, torch.int32):
        raise TypeError("rdc_amd: pack_pairs takes float32 or int32 values, got %s" % values.dtype)
    if indices.shape != values.shape:
        raise ValueError("rdc_amd: pack_pairs needs values and indices of one shape")
    return torch.stack((values.contiguous().view(torch.int32), indices.to(torch.int32)), dim=-1).contiguous()


def unpack_pairs(pairs, value="float32"):
    """``(values, indices)`` of a tensor made by ``pack_pairs``; ``value`` says
    how to read the value bits ("float32" or "int32")."""
    import torch
    if pairs.dtype != torch.int32 or pairs.dim() < 1 or pairs.shape[-1] != 2:
        raise TypeError("rdc_amd: unpack_pairs takes a torch.int32 tensor whose last dimension is 2")
    if value not in ("float32", "int32"):
        raise TypeError("rdc_amd: value must be \"float32\" or \"int32\", got %r" % (value,))
    v = pairs[..., 0].contiguous()
    return (v.view(torch.float32) if value == "float32" else v), pairs[..., 1].contiguous()


def pack_pairs16(values, indices):
    """The 16-byte (value, index) pairs (F64_I64 / I64_I64): a contiguous
    ``torch.int64`` tensor of shape ``values.shape + (2,)`` holding each
    value's bits (``values``: float64 or int64) and its int64 index.  Pass it
    with ``value="float64"`` or ``value="int64"``.  torch allocations are
    16-byte aligned, as these pairs must be."""
    import torch
    if values.dtype not in (torch.float64, torch.int64):
        raise TypeError("rdc_amd: pack_pairs16 takes float64 or int64 values, got %s" % values.dtype)
    if indices.shape != values.shape:
        raise ValueError("rdc_amd: pack_pairs16 needs values and indices of one shape")
    return torch.stack((values.contiguous().view(torch.int64), indices.to(torch.int64)), dim=-1).contiguous()


def unpack_pairs16(pairs, value):
    """``(values, indices)`` of a tensor made by ``pack_pairs16``; ``value``
    says how to read the value bits ("float64" or "int64")."""
    import torch
    if pairs.dtype != torch.int64 or pairs.dim() < 1 or pairs.shape[-1] != 2:
        raise TypeError("rdc_amd: unpack_pairs16 takes a torch.int64 tensor whose last dimension is 2")
    if value not in ("float64", "int64"):
        raise TypeError("rdc_amd: value must be \"float64\" or \"int64\", got %r" % (value,))
    v = pairs[..., 0].contiguous()
    return (v.view(torch.float64) if value == "float64" else v), pairs[..., 1].contiguous()
