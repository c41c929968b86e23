"""numpy arrays and torch tensors -> the arguments of the C ABI: the one marshalling layer of the op modules (`_lib` stays the ctypes binding).
Which stream, device and memory kind a call gets, how pointers and strides are taken, and when a strided view is read in place are decided
here and nowhere else.  torch is imported inside the functions that need it: numpy callers never import it through this module."""
from __future__ import annotations

import numpy as np

from . import _lib

FLOATS, NARROW = ("float16", "float32"), ("uint8", "int8", "int16")


def is_np(a):
    return isinstance(a, np.ndarray)


_NAMES = {}


def dtype_name(a):
    """'float16', 'int64', ... of an array, a tensor or a dtype of either library"""
    d = getattr(a, "dtype", a)
    name = _NAMES.get(d)
    if name is None:
        name = _NAMES[d] = str(d).replace("torch.", "")
    return name


def stream(a):
    """torch's current stream on the tensor's device: the op must run behind whatever produced the tensor.  None, the null stream, for numpy
    arrays and CPU tensors: the library stages them through the device and completes the call before it returns."""
    if isinstance(a, np.ndarray) or not a.is_cuda:
        return None
    import torch
    return torch.cuda.current_stream(a.device).cuda_stream


def device(a):
    return 0 if isinstance(a, np.ndarray) or not a.is_cuda else a.device.index or 0


def mem_kind(a):
    return _lib.MEM_HOST if isinstance(a, np.ndarray) or not a.is_cuda else _lib.MEM_DEVICE


def data_ptr(a):
    """the address of the first element; None for an absent operand"""
    return None if a is None else a.ctypes.data if is_np(a) else a.data_ptr()


def strides(a):
    """strides in elements"""
    return tuple(s // a.itemsize for s in a.strides) if is_np(a) else a.stride()


def empty(like, shape, dtype):
    """an uninitialised output where `like` lives: numpy for numpy, else a tensor on the same device"""
    name = dtype if isinstance(dtype, str) else dtype_name(dtype)
    if is_np(like):
        return np.empty(shape, name)
    import torch
    return torch.empty(shape, dtype=getattr(torch, name), device=like.device)


def cast(a, dtype):
    """`a` itself where it has that dtype already, else a converted copy"""
    name = dtype if isinstance(dtype, str) else dtype_name(dtype)
    if dtype_name(a) == name:
        return a
    if is_np(a):
        return a.astype(name)
    import torch
    return a.to(getattr(torch, name))


def common_dtype(a, b, kept, other):
    """the dtype two operands are read in: their own where both have the same one of `kept`, else `other`"""
    name = dtype_name(a)
    return name if name == dtype_name(b) and name in kept else other


def values(a):
    """fp16 and fp32 values as they are, every other dtype as fp32"""
    return a if dtype_name(a) in FLOATS else cast(a, "float32")


def _lds(shape, st):
    if len(shape) == 2:
        return (shape[1] if shape[0] == 1 else st[0],)
    tok = shape[2] if shape[1] == 1 else st[1]
    return (shape[1] * tok if shape[0] == 1 else st[0], tok)


def lds(a):
    """The outer strides of a 2-D or 3-D operand in elements, as the C entry points take them (row stride; batch stride, token stride): the
    stride of a dimension of size 1 is free, so it is reported packed."""
    return _lds(tuple(a.shape), strides(a))


def as_read(a, disjoint=True):
    """A 2-D or 3-D operand as the kernels read it -> (operand, lds(operand)): `a` itself where the C entry point can read it in place,
    otherwise one packed copy.  The rule: the last dimension has unit stride, or size 1; every outer dimension of size > 1 has a stride of
    at least the minimum below (for numpy also a non-negative multiple of the item size); a dimension of size 1 has a free stride; an empty
    operand is returned as it is.  The minimum is what the dimensions inside span, so that rows and batches do not overlap (disjoint=True:
    batch stride >= (L - 1) * token stride + D, what the lexical heads check), or just the last dimension (disjoint=False: batch stride >= D,
    what dhr_maxsim_scores checks)."""
    shape, st = tuple(a.shape), strides(a)
    ld = _lds(shape, st)
    if 0 in shape:
        return a, ld
    cols = shape[-1]
    ok = (cols == 1 or st[-1] == 1) and (shape[-2] == 1 or ld[-1] >= cols)
    if ok and len(shape) == 3:
        ok = shape[0] == 1 or ld[0] >= ((shape[1] - 1) * ld[1] + cols if disjoint else cols)
    if ok and is_np(a):
        ok = all(s % a.itemsize == 0 for s, n in zip(a.strides, shape) if n > 1)
    if ok:
        return a, ld
    a = np.ascontiguousarray(a) if is_np(a) else a.contiguous()
    return a, lds(a)


def grad_rows(grad, rows, cols, dtype="float32"):
    """The upstream gradient of a [rows, cols] output as the kernels read it -> (tensor, row stride): detached, in `dtype`, read in place
    where as_read allows it (a transposed or expanded gradient, what sum().backward() produces, is copied)."""
    g, ld = as_read(cast(grad.detach().reshape(rows, cols), dtype))
    return g, ld[0]
