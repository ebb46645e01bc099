"""What the row-streaming drivers (segmentation/augment.py, pretraining/augment.py, datagen/views.py) share on the Python side of
csrc/amx_stream.h's units: the record table that carries per-row parameters to the kernels, the checks every device tensor passes
first, the broadcast of a parameter over rows, and the min / max of rows."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib


class RecordTable:
    """The per-row records of one batch: filled on the host, copied to the device once (``device()``).  A driver's table names its
    record: the numpy ``DTYPE``, the C struct (``STRUCT``) with the library's ``SIZE_SYMBOL`` for it, and the fields that do not start at 0."""
    DTYPE, STRUCT, SIZE_SYMBOL, DEFAULTS = None, None, None, {}

    def __init__(self, n):
        nbytes = getattr(_lib.load(), self.SIZE_SYMBOL)()
        if nbytes != self.DTYPE.itemsize:
            raise _lib.AmxError(f"{self.STRUCT} is {nbytes} bytes in the library and {self.DTYPE.itemsize} here")
        self.host = np.zeros(n, self.DTYPE)
        for field, value in self.DEFAULTS.items():
            self.host[field] = value
        self.dev = None

    def device(self, dev):
        self.dev = torch.from_numpy(self.host.view(np.uint8).reshape(-1)).to(dev)
        return self

    @property
    def args(self):
        return ctypes.c_void_p(self.host.ctypes.data), _lib.ptr(self.dev)


def device_tensor(x, name, dtypes, what):
    """``x``, or the error of a value that is no tensor, lives on the host or has another dtype: ``what`` ("augmentation",
    "data generation") has no host path and converts nothing."""
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{name}: a torch tensor (got {type(x).__name__})")
    if not x.is_cuda:
        raise RuntimeError(f"{name}: the {what} runs on the GPU and has no host path (got a {x.device} tensor)")
    if x.dtype not in dtypes:
        raise TypeError(f"{name}: {' or '.join(str(d).split('.')[1] for d in dtypes)} (got {x.dtype})")
    return x


def per_row(v, shape, name, tail, got="got shape", dtype=np.float64):
    """``v`` (a tensor, an array or a scalar) broadcast to the contiguous array ``shape``, rows in front; what does not broadcast
    raises ``name: tail (got <its shape>)``."""
    a = np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v, dtype=dtype)
    try:
        return np.ascontiguousarray(np.broadcast_to(a, shape))
    except ValueError:
        raise ValueError(f"{name}: {tail} ({got} {a.shape})") from None


def minmax_finalize(scratch, nbytes, n, V, dev):
    """{min, max} [n, 2] of n rows of V from the per-workgroup partials a kernel left in ``scratch``."""
    mm = torch.empty((n, 2), dtype=torch.float32, device=dev)
    _lib.check_envelope(_lib.load().amx_segaug_minmax_finalize(_lib.ptr(scratch), nbytes, n, V, _lib.ptr(mm), _lib.stream(dev)))
    return mm


def minmax(rows, scratch=None):
    """{min, max} [n, 2] of the n rows of a contiguous float32 tensor [n, ...]."""
    n, V = rows.shape[0], rows[0].numel()
    lib = _lib.load()
    mm = torch.empty((n, 2), dtype=torch.float32, device=rows.device)
    nb = lib.amx_segaug_scratch_bytes(n, V)
    sc = _lib.scratch(nb, rows.device) if scratch is None else scratch
    _lib.check_envelope(lib.amx_segaug_minmax(_lib.ptr(rows), n, V, _lib.ptr(mm), _lib.ptr(sc), nb, _lib.stream(rows.device)))
    return mm
