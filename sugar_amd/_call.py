"""The one way the Python modules call the C ABI of libsugar_raster.so: tensor -> pointer, the current stream, the device guard
around an entry point and its return-code check, the "tensors must be on the GPU" guard, and the row -> items list (CSR) that the
mesh kernels walk.  `call` covers the entry points that take the stream as their last argument; the few that take none, or take it
elsewhere, are called on `_lib.load()` directly with `ptr` / `stream`.  The step loop of train_step.NativeTrainer and the rasterizer's
forward / backward keep their own inlined calls: they are the host-bound inner loop."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib


def ptr(t):
    """c_void_p of a tensor's storage; a null pointer for None"""
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def stream(device):
    """the current stream of `device` as the hipStream_t the library takes"""
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def call(name, device, *args):
    """lib.<name>(*args, current stream of `device`) with `device` current; a negative return code raises with the library's message,
    any other is returned (some entry points report a count)"""
    with torch.cuda.device(device):
        rc = getattr(_lib.load(), name)(*args, stream(device))
    if rc < 0:
        raise RuntimeError(f"{name} failed ({rc}): {_lib.last_error()}")
    return rc


def need_gpu(what, **tensors):
    for name, t in tensors.items():
        if not torch.is_tensor(t) or not t.is_cuda:
            raise RuntimeError(f"{what}: {name} must be a tensor on a ROCm device; there is no CPU fallback")


def csr(flat, n_rows):
    """(offsets[n_rows+1] int32, items[len(flat)] int32): row r owns items[offsets[r]:offsets[r+1]] = the positions i with flat[i] == r,
    ascending.  Values must lie in [0, n_rows).  No host read (searchsorted, not bincount: bincount reads its input's maximum on the
    host); works on CPU tensors too."""
    sorted_flat, items = torch.sort(flat.reshape(-1).to(torch.int64), stable=True)
    offsets = torch.searchsorted(sorted_flat, torch.arange(n_rows + 1, device=flat.device))
    return offsets.to(torch.int32), items.to(torch.int32)
