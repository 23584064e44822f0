"""Contexts and sides of the batch API over libfdhip.so: the fd_ctx wrapper and the per-GPU default contexts, which side
(host numpy / torch device) an argument is on, the context and the stream of a call, and the tail every wrapper ends in.
Shared by every module of the package that calls the library with a context.
"""
from __future__ import annotations

import ctypes
import os
import threading

import numpy as np

from . import _lib

# order of equal responses in the selection (include/fd_hip.h fd_ctx_set_tie_order)
TIES = {"raster": 0, "reference": 1}

_ctx_lock = threading.Lock()
_contexts: dict[int, "Context"] = {}


class Context:
    """One fd_ctx: a HIP stream and grow-only device workspace on one GPU (not thread-safe)."""

    def __init__(self, device: int = 0):
        L = _lib.load()
        p = ctypes.c_void_p()
        rc = L.fd_ctx_create(int(device), ctypes.byref(p))
        if rc != _lib.FD_OK:
            raise _lib.FdError(rc, f"fd_ctx_create(device={device}) failed (is a GPU visible?)")
        self.ptr = p
        self.device = int(device)

    def close(self):
        if self.ptr:
            _lib.load().fd_ctx_destroy(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_handle: int | None):
        """Run on the given hipStream_t (0 = the HIP null stream); None = the context's own stream."""
        if stream_handle is None:
            _lib.check(self.ptr, _lib.load().fd_ctx_use_own_stream(self.ptr))
        else:
            _lib.check(self.ptr, _lib.load().fd_ctx_set_stream(self.ptr, ctypes.c_void_p(int(stream_handle))))

    def synchronize(self):
        _lib.check(self.ptr, _lib.load().fd_ctx_synchronize(self.ptr))

    def reserve(self, kind: int, batch: int, rows: int, cols: int, max_prior_total: int = 0):
        _lib.check(self.ptr, _lib.load().fd_ctx_reserve(self.ptr, kind, batch, rows, cols, max_prior_total))

    def set_tie_order(self, ties: str):
        """'raster' (equal responses by raster index) or 'reference' (the reference's std::sort order)."""
        _lib.check(self.ptr, _lib.load().fd_ctx_set_tie_order(self.ptr, TIES[ties]))

    def frame_status(self, batch: int, out=None):
        """Per-frame FD_FRAME_* words of the last selection call: numpy uint32 [batch] (synchronous), or
        copied asynchronously into `out` (a device int32 tensor [batch]) on the context stream."""
        if out is not None:
            _lib.check(self.ptr, _lib.load().fd_ctx_frame_status(self.ptr, ctypes.c_void_p(out.data_ptr()), batch, 1))
            return out
        st = np.zeros((batch,), np.uint32)
        _lib.check(self.ptr, _lib.load().fd_ctx_frame_status(self.ptr, ctypes.c_void_p(st.ctypes.data), batch, 0))
        return st


def _default_device() -> int:
    return int(os.environ.get("FD_DEVICE", "0"))


def default_context(device: int | None = None) -> Context:
    """The shared context of a GPU (default: $FD_DEVICE or 0), created on first use."""
    device = _default_device() if device is None else int(device)
    with _ctx_lock:
        c = _contexts.get(device)
        if c is None:
            c = Context(device)
            _contexts[device] = c
        return c


def is_device_tensor(x) -> bool:
    return type(x).__module__.startswith("torch") and getattr(x, "is_cuda", False)


def as_frames(x):
    """(pointer, on_device, batch, rows, cols, keepalive) for a u8 [B,]R,C array or tensor."""
    if is_device_tensor(x):
        import torch

        if x.dtype != torch.uint8:
            raise TypeError("frames must be uint8")
        if not x.is_contiguous():
            x = x.contiguous()
        shape = tuple(x.shape)
        ptr, on_dev = x.data_ptr(), 1
    else:
        x = np.ascontiguousarray(x)
        if x.dtype != np.uint8:
            raise TypeError("frames must be uint8")
        shape = x.shape
        ptr, on_dev = x.ctypes.data, 0
    if len(shape) == 2:
        b, r, c = 1, shape[0], shape[1]
    elif len(shape) == 3:
        b, r, c = shape
    else:
        raise ValueError("frames must be [rows, cols] or [batch, rows, cols]")
    return ptr, on_dev, int(b), int(r), int(c), x


def resolve_ctx(ctx: Context | None, *inputs) -> Context:
    """The context of a call: `ctx`, or the default context of the GPU the torch inputs live on. A
    context on another device than its inputs is an error (its workspace and stream are per device)."""
    dev = None
    for x in inputs:
        if is_device_tensor(x):
            import torch

            d = x.device.index if x.device.index is not None else torch.cuda.current_device()
            if dev is not None and d != dev:
                raise ValueError(f"inputs on different devices ({dev} and {d})")
            dev = d
    if ctx is None:
        return default_context(dev)
    if dev is not None and ctx.device != dev:
        raise ValueError(f"context is on device {ctx.device} but the inputs are on device {dev}")
    return ctx


def bind_stream(ctx: Context, on_device: bool):
    """Device inputs run on torch's current stream of the context's device; host inputs on the
    context's own stream. (The library orders a stream switch after the previous stream's work.)"""
    if on_device:
        import torch

        ctx.set_stream(torch.cuda.current_stream(ctx.device).cuda_stream)
    else:
        ctx.set_stream(None)


def frame_output(shape, dtype, on_dev, device, out, msg):
    """A whole-frame result of `shape` and `dtype` (its name): a fresh array on the inputs' side (`device`: the torch
    device), or the caller's out=, which must be on that side (a ValueError of its own) and a contiguous array of that
    dtype and shape, on the host a writeable numpy one (ValueError(msg))."""
    if out is None:
        if on_dev:
            import torch

            return torch.empty(shape, dtype=getattr(torch, dtype), device=device)
        return np.empty(shape, dtype)
    if is_device_tensor(out) != on_dev:
        raise ValueError("out must be on the side of the frames")
    if on_dev:
        import torch

        ok = out.dtype == getattr(torch, dtype) and out.is_contiguous()
    else:
        ok = isinstance(out, np.ndarray) and out.dtype == dtype and out.flags.c_contiguous and out.flags.writeable
    if not ok or tuple(out.shape) != shape:
        raise ValueError(msg)
    return out


def invoke(ctx: Context, on_device: bool, name: str, *args):
    """The tail of a wrapper: the context's stream for the side of the call, the library's entry point `name` on
    (ctx, *args), and its status (FdError with the context's message)."""
    bind_stream(ctx, on_device)
    _lib.check(ctx.ptr, getattr(_lib.load(), name)(ctx.ptr, *args))
