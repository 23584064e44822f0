"""Arguments of the stages as the C ABI takes them: pointers, [batch][stride] slot arrays with optional counts [batch]
and valid [batch][stride], on the host (numpy) or on the device (torch), and the outputs of a call.
Shared by every module that hands arrays to the library (ptr); the slot helpers by descriptor, match, flow, refine, geometry, lines, warp.
"""
from __future__ import annotations

import ctypes

import numpy as np


def ptr(x):
    if x is None:
        return None
    return ctypes.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else x.ctypes.data)


def _xp(on_dev):
    if on_dev:
        import torch

        return torch
    return np


def f32(x, name, on_dev, convert=False):
    """x as a contiguous float32 tensor (device) or array (host). Another dtype is a TypeError, or with
    convert (brief_compute's uv) converted."""
    xp = _xp(on_dev)
    if not on_dev:
        x = np.asarray(x)
    if x.dtype != xp.float32:
        if not convert:
            raise TypeError(f"{name} must be float32")
        x = x.to(xp.float32) if on_dev else x.astype(np.float32)
    return x.contiguous() if on_dev else np.ascontiguousarray(x)


def positions(x, name, on_dev, convert=False, msg=None):
    """Positions float32 [B, S, 2]; [S, 2] becomes batch 1. The caller checks B (and S) against its other arguments."""
    x = f32(x, name, on_dev, convert)
    if len(x.shape) == 2:
        x = x[None]
    if len(x.shape) != 3 or x.shape[2] != 2:
        raise ValueError(msg or f"{name} must be [batch, S, 2] or [S, 2]")
    return x


def slot_arg(x, dtype, shape, on_dev):
    """An optional integer argument (valid uint8 [B, S], counts int32 [B], matches int32 [B, S]) converted to
    `dtype` (its name) and `shape`, contiguous; None stays None."""
    if x is None:
        return None
    if on_dev:
        import torch

        return x.to(getattr(torch, dtype)).contiguous().reshape(shape)
    return np.ascontiguousarray(np.asarray(x).astype(dtype, copy=False).reshape(shape))


def outputs(specs, out, on_dev, device=None, msg=None):
    """A call's output arrays, one per (shape, dtype name, fill) of specs: fresh ones on the inputs' side, or
    (device path only) the caller's out= tuple, checked against specs."""
    if not on_dev:
        if out is not None:
            raise ValueError("out= is for device tensors")
        return tuple(np.full(shape, fill, dt) for shape, dt, fill in specs)
    import torch

    if out is None:
        return tuple(torch.full(shape, fill, dtype=getattr(torch, dt), device=device) for shape, dt, fill in specs)
    out = tuple(out)
    ok = len(out) == len(specs) and all(
        tuple(t.shape) == tuple(shape) and t.dtype == getattr(torch, dt) and t.is_contiguous()
        for t, (shape, dt, _) in zip(out, specs))
    if not ok:
        raise ValueError(msg or "out must be contiguous tensors: " + ", ".join(f"{dt} {tuple(shape)}" for shape, dt, _ in specs))
    return out
