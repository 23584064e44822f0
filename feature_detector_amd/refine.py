"""Sub-pixel corner refinement over the C ABI (fd_points_refine).

An MI355X extension (the reference's detectors stop at integer pixels): the cornerSubPix step between
detect_points and track_lk, on the [batch][stride] layouts detect_points writes, so detect -> refine ->
track -> verify stays on the GPU. The arithmetic (exact integer window sums, one 2 x 2 solve in double per
iteration) is in include/fd_hip.h.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import fd_refine_opts
from .flow import Pyramid, _ptr
from .points import Context, _bind_stream, _frames, _is_torch_device_tensor, _resolve_ctx


@dataclass
class RefineResult:
    xy: object      # float32 [B, S, 2]: refined positions (x, y); the input position where status != 1
    status: object  # uint8 [B, S]: 1 = refined (fd_refine_status)
    counts: object  # int32 [B]: refined slots per frame


def refine_points(frames, xy, counts=None, valid=None, half_window: int = 5, max_iters: int = 20, epsilon: float = 0.01,
                  min_eigen: float = 1e-3, max_shift: float | None = None, out=None,
                  ctx: Context | None = None) -> RefineResult:
    """fd_points_refine: move the features xy of every frame onto the corners they sit near.

    frames: a uint8 batch [B, rows, cols] (or [rows, cols]), numpy or a torch device tensor, or a Pyramid
    (its level 0 is used). xy: float32 [B, S, 2] (or [S, 2] for batch 1), (x, y) as detect_points writes
    them; counts int32 [B] (None = S each; detect_points' device counts pass as they are); valid uint8
    [B, S] (None = all valid). max_shift None means half_window.

    Host (numpy) xy gives numpy outputs; torch device xy gives torch outputs, asynchronous on torch's
    current stream. Slots the call does not write (>= counts[b]) are 0. Device path only: out =
    preallocated contiguous tensors (xy float32 [B, S, 2], status uint8 [B, S], counts int32 [B]); unwritten
    slots then keep their contents, out[0] may be xy itself (in place), and with device frames the call is
    kernels only (graph-capturable).

    The defaults (an 11 x 11 window, 20 iterations, epsilon 0.01) are the usual conventions of cornerSubPix
    callers, not values tuned for this library.
    """
    if isinstance(frames, Pyramid):
        frames = frames.level(0)
    ptr, f_dev, b, rows, cols, keep = _frames(frames)
    on_dev = _is_torch_device_tensor(xy)
    ctx = _resolve_ctx(ctx, xy, keep)
    if on_dev:
        import torch

        if xy.dtype != torch.float32:
            raise TypeError("xy must be float32")
        pxy = xy if xy.is_contiguous() else xy.contiguous()
        if pxy.dim() == 2:
            pxy = pxy.unsqueeze(0)
    else:
        pxy = np.asarray(xy)
        if pxy.dtype != np.float32:
            raise TypeError("xy must be float32")
        pxy = np.ascontiguousarray(pxy)
        if pxy.ndim == 2:
            pxy = pxy[None]
    if len(pxy.shape) != 3 or pxy.shape[2] != 2:
        raise ValueError("xy must be [batch, S, 2] or [S, 2]")
    s = int(pxy.shape[1])
    if int(pxy.shape[0]) != b:
        raise ValueError("xy and the frames must have the same batch")
    if on_dev:
        v = None if valid is None else valid.to(torch.uint8).contiguous().reshape(b, s)
        cn = None if counts is None else counts.to(torch.int32).contiguous().reshape(b)
        if out is not None:
            oxy, ost, ocnt = out
            for t, shape, dt in ((oxy, (b, s, 2), torch.float32), (ost, (b, s), torch.uint8), (ocnt, (b,), torch.int32)):
                if tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous():
                    raise ValueError(f"out must be contiguous tensors: float32 {(b, s, 2)}, uint8 {(b, s)}, int32 {(b,)}")
        else:
            oxy = torch.zeros((b, s, 2), dtype=torch.float32, device=pxy.device)
            ost = torch.zeros((b, s), dtype=torch.uint8, device=pxy.device)
            ocnt = torch.zeros((b,), dtype=torch.int32, device=pxy.device)
    else:
        if out is not None:
            raise ValueError("out= is for device tensors")
        v = None if valid is None else np.ascontiguousarray(np.asarray(valid, np.uint8).reshape(b, s))
        cn = None if counts is None else np.ascontiguousarray(np.asarray(counts).astype(np.int32).reshape(b))
        oxy, ost, ocnt = np.zeros((b, s, 2), np.float32), np.zeros((b, s), np.uint8), np.zeros((b,), np.int32)
    opts = fd_refine_opts(int(half_window), int(max_iters), float(epsilon), float(min_eigen),
                          float(half_window if max_shift is None else max_shift))
    _bind_stream(ctx, on_dev or bool(f_dev))
    rc = _lib.load().fd_points_refine(ctx.ptr, ctypes.c_void_p(ptr), f_dev, b, rows, cols, ctypes.byref(opts), _ptr(pxy),
                                      _ptr(v), _ptr(cn), s, _ptr(oxy), _ptr(ost), _ptr(ocnt), 1 if on_dev else 0)
    _lib.check(ctx.ptr, rc)
    return RefineResult(oxy, ost, ocnt)
