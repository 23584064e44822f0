"""Sub-pixel corner refinement over the C ABI (fd_points_refine).

An MI355X extension (the reference's detectors stop at integer pixels): the cornerSubPix step between
detect_points and track_lk, on the [batch][stride] layouts detect_points writes, so detect -> refine ->
track -> verify stays on the GPU. The arithmetic (exact integer window sums, one 2 x 2 solve in double per
iteration) is in include/fd_hip.h.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

from ._lib import fd_refine_opts
from ._slots import outputs, positions, ptr, slot_arg
from .flow import Pyramid
from ._context import Context, as_frames, invoke, is_device_tensor, resolve_ctx


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
    _, f_dev, b, rows, cols, keep = as_frames(frames)
    on_dev = is_device_tensor(xy)
    ctx = resolve_ctx(ctx, xy, keep)
    pxy = positions(xy, "xy", on_dev)
    s = int(pxy.shape[1])
    if int(pxy.shape[0]) != b:
        raise ValueError("xy and the frames must have the same batch")
    v, cn = slot_arg(valid, "uint8", (b, s), on_dev), slot_arg(counts, "int32", (b,), on_dev)
    oxy, ost, ocnt = outputs((((b, s, 2), "float32", 0), ((b, s), "uint8", 0), ((b,), "int32", 0)), out, on_dev,
                             pxy.device if on_dev else None)
    opts = fd_refine_opts(int(half_window), int(max_iters), float(epsilon), float(min_eigen),
                          float(half_window if max_shift is None else max_shift))
    invoke(ctx, on_dev or bool(f_dev), "fd_points_refine", ptr(keep), f_dev, b, rows, cols, ctypes.byref(opts), ptr(pxy),
           ptr(v), ptr(cn), s, ptr(oxy), ptr(ost), ptr(ocnt), 1 if on_dev else 0)
    return RefineResult(oxy, ost, ocnt)
