"""Line band descriptor over the C ABI (fd_lines_describe).

An MI355X extension (the reference's line path stops at the rectangles): the stage between lsd_lines and
nn_match, so that the segments of two frames can be matched, unguided or by their midpoints, with the matchers
as they are. The arithmetic (integer gradient sums per row of the support region, band statistics and norms in
double) is in include/fd_hip.h.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import fd_line_desc_opts
from ._slots import f32, outputs, ptr, slot_arg
from .points import Context, _bind_stream, _frames, _is_torch_device_tensor, _resolve_ctx


@dataclass
class LineDescResult:
    desc: object    # float32 [B, S, 8 * bands]: unit-norm descriptors, all zero where valid == 0
    xy: object      # float32 [B, S, 2]: segment midpoints (x, y): nn_match's q_xy / t_xy
    valid: object   # uint8 [B, S]: 0 = degenerate line or flat support region: nn_match's q_valid / t_valid
    counts: object  # int32 [B]: lines per frame: nn_match's q_counts / t_counts


def _padded(lines):
    """lsd_lines' list of [n, 4 or 12] arrays as one zero-padded float32 [B, S, floats] array and its counts."""
    arrays = [np.asarray(x, np.float32) for x in lines]
    floats = {a.shape[1] for a in arrays if a.ndim == 2}
    if any(a.ndim != 2 for a in arrays) or len(floats) != 1:
        raise ValueError("a list of lines must hold [n, 4] or [n, 12] arrays of one width")
    stride = max(a.shape[0] for a in arrays)
    out = np.zeros((len(arrays), stride, floats.pop()), np.float32)
    for b, a in enumerate(arrays):
        out[b, :a.shape[0]] = a
    return out, np.array([a.shape[0] for a in arrays], np.int32)


def describe_lines(frames, lines, counts=None, bands: int = 9, band_width: int = 7, out=None,
                   ctx: Context | None = None) -> LineDescResult:
    """fd_lines_describe: the band descriptor of every line of every frame.

    frames: uint8 [B, rows, cols] or [rows, cols], numpy or a torch device tensor. lines: what lsd_lines
    returns (a list over frames of float32 [n, 12] arrays; [n, 4] endpoints pass too), or a padded float32
    array or torch device tensor [B, S, 4 or 12] ([S, 4 or 12] for batch 1) with counts int32 [B] (None = S
    each). Floats 0..3 of a line are (start x, start y, end x, end y).

    Returns descriptors, midpoints, valid flags and counts, padded to one stride, on the side of lines: numpy
    for a list or an array (slots past a frame's count are 0), torch tensors for a device tensor (asynchronous
    on torch's current stream). They pass to nn_match as they are:

        a, b = describe_lines(f0, l0), describe_lines(f1, l1)
        nn_match(a.desc, b.desc, a.counts, b.counts, a.valid, b.valid, max_ratio=0.8, cross_check=True,
                 q_xy=a.xy, t_xy=b.xy, radius=40.0)

    Device path only: out = preallocated contiguous tensors (desc float32 [B, S, 8 * bands], xy float32
    [B, S, 2], valid uint8 [B, S]); slots past a count then keep their contents, and with device frames the
    call is one kernel (graph-capturable).
    """
    fptr, f_dev, b, rows, cols, keep = _frames(frames)
    if isinstance(lines, (list, tuple)):
        if counts is not None:
            raise ValueError("a list of lines carries its own counts")
        lines, counts = _padded(lines)
    on_dev = _is_torch_device_tensor(lines)
    ctx = _resolve_ctx(ctx, lines, keep)
    ln = f32(lines, "lines", on_dev)
    if len(ln.shape) == 2:
        ln = ln[None]
    if len(ln.shape) != 3 or int(ln.shape[2]) not in (4, 12):
        raise ValueError("lines must be [batch, S, 4 or 12] or [S, 4 or 12]")
    if int(ln.shape[0]) != b:
        raise ValueError("lines and the frames must have the same batch")
    if not 1 <= int(bands) <= 32 or not 1 <= int(band_width) <= 16:
        raise ValueError("bands must be in [1, 32] and band_width in [1, 16]")
    s, floats, dim = int(ln.shape[1]), int(ln.shape[2]), 8 * int(bands)
    cn = slot_arg(counts, "int32", (b,), on_dev)
    desc, xy, valid = outputs((((b, s, dim), "float32", 0), ((b, s, 2), "float32", 0), ((b, s), "uint8", 0)), out, on_dev,
                              ln.device if on_dev else None)
    opts = fd_line_desc_opts(int(bands), int(band_width))
    if s > 0:  # (an empty array has no address to hand over; the library does no work for stride 0 either)
        _bind_stream(ctx, on_dev or bool(f_dev))
        rc = _lib.load().fd_lines_describe(ctx.ptr, ctypes.c_void_p(fptr), f_dev, b, rows, cols, ctypes.byref(opts), ptr(ln),
                                           floats, ptr(cn), s, ptr(desc), ptr(xy), ptr(valid), 1 if on_dev else 0)
        _lib.check(ctx.ptr, rc)
    if cn is None:
        if on_dev:
            import torch

            cn = torch.full((b,), s, dtype=torch.int32, device=ln.device)
        else:
            cn = np.full((b,), s, np.int32)
    return LineDescResult(desc, xy, valid, cn)
