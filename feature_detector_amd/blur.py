"""Gaussian smoothing over the C ABI (fd_blur_taps, fd_frames_blur).

An MI355X extension (the reference has no such stage): the low-pass a front end runs ahead of brief_compute
(ORB smooths with a 7 x 7, sigma 2 kernel before it compares single samples) and, with step 2, one level of a
Gaussian pyramid (build_pyramid(kernel="gauss") builds all of them), so ingest -> blur -> describe stays on the
GPU. The arithmetic, integers only, is in include/fd_hip.h.
"""
from __future__ import annotations

import ctypes

from . import _lib
from ._lib import FD_BLUR_MAX_RADIUS, fd_blur_opts
from ._slots import ptr
from ._context import Context, as_frames, frame_output, invoke, resolve_ctx


def gaussian_taps(sigma: float, radius: int | None = None) -> tuple[int, list[int]]:
    """fd_blur_taps: (radius, [w[0], ..., w[radius]]), the integer taps of a Gaussian of standard deviation
    sigma with w[0] + 2 * (w[1] + ... + w[radius]) == 256. radius None (or 0): min(15, max(1, ceil(3 sigma)))."""
    opts = fd_blur_opts()
    rc = _lib.load().fd_blur_taps(float(sigma), 0 if radius is None else int(radius), ctypes.byref(opts))
    if rc != _lib.FD_OK:
        raise _lib.FdError(rc, "fd_blur_taps: sigma must be finite and > 0, and the rounded taps must not dip at the centre")
    return int(opts.radius), [int(opts.taps[k]) for k in range(opts.radius + 1)]


def _options(sigma, radius, taps, step) -> fd_blur_opts:
    if (sigma is None) == (taps is None):
        raise ValueError("give either sigma or taps")
    if taps is None:
        radius, taps = gaussian_taps(sigma, radius)
    else:
        taps = [int(t) for t in taps]
        if radius is not None and int(radius) != len(taps) - 1:
            raise ValueError("taps must have radius + 1 entries")
        if not 1 <= len(taps) <= FD_BLUR_MAX_RADIUS + 1:
            raise ValueError(f"taps must have 1 to {FD_BLUR_MAX_RADIUS + 1} entries: w[0], ..., w[radius]")
    opts = fd_blur_opts()
    opts.radius = len(taps) - 1
    for k, t in enumerate(taps):
        opts.taps[k] = t
    opts.step = int(step)
    return opts


def blur_frames(frames, sigma=None, radius=None, taps=None, step=1, out=None, ctx: Context | None = None):
    """fd_frames_blur: every frame smoothed by a separable symmetric integer kernel, reflect-101 borders, one
    rounding at the end.

    frames: uint8 [B, rows, cols] or [rows, cols], numpy or a torch device tensor. Give either sigma (the taps
    are gaussian_taps(sigma, radius)) or taps = [w[0], ..., w[r]] (r <= 15, every tap >= 0, w[0] + 2 * the rest
    == 256; [96, 64, 16] is pyrDown's kernel). step 2 keeps every second row and column: the output is
    [(rows + 1) // 2, (cols + 1) // 2].

    Returns the smoothed frames on the frames' side: a torch tensor for device frames (asynchronous on torch's
    current stream; one kernel, graph-capturable), numpy otherwise. out: a preallocated contiguous uint8 array
    or tensor of the output's shape on the frames' side; it must not be frames (there is no in-place blur).
    Options the library rejects (radius, tap sum, step) raise FdError.
    """
    _, f_dev, b, rows, cols, keep = as_frames(frames)
    if rows < 1 or cols < 1 or b < 1:
        raise ValueError("frames must not be empty")
    opts = _options(sigma, radius, taps, step)
    on_dev = bool(f_dev)
    s = 2 if opts.step == 2 else 1  # (any other step is refused by the library)
    shape = tuple(keep.shape[:-2]) + ((rows + s - 1) // s, (cols + s - 1) // s)
    out = frame_output(shape, "uint8", on_dev, keep.device if on_dev else None, out,
                       f"out must be a contiguous uint8 array of shape {shape}")
    ctx = resolve_ctx(ctx, keep, out)
    invoke(ctx, on_dev, "fd_frames_blur", ptr(keep), f_dev, b, rows, cols, ctypes.byref(opts), ptr(out), 1 if on_dev else 0)
    return out
