"""Contrast-limited adaptive histogram equalization over the C ABI (fd_frames_equalize).

An MI355X extension (the reference has no such stage): the photometric pre-processing a visual-odometry front
end runs ahead of detect_points (absolute response thresholds, FAST's intensity threshold) and track_lk
(brightness constancy), so ingest -> equalize -> detect ... stays on the GPU. The arithmetic, integers only, is
in include/fd_hip.h.
"""
from __future__ import annotations

import ctypes

import numpy as np

from ._lib import fd_equalize_opts
from ._slots import ptr
from ._context import Context, as_frames, frame_output, invoke, resolve_ctx

MAX_TILES = 32
MAX_TILE_AREA = 1 << 24


def _options(tiles, clip_limit, rows, cols):
    """(tiles_x, tiles_y, clip_milli), checked as fd_frames_equalize checks them."""
    if isinstance(tiles, (int, np.integer)):
        tiles = (tiles, tiles)
    if len(tiles) != 2:
        raise ValueError("tiles must be (tiles_x, tiles_y) or one int")
    tiles_x, tiles_y = int(tiles[0]), int(tiles[1])
    if not 1 <= tiles_x <= min(MAX_TILES, cols) or not 1 <= tiles_y <= min(MAX_TILES, rows):
        raise ValueError(f"tiles must be in [1, min({MAX_TILES}, cols)] x [1, min({MAX_TILES}, rows)]")
    clip = 0.0 if clip_limit is None else float(clip_limit)
    if not 0.0 <= clip <= 2.0e6:  # (false for NaN)
        raise ValueError("clip_limit must be in [0, 2e6]")
    if -(-cols // tiles_x) * -(-rows // tiles_y) > MAX_TILE_AREA:
        raise ValueError("a tile must not have more than 2^24 pixels: use more tiles")
    return tiles_x, tiles_y, int(round(clip * 1000))


def equalize_frames(frames, tiles=(8, 8), clip_limit=3.0, out=None, ctx: Context | None = None):
    """fd_frames_equalize: CLAHE of every frame (OpenCV's createCLAHE(clip_limit, tiles) semantics in exact
    integer arithmetic; the tiles are the frame cut without padding).

    frames: uint8 [B, rows, cols] or [rows, cols], numpy or a torch device tensor. tiles: (tiles_x, tiles_y) or
    one int for both, each 1..32 and no larger than its dimension. clip_limit: a float, 0 or None: no clipping
    (tiles 1 and no clipping is plain global histogram equalization).

    Returns the equalized frames in the frames' shape, on the frames' side: a torch tensor for device frames
    (asynchronous on torch's current stream; kernels only and graph-capturable once a call of the shape has
    run), numpy otherwise. out: a preallocated contiguous uint8 array or tensor of the frames' shape on the
    frames' side; it may be frames itself (in place).
    """
    _, f_dev, b, rows, cols, keep = as_frames(frames)
    if rows < 1 or cols < 1 or b < 1:
        raise ValueError("frames must not be empty")
    tiles_x, tiles_y, clip_milli = _options(tiles, clip_limit, rows, cols)
    on_dev = bool(f_dev)
    shape = tuple(keep.shape)
    out = frame_output(shape, "uint8", on_dev, keep.device if on_dev else None, out,
                       f"out must be a contiguous uint8 array of shape {shape}")
    ctx = resolve_ctx(ctx, keep, out)
    opts = fd_equalize_opts(tiles_x, tiles_y, clip_milli)
    invoke(ctx, on_dev, "fd_frames_equalize", ptr(keep), f_dev, b, rows, cols, ctypes.byref(opts), ptr(out), 1 if on_dev else 0)
    return out
