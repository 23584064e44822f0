"""The line stage over the C ABI: the level-line map (fd_lsd_map), the LSD segments (fd_lsd_lines) and their band
descriptor (fd_lines_describe).

The descriptor is an MI355X extension (the reference's line path stops at the rectangles): the stage between lsd_lines and
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
from ._context import Context, as_frames, invoke, is_device_tensor, resolve_ctx


def lsd_map(frames, min_norm: float = 20.0, cap: int | None = None, ctx: Context | None = None, out=None):
    """ComputeLineLevelAngleMap (fd_lsd_map / fd_lsd_map_pitched).

    Host (numpy) frames: returns per frame (norm, angle, valid, valid_idx_colmajor); maps are
    (rows-1, cols-1). Torch device frames: returns device tensors (norm [B, R-1, C-1] f32, angle f32,
    valid u8, valid_idx int32 [B, cap], counts int64 [B]), asynchronous on torch's current stream;
    the maps are views of storage whose rows are padded to 16 entries (aligned row stores); `out` may
    pass them preallocated (graph capture), contiguous or as such row-padded views sharing one row
    pitch; any of norm/angle/valid may be None to skip.
    """
    _, on_dev, b, r, c, keep = as_frames(frames)
    ctx = resolve_ctx(ctx, frames)
    mr, mc = r - 1, c - 1
    cap = mr * mc if cap is None else cap
    if on_dev:
        import torch

        if out is None:
            dev = frames.device
            pitch = (mc + 15) // 16 * 16
            out = (torch.empty((b, mr, pitch), dtype=torch.float32, device=dev)[..., :mc],
                   torch.empty((b, mr, pitch), dtype=torch.float32, device=dev)[..., :mc],
                   torch.empty((b, mr, pitch), dtype=torch.uint8, device=dev)[..., :mc],
                   torch.empty((b, max(cap, 1)), dtype=torch.int32, device=dev),
                   torch.empty((b,), dtype=torch.int64, device=dev))
        norm, ang, val, idx, cnt = out
        pitch = None
        for t in (norm, ang, val):
            if t is None:
                continue
            if tuple(t.shape) != (b, mr, mc) or t.stride(2) != 1 or t.stride(0) != mr * t.stride(1):
                raise ValueError(f"lsd_map: maps must be [{b}, {mr}, {mc}] with unit column stride and rows "
                                 "packed at one pitch")
            if pitch not in (None, t.stride(1)):
                raise ValueError("lsd_map: norm / angle / valid must share one row pitch")
            pitch = t.stride(1)
        pitch = mc if pitch is None else pitch
        invoke(ctx, True, "fd_lsd_map_pitched", ptr(keep), 1, b, r, c, float(min_norm), ptr(norm), ptr(ang), ptr(val),
               int(pitch), ptr(idx), int(idx.shape[1]), ptr(cnt), 1)
        return out
    norm = np.zeros((b, mr, mc), np.float32)
    ang = np.zeros((b, mr, mc), np.float32)
    val = np.zeros((b, mr, mc), np.uint8)
    idx = np.zeros((b, max(cap, 1)), np.int32)
    cnt = np.zeros((b,), np.int64)
    invoke(ctx, False, "fd_lsd_map", ptr(keep), 0, b, r, c, float(min_norm), ptr(norm), ptr(ang), ptr(val), ptr(idx), int(cap),
           ptr(cnt), 0)
    return [(norm[i], ang[i], val[i], idx[i, :cnt[i]].copy()) for i in range(b)]


# FeatureLineDetector::Options defaults (feature_line_detector.h:40-45); kDegToRad = kPai / 180 in float.
LSD_TOL_RAD = float(np.float32(22.5) * (np.float32(3.14159265358979323846) / np.float32(180.0)))


def lsd_lines(frames, needed: int = 1, min_norm: float = 20.0, tol_rad: float = LSD_TOL_RAD, min_length: float = 20.0,
              min_inlier: float = 0.6, max_lines: int = 4096, threads: int = 0, ctx: Context | None = None):
    """FeatureLineDetector::DetectGoodFeatures for a batch (fd_lsd_lines): GPU level-line map (compact
    lists), region growing and rectangle fitting on `threads` host threads (0: all, capped by
    OMP_NUM_THREADS). frames: numpy [B, R, C] / [R, C] u8 or a torch device tensor.

    Returns a list over frames of float32 arrays [n, 12] (start x, y, end x, y, center x, y, length,
    width, angle, dir x, y, inlier ratio); columns 0-3 are the reference's Vec4 features."""
    _, on_dev, b, r, c, keep = as_frames(frames)
    ctx = resolve_ctx(ctx, frames)
    opts = _lib.fd_lsd_opts(float(min_norm), float(tol_rad), float(min_length), float(min_inlier))
    out = np.empty((b, max(max_lines, 1), _lib.LSD_RECT_FLOATS), np.float32)
    cnt = np.zeros((b,), np.int32)
    invoke(ctx, on_dev, "fd_lsd_lines", ptr(keep), 1 if on_dev else 0, b, r, c, ctypes.byref(opts), int(needed), ptr(out),
           int(max_lines), ptr(cnt), int(threads))
    if (cnt > max_lines).any():
        raise _lib.FdError(_lib.FD_ERR_CAPACITY, f"max_lines={max_lines} < {int(cnt.max())} segments found")
    return [out[i, :cnt[i]].copy() for i in range(b)]


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
    _, f_dev, b, rows, cols, keep = as_frames(frames)
    if isinstance(lines, (list, tuple)):
        if counts is not None:
            raise ValueError("a list of lines carries its own counts")
        lines, counts = _padded(lines)
    on_dev = is_device_tensor(lines)
    ctx = resolve_ctx(ctx, lines, keep)
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
        invoke(ctx, on_dev or bool(f_dev), "fd_lines_describe", ptr(keep), f_dev, b, rows, cols, ctypes.byref(opts), ptr(ln),
               floats, ptr(cn), s, ptr(desc), ptr(xy), ptr(valid), 1 if on_dev else 0)
    if cn is None:
        if on_dev:
            import torch

            cn = torch.full((b,), s, dtype=torch.int32, device=ln.device)
        else:
            cn = np.full((b,), s, np.int32)
    return LineDescResult(desc, xy, valid, cn)
