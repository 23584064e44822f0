"""Batch host API over libfdhip.so: point detection, selection over given candidates, the per-pixel stage alone.

Inputs are numpy arrays (host memory, staged by the library) or torch CUDA/ROCm tensors (device
memory, used in place on the context's stream, which follows torch's current stream). Every call
runs the HIP kernels; there is no CPU path. Contexts and sides are _context.py's.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._context import TIES, Context, bind_stream, default_context, as_frames, invoke, resolve_ctx  # noqa: F401
from ._lib import FD_FAST, FD_HARRIS, FD_SHI_TOMASI, fd_point_opts
from ._slots import ptr

KINDS = {"harris": FD_HARRIS, "shi_tomasi": FD_SHI_TOMASI, "fast": FD_FAST}
FRAME_TIES, FRAME_RESOLVED, FRAME_UNRESOLVED, FRAME_VALUE_RANGE, FRAME_GUARD = 0x1, 0x2, 0x4, 0x40000000, 0xBE000000
FRAME_REDETECTED = 0x8  # FAST, raster order: selected a second time without the adaptive emission cut


def _priors(prior, batch):
    """prior: None, or a list (per frame) of (n_i, 2) float arrays of (x, y)."""
    if prior is None:
        return None, None, None
    if len(prior) != batch:
        raise ValueError("prior must have one entry per frame")
    counts = np.array([len(p) for p in prior], np.int32)
    flat = (np.concatenate([np.asarray(p, np.float32).reshape(-1, 2) for p in prior]) if counts.sum() > 0
            else np.zeros((1, 2), np.float32))
    flat = np.ascontiguousarray(flat, np.float32)
    return flat, counts, (flat, counts)


@dataclass
class DetectResult:
    xy: object  # [batch, stride, 2] float32 (numpy or torch)
    counts: object  # [batch] int32
    status: object = None  # [batch] FD_FRAME_* words (numpy uint32, or a device int32 tensor), if fetched

    def features(self, b: int) -> np.ndarray:
        xy = self.xy if isinstance(self.xy, np.ndarray) else self.xy.cpu().numpy()
        n = int(self.counts[b]) if isinstance(self.counts, np.ndarray) else int(self.counts[b].item())
        return xy[b, :n].copy()

    def frame_flags(self) -> np.ndarray:
        """Per-frame FD_FRAME_* words as numpy uint32 (synchronises a device result)."""
        if self.status is None:
            raise ValueError("status was not fetched (out= without a status tensor)")
        st = self.status if isinstance(self.status, np.ndarray) else self.status.cpu().numpy()
        return st.astype(np.uint32)

    def check(self) -> "DetectResult":
        """Raise if a frame tripped an internal guard, or was left unresolved in the reference tie order
        (FRAME_UNRESOLVED: device results carry no flags in their counts)."""
        bad = np.nonzero(self.frame_flags() & np.uint32(FRAME_GUARD | FRAME_VALUE_RANGE | FRAME_UNRESOLVED))[0]
        if len(bad):
            raise _lib.FdError(_lib.FD_ERR_HIP, f"selection flags 0x{int(self.frame_flags()[bad[0]]):x} on frame {bad[0]}")
        return self


def detect_points(kind, frames, need: int, min_feature_distance: int = 15, min_valid_response: float = 0.1,
                  prior=None, ctx: Context | None = None, out=None, ties: str | None = None) -> DetectResult:
    """FeaturePointDetector::DetectGoodFeatures on a batch (include/fd_hip.h fd_points_detect).

    Returns the NEW features per frame (x, y), in selection order, and the per-frame status words.
    ties="reference": frames whose greedy scan meets equal responses are re-selected in the
    reference's std::sort order (libstdc++'s introsort emulated on the GPU, k_select_reference), so
    every frame equals the reference's DetectGoodFeatures; asynchronous and graph-capturable once the
    workspace exists (one call of the shape first). ties="raster": equal responses by raster index;
    identical to "reference" wherever no tie reaches the scan, and FD_FRAME_TIES in the status words
    marks the frames where one did. Default (None): "reference" for host frames
    (the reference API's semantics), "raster" for torch device frames (asynchronous; check
    `frame_flags() & FRAME_TIES` or pass ties="reference" to get the reference order there too).
    With torch device frames the outputs are device tensors (on the current stream); `out` may pass
    preallocated (xy, counts) or (xy, counts, status) tensors so that repeated calls allocate nothing.
    """
    kind = KINDS[kind] if isinstance(kind, str) else int(kind)
    ptr, on_dev, b, r, c, keep = as_frames(frames)
    ctx = resolve_ctx(ctx, frames)
    bind_stream(ctx, bool(on_dev))
    if ties is None:
        ties = "raster" if on_dev else "reference"
    ctx.set_tie_order(ties)
    opts = fd_point_opts(int(min_feature_distance), float(min_valid_response))
    pxy, pcnt, _keep2 = _priors(prior, b)
    stride = max(int(need), 1) + 1
    status = None
    if on_dev:
        import torch

        if out is None:
            xy = torch.empty((b, stride, 2), dtype=torch.float32, device=frames.device)
            cnt = torch.empty((b,), dtype=torch.int32, device=frames.device)
            status = torch.empty((b,), dtype=torch.int32, device=frames.device)
        else:
            xy, cnt = out[0], out[1]
            status = out[2] if len(out) > 2 else None
            stride = xy.shape[1]
        xy_ptr, cnt_ptr = xy.data_ptr(), cnt.data_ptr()
    else:
        xy = np.zeros((b, stride, 2), np.float32)
        cnt = np.zeros((b,), np.int32)
        xy_ptr, cnt_ptr = xy.ctypes.data, cnt.ctypes.data
    rc = _lib.load().fd_points_detect(
        ctx.ptr, kind, ctypes.c_void_p(ptr), on_dev, b, r, c, ctypes.byref(opts),
        ctypes.c_void_p(pxy.ctypes.data) if pxy is not None else None,
        ctypes.c_void_p(pcnt.ctypes.data) if pcnt is not None else None,
        int(need), ctypes.c_void_p(xy_ptr), stride, ctypes.c_void_p(cnt_ptr), on_dev)
    _lib.check(ctx.ptr, rc)
    del keep
    if on_dev:
        if status is not None:
            ctx.frame_status(b, out=status)
    else:
        status = ctx.frame_status(b)
    return DetectResult(xy, cnt, status)


def select_points(candidates, rows: int, cols: int, need: int, min_feature_distance: int = 15, prior=None,
                  ties: str | None = None, ctx: Context | None = None, out=None) -> DetectResult:
    """SelectGoodFeatures over caller-supplied candidates (fd_points_select): the ComputeCandidates
    seam of a detector whose candidates come from elsewhere (feature_point_detector.h:44).

    candidates: a list (per frame) of (resp, x, y) arrays in the order they were pushed -- host
    arrays, returns numpy results (ties default "reference"); or a tuple of torch device tensors
    (resp [B, cap] float32, x [B, cap] int32, y [B, cap] int32, counts [B] int64), returns device
    tensors asynchronously (ties default "raster"; `out` as in detect_points).
    """
    opts = fd_point_opts(int(min_feature_distance), 0.0)
    L = _lib.load()
    if isinstance(candidates, tuple) and hasattr(candidates[0], "data_ptr"):
        import torch

        resp, xs, ys, counts = candidates
        b, cap = resp.shape
        for t, dt in ((resp, torch.float32), (xs, torch.int32), (ys, torch.int32)):
            if t.dtype != dt or tuple(t.shape) != (b, cap) or not t.is_cuda or not t.is_contiguous():
                raise ValueError("device candidates: contiguous resp f32 / x, y int32 [B, cap] tensors")
        if counts.dtype != torch.int64 or tuple(counts.shape) != (b,) or not counts.is_cuda:
            raise ValueError("device candidates: counts int64 [B]")
        ctx = resolve_ctx(ctx, resp)
        bind_stream(ctx, True)
        ctx.set_tie_order(ties or "raster")
        pxy, pcnt, _keep2 = _priors(prior, b)
        stride = max(int(need), 1) + 1
        status = None
        if out is None:
            xy = torch.empty((b, stride, 2), dtype=torch.float32, device=resp.device)
            cnt = torch.empty((b,), dtype=torch.int32, device=resp.device)
            status = torch.empty((b,), dtype=torch.int32, device=resp.device)
        else:
            xy, cnt = out[0], out[1]
            status = out[2] if len(out) > 2 else None
            stride = xy.shape[1]
        rc = L.fd_points_select(ctx.ptr, b, rows, cols, ctypes.byref(opts), ctypes.c_void_p(resp.data_ptr()),
                                ctypes.c_void_p(xs.data_ptr()), ctypes.c_void_p(ys.data_ptr()),
                                ctypes.c_void_p(counts.data_ptr()), int(cap), 1,
                                ctypes.c_void_p(pxy.ctypes.data) if pxy is not None else None,
                                ctypes.c_void_p(pcnt.ctypes.data) if pcnt is not None else None,
                                int(need), ctypes.c_void_p(xy.data_ptr()), stride, ctypes.c_void_p(cnt.data_ptr()), 1)
        _lib.check(ctx.ptr, rc)
        if status is not None:
            ctx.frame_status(b, out=status)
        return DetectResult(xy, cnt, status)
    b = len(candidates)
    counts = np.array([len(c[0]) for c in candidates], np.int64)
    cap = max(int(counts.max()) if b else 0, 1)
    resp = np.zeros((b, cap), np.float32)
    xs = np.zeros((b, cap), np.int32)
    ys = np.zeros((b, cap), np.int32)
    for i, (r_, x_, y_) in enumerate(candidates):
        n = counts[i]
        if len(x_) != n or len(y_) != n:
            raise ValueError(f"frame {i}: resp, x and y differ in length")
        resp[i, :n], xs[i, :n], ys[i, :n] = r_, x_, y_
    ctx = resolve_ctx(ctx)
    bind_stream(ctx, False)
    ctx.set_tie_order(ties or "reference")
    pxy, pcnt, _keep2 = _priors(prior, b)
    stride = max(int(need), 1) + 1
    xy = np.zeros((b, stride, 2), np.float32)
    cnt = np.zeros((b,), np.int32)
    rc = L.fd_points_select(ctx.ptr, b, rows, cols, ctypes.byref(opts), ctypes.c_void_p(resp.ctypes.data),
                            ctypes.c_void_p(xs.ctypes.data), ctypes.c_void_p(ys.ctypes.data),
                            ctypes.c_void_p(counts.ctypes.data), cap, 0,
                            ctypes.c_void_p(pxy.ctypes.data) if pxy is not None else None,
                            ctypes.c_void_p(pcnt.ctypes.data) if pcnt is not None else None,
                            int(need), ctypes.c_void_p(xy.ctypes.data), stride, ctypes.c_void_p(cnt.ctypes.data), 0)
    _lib.check(ctx.ptr, rc)
    return DetectResult(xy, cnt, ctx.frame_status(b))


def point_response(kind, frames, min_valid_response: float = 0.1, out=None, ctx: Context | None = None,
                   append: bool = False):
    """The per-pixel stage alone (fd_points_response) on torch device frames [B, R, C].

    Returns (resp, idx, counts): resp float32 [B, cap], idx int32 [B, cap] (raster index), in
    unspecified order, counts int32 [B]. Asynchronous on torch's current stream. append=True
    (fd_points_response_append, needs out=) keeps the counts in out and appends after them, so the
    call is the per-pixel kernel alone (no count reset).
    """
    import torch

    kind = KINDS[kind] if isinstance(kind, str) else int(kind)
    _, on_dev, b, r, c, keep = as_frames(frames)
    if not on_dev:
        raise TypeError("point_response takes device frames")
    ctx = resolve_ctx(ctx, frames)
    cap = r * c if kind == FD_FAST else r * c // 2 + 64
    if out is None:
        resp = torch.empty((b, cap), dtype=torch.float32, device=frames.device)
        idx = torch.empty((b, cap), dtype=torch.int32, device=frames.device)
        counts = torch.empty((b,), dtype=torch.int32, device=frames.device)
    else:
        resp, idx, counts = out
        cap = resp.shape[1]
    if append and out is None:
        raise ValueError("append=True needs out=(resp, idx, counts)")
    opts = fd_point_opts(15, float(min_valid_response))
    invoke(ctx, True, "fd_points_response_append" if append else "fd_points_response", kind, ptr(keep), b, r, c,
           ctypes.byref(opts), ptr(resp), ptr(idx), int(cap), ptr(counts))
    return resp, idx, counts


def point_candidates(kind, frames, min_feature_distance: int = 15, min_valid_response: float = 0.1, prior=None,
                     cap: int | None = None, response_map: bool = False, ctx: Context | None = None):
    """The ComputeCandidates seam (fd_points_candidates): raster-ordered candidates per frame.

    Host (numpy) frames only. Returns a list of (resp, x, y) arrays per frame, and the response map
    [batch, rows, cols] if requested.
    """
    kind = KINDS[kind] if isinstance(kind, str) else int(kind)
    _, on_dev, b, r, c, keep = as_frames(frames)
    if on_dev:
        raise TypeError("point_candidates takes host frames")
    ctx = resolve_ctx(ctx, frames)
    opts = fd_point_opts(int(min_feature_distance), float(min_valid_response))
    pxy, pcnt, _keep2 = _priors(prior, b)
    if cap is None:
        cap = r * c if kind == FD_FAST else r * c // 2 + 16
    resp = np.zeros((b, max(cap, 1)), np.float32)
    xs = np.zeros((b, max(cap, 1)), np.int32)
    ys = np.zeros((b, max(cap, 1)), np.int32)
    counts = np.zeros((b,), np.int64)
    rmap = np.zeros((b, r, c), np.float32) if response_map else None
    invoke(ctx, False, "fd_points_candidates", kind, ptr(keep), 0, b, r, c, ctypes.byref(opts), ptr(pxy), ptr(pcnt),
           ptr(resp), ptr(xs), ptr(ys), int(cap), ptr(counts), ptr(rmap), 0)
    out = [(resp[i, :counts[i]].copy(), xs[i, :counts[i]].copy(), ys[i, :counts[i]].copy()) for i in range(b)]
    return (out, rmap) if response_map else out
