"""Image pyramids and pyramidal Lucas-Kanade feature tracking over the C ABI (fd_pyr_build, fd_pyr_build_gauss,
fd_flow_lk).

An MI355X extension (the reference has no tracker): the step before detect_points in a VIO / SLAM front
end, on the [batch][stride] layouts detect_points writes, so detect -> track -> (mask survivors) -> detect
stays on the GPU. The arithmetic (exact integer window sums, one 2 x 2 solve in double) is in
include/fd_hip.h.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import fd_flow_opts
from ._slots import f32, outputs, positions, ptr, slot_arg
from ._context import Context, as_frames, invoke, is_device_tensor, resolve_ctx


def pyramid_layout(batch: int, rows: int, cols: int, levels: int) -> list[int]:
    """fd_pyr_layout: byte offsets of the levels in the packed pyramid; the last entry is the total size."""
    off = (ctypes.c_int64 * (max(int(levels), 0) + 1))()
    rc = _lib.load().fd_pyr_layout(int(batch), int(rows), int(cols), int(levels), off)
    if rc != _lib.FD_OK:
        raise _lib.FdError(rc, "fd_pyr_layout: need batch, rows, cols >= 1, levels in [1, 6] and a top level that keeps a pixel")
    return list(off)


@dataclass
class Pyramid:
    data: object   # packed uint8 buffer (fd_pyr_layout): a torch device tensor, or a numpy array (host frames)
    batch: int
    rows: int
    cols: int
    levels: int
    offsets: list  # byte offset per level, then the total size

    def level(self, l: int):
        """Level l as a [batch, rows >> l, cols >> l] view of the packed buffer."""
        r, c = self.rows >> l, self.cols >> l
        return self.data[self.offsets[l]:self.offsets[l] + self.batch * r * c].reshape(self.batch, r, c)


def build_pyramid(frames, levels: int = 3, ctx: Context | None = None, device_out: bool | None = None,
                  kernel: str = "box") -> Pyramid:
    """fd_pyr_build for a batch of uint8 frames [B, rows, cols] (or [rows, cols]): level 0 is the frames,
    every further level the rounded 2 x 2 box mean of the one below it. kernel="gauss" (fd_pyr_build_gauss):
    every further level is the one below it smoothed by the 5 x 5 binomial kernel [1 4 6 4 1] (blur_frames with
    taps [96, 64, 16]) and decimated by 2, pyrDown's arithmetic, in the same layout: track_lk takes either kind.

    Torch device frames give a device pyramid, asynchronous on torch's current stream (kernels and one
    copy: graph-capturable). Host (numpy) frames give a numpy pyramid, or with device_out=True a device
    pyramid (what track_lk builds from host frames).
    """
    if kernel not in ("box", "gauss"):
        raise ValueError('kernel must be "box" or "gauss"')
    _, on_dev, b, r, c, keep = as_frames(frames)
    ctx = resolve_ctx(ctx, frames)
    off = pyramid_layout(b, r, c, levels)
    dev_out = bool(on_dev) if device_out is None else bool(device_out)
    if on_dev and not dev_out:
        raise ValueError("device frames give a device pyramid")
    if dev_out:
        import torch

        data = torch.empty((off[-1],), dtype=torch.uint8, device=keep.device if on_dev else f"cuda:{ctx.device}")
    else:
        data = np.zeros((off[-1],), np.uint8)
    invoke(ctx, bool(on_dev), "fd_pyr_build_gauss" if kernel == "gauss" else "fd_pyr_build", ptr(keep), on_dev, b, r, c, int(levels),
           ptr(data), 1 if dev_out else 0)
    return Pyramid(data, b, r, c, int(levels), off)


@dataclass
class FlowResult:
    xy: object      # float32 [B, S, 2]: tracked positions (x, y) in the next frame
    status: object  # uint8 [B, S]: 1 = tracked, everything else lost (fd_flow_status)
    err: object     # float32 [B, S]: mean absolute residual of the window, in intensity units
    counts: object  # int32 [B]: tracked slots per frame


def _device_pyramid(p, levels, ctx, name):
    """A device Pyramid from a Pyramid (host ones are uploaded) or a frame batch."""
    if isinstance(p, Pyramid):
        if p.levels != int(levels):
            raise ValueError(f"{name}: the pyramid has {p.levels} levels, the call asks for {levels}")
        if is_device_tensor(p.data):
            return p
        import torch

        return Pyramid(torch.from_numpy(p.data).to(f"cuda:{ctx.device}"), p.batch, p.rows, p.cols, p.levels, p.offsets)
    return build_pyramid(p, levels, ctx=ctx, device_out=True)


def track_lk(prev, next, xy, counts=None, valid=None, guess=None, levels: int = 3, half_window: int = 7,
             max_iters: int = 30, epsilon: float = 0.01, min_eigen: float = 1e-3, fb_max_dist: float = -1,
             max_error: float = -1, out=None, ctx: Context | None = None) -> FlowResult:
    """fd_flow_lk: track the features xy of every frame of `prev` into the frame of `next` with the same index.

    prev / next: uint8 frame batches [B, rows, cols] (or [rows, cols]) or Pyramids (build_pyramid with the
    same `levels`), so a tracking loop builds each frame's pyramid once. xy: float32 [B, S, 2] (or [S, 2]
    for batch 1), (x, y) as detect_points writes them; counts int32 [B] (None = S each; detect_points'
    device counts pass as they are); valid uint8 [B, S] (None = all valid); guess as xy: the expected
    positions in `next` (None = xy).

    Host (numpy) xy gives numpy outputs; torch device xy gives torch outputs, asynchronous on torch's
    current stream. Slots the call does not write (>= counts[b]) are 0. Device path only: out =
    preallocated contiguous tensors (xy float32 [B, S, 2], status uint8 [B, S], err float32 [B, S], counts
    int32 [B]); unwritten slots then keep their contents, and with Pyramid inputs the call is kernels only
    (graph-capturable once a first call of the shape has run).

    The defaults (3 levels, a 15 x 15 window, 30 iterations, epsilon 0.01, min_eigen 1e-3) are the usual
    conventions of pyramidal LK front ends, not values tuned for this library. fb_max_dist >= 0 turns the
    forward-backward check on (a second pass), max_error >= 0 the residual test.
    """
    on_dev = is_device_tensor(xy)
    ctx = resolve_ctx(ctx, xy, prev.data if isinstance(prev, Pyramid) else prev,
                       next.data if isinstance(next, Pyramid) else next)
    pxy = positions(xy, "xy", on_dev)
    b, s = int(pxy.shape[0]), int(pxy.shape[1])
    pp, pn = _device_pyramid(prev, levels, ctx, "prev"), _device_pyramid(next, levels, ctx, "next")
    if (pp.batch, pp.rows, pp.cols) != (pn.batch, pn.rows, pn.cols):
        raise ValueError("prev and next must have the same batch, rows and cols")
    if pp.batch != b:
        raise ValueError("xy and the frames must have the same batch")
    if guess is not None and is_device_tensor(guess) != on_dev:
        raise ValueError("guess must be on the side (host / device) of xy")
    v, cn = slot_arg(valid, "uint8", (b, s), on_dev), slot_arg(counts, "int32", (b,), on_dev)
    g = None if guess is None else f32(guess, "guess", on_dev).reshape(b, s, 2)
    oxy, ost, oerr, ocnt = outputs((((b, s, 2), "float32", 0), ((b, s), "uint8", 0), ((b, s), "float32", 0),
                                    ((b,), "int32", 0)), out, on_dev, pxy.device if on_dev else None)
    opts = fd_flow_opts(int(half_window), int(max_iters), float(epsilon), float(min_eigen), float(fb_max_dist),
                        float(max_error))
    invoke(ctx, on_dev, "fd_flow_lk", b, pp.rows, pp.cols, int(levels), ctypes.byref(opts), ptr(pp.data), ptr(pn.data),
           ptr(pxy), ptr(v), ptr(cn), s, ptr(g), ptr(oxy), ptr(ost), ptr(oerr), ptr(ocnt), 1 if on_dev else 0)
    return FlowResult(oxy, ost, oerr, ocnt)
