"""Image warp by a homography or a camera model over the C ABI (fd_frames_warp).

An MI355X extension (the reference has no such stage): registration of a frame by verify_geometry's
homography at one end of the chain, lens undistortion / stereo rectification ahead of detect_points at the
other, so ingest -> undistort -> detect ... verify -> register stays on the GPU. The arithmetic (the source
position in double, fd_flow_lk's bilinear sum) is in include/fd_hip.h.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._lib import fd_warp_opts
from ._slots import outputs, ptr
from ._context import Context, as_frames, invoke, is_device_tensor, resolve_ctx

MODELS = {"homography": (_lib.FD_WARP_HOMOGRAPHY, 9), "camera": (_lib.FD_WARP_CAMERA, 22)}


def camera_params(new_K, K, dist, R=None):
    """The 22 doubles of model="camera" from an OpenCV-style calibration: new_K the 3 x 3 intrinsics of the
    destination (ideal pinhole) image, K and dist = (k1, k2, p1, p2[, k3]) the source camera's, R the 3 x 3
    rotation taking a destination ray to a source-camera ray (None: the identity, plain undistortion; for a
    stereo pair pass the transpose of stereoRectify's R1 / R2)."""
    new_K, K = np.asarray(new_K, np.float64), np.asarray(K, np.float64)
    R = np.eye(3) if R is None else np.asarray(R, np.float64)
    dist = np.asarray(dist, np.float64).reshape(-1)
    if new_K.shape != (3, 3) or K.shape != (3, 3) or R.shape != (3, 3):
        raise ValueError("new_K, K and R must be 3 x 3")
    if dist.size not in (4, 5):
        raise ValueError("dist must be (k1, k2, p1, p2) or (k1, k2, p1, p2, k3)")
    p = np.zeros(22)
    p[0:4] = new_K[0, 0], new_K[1, 1], new_K[0, 2], new_K[1, 2]
    p[4:13] = R.reshape(9)
    p[13:17] = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    p[17:17 + dist.size] = dist
    return p


def warp_frames(frames, params, out_shape=None, model: str = "homography", fill: int = 0, return_mask: bool = False,
                ctx: Context | None = None, out=None):
    """fd_frames_warp: every destination pixel sampled bilinearly from its frame at the position the model gives.

    frames: a uint8 batch [B, rows, cols] (or [rows, cols]), numpy or a torch device tensor. params: float64
    [B, P] or [P] (one set for every frame), P = 9 for "homography" (row-major 3 x 3, destination -> source:
    a GeometryResult's model of verify_geometry(previous, next) warps the next frame onto the previous one as
    it is, and its device tensor is used without a copy) or 22 for "camera" (camera_params). out_shape =
    (out_rows, out_cols), None: the frames' shape. fill 0..255: the value of pixels with no source.

    Returns out uint8 [B, out_rows, out_cols], or (out, mask) with return_mask (mask 1 where the pixel has a
    source). The outputs are on the side of the frames: torch tensors for device frames (asynchronous on
    torch's current stream; kernels only and graph-capturable when params is a device tensor too), numpy
    otherwise. Device path only: out = a preallocated contiguous uint8 tensor, or (out, mask) with return_mask.
    """
    if model not in MODELS:
        raise ValueError(f"model must be one of {sorted(MODELS)}")
    kind, per = MODELS[model]
    _, f_dev, b, rows, cols, keep = as_frames(frames)
    p_dev = is_device_tensor(params)
    ctx = resolve_ctx(ctx, keep, params)
    if p_dev:
        import torch

        if params.dtype != torch.float64:
            raise TypeError("params must be float64")
        p = params.contiguous()
    else:
        p = np.ascontiguousarray(params, dtype=np.float64)
    shape = tuple(p.shape)
    if shape not in ((per,), (b, per)):
        raise ValueError(f"params must be [{per}] or [{b}, {per}] for model {model!r}")
    out_rows, out_cols = (rows, cols) if out_shape is None else (int(out_shape[0]), int(out_shape[1]))
    if out_rows < 0 or out_cols < 0:
        raise ValueError("out_shape must not be negative")
    on_dev = bool(f_dev)
    spec = ((b, out_rows, out_cols), "uint8", 0)
    if out is not None and not return_mask:
        out = (out,)
    o = outputs((spec, spec) if return_mask else (spec,), out, on_dev, keep.device if on_dev else None)
    if not 0 <= int(fill) <= 255:
        raise ValueError("fill must be in [0, 255]")
    if out_rows == 0 or out_cols == 0:  # nothing to write (an empty array has no pointer to pass)
        return (o[0], o[1]) if return_mask else o[0]
    opts = fd_warp_opts(kind, 1 if len(shape) == 1 else 0, int(fill))
    invoke(ctx, on_dev or p_dev, "fd_frames_warp", ptr(keep), f_dev, b, rows, cols, ctypes.byref(opts), ptr(p), 1 if p_dev else 0,
           out_rows, out_cols, ptr(o[0]), ptr(o[1]) if return_mask else None, 1 if on_dev else 0)
    return (o[0], o[1]) if return_mask else o[0]
