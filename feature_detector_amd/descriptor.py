"""Steered BRIEF descriptors over the C ABI (fd_brief_compute), SURVEY §8 row f1.

Mirrors feature_detector::BriefDescriptor (descriptor_brief.h:14-37) for batches: Options kLength /
kHalfPatchSize, plus the float-coordinate sampler the reference takes from its un-vendored
GrayImage (bilinear by default, truncation selectable; DESIGN.md: parity unpinned for the sampled
bits, exact for everything before them). Keypoints are (x, y) = (col, row), the layout
detect_points returns, so a device-side detect -> describe chain stays on the GPU.
"""
from __future__ import annotations

import ctypes

import numpy as np

from ._lib import FD_SAMPLE_BILINEAR, FD_SAMPLE_TRUNCATE, fd_brief_opts
from ._slots import outputs, positions, ptr, slot_arg
from ._context import Context, as_frames, invoke, is_device_tensor, resolve_ctx

SAMPLERS = {"bilinear": FD_SAMPLE_BILINEAR, "truncate": FD_SAMPLE_TRUNCATE}


def brief_compute(frames, uv, counts=None, length: int = 256, half_patch_size: int = 8, sampler="bilinear",
                  with_valid: bool = False, out=None, ctx: Context | None = None):
    """Descriptor<BriefType>::Compute (descriptor.h:27-40) for a batch.

    frames: u8 [B, R, C] or [R, C]; uv: float32 [B, S, 2] or [S, 2] keypoints (x, y); counts: int32 [B]
    keypoints per frame (None = S each). Host (numpy) frames/uv give numpy outputs; torch device uv
    (with device frames) gives torch outputs, asynchronous on torch's current stream.
    Returns bits uint32 [B, S, ceil(length/32)] (bit i of a descriptor = bit i%32 of word i/32;
    slots >= counts[b] are left zero), and valid uint8 [B, S] if with_valid. Device path only: out=
    a preallocated int32 [B, S, words] tensor (slots >= counts[b] then keep their contents), so the
    call is the kernel alone (graph-capturable without an allocation or fill).
    """
    smp = SAMPLERS[sampler] if isinstance(sampler, str) else int(sampler)
    _, f_on_dev, b, r, c, keep_f = as_frames(frames)
    ctx = resolve_ctx(ctx, frames, uv)
    nw = (int(length) + 31) // 32
    opts = fd_brief_opts(int(length), int(half_patch_size), smp)
    on_dev = is_device_tensor(uv)
    msg = "uv must be [batch, S, 2] matching frames"
    puv = positions(uv, "uv", on_dev, convert=True, msg=msg)
    if puv.shape[0] != b:
        raise ValueError(msg)
    s = int(puv.shape[1])
    cn = slot_arg(counts, "int32", (b,), on_dev)
    dev = puv.device if on_dev else None
    # (device words are int32: torch has no uint32 arithmetic; host calls take no out= and ignore one)
    bits, = outputs([((b, s, nw), "int32" if on_dev else "uint32", 0)], (out,) if on_dev and out is not None else None,
                    on_dev, dev, f"out must be a contiguous int32 tensor of shape {(b, s, nw)}")
    valid = outputs([((b, s), "uint8", 0)], None, on_dev, dev)[0] if with_valid else None
    invoke(ctx, on_dev or bool(f_on_dev), "fd_brief_compute", ptr(keep_f), f_on_dev, b, r, c, ctypes.byref(opts), ptr(puv), ptr(cn),
           s, ptr(bits), ptr(valid), 1 if on_dev else 0)
    return (bits, valid) if with_valid else bits


def unpack_bits(bits, length: int) -> np.ndarray:
    """[..., words] uint32 -> [..., length] bool (BriefType = std::vector<bool>, descriptor_brief.h:10)."""
    w = np.asarray(bits).astype(np.uint32)
    idx = np.arange(length)
    return ((w[..., idx >> 5] >> (idx & 31).astype(np.uint32)) & 1).astype(bool)


def to_float(bits, length: int) -> np.ndarray:
    """Descriptor::Compute's std::vector<Vec> overload: bit -> +1.0f / -1.0f (descriptor.h:50-53)."""
    return np.where(unpack_bits(bits, length), np.float32(1.0), np.float32(-1.0)).astype(np.float32)
