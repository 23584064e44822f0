"""Nearest-neighbour matching over the C ABI: Hamming distance of BRIEF descriptors (fd_brief_match) and
squared L2 distance of NN float descriptors (fd_nn_match).

An MI355X extension (the reference has no matcher): the stage after detect_points -> brief_compute, on
the same [batch][stride] layouts, so a detect -> describe -> match chain stays on the GPU; nn_match is
the same stage after nn_descriptors / nn_select_list. The semantics (validity, ties, the three acceptance tests) are in include/fd_hip.h.

Both take an optional search window (q_xy, t_xy, radius): guided matching over fd_brief_match_guided /
fd_nn_match_guided, where a train keypoint is a candidate of a query only within radius pixels of it. With a
two-view model (model, model_kind, threshold) the pair must agree with it as well: the second, model-gated
matching pass over fd_brief_match_model / fd_nn_match_model.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np

from ._lib import fd_match_gate, fd_match_model_gate, fd_match_opts, fd_nn_match_opts
from .geometry import MODELS, GeometryResult
from ._slots import outputs, positions, ptr, slot_arg
from ._context import Context, invoke, is_device_tensor, resolve_ctx


@dataclass
class MatchResult:
    idx: object     # int32 [B, Sq]: accepted train index per query slot, else -1
    dist: object    # [B, Sq, 2]: raw best / second-best distance (-1: absent); int32 (brief_match) or float32 (nn_match)
    counts: object  # int32 [B]: accepted matches per frame


OPEN_RADIUS = 3.0e38  # a window that holds every finite position


def _guided(q_xy, t_xy, radius, model=None, model_kind="fundamental") -> bool:
    """Whether the call is the guided one: all three given; none given is the unguided call. With a model
    the positions are needed and radius is optional."""
    if model is not None:
        if q_xy is None or t_xy is None:
            raise ValueError("model-gated matching needs q_xy and t_xy")
        if model_kind not in MODELS:
            raise ValueError(f"model_kind must be one of {sorted(MODELS)}")
        return True
    given = [x is not None for x in (q_xy, t_xy, radius)]
    if any(given) and not all(given):
        raise ValueError("guided matching needs q_xy, t_xy and radius together")
    return all(given)


def _gate(q_xy, t_xy, radius, on_dev, b, sq, st, model=None, model_kind="fundamental", threshold=1.0):
    """The guided call's (gate, q_xy, t_xy), the model-gated call's (gate, q_xy, t_xy, model), or None for the
    unguided call."""
    if not _guided(q_xy, t_xy, radius, model, model_kind):
        return None
    if model is not None:
        if isinstance(model, GeometryResult):
            model = model.model
        if is_device_tensor(model) != on_dev:
            raise ValueError("model must be on the side (host / device) of the descriptors")
        if not on_dev:
            model = np.asarray(model)
        if str(model.dtype).split(".")[-1] != "float64":
            raise TypeError("model must be float64")
        if tuple(int(d) for d in model.shape) not in (((b, 9),) + (((9,),) if b == 1 else ())):
            raise ValueError(f"model must be [{b}, 9]" + (" or [9]" if b == 1 else ""))
        model = model.contiguous() if on_dev else np.ascontiguousarray(model)
        if radius is None:
            radius = OPEN_RADIUS
    try:
        rx, ry = (float(r) for r in radius)
    except TypeError:
        rx = ry = float(radius)
    sides = []
    for xy, s, name in ((q_xy, sq, "q"), (t_xy, st, "t")):
        if is_device_tensor(xy) != on_dev:
            raise ValueError(f"{name}_xy must be on the side (host / device) of the descriptors")
        msg = f"{name}_xy must be [{b}, {s}, 2]" + (f" or [{s}, 2]" if b == 1 else "")
        p = positions(xy, f"{name}_xy", on_dev, msg=msg)
        if tuple(int(d) for d in p.shape) != (b, s, 2):
            raise ValueError(msg)
        sides.append(p)
    if model is not None:
        return fd_match_model_gate(MODELS[model_kind], float(threshold), rx, ry), sides[0], sides[1], model
    return fd_match_gate(rx, ry), sides[0], sides[1]


def _side(x, valid, counts, on_dev, name, check):
    """One set as the library takes it: (x [B, S, n], valid uint8 [B, S] or None, counts int32 [B] or None, B, S).
    check(x, xp, name), xp = torch or numpy, is the matcher's rule: TypeError for x's dtype, ValueError for its axes."""
    if on_dev:
        import torch as xp
    else:
        xp, x = np, np.asarray(x)
    if x.ndim == 2:
        x = x[None]
    check(x, xp, name)
    b, s = int(x.shape[0]), int(x.shape[1])
    x = x.contiguous() if on_dev else np.ascontiguousarray(x)
    return x, slot_arg(valid, "uint8", (b, s), on_dev), slot_arg(counts, "int32", (b,), on_dev), b, s


def _run(ctx, entry, opts, q, t, gate, on_dev, dist, out, out_msg=None):
    """What both matchers end with: the outputs (dist: the distances' dtype name; out: the caller's tensors,
    checked against their shapes), then the entry point `entry`, or with a gate `entry`_guided, or with a
    gate that carries a model `entry`_model."""
    (qx, qv, qc, b, sq), (tx, tv, tc, _, st) = q, t
    specs = (((b, sq), "int32", -1), ((b, sq, 2), dist, -1), ((b,), "int32", 0))
    idx, dst, counts = outputs(specs, out, on_dev, qx.device if on_dev else None,
                               out_msg and out_msg.format(*(shape for shape, _, _ in specs)))
    head, outs = (b, ctypes.byref(opts)), (ptr(idx), ptr(dst), ptr(counts), 1 if on_dev else 0)
    qa, ta = (ptr(qx), ptr(qv), ptr(qc), sq), (ptr(tx), ptr(tv), ptr(tc), st)
    if gate is None:
        invoke(ctx, on_dev, entry, *head, *qa, *ta, *outs)
    elif len(gate) == 4:
        invoke(ctx, on_dev, entry + "_model", *head, ctypes.byref(gate[0]), ptr(gate[3]), *qa, ptr(gate[1]), *ta, ptr(gate[2]), *outs)
    else:
        invoke(ctx, on_dev, entry + "_guided", *head, ctypes.byref(gate[0]), *qa, ptr(gate[1]), *ta, ptr(gate[2]), *outs)
    return MatchResult(idx, dst, counts)


def brief_match(q_bits, t_bits, q_counts=None, t_counts=None, q_valid=None, t_valid=None, length: int = 256,
                max_distance: int = -1, max_ratio: float = 0.0, cross_check: bool = False, out=None,
                ctx: Context | None = None, q_xy=None, t_xy=None, radius=None, model=None,
                model_kind: str = "fundamental", threshold: float = 1.0) -> MatchResult:
    """fd_brief_match for a batch: frame b of the query set against frame b of the train set.

    q_bits / t_bits: int32 or uint32 words [B, S, ceil(length/32)] or [S, words] (batch 1), as
    brief_compute returns them; *_counts int32 [B] (None = S each; detect_points' device counts pass as
    they are); *_valid uint8 [B, S] (None = all valid). Host (numpy) inputs give numpy outputs; torch
    device inputs give torch outputs, asynchronous on torch's current stream. Slots >= q_counts[b] of
    idx and dist are -1. Device path only: out = preallocated contiguous int32 tensors (idx [B, Sq],
    dist [B, Sq, 2], counts [B]); slots >= q_counts[b] then keep their contents and the call is kernels
    only (graph-capturable once a first call of the shape has run).

    Guided matching (fd_brief_match_guided): q_xy / t_xy float32 positions [B, S, 2] (or [S, 2] for batch
    1) on the descriptors' side, as detect_points leaves them, and radius, a float or an (rx, ry) pair:
    train entry j is a candidate of query i only if |t_xy[j] - q_xy[i]| <= radius on both axes. Give all
    three or none.

    Model-gated matching (fd_brief_match_model): model, float64 [B, 9] (or [9] for batch 1) on the
    descriptors' side, or the GeometryResult of verify_geometry / refit_geometry; model_kind "fundamental" or
    "homography"; threshold in pixels. Train entry j is then a candidate of query i only if the pair passes
    the model's Sampson (F) or forward transfer (H) test, and the window if radius is given (None: open).
    q_xy and t_xy are required. A frame whose model is all zeros (no model) is gated by the window alone.
    """
    _guided(q_xy, t_xy, radius, model, model_kind)
    ctx = resolve_ctx(ctx, q_bits, t_bits)
    nw = (int(length) + 31) // 32 if 1 <= int(length) <= 256 else 0
    opts = fd_match_opts(int(length), int(max_distance), float(max_ratio), 1 if cross_check else 0)
    on_dev = is_device_tensor(q_bits)
    if on_dev != is_device_tensor(t_bits):
        raise ValueError("q_bits and t_bits must both be device tensors or both host arrays")
    if nw == 0:  # (the library reports the bad length: any word count is taken)
        nw = int(q_bits.shape[-1])

    def check(w, xp, name):
        if w.dtype not in (xp.int32, getattr(xp, "uint32", xp.int32)):
            raise TypeError(f"{name}_bits must be int32 or uint32 words")
        if w.ndim != 3 or w.shape[2] != nw:
            raise ValueError(f"{name}_bits must be [batch, S, {nw}] or [S, {nw}]")

    q = _side(q_bits, q_valid, q_counts, on_dev, "q", check)
    t = _side(t_bits, t_valid, t_counts, on_dev, "t", check)
    if t[3] != q[3]:
        raise ValueError("q_bits and t_bits must have the same batch")
    gate = _gate(q_xy, t_xy, radius, on_dev, q[3], q[4], t[4], model, model_kind, threshold)
    return _run(ctx, "fd_brief_match", opts, q, t, gate, on_dev, "int32", out,
                "out must be contiguous int32 tensors of shapes {}, {}, {}")


def nn_match(q_desc, t_desc, q_counts=None, t_counts=None, q_valid=None, t_valid=None, max_distance: float = -1.0,
             max_ratio: float = 0.0, cross_check: bool = False, out=None, ctx: Context | None = None, q_xy=None,
             t_xy=None, radius=None, model=None, model_kind: str = "fundamental", threshold: float = 1.0) -> MatchResult:
    """fd_nn_match for a batch: frame b of the query set against frame b of the train set, squared L2.

    q_desc / t_desc: float32 [B, S, dim] or [S, dim] (batch 1), as nn_descriptors / nn_select_list return
    them; dim is the last axis (a multiple of 4, 4..256). *_counts, *_valid, host / device inputs and
    out= are as in brief_match, except that dist (and out's dist tensor) is float32 [B, Sq, 2]: squared
    distances, -1.0 where absent. max_distance bounds the squared distance; max_ratio is Lowe's ratio of
    distances (applied squared to the squared distances). q_xy, t_xy and radius give the guided call
    (fd_nn_match_guided), and model, model_kind and threshold the model-gated call (fd_nn_match_model), as in
    brief_match.
    """
    _guided(q_xy, t_xy, radius, model, model_kind)
    ctx = resolve_ctx(ctx, q_desc, t_desc)
    on_dev = is_device_tensor(q_desc)
    if on_dev != is_device_tensor(t_desc):
        raise ValueError("q_desc and t_desc must both be device tensors or both host arrays")

    def check(d, xp, name):
        if d.dtype != xp.float32:
            raise TypeError(f"{name}_desc must be float32")
        if d.ndim != 3:
            raise ValueError(f"{name}_desc must be [batch, S, dim] or [S, dim]")

    q = _side(q_desc, q_valid, q_counts, on_dev, "q", check)
    t = _side(t_desc, t_valid, t_counts, on_dev, "t", check)
    if t[3] != q[3]:
        raise ValueError("q_desc and t_desc must have the same batch")
    dim = int(q[0].shape[2])
    if int(t[0].shape[2]) != dim:
        raise ValueError("q_desc and t_desc must have the same dim")
    opts = fd_nn_match_opts(dim, float(max_distance), float(max_ratio), 1 if cross_check else 0)
    gate = _gate(q_xy, t_xy, radius, on_dev, q[3], q[4], t[4], model, model_kind, threshold)
    return _run(ctx, "fd_nn_match", opts, q, t, gate, on_dev, "float32", out)
