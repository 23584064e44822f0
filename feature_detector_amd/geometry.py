"""RANSAC verification of matches and tracks over the C ABI (fd_ransac), the refit of its model
(fd_ransac_refit), the relative pose of a fundamental matrix (fd_pose_recover) and triangulation (fd_triangulate),
the absolute pose from 3-D points (fd_pnp_ransac, fd_pnp_refit), bundle adjustment (fd_bundle_adjust) and the alignment
of two 3-D point sets (fd_align_ransac, fd_align_refit, fd_align_apply).

An MI355X extension (the reference has no such stage): the step after brief_match / nn_match or track_lk
in a VIO / SLAM front end, on their [batch][stride] layouts, so detect -> describe -> match -> verify and
detect -> track -> verify stay on the GPU. The arithmetic (a counter-based sampler, one solve in double per
hypothesis, every hypothesis evaluated) is in include/fd_hip.h.
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import fd_align_opts, fd_ba_opts, fd_pnp_opts, fd_pose_opts, fd_ransac_opts, fd_refit_opts
from ._slots import f32, outputs, positions, ptr, slot_arg
from ._context import Context, invoke, is_device_tensor, resolve_ctx

MODELS = {"fundamental": _lib.FD_RANSAC_FUNDAMENTAL, "homography": _lib.FD_RANSAC_HOMOGRAPHY}


@dataclass
class GeometryResult:
    model: object    # float64 [B, 9]: row-major 3 x 3 in pixel coordinates, largest entry 1.0; zeros: no model
    inliers: object  # uint8 [B, S]: 1 = a correspondence the model classifies as an inlier
    counts: object   # int32 [B]: inliers per frame
    best: object     # int32 [B]: the winning hypothesis, -1: no model


def conditioning(image_size=None):
    """The fixed conditioning transform of verify_geometry: ((center_x, center_y), scale)."""
    if image_size is None:
        return (0.0, 0.0), 1.0 / 256
    rows, cols = image_size
    return ((cols - 1) / 2, (rows - 1) / 2), 2.0 / (rows + cols)


def _slots(on_dev, b, s, ts, first, matches, valid, counts):
    """The slot arguments every wrapper shares, checked (`first`: the array slot i pairs with): matches, valid, counts."""
    if matches is None and ts < s:
        raise ValueError(f"without matches slot i pairs with slot i: t_xy needs at least as many slots as {first}")
    return (slot_arg(matches, "int32", (b, s), on_dev), slot_arg(valid, "uint8", (b, s), on_dev),
            slot_arg(counts, "int32", (b,), on_dev))


def _call(fn, ctx, on_dev, like, head, opts, inputs, specs, out):
    """The tail every wrapper shares: the outputs of `specs` (fresh ones on the side and device of `like`, or out=), the
    context's stream, the C function `fn` on (ctx, *head, opts, *inputs, *outputs, io_on_device) and its status. head: the
    batch (and cameras); inputs: arrays (None: a null pointer) and the strides between them. Returns the outputs."""
    outs = outputs(specs, out, on_dev, like.device if on_dev else None)
    args = [x if isinstance(x, int) else ptr(x) for x in (*inputs, *outs)]
    invoke(ctx, on_dev, fn, *head, ctypes.byref(opts), *args, 1 if on_dev else 0)
    return outs


def _model_specs(b, s, w):
    """The outputs of a RANSAC or refit call: model [B, W], inliers [B, S], counts [B], best or rounds [B]."""
    return ((b, w), "float64", 0), ((b, s), "uint8", 0), ((b,), "int32", 0), ((b,), "int32", 0)


def _unwrap(points, valid):
    """A PointsResult / PoseResult taken apart: its points, and its valid bytes unless `valid` is given."""
    if isinstance(points, PointsResult):
        return points.points, (points.valid if valid is None else valid)
    return points, valid


def _xyz(x, name, b=None, whose=None):
    """The [B, S, 3] shape of a point array ([S, 3]: batch 1), checked against the batch b (`whose`, for the message)."""
    shape = tuple(x.shape)
    if len(shape) == 2:
        shape = (1,) + shape
    if len(shape) != 3 or shape[2] != 3 or (b is not None and shape[0] != b):
        raise ValueError(f"{name} must be float32 [B, S, 3] (or [S, 3] for batch 1)" + ("" if b is None else f" with {whose} batch"))
    return shape


def _pairs(q_xy, t_xy, others, side_error, matches, valid, counts, ctx):
    """What the wrappers on image pairs share: the side of the call (q_xy's; t_xy and `others` must be on it), the
    context, the checked positions and their sizes, and the slot arguments."""
    on_dev = is_device_tensor(q_xy)
    if any(is_device_tensor(x) != on_dev for x in (t_xy, *others)):
        raise ValueError(side_error)
    ctx = resolve_ctx(ctx, q_xy, t_xy)
    pq, pt = positions(q_xy, "q_xy", on_dev), positions(t_xy, "t_xy", on_dev)
    b, s, ts = int(pq.shape[0]), int(pq.shape[1]), int(pt.shape[1])
    if int(pt.shape[0]) != b:
        raise ValueError("q_xy and t_xy must have the same batch")
    return (ctx, on_dev, pq, pt, b, s, ts, *_slots(on_dev, b, s, ts, "q_xy", matches, valid, counts))


def verify_geometry(q_xy, t_xy, matches=None, valid=None, counts=None, model: str = "fundamental", hypotheses: int = 256,
                    seed: int = 0, threshold: float = 1.0, image_size=None, out=None,
                    ctx: Context | None = None) -> GeometryResult:
    """fd_ransac: the fundamental matrix ("fundamental", 8-point samples) or homography ("homography",
    4-point samples) with the most inliers among `hypotheses` minimal samples, and the inlier mask.

    q_xy: float32 [B, S, 2] (or [S, 2] for batch 1), t_xy: float32 [B, T, 2], (x, y) as detect_points and
    track_lk write them. matches int32 [B, S]: the train index of every query slot as brief_match /
    nn_match return it (-1: none); None pairs slot i with slot i (tracks: T >= S). valid uint8 [B, S]: a slot
    takes part only where it is 1, so track_lk's status passes as it is (None: all). counts int32 [B]
    (None: S each). threshold is in pixels: the Sampson distance (F) or the forward transfer error (H).

    image_size = (rows, cols) conditions the coordinates with center = ((cols - 1) / 2, (rows - 1) / 2) and
    scale = 2 / (rows + cols); without it the center is (0, 0) and the scale 1 / 256.

    Host (numpy) q_xy gives numpy outputs; torch device q_xy gives torch outputs, asynchronous on torch's
    current stream. Inlier slots the call does not write (>= counts[b]) are 0. Device path only: out =
    preallocated contiguous tensors (model float64 [B, 9], inliers uint8 [B, S], counts int32 [B], best
    int32 [B]); unwritten slots then keep their contents, and the call is kernels only (graph-capturable
    once a first call of the shape has run). The inlier mask can be passed as the next track_lk's valid.
    """
    if model not in MODELS:
        raise ValueError(f"model must be one of {sorted(MODELS)}")
    ctx, on_dev, pq, pt, b, s, ts, mi, v, cn = _pairs(
        q_xy, t_xy, (), "t_xy must be on the side (host / device) of q_xy", matches, valid, counts, ctx)
    (cx, cy), scale = conditioning(image_size)
    opts = fd_ransac_opts(MODELS[model], int(hypotheses), int(seed) & 0xFFFFFFFF, float(threshold), float(cx), float(cy),
                          float(scale))
    return GeometryResult(*_call("fd_ransac", ctx, on_dev, pq, (b,), opts, (pq, cn, s, pt, ts, mi, v), _model_specs(b, s, 9), out))


@dataclass
class RefitResult(GeometryResult):
    rounds: object = None  # int32 [B]: accepted refit rounds; 0: model and inliers are the given ones


def refit_geometry(q_xy, t_xy, result: GeometryResult, matches=None, valid=None, counts=None, model: str = "fundamental",
                   rounds: int = 2, threshold: float = 1.0, image_size=None, out=None,
                   ctx: Context | None = None) -> RefitResult:
    """fd_ransac_refit: the least-squares refit of verify_geometry's model on its inliers, the inliers
    classified again, up to `rounds` (1..4) times while their number does not fall; a fundamental matrix comes
    back with rank 2. This is the model to hand to warp_frames.

    q_xy, t_xy, matches, valid, counts, model, threshold and image_size are verify_geometry's: pass the same
    ones. result: what verify_geometry returned (its model float64 [B, 9] and inliers uint8 [B, S], on the
    side of q_xy). A frame whose first refit is rejected (too few inliers, a degenerate inlier set, fewer
    inliers than before) keeps its model bit for bit and has rounds 0.

    Returns a RefitResult: model, inliers, counts as verify_geometry's, best as given, and rounds int32 [B].
    Host and device inputs and out= (model float64 [B, 9], inliers uint8 [B, S], counts int32 [B], rounds
    int32 [B]) behave as in verify_geometry; out= may hold result's own model and inliers tensors.
    """
    if model not in MODELS:
        raise ValueError(f"model must be one of {sorted(MODELS)}")
    ctx, on_dev, pq, pt, b, s, ts, mi, v, cn = _pairs(
        q_xy, t_xy, (result.model, result.inliers), "t_xy and result must be on the side (host / device) of q_xy",
        matches, valid, counts, ctx)
    im, ii = slot_arg(result.model, "float64", (b, 9), on_dev), slot_arg(result.inliers, "uint8", (b, s), on_dev)
    (cx, cy), scale = conditioning(image_size)
    opts = fd_refit_opts(MODELS[model], int(rounds), float(threshold), float(cx), float(cy), float(scale))
    om, oi, oc, orr = _call("fd_ransac_refit", ctx, on_dev, pq, (b,), opts, (pq, cn, s, pt, ts, mi, v, im, ii),
                            _model_specs(b, s, 9), out)
    return RefitResult(om, oi, oc, result.best, orr)


@dataclass
class PointsResult:
    points: object  # float32 [B, S, 3]: the 3-D point of every valid slot in the query camera's frame; zeros elsewhere
    valid: object   # uint8 [B, S]: 1 = a participating correspondence whose point is in front of both cameras
    counts: object  # int32 [B]: valid points per frame


@dataclass
class PoseResult(PointsResult):
    pose: object = None    # float64 [B, 12]: R row-major, then t of unit length, X_t = R X_q + t; zeros: no pose
    choice: object = None  # int32 [B]: the winning candidate 0..3, -1: no pose

    def rotation(self, b=0):
        """Frame b's R as a [3, 3] view."""
        return self.pose[b, :9].reshape(3, 3)

    def translation(self, b=0):
        return self.pose[b, 9:]


def intrinsics(K, name="K"):
    """(fx, fy, cx, cy) as floats from a 3 x 3 camera matrix or those four values. A non-zero skew, a last row
    other than (0, 0, 1), a non-finite value and a zero focal length are a ValueError."""
    k = np.asarray(K.cpu() if hasattr(K, "cpu") else K, np.float64)
    if k.shape == (3, 3):
        if k[0, 1] != 0.0 or k[1, 0] != 0.0 or k[2, 0] != 0.0 or k[2, 1] != 0.0 or k[2, 2] != 1.0:
            raise ValueError(f"{name} must be a zero-skew pinhole matrix [[fx, 0, cx], [0, fy, cy], [0, 0, 1]]")
        k = np.array([k[0, 0], k[1, 1], k[0, 2], k[1, 2]])
    if k.shape != (4,):
        raise ValueError(f"{name} must be a 3 x 3 matrix or (fx, fy, cx, cy)")
    if not np.all(np.isfinite(k)) or k[0] == 0.0 or k[1] == 0.0:
        raise ValueError(f"{name} must be finite with non-zero fx and fy")
    return tuple(float(v) for v in k)


def _pose_call(q_xy, t_xy, given, given_name, given_width, K, K_t, matches, valid, counts, inliers, max_depth, min_parallax, ctx):
    """What recover_pose and triangulate share: the checked arguments of the two entry points."""
    ctx, on_dev, pq, pt, b, s, ts, mi, v, cn = _pairs(
        q_xy, t_xy, (given,) if inliers is None else (given, inliers),
        f"t_xy, {given_name} and the inliers must be on the side (host / device) of q_xy", matches, valid, counts, ctx)
    if not (max_depth > 0) or not 0.0 <= min_parallax <= 1.0 or math.isnan(min_parallax):
        raise ValueError("max_depth must be > 0 and min_parallax in [0, 1]")
    cam_q = intrinsics(K)
    cam_t = cam_q if K_t is None else intrinsics(K_t, "K_t")
    opts = fd_pose_opts(*cam_q, *cam_t, float(max_depth), float(min_parallax))
    gm, ii = slot_arg(given, "float64", (b, given_width), on_dev), slot_arg(inliers, "uint8", (b, s), on_dev)
    return ctx, on_dev, pq, pt, b, s, ts, opts, mi, v, cn, gm, ii


POINT_SPECS = lambda b, s: (((b, s, 3), "float32", 0), ((b, s), "uint8", 0), ((b,), "int32", 0))  # noqa: E731


def triangulate(q_xy, t_xy, pose, K, K_t=None, matches=None, valid=None, counts=None, inliers=None,
                max_depth: float = math.inf, min_parallax: float = 1e-3, out=None, ctx: Context | None = None) -> PointsResult:
    """fd_triangulate: the 3-D point of every correspondence under a known relative pose (a calibrated stereo
    rig behind track_lk, or a pose from elsewhere), in the query camera's frame.

    q_xy, t_xy, matches, valid and counts are verify_geometry's. pose: float64 [B, 12] (or [12] for batch 1), R
    row-major then t, X_t = R X_q + t; the points come out in the unit of t. K, K_t: the query and train
    cameras as 3 x 3 zero-skew pinhole matrices or (fx, fy, cx, cy) (K_t None: the same camera). inliers uint8
    [B, S] (None: every correspondence): only the slots equal to 1 take part. A point is valid when both
    depths are positive and at most max_depth, and the sine of the angle between the rays exceeds min_parallax.

    Returns a PointsResult. Host and device inputs and out= (points float32 [B, S, 3], valid uint8 [B, S],
    counts int32 [B]) behave as in verify_geometry.
    """
    ctx, on_dev, pq, pt, b, s, ts, opts, mi, v, cn, gm, ii = _pose_call(
        q_xy, t_xy, pose, "pose", 12, K, K_t, matches, valid, counts, inliers, max_depth, min_parallax, ctx)
    return PointsResult(*_call("fd_triangulate", ctx, on_dev, pq, (b,), opts, (pq, cn, s, pt, ts, mi, v, gm, ii), POINT_SPECS(b, s), out))


def recover_pose(q_xy, t_xy, result: GeometryResult, K, K_t=None, matches=None, valid=None, counts=None,
                 max_depth: float = math.inf, min_parallax: float = 1e-3, out=None, ctx: Context | None = None) -> PoseResult:
    """fd_pose_recover: the relative camera pose of a fundamental matrix and the 3-D points of its inliers, the
    step after verify_geometry / refit_geometry (model="fundamental") in a VIO / SLAM front end.

    q_xy, t_xy, matches, valid and counts are verify_geometry's: pass the same ones. result: what
    verify_geometry or refit_geometry returned (its model float64 [B, 9] and inliers uint8 [B, S], on the side
    of q_xy). K, K_t, max_depth and min_parallax: as in triangulate. Of the four poses an essential matrix
    allows, the one with the most inliers in front of both cameras wins (the lowest index among equals).

    Returns a PoseResult: pose float64 [B, 12] (R row-major, then t of unit length; X_t = R X_q + t), choice
    int32 [B] (-1 and a zero pose: no pose, e.g. a zero or rank-1 model, a pure rotation, no inlier in front),
    and the winner's points, valid and counts. Host and device inputs and out= (pose float64 [B, 12], choice
    int32 [B], points float32 [B, S, 3], valid uint8 [B, S], counts int32 [B]) behave as in verify_geometry.
    """
    ctx, on_dev, pq, pt, b, s, ts, opts, mi, v, cn, gm, ii = _pose_call(
        q_xy, t_xy, result.model, "result", 9, K, K_t, matches, valid, counts, result.inliers, max_depth, min_parallax, ctx)
    oo, och, op, ov, oc = _call("fd_pose_recover", ctx, on_dev, pq, (b,), opts, (pq, cn, s, pt, ts, mi, v, gm, ii),
                                (((b, 12), "float64", 0), ((b,), "int32", 0)) + POINT_SPECS(b, s), out)
    return PoseResult(op, ov, oc, oo, och)


@dataclass
class PnpResult:
    pose: object     # float64 [B, 12]: R row-major, then t, X_t = R X + t in the units of the points; zeros: no pose
    inliers: object  # uint8 [B, S]: 1 = a correspondence within `threshold` pixels of its reprojection
    counts: object   # int32 [B]: inliers per frame
    best: object     # int32 [B]: the winning hypothesis, -1: no pose

    def rotation(self, b=0):
        """Frame b's R as a [3, 3] view."""
        return self.pose[b, :9].reshape(3, 3)

    def translation(self, b=0):
        return self.pose[b, 9:]


@dataclass
class PnpRefineResult(PnpResult):
    rounds: object = None  # int32 [B]: accepted Gauss-Newton rounds; 0: pose and inliers are the given ones


def _pnp_call(points, t_xy, K, matches, valid, point_valid, counts, extra, ctx):
    """What solve_pnp and refine_pnp share: the checked arguments of the two entry points. `extra`: further
    arrays that must be on the side of t_xy."""
    points, point_valid = _unwrap(points, point_valid)
    on_dev = is_device_tensor(t_xy)
    sides = [is_device_tensor(points)] + [is_device_tensor(x) for x in extra]
    if point_valid is not None:
        sides.append(is_device_tensor(point_valid))
    if any(side != on_dev for side in sides):
        raise ValueError("points, point_valid and the given result must be on the side (host / device) of t_xy")
    ctx = resolve_ctx(ctx, t_xy, points)
    pt = positions(t_xy, "t_xy", on_dev)
    b, ts = int(pt.shape[0]), int(pt.shape[1])
    s = int(_xyz(points, "points", b, "t_xy's")[1])
    pp = slot_arg(points, "float32", (b, s, 3), on_dev)
    mi, v, cn = _slots(on_dev, b, s, ts, "points", matches, valid, counts)
    pv = slot_arg(point_valid, "uint8", (b, s), on_dev)
    return ctx, on_dev, pp, pv, pt, b, s, ts, intrinsics(K), mi, v, cn


def solve_pnp(points, t_xy, K, matches=None, valid=None, point_valid=None, counts=None, hypotheses: int = 256, seed: int = 0,
              threshold: float = 2.0, center=None, scale: float = 1.0, out=None, ctx: Context | None = None) -> PnpResult:
    """fd_pnp_ransac: the camera pose of an image against known 3-D points, the step that places the next frame
    against the points recover_pose / triangulate left (at their scale): the 6-point DLT camera matrix with the
    most inliers among `hypotheses` samples, made a rotation and a translation.

    points: float32 [B, S, 3] (or [S, 3] for batch 1), or a PointsResult / PoseResult as it is (its valid bytes
    then are point_valid). t_xy: float32 [B, T, 2], the image positions. K: the image's camera as in
    triangulate. matches, valid, counts: verify_geometry's (track_lk's status passes as valid). threshold is
    the reprojection error in pixels. center (three values, default 0) and scale condition the 3-D points,
    Xc = (X - center) * scale: the scene's centroid and the inverse of its spread are a good choice. A planar
    scene has no DLT pose.

    Returns a PnpResult. Host and device inputs and out= (pose float64 [B, 12], inliers uint8 [B, S], counts
    int32 [B], best int32 [B]) behave as in verify_geometry.
    """
    ctx, on_dev, pp, pv, pt, b, s, ts, cam, mi, v, cn = _pnp_call(points, t_xy, K, matches, valid, point_valid, counts, (), ctx)
    c3 = (0.0, 0.0, 0.0) if center is None else tuple(float(x) for x in np.asarray(center, np.float64).reshape(3))
    opts = fd_pnp_opts(int(hypotheses), int(seed) & 0xFFFFFFFF, 1, float(threshold), *cam, (ctypes.c_double * 3)(*c3), float(scale))
    return PnpResult(*_call("fd_pnp_ransac", ctx, on_dev, pt, (b,), opts, (pp, pv, cn, s, pt, ts, mi, v), _model_specs(b, s, 12), out))


def refine_pnp(points, t_xy, result: PnpResult, K, matches=None, valid=None, point_valid=None, counts=None, rounds: int = 4,
               threshold: float = 2.0, out=None, ctx: Context | None = None) -> PnpRefineResult:
    """fd_pnp_refit: Gauss-Newton on the reprojection error over solve_pnp's inliers, the inliers classified
    again, up to `rounds` (1..8) times while their number does not fall.

    points, t_xy, K, matches, valid, point_valid, counts and threshold are solve_pnp's: pass the same ones.
    result: what solve_pnp returned (its pose float64 [B, 12] and inliers uint8 [B, S], on the side of t_xy). A
    frame whose first round is rejected keeps its pose bit for bit and has rounds 0.

    Returns a PnpRefineResult: pose, inliers, counts as solve_pnp's, best as given, and rounds int32 [B]. Host
    and device inputs and out= (pose float64 [B, 12], inliers uint8 [B, S], counts int32 [B], rounds int32 [B])
    behave as in verify_geometry; out= may hold result's own pose and inliers tensors.
    """
    ctx, on_dev, pp, pv, pt, b, s, ts, cam, mi, v, cn = _pnp_call(points, t_xy, K, matches, valid, point_valid, counts,
                                                                  (result.pose, result.inliers), ctx)
    ip, ii = slot_arg(result.pose, "float64", (b, 12), on_dev), slot_arg(result.inliers, "uint8", (b, s), on_dev)
    opts = fd_pnp_opts(1, 0, int(rounds), float(threshold), *cam, (ctypes.c_double * 3)(0.0, 0.0, 0.0), 1.0)
    oo, oi, oc, orr = _call("fd_pnp_refit", ctx, on_dev, pt, (b,), opts, (pp, pv, cn, s, pt, ts, mi, v, ip, ii),
                            _model_specs(b, s, 12), out)
    return PnpRefineResult(oo, oi, oc, result.best, orr)


@dataclass
class BundleResult:
    poses: object    # float64 [B, C, 12]: per camera R row-major, then t; a held camera's are the given ones bit for bit
    points: object   # float32 [B, S, 3]: the refined points; slots without an observation keep the given bits
    inliers: object  # uint8 [B, C, O]: 1 = an observation within `threshold` pixels of its reprojection at the final state
    counts: object   # int32 [B]: inlier observations per problem
    cost: object     # float64 [B, 2]: the truncated reprojection cost of the given and of the final state
    rounds: object   # int32 [B]: accepted Levenberg-Marquardt trials; 0: poses and points are the given ones

    def rotation(self, b=0, c=0):
        """Camera c of problem b: its R as a [3, 3] view."""
        return self.poses[b, c, :9].reshape(3, 3)

    def translation(self, b=0, c=0):
        return self.poses[b, c, 9:]


def _stack_poses(poses, on_dev):
    """poses as [B, C, 12]: an array or tensor, or a list with one entry per camera of PnpResult / PoseResult (their
    pose [B, 12]) or [B, 12] arrays."""
    if isinstance(poses, (list, tuple)):
        each = [getattr(p, "pose", p) for p in poses]
        if on_dev:
            import torch

            return torch.stack([e.to(torch.float64).reshape(-1, 12) for e in each], 1).contiguous()
        return np.ascontiguousarray(np.stack([np.asarray(e, np.float64).reshape(-1, 12) for e in each], 1))
    if len(poses.shape) == 2:
        poses = poses[None]
    return poses


def bundle_adjust(poses, points, obs_xy, K, obs_valid=None, point_valid=None, counts=None, fixed=None, rounds: int = 8,
                  threshold: float = 2.0, lam: float = 1e-3, up: float = 10.0, down: float = 0.1, out=None,
                  ctx: Context | None = None) -> BundleResult:
    """fd_bundle_adjust: the poses of up to 8 cameras and the 3-D points they share refined together, the local bundle
    adjustment over the last few keyframes after recover_pose / solve_pnp / refine_pnp. Levenberg-Marquardt on the
    reprojection cost truncated at `threshold` pixels, the points eliminated by the Schur complement.

    poses: float64 [B, C, 12] (or [C, 12] for batch 1), per camera R row-major then t, X_c = R X + t; or a list with
    one PnpResult / PoseResult / [B, 12] array per camera (the first camera of a two-view start is the identity).
    points: float32 [B, S, 3], or a PointsResult / PoseResult as it is (its valid bytes then are point_valid).
    obs_xy: float32 [B, C, O, 2] with O >= S, and obs_valid uint8 [B, C, O]: per camera track_lk's positions and
    status; slot i of every camera observes point i (gather matched features into slot order first). K: the one
    camera of all views, as in triangulate. fixed: uint8 [B, C] (a nested list will do), non-zero holds a camera (None: camera 0 alone; two
    held cameras pin the scale). rounds (1..16) counts accepted and rejected trials; lam, up, down: the initial
    damping, its factor after a rejected and after an accepted trial.

    Returns a BundleResult. Host and device inputs and out= (poses float64 [B, C, 12], points float32 [B, S, 3],
    inliers uint8 [B, C, O], counts int32 [B], cost float64 [B, 2], rounds int32 [B]) behave as in verify_geometry;
    out= may hold the given poses and points tensors themselves.
    """
    points, point_valid = _unwrap(points, point_valid)
    on_dev = is_device_tensor(obs_xy)
    poses = _stack_poses(poses, on_dev)
    if on_dev and isinstance(fixed, (list, tuple)):  # a few flags written out by hand
        import torch

        fixed = torch.tensor(fixed, dtype=torch.uint8, device=obs_xy.device)
    sides = [is_device_tensor(points), is_device_tensor(poses)]
    sides += [is_device_tensor(x) for x in (obs_valid, point_valid, counts, fixed) if x is not None]
    if any(side != on_dev for side in sides):
        raise ValueError("poses, points and the masks must be on the side (host / device) of obs_xy")
    ctx = resolve_ctx(ctx, obs_xy, points)
    oshape = tuple(obs_xy.shape)
    if len(oshape) == 3:
        oshape = (1,) + oshape
    if len(oshape) != 4 or oshape[3] != 2:
        raise ValueError("obs_xy must be float32 [B, C, O, 2] (or [C, O, 2] for batch 1)")
    b, c, o = int(oshape[0]), int(oshape[1]), int(oshape[2])
    po = f32(obs_xy, "obs_xy", on_dev).reshape(oshape)
    s = int(_xyz(points, "points", b, "obs_xy's")[1])
    if o < s:
        raise ValueError("slot i of a camera observes point i: obs_xy needs at least as many slots as points")
    if tuple(poses.shape) != (b, c, 12):
        raise ValueError("poses must be float64 [B, C, 12] with obs_xy's batch and cameras")
    pp = slot_arg(points, "float32", (b, s, 3), on_dev)
    ip = slot_arg(poses, "float64", (b, c, 12), on_dev)
    ov, pv = slot_arg(obs_valid, "uint8", (b, c, o), on_dev), slot_arg(point_valid, "uint8", (b, s), on_dev)
    cn, fx = slot_arg(counts, "int32", (b,), on_dev), slot_arg(fixed, "uint8", (b, c), on_dev)
    opts = fd_ba_opts(int(rounds), float(threshold), *intrinsics(K), float(lam), float(up), float(down))
    specs = (((b, c, 12), "float64", 0), ((b, s, 3), "float32", 0), ((b, c, o), "uint8", 0), ((b,), "int32", 0),
             ((b, 2), "float64", 0), ((b,), "int32", 0))
    return BundleResult(*_call("fd_bundle_adjust", ctx, on_dev, po, (b, c), opts, (ip, fx, pp, pv, cn, s, po, ov, o), specs, out))


ALIGN_KINDS = {"similarity": _lib.FD_ALIGN_SIMILARITY, "rigid": _lib.FD_ALIGN_RIGID}


@dataclass
class AlignResult:
    model: object    # float64 [B, 13]: R row-major, then t, then s, Y = s R X + t; zeros: no model
    inliers: object  # uint8 [B, S]: 1 = a correspondence within `threshold` of its mapped point, in the target's units
    counts: object   # int32 [B]: inliers per frame
    best: object     # int32 [B]: the winning hypothesis, -1: no model

    def rotation(self, b=0):
        """Frame b's R as a [3, 3] view."""
        return self.model[b, :9].reshape(3, 3)

    def translation(self, b=0):
        return self.model[b, 9:12]

    def scale(self, b=0):
        return self.model[b, 12]


@dataclass
class AlignRefineResult(AlignResult):
    rounds: object = None  # int32 [B]: accepted refit rounds; 0: model and inliers are the given ones


def _align_call(q_xyz, t_xyz, matches, valid, q_valid, t_valid, counts, kind, extra, ctx):
    """What align_points and refine_alignment share: the checked arguments of the two entry points. `extra`: further
    arrays that must be on the side of q_xyz."""
    if kind not in ALIGN_KINDS:
        raise ValueError(f"kind must be one of {sorted(ALIGN_KINDS)}")
    (q_xyz, q_valid), (t_xyz, t_valid) = _unwrap(q_xyz, q_valid), _unwrap(t_xyz, t_valid)
    on_dev = is_device_tensor(q_xyz)
    others = [t_xyz, *extra] + [x for x in (q_valid, t_valid) if x is not None]
    if any(is_device_tensor(x) != on_dev for x in others):
        raise ValueError("t_xyz, the masks and the given result must be on the side (host / device) of q_xyz")
    ctx = resolve_ctx(ctx, q_xyz, t_xyz)
    qs, ts = _xyz(q_xyz, "q_xyz"), _xyz(t_xyz, "t_xyz")
    b, s, t = int(qs[0]), int(qs[1]), int(ts[1])
    if ts[0] != b:
        raise ValueError("q_xyz and t_xyz must have the same batch")
    pq, pt = f32(q_xyz, "q_xyz", on_dev).reshape(qs), f32(t_xyz, "t_xyz", on_dev).reshape(ts)
    mi, v, cn = _slots(on_dev, b, s, t, "q_xyz", matches, valid, counts)
    qv, tv = slot_arg(q_valid, "uint8", (b, s), on_dev), slot_arg(t_valid, "uint8", (b, t), on_dev)
    return ctx, on_dev, pq, qv, pt, tv, b, s, t, mi, v, cn


def align_points(q_xyz, t_xyz, matches=None, valid=None, q_valid=None, t_valid=None, counts=None, kind: str = "similarity",
                 hypotheses: int = 256, seed: int = 0, threshold: float = 0.1, out=None, ctx: Context | None = None) -> AlignResult:
    """fd_align_ransac: the similarity ("similarity": Y = s R X + t) or rigid ("rigid": s = 1) transform between two
    sets of 3-D points with the most inliers among `hypotheses` 3-point samples: what joins a keyframe window to the
    map before it, closes a loop at a drifted scale, or registers recover_pose's points against metric ones.

    q_xyz: float32 [B, S, 3] (or [S, 3] for batch 1) and t_xyz: float32 [B, T, 3], or a PointsResult / PoseResult as
    it is on either side (its valid bytes then are q_valid / t_valid). matches, valid, counts: verify_geometry's.
    q_valid uint8 [B, S], t_valid uint8 [B, T]: a point takes part only where its byte is 1 (None: all). threshold is
    the distance |Y - (s R X + t)| in the target's units, absolute: choose it for the target's scale. Planar point sets
    are fine; duplicate and collinear samples are rejected.

    Returns an AlignResult. Host and device inputs and out= (model float64 [B, 13], inliers uint8 [B, S], counts
    int32 [B], best int32 [B]) behave as in verify_geometry.
    """
    ctx, on_dev, pq, qv, pt, tv, b, s, t, mi, v, cn = _align_call(q_xyz, t_xyz, matches, valid, q_valid, t_valid, counts, kind,
                                                                  (), ctx)
    opts = fd_align_opts(ALIGN_KINDS[kind], int(hypotheses), int(seed) & 0xFFFFFFFF, 1, float(threshold))
    return AlignResult(*_call("fd_align_ransac", ctx, on_dev, pq, (b,), opts, (pq, qv, cn, s, pt, tv, t, mi, v), _model_specs(b, s, 13), out))


def refine_alignment(q_xyz, t_xyz, result: AlignResult, matches=None, valid=None, q_valid=None, t_valid=None, counts=None,
                     kind: str = "similarity", rounds: int = 4, threshold: float = 0.1, out=None,
                     ctx: Context | None = None) -> AlignRefineResult:
    """fd_align_refit: the closed-form least-squares transform (Horn's quaternion method) on align_points' inliers, the
    inliers classified again, up to `rounds` (1..8) times while their number does not fall.

    q_xyz, t_xyz, matches, valid, q_valid, t_valid, counts, kind and threshold are align_points': pass the same ones.
    result: what align_points returned (its model float64 [B, 13] and inliers uint8 [B, S], on the side of q_xyz). A
    frame whose first round is rejected (fewer than 3 members, fewer inliers than before) keeps its model bit for bit
    and has rounds 0. Collinear members leave the roll about their line arbitrary.

    Returns an AlignRefineResult: model, inliers, counts as align_points', best as given, and rounds int32 [B]. Host
    and device inputs and out= (model float64 [B, 13], inliers uint8 [B, S], counts int32 [B], rounds int32 [B])
    behave as in verify_geometry; out= may hold result's own model and inliers tensors.
    """
    ctx, on_dev, pq, qv, pt, tv, b, s, t, mi, v, cn = _align_call(q_xyz, t_xyz, matches, valid, q_valid, t_valid, counts, kind,
                                                                  (result.model, result.inliers), ctx)
    im, ii = slot_arg(result.model, "float64", (b, 13), on_dev), slot_arg(result.inliers, "uint8", (b, s), on_dev)
    opts = fd_align_opts(ALIGN_KINDS[kind], 1, 0, int(rounds), float(threshold))
    om, oi, oc, orr = _call("fd_align_refit", ctx, on_dev, pq, (b,), opts, (pq, qv, cn, s, pt, tv, t, mi, v, im, ii),
                            _model_specs(b, s, 13), out)
    return AlignRefineResult(om, oi, oc, result.best, orr)


def transform_points(model, xyz, valid=None, counts=None, out=None, ctx: Context | None = None):
    """fd_align_apply: (float32)(s R X + t) of every valid point, so that a merged point set stays on the device.

    model: an AlignResult / AlignRefineResult, or float64 [B, 13] (or [13] for batch 1). xyz: float32 [B, S, 3] (or
    [S, 3]), or a PointsResult / PoseResult as it is (its valid bytes then are `valid`). valid uint8 [B, S] (None: all)
    and counts int32 [B] (None: S each): a slot is transformed where its byte is 1 and it lies below its frame's count.

    Returns float32 [B, S, 3] on xyz's side: a copy of xyz with the transformed slots replaced. Device path only: out =
    a preallocated contiguous float32 [B, S, 3] tensor, of which the transformed slots alone are written; out may be
    xyz itself (in place; kernels only, graph-capturable).
    """
    xyz, valid = _unwrap(xyz, valid)
    model = getattr(model, "model", model)
    on_dev = is_device_tensor(xyz)
    if is_device_tensor(model) != on_dev or any(is_device_tensor(x) != on_dev for x in (valid, counts) if x is not None):
        raise ValueError("model, valid and counts must be on the side (host / device) of xyz")
    ctx = resolve_ctx(ctx, xyz, xyz)
    shape = _xyz(xyz, "xyz")
    b, s = int(shape[0]), int(shape[1])
    px = f32(xyz, "xyz", on_dev).reshape(shape)
    pm = slot_arg(model, "float64", (b, 13), on_dev)
    pv, cn = slot_arg(valid, "uint8", (b, s), on_dev), slot_arg(counts, "int32", (b,), on_dev)
    if out is None:
        res = px.clone() if on_dev else px.copy()
    else:
        (res,) = outputs(((shape, "float32", 0),), (out,), on_dev)
    invoke(ctx, on_dev, "fd_align_apply", b, ptr(pm), ptr(px), ptr(pv), ptr(cn), s, ptr(res), 1 if on_dev else 0)
    return res


def transform_poses(model, poses):
    """The window's cameras after its points moved by a model (host arithmetic, numpy float64): a camera X_c = R_c X + t_c
    of the source frame becomes R_c' = R_c R^T, t_c' = s t_c - R_c' t in the target frame. The camera's depth unit scales
    by s with it: a point X has the camera coordinates s X_c under the new pose, so its image position is unchanged.

    model: float64 [13] or [B, 13] (an AlignResult passes; device tensors are copied to the host). poses: float64
    [B, 12] or [B, C, 12] (or [12]), R row-major then t, as solve_pnp / recover_pose / bundle_adjust return them.
    Returns the new poses as a numpy float64 array of poses' shape.
    """
    host = lambda x: np.asarray(x.cpu() if hasattr(x, "cpu") else x, np.float64)  # noqa: E731
    model, poses = host(getattr(model, "model", model)), host(getattr(poses, "pose", poses))
    shape = poses.shape
    if shape[-1] != 12 or model.shape[-1] != 13:
        raise ValueError("poses must be [..., 12] and model [13] or [B, 13]")
    model = model.reshape(-1, 13)
    p = poses.reshape((1, 1, 12) if poses.ndim == 1 else (shape[0], -1, 12))
    if model.shape[0] not in (1, p.shape[0]):
        raise ValueError("model must be [13] or have the poses' batch")
    out = np.empty_like(p)
    for b in range(p.shape[0]):
        m = model[b if model.shape[0] > 1 else 0]
        R, t, s = m[:9].reshape(3, 3), m[9:12], m[12]
        for c in range(p.shape[1]):
            Rn = p[b, c, :9].reshape(3, 3) @ R.T
            out[b, c, :9] = Rn.reshape(9)
            out[b, c, 9:] = s * p[b, c, 9:] - Rn @ t
    return out.reshape(shape)
