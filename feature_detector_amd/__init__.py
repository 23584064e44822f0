"""MI355X-native feature-detection hot path (Horizon1026/Feature_Detector drop-in for its per-pixel stages).

Layers:
  include/fd_hip.h          C ABI (libfdhip.so: gfx950 HIP kernels + runtime)
  include/feature_detector/ C++ classes with the reference's API (libfeature_detector.so)
  feature_detector_amd      Python batch API over the C ABI (this package: _lib, _context, _slots, one module per stage)
"""
from ._lib import FD_FAST, FD_HARRIS, FD_SHI_TOMASI, FdError, LIB_PATH, load  # noqa: F401
from .points import Context, DetectResult, default_context, detect_points, point_candidates, point_response, select_points  # noqa: F401
from .descriptor import brief_compute, to_float, unpack_bits  # noqa: F401
from .match import MatchResult, brief_match, nn_match  # noqa: F401
from .flow import FlowResult, Pyramid, build_pyramid, pyramid_layout, track_lk  # noqa: F401
from .refine import RefineResult, refine_points  # noqa: F401
from .geometry import (AlignRefineResult, AlignResult, BundleResult, GeometryResult, PnpRefineResult, PnpResult, PoseResult, PointsResult, RefitResult,  # noqa: F401
                       align_points, bundle_adjust, recover_pose, refine_alignment, refine_pnp, refit_geometry, solve_pnp, transform_points, transform_poses,
                       triangulate, verify_geometry)
from .warp import camera_params, warp_frames  # noqa: F401
from .equalize import equalize_frames  # noqa: F401
from .blur import blur_frames, gaussian_taps  # noqa: F401
from .lines import LineDescResult, describe_lines, lsd_lines, lsd_map  # noqa: F401
from .ingest import Ingest, load_png, png_frames, png_info  # noqa: F401

__all__ = [
    "FD_HARRIS", "FD_SHI_TOMASI", "FD_FAST", "FdError", "Context", "DetectResult", "default_context",
    "detect_points", "point_candidates", "point_response", "select_points", "lsd_map", "lsd_lines", "load", "brief_compute", "unpack_bits",
    "to_float", "brief_match", "nn_match", "MatchResult", "build_pyramid", "pyramid_layout", "track_lk", "Pyramid",
    "FlowResult", "refine_points", "RefineResult", "verify_geometry", "GeometryResult", "refit_geometry", "RefitResult", "recover_pose", "PoseResult", "triangulate", "PointsResult", "solve_pnp", "PnpResult", "refine_pnp", "PnpRefineResult", "bundle_adjust", "BundleResult", "align_points", "AlignResult", "refine_alignment", "AlignRefineResult", "transform_points", "transform_poses", "warp_frames", "camera_params", "equalize_frames", "blur_frames", "gaussian_taps", "describe_lines", "LineDescResult", "Ingest", "load_png", "png_frames", "png_info",
]
