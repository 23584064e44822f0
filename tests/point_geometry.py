"""The point detectors' launch geometry and staging capacities (choose_tile_h, point_geom, use_seg_lists and
corner_px in fd_rt_points.cpp; decode_tile in fd_corner_common.h; the staging of fd_points.hip and
fd_corner_lp.hip), restated for the tests: a test asserts from these formulas which workgroups of its frames
overflow their staging, so that a later geometry or capacity change cannot silently move it off that branch."""
import os
import re

import numpy as np

TILE_W = 248  # fdk::kTileW
SELECT_THREADS = 1024  # fdk::kSelectThreads
LP_SLOTS_HIST = 11  # kLpSlotsHist (fd_corner_lp.hip): lane-private slots per lane with the selection histogram


def _makefile_default(name):
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "feature_detector_amd", "csrc", "Makefile")
    with open(path) as fh:
        return int(re.search(r"^%s \?= (\d+)" % name, fh.read(), re.M).group(1))


STAGE_CORNER = _makefile_default("STAGE_CORNER")  # candidates a k_corner wave stages
STAGE_FAST = _makefile_default("STAGE_FAST")  # candidates a k_fast wave stages


def lp_tile_w(px):
    return (64 - 2 * (2 if px == 2 else 1)) * px


def choose_tile_h(batch, tiles_x, out_rows, period, max_mult):
    h = (batch * tiles_x * out_rows) // 10240
    if h < period and period == 6:
        h = 3
    else:
        h = -(-max(h, period) // period) * period
    return min(h, period * max_mult)


def corner_px(kind, batch, rows, cols, thr, forced=None):
    """Columns per lane of k_corner_lp, 0 = k_corner / k_fast; forced: the FD_PX override."""
    if kind == 2 or not thr >= 0.0 or rows * cols >= 1 << 30:
        return 0
    if forced is not None:
        return forced
    return 4 if batch * rows * cols >= 1 << 21 else 0


def point_geom(kind, batch, rows, cols, px=0):
    """dict(border, tile_w, tile_h, tiles_x, tiles_y, blocks_per_frame) of a non-empty launch."""
    border = 3 if kind == 2 else 2
    out_rows = rows - 2 * border
    assert out_rows > 0 and cols - 2 * border > 0
    tw = lp_tile_w(px) if px else TILE_W
    tiles_x = max(1, (cols - border + tw - 1) // tw)
    tile_h = choose_tile_h(batch, tiles_x, out_rows, 7 if kind == 2 else 6, 9 if kind == 2 else 100)
    tiles_y = (out_rows + tile_h - 1) // tile_h
    return dict(border=border, tile_w=tw, tile_h=tile_h, tiles_x=tiles_x, tiles_y=tiles_y,
                blocks_per_frame=(tiles_x * tiles_y + 3) // 4)


def use_seg_lists(g, rows, cols):
    return g["blocks_per_frame"] <= SELECT_THREADS and rows * cols < 1 << 20


def tile_of(g, x, y):
    """Tile index (ty * tiles_x + tx) of candidate pixels; tile t is wave t % 4 of the frame's workgroup t // 4."""
    return ((np.asarray(y) - g["border"]) // g["tile_h"]) * g["tiles_x"] + np.asarray(x) // g["tile_w"]


def overflowing_workgroups(g, x, y, kind, px):
    """Workgroups of one frame (a set of indices) in which a wave flushes its staging before the end of its
    tile, from the frame's candidate positions. k_corner / k_fast: a wave's candidates exceed its staging.
    k_corner_lp: before some row of the tile a lane (px columns) already holds LP_SLOTS_HIST - px / 2 entries."""
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    t = tile_of(g, x, y)
    if px == 0:
        cnt = np.bincount(t, minlength=g["tiles_x"] * g["tiles_y"])
        return set((np.nonzero(cnt > (STAGE_FAST if kind == 2 else STAGE_CORNER))[0] // 4).tolist())
    over = set()
    lane = x // px  # (a lane's columns never straddle two tiles: the tile width is a multiple of px)
    row_in_tile = (y - g["border"]) % g["tile_h"]
    per = np.zeros((g["tiles_x"] * g["tiles_y"], g["tile_h"], (g["tiles_x"] * g["tile_w"]) // px + 1), np.int64)
    np.add.at(per, (t, row_in_tile, lane), 1)
    before = np.cumsum(per, axis=1) - per  # entries a lane holds when the row's check runs
    hit = (before >= LP_SLOTS_HIST - px // 2).any(axis=(1, 2))
    return set((np.nonzero(hit)[0] // 4).tolist())
