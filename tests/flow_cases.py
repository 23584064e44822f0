"""Inputs of the tracker's edge tests, shared by tests/test_flow_host.py (which checks on the restatement that
each input has the property it was built for) and tests/test_gpu_flow_edges.py (which compares the kernel
with the restatement on it)."""
import numpy as np

import flow_ref as R

ROWS, COLS = 96, 128


def rounds(r):
    """Window pixels per lane of a 64-lane wave: the ROUNDS instance launch_flow_lk picks for half_window r."""
    return ((2 * r + 1) ** 2 + 63) // 64


# ---- saturated contrast: window sums past 2^31 -----------------------------------------------------------

SAT_SHIFT = (-1, -1)


def sat_frames(shift=SAT_SHIFT):
    """prev, next [1, 96, 128]: random 0 / 255 blocks 2 px wide; next's content sits `shift` = (sx, sy) pixels
    right / down of prev's.

    The binary array is the column parity with 30 % of its cells flipped. Fair coin flips put a step under
    half of the horizontal central differences, which leaves sum gx*gx of a 21 x 21 window near 3.7e9, short
    of 2^32; this bias puts one under 58 % of them and still leaves 42 % of the vertical ones a step, so
    the features stay trackable. With the content moving left / up, d = I - J has the sign opposite to the
    gradient wherever both are non-zero: b1 and b2 are large and negative."""
    rng = np.random.default_rng(1)
    shape = (ROWS // 2 + 2, COLS // 2 + 2)
    cells = ((np.arange(shape[1])[None] & 1) ^ (rng.random(shape) < 0.3)).astype(np.uint8) * 255
    big = np.kron(cells, np.ones((2, 2), np.uint8))
    sx, sy = shift
    prev = big[2:2 + ROWS, 2:2 + COLS]
    nxt = big[2 - sy:2 - sy + ROWS, 2 - sx:2 - sx + COLS]
    return np.ascontiguousarray(prev[None]), np.ascontiguousarray(nxt[None])


def sat_features():
    """[1, 24, 2] positions in [14, size - 15], the first eight integral."""
    rng = np.random.default_rng(1)
    xy = np.stack([rng.uniform(14, COLS - 15, 24), rng.uniform(14, ROWS - 15, 24)], -1).astype(np.float32)
    xy[:8] = np.rint(xy[:8])
    return xy[None]


def level0_sums(prev, nxt, xy, r):
    """(a11, b1, b2) of level 0 at the first iteration with d = 0, as Python ints, formed from R._raw_sum the
    way R.track_one forms them. prev, nxt [rows, cols]."""
    p, q = prev.astype(np.int64), nxt.astype(np.int64)
    x, y = np.float32(xy[0]), np.float32(xy[1])
    vs, us = np.meshgrid(np.arange(-r, r + 1), np.arange(-r, r + 1), indexing="ij")
    iq = (R._raw_sum(p, x, y, us, vs) + 2 ** 14) >> 15
    gx = (R._raw_sum(p, x, y, us + 1, vs) - R._raw_sum(p, x, y, us - 1, vs) + 2 ** 15) >> 16
    gy = (R._raw_sum(p, x, y, us, vs + 1) - R._raw_sum(p, x, y, us, vs - 1) + 2 ** 15) >> 16
    d = iq - ((R._raw_sum(q, x, y, us, vs) + 2 ** 14) >> 15)
    return int((gx * gx).sum()), int((d * gx).sum()), int((d * gy).sum())


# ---- odd sizes and the far edge --------------------------------------------------------------------------

ODD_ROWS, ODD_COLS = 97, 131


def odd_features():
    """[3, 20, 2]: the far edges and corners of a 97 x 131 frame, then a dozen interior positions (the same
    in every frame of the batch; the frames differ)."""
    c, r = ODD_COLS, ODD_ROWS
    edge = [(c - 1, r - 1), (c - 1, 40), (50, r - 1), (c - 1.25, r - 1.5), (0, 0), (c - 1, 0), (0, r - 1), (c - 1.5, 33.25)]
    rng = np.random.default_rng(7)
    inner = np.stack([rng.uniform(12, c - 13, 12), rng.uniform(12, r - 13, 12)], -1)
    inner[:4] = np.rint(inner[:4])
    xy = np.concatenate([np.array(edge, np.float64), inner]).astype(np.float32)
    return np.ascontiguousarray(np.broadcast_to(xy, (3,) + xy.shape))


def beyond_last_column(xy, cols, levels):
    """[(feature, level)] with x * 2^-l > (cols >> l) - 1: the whole template patch reads the clamp column."""
    return [(i, l) for i, p in enumerate(xy) for l in range(levels)
            if np.float32(p[0]) * np.float32(2.0 ** -l) > (cols >> l) - 1]


# ---- blobs-plus-noise frames of any size -------------------------------------------------------------------

def _box(a, k):
    p = np.pad(a, k // 2, mode="edge")
    c = np.cumsum(np.cumsum(np.pad(p, ((1, 0), (1, 0))), 0), 1)
    return (c[k:, k:] - c[:-k, k:] - c[k:, :-k] + c[:-k, :-k]) / (k * k)


def blob_pair(oracle, seeds, rows, cols, shift, pad=8):
    """prev, next [len(seeds), rows, cols]: smoothed 8 px blobs (0.85) plus pixel noise (0.15), the recipe of
    test_gpu_flow.py's canvas at any frame size; next's content sits `shift` = (sx, sy) right / down of prev's."""
    r, c = rows + 2 * pad, cols + 2 * pad
    out = []
    for seed in seeds:
        coarse = oracle.make_frame("noise", seed, r // 8 + 1, c // 8 + 1).astype(np.float64)
        fine = oracle.make_frame("noise", seed + 100, r, c).astype(np.float64)
        blobs = _box(np.kron(coarse, np.ones((8, 8)))[:r, :c], 7)
        out.append(np.clip(np.rint(0.85 * blobs + 0.15 * fine), 0, 255).astype(np.uint8))
    big = np.stack(out)
    sx, sy = shift
    return (np.ascontiguousarray(big[:, pad:pad + rows, pad:pad + cols]),
            np.ascontiguousarray(big[:, pad - sy:pad - sy + rows, pad - sx:pad - sx + cols]))
