"""Deterministic adversarial frames for the point path (numpy only; a plain module like match_ref.py).

Three input families that uniform noise, the 60/180 checker and image.png do not reach:

* saturated frames (two_level, n_level, stripes, blocks): tensor sums at the ends of their domain
  (Sxx = 9*255^2 with Syy = 0, Sxy = +-9*255^2), responses in the top and bottom level-0 key bins, and
  hundreds of candidates with equal responses;
* stamp frames (stamp_frame): any exact number of candidates with one bit-identical response, produced by
  the detector itself;
* FAST patch frames (fast_pairs, fast_rings): every (centre, sample) value pair and every 16-bit ring
  pattern, each centre at pitch 7 so that it walks through all four byte positions of a dword.

fast_rule() restates the FAST score from its definition, independently of the oracle.
"""
import numpy as np

# kFastIndice (feature_point_fast_detector.cpp:7-8): ring sample k at (dx, dy)
FAST_RING = ((0, -3), (1, -3), (2, -2), (3, -1), (3, 0), (3, 1), (2, 2), (1, 3),
             (0, 3), (-1, 3), (-2, 2), (-3, 1), (-3, 0), (-3, -1), (-2, -2), (-1, -3))
FAST_DIFF = 15  # feature_point_fast_detector.h:14
PATCH = 7  # a FAST patch: the centre and its radius-3 ring

STAMP = np.full((9, 9), 100, np.uint8)
STAMP[2:5, 2:5] = 250
STAMP[4:7, 4:7] = 10
STAMP_ORIGIN = 4  # first stamp origin, and the free margin kept after the last stamp


def two_level(rows, cols, seed, levels=(0, 255)):
    """Each pixel one of `levels`, uniformly (RandomState: its stream is frozen across numpy versions)."""
    lv = np.asarray(levels, np.uint8)
    return lv[np.random.RandomState(seed).randint(0, len(lv), size=(rows, cols))]


def n_level(rows, cols, seed, n):
    """n equally spaced levels from 0 to 255 (n = 4: 0, 85, 170, 255)."""
    return two_level(rows, cols, seed, [round(i * 255 / (n - 1)) for i in range(n)])


def stripes(rows, cols, kind):
    """0/255 stripes of period 4 (0, 0, 255, 255) along x ('v'), y ('h'), x + y ('diag'), x - y ('anti')."""
    y, x = np.mgrid[0:rows, 0:cols]
    t = {"v": x, "h": y, "diag": x + y, "anti": x - y}[kind]
    return (((t // 2) % 2) * 255).astype(np.uint8)


def blocks(rows, cols, s):
    """0/255 checkerboard of s x s blocks."""
    y, x = np.mgrid[0:rows, 0:cols]
    return ((((x // s) + (y // s)) % 2) * 255).astype(np.uint8)


def stamp_grid(rows, cols, pitch=12):
    """(stamps per column, stamps per row) that fit: origins 4 + pitch * i, 4 free pixels after the last."""
    fit = lambda size: max((size - 2 * STAMP_ORIGIN - STAMP.shape[0]) // pitch + 1, 0)
    return fit(rows), fit(cols)


def stamp_shape(n, pitch=12):
    """The smallest near-square frame that holds n stamps."""
    k = int(np.ceil(np.sqrt(n)))
    size = lambda m: pitch * (m - 1) + STAMP.shape[0] + 2 * STAMP_ORIGIN
    return size(-(-n // k)), size(k)


def stamp_frame(rows, cols, n, pitch=12):
    """Background 100 with the first n stamp positions (raster order) stamped. Returns (frame, origins
    [n, 2] int32 (x, y))."""
    ny, nx = stamp_grid(rows, cols, pitch)
    assert n <= ny * nx, f"{rows}x{cols} holds {ny * nx} stamps at pitch {pitch}, not {n}"
    img = np.full((rows, cols), 100, np.uint8)
    origins = np.zeros((n, 2), np.int32)
    for k in range(n):
        y0, x0 = STAMP_ORIGIN + pitch * (k // nx), STAMP_ORIGIN + pitch * (k % nx)
        img[y0:y0 + 9, x0:x0 + 9] = STAMP
        origins[k] = (x0, y0)
    return img, origins


def _set_ring(img, cy, cx, values):
    """values [n, 16] -> ring sample k of centre (cy[i], cx[i])."""
    for k, (dx, dy) in enumerate(FAST_RING):
        img[cy + dy, cx + dx] = values[:, k]


def patch_centres(n_rows, n_cols):
    """(y, x) of every 7x7 patch centre of an n_rows x n_cols patch grid, raster order."""
    py, px = np.divmod(np.arange(n_rows * n_cols), n_cols)
    return py * PATCH + 3, px * PATCH + 3


def fast_pairs(p_lo, p_hi):
    """7x7 patches (p, v), p in [p_lo, p_hi) down, v in [0, 256) across: filled with p, ring samples v."""
    n = p_hi - p_lo
    p = np.repeat(np.arange(p_lo, p_hi, dtype=np.uint8), PATCH)
    img = np.repeat(p[:, None], PATCH * 256, axis=1)
    cy, cx = patch_centres(n, 256)
    v = (np.arange(n * 256) % 256).astype(np.uint8)
    _set_ring(img, cy, cx, np.repeat(v[:, None], 16, axis=1))
    return np.ascontiguousarray(img)


def fast_rings(lo, hi, mode):
    """7x7 patches of the ring patterns lo..hi-1, 256 to a row, filled with 128. Ring sample k where bit k
    is set / clear: 'bright' 255 / 128, 'mixed' 255 / 0, 'dark' 0 / 128."""
    on, off = {"bright": (255, 128), "mixed": (255, 0), "dark": (0, 128)}[mode]
    n = hi - lo
    assert n % 256 == 0
    img = np.full((PATCH * (n // 256), PATCH * 256), 128, np.uint8)
    cy, cx = patch_centres(n // 256, 256)
    bits = (np.arange(lo, hi)[:, None] >> np.arange(16)[None, :]) & 1
    _set_ring(img, cy, cx, np.where(bits == 1, on, off).astype(np.uint8))
    return img


def fast_rule(img, cy, cx):
    """FAST-12 score at the centres (cy, cx), from the definition (feature_point_fast_detector.cpp:11-81):
    a sample's class is +1 above p + 15, -1 below p - 15, else 0; the pre-check asks samples 4, 8 and 12
    for one class other than 0; the score is the longest run of one non-zero class met while walking the
    ring twice with counters that are never reset between the passes, the walk ending once a pass has
    reached 16."""
    img = img.astype(np.int32)
    p = img[cy, cx]
    cls = np.zeros((len(p), 16), np.int32)
    for k, (dx, dy) in enumerate(FAST_RING):
        v = img[cy + dy, cx + dx]
        cls[:, k] = np.where(v > p + FAST_DIFF, 1, np.where(v < p - FAST_DIFF, -1, 0))
    pre = (cls[:, 4] != 0) & (cls[:, 4] == cls[:, 8]) & (cls[:, 8] == cls[:, 12])
    run = np.zeros(len(p), np.int32)
    last = np.zeros(len(p), np.int32)
    best = np.zeros(len(p), np.int32)
    for step in range(32):
        if step == 16:
            done = best >= 16
        c = cls[:, step % 16]
        run = np.where(c == 0, 0, np.where(c == last, run + 1, 1))
        last = c
        best = np.maximum(best, run) if step < 16 else np.where(done, best, np.maximum(best, run))
    return np.where(pre, best, 0)


def fast_expected_at_centres(img, thr=10.0):
    """(cy, cx, score, response) at every patch centre of a fast_pairs / fast_rings frame by the rule: the
    response is fl(score + offset) where that exceeds thr, else 0 (no candidate). No mask."""
    rows, cols = img.shape
    cy, cx = patch_centres(rows // PATCH, cols // PATCH)
    score = fast_rule(img, cy, cx)
    resp = score.astype(np.float32) + fast_offsets(rows, cols, cy, cx)
    return cy, cx, score, np.where(resp > np.float32(thr), resp, np.float32(0))


def fast_offsets(rows, cols, cy, cx):
    """The running float offset (feature_point_fast_detector.cpp:85, :93) at unmasked pixels (cy, cx):
    o_0 = 1e-5f, o_{k+1} = fl(o_k + 1e-5f), k counting the pixels of [3, rows-3) x [3, cols-3) in raster
    order. (A float32 cumsum adds sequentially.)"""
    seq = np.cumsum(np.full((rows - 6) * (cols - 6), 1e-5, np.float32), dtype=np.float32)
    return seq[(cy - 3) * (cols - 6) + (cx - 3)]
