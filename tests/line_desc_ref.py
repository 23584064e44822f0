"""numpy restatement of fd_lines_describe (include/fd_hip.h): the line band descriptor, per line, in the
contract's operation order. Per-sample coordinates are float64 array operations (one rounding each, numpy does
not fuse separate calls), sums of gradients are int64, the band statistics and norms are Python floats summed
serially. describe() also returns every line's N, S and flip, so tests can assert which branches they hit."""
import math

import numpy as np

MAX_SAMPLES = 4096
Q = 16384.0


def _rint(v):
    return int(np.rint(v))  # round half to even


def row_sums(frame, sx, sy, ex, ey, bands, w):
    """(v int64 [H, 4], N, c), or (None, 0, c) for an invalid line; c is None where an endpoint is not finite."""
    f = [float(np.float32(t)) for t in (sx, sy, ex, ey)]
    if not all(math.isfinite(t) for t in f):
        return None, 0, None
    sx, sy, ex, ey = f
    dx, dy = ex - sx, ey - sy
    L = math.sqrt(dx * dx + dy * dy)
    c = ((sx + ex) * 0.5, (sy + ey) * 0.5)
    if not L >= 1.0:
        return None, 0, c
    dlx, dly = dx / L, dy / L
    nx, ny = -dly, dlx
    dqx, dqy = _rint(dlx * Q), _rint(dly * Q)
    nqx, nqy = -dqy, dqx
    N = int(min(math.floor(L), MAX_SAMPLES))
    H = bands * w
    rows, cols = frame.shape
    a = np.arange(N, dtype=np.float64)[None, :] - (N - 1) * 0.5
    b = np.arange(H, dtype=np.float64)[:, None] - (H - 1) * 0.5
    x = c[0] + (a * dlx + b * nx)
    y = c[1] + (a * dly + b * ny)
    fx, fy = np.floor(x + 0.5), np.floor(y + 0.5)
    ok = (fx >= 1.0) & (fx <= cols - 2) & (fy >= 1.0) & (fy <= rows - 2)
    px = np.where(ok, fx, 1.0).astype(np.int64)
    py = np.where(ok, fy, 1.0).astype(np.int64)
    img = frame.astype(np.int64)
    gx = img[py, px + 1] - img[py, px - 1]
    gy = img[py + 1, px] - img[py - 1, px]
    gp = np.where(ok, gx * nqx + gy * nqy, 0)
    gl = np.where(ok, gx * dqx + gy * dqy, 0)
    v = np.stack([np.maximum(gp, 0).sum(1), np.maximum(-gp, 0).sum(1), np.maximum(gl, 0).sum(1), np.maximum(-gl, 0).sum(1)], 1)
    return v.astype(np.int64), N, c


def bands_of(r, bands, w):
    """Raw descriptor D (a list of 8 * bands Python floats) of oriented row sums r int64 [H, 4]."""
    H = bands * w
    D = [0.0] * (8 * bands)
    for k in range(bands):
        for m in range(4):
            u = []
            for t in range(3 * w):
                j = (k - 1) * w + t
                if j < 0 or j >= H:
                    continue
                g, l = H - abs(2 * j - (H - 1)), 3 * w - abs(2 * t - (3 * w - 1))
                ui = g * l * int(r[j, m])
                assert ui < 2 ** 53
                u.append(float(ui))
            n_rows = float(len(u))
            s = 0.0
            for t in u:
                s += t
            mean = s / n_rows
            acc = 0.0
            for t in u:
                d = t - mean
                acc += d * d
            D[8 * k + m] = mean
            D[8 * k + 4 + m] = math.sqrt(acc / n_rows)
    return D


def normalise(D, bands):
    """(float32 [8 * bands], valid) of a raw descriptor."""
    D = list(D)
    qs = []
    for off in (0, 4):
        idx = [8 * k + off + m for k in range(bands) for m in range(4)]
        s = 0.0
        for i in idx:
            s += D[i] * D[i]
        q = math.sqrt(s)
        if q > 0.0:
            for i in idx:
                D[i] = min(D[i] / q, 0.4)
        qs.append(q)
    s = 0.0
    for v in D:
        s += v * v
    q = math.sqrt(s)
    out = np.array([v / q if q > 0.0 else 0.0 for v in D], np.float64).astype(np.float32)
    return out, qs[0] > 0.0 or qs[1] > 0.0


def describe_line(frame, line, bands=9, w=7):
    """One line (4 floats): dict(desc float32 [8 * bands], xy float32 [2], valid, N, S, flip)."""
    v, N, c = row_sums(frame, line[0], line[1], line[2], line[3], bands, w)
    xy = np.zeros(2, np.float32) if c is None else np.array(c, np.float64).astype(np.float32)
    if v is None:
        return dict(desc=np.zeros(8 * bands, np.float32), xy=xy, valid=0, N=0, S=0, flip=False, vmax=0)
    S = int(v[:, 0].sum() - v[:, 1].sum())
    flip = S < 0
    r = v[::-1][:, [1, 0, 3, 2]] if flip else v
    desc, valid = normalise(bands_of(r, bands, w), bands)
    return dict(desc=desc, xy=xy, valid=int(valid), N=N, S=S, flip=flip, vmax=int(v.max()))


def describe(frames, lines, counts=None, bands=9, w=7, fill=0.0, valid_fill=0):
    """A batch: frames uint8 [B, R, C], lines float32 [B, S, >= 4], counts int [B] or None (bits 25..31 ignored).
    Returns (desc float32 [B, S, 8 * bands], xy float32 [B, S, 2], valid uint8 [B, S], info), slots past a count
    filled with `fill` (valid: with valid_fill), info[b] = the written slots' dicts."""
    frames, lines = np.asarray(frames), np.asarray(lines, np.float32)
    B, S = lines.shape[0], lines.shape[1]
    desc = np.full((B, S, 8 * bands), fill, np.float32)
    xy = np.full((B, S, 2), fill, np.float32)
    valid = np.full((B, S), valid_fill, np.uint8)
    info = []
    for b in range(B):
        n = S if counts is None else min(int(counts[b]) & 0x01FFFFFF, S)
        info.append([describe_line(frames[b], lines[b, s, :4], bands, w) for s in range(n)])
        for s, d in enumerate(info[b]):
            desc[b, s], xy[b, s], valid[b, s] = d["desc"], d["xy"], d["valid"]
    return desc, xy, valid, info
