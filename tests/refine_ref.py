"""numpy restatement of fd_points_refine as include/fd_hip.h states it: the yardstick of
tests/test_refine_host.py, tests/test_gpu_refine.py and tests/test_cpp_refine.py.

Written unlike the kernel on purpose: one feature at a time, a plain loop over the iterations, whole windows
as int64 arrays summed into Python ints, np.float32 scalars for the float steps and Python floats for the
double steps.
"""
import numpy as np

f32 = np.float32

ST_INVALID, ST_REFINED, ST_OUTSIDE, ST_FLAT, ST_DIVERGED = 0, 1, 2, 3, 4


def _raw_sum(img, x, y, us, vs):
    """S(u, v) of the contract at the float position (x, y) for the integer arrays us, vs; img int64 [rows, cols]."""
    rows, cols = img.shape
    fx, fy = np.floor(x), np.floor(y)
    ix, iy = int(fx), int(fy)
    qx, qy = int(f32(f32(x - fx) * f32(1024.0))), int(f32(f32(y - fy) * f32(1024.0)))

    def at(yy, xx):
        return img[np.clip(yy, 0, rows - 1), np.clip(xx, 0, cols - 1)]

    xx, yy = ix + us, iy + vs
    return ((1024 - qx) * (1024 - qy) * at(yy, xx) + qx * (1024 - qy) * at(yy, xx + 1)
            + (1024 - qx) * qy * at(yy + 1, xx) + qx * qy * at(yy + 1, xx + 1))


def _inside(x, y, rows, cols):
    return bool(f32(0) <= x <= f32(cols - 1) and f32(0) <= y <= f32(rows - 1))  # (False on NaN)


def refine_one(img, xy, r, max_iters, epsilon, min_eigen, max_shift, trace=None):
    """One feature on img (int64 [rows, cols]). Returns (out_xy float32 [2], status). trace (a list) receives
    per iteration ((G11, G12, G22, B1, B2) as Python ints, the largest |single term| of the five sums)."""
    rows, cols = img.shape
    with np.errstate(all="ignore"):
        x, y = f32(xy[0]), f32(xy[1])
        back = np.array([x, y], f32)
        if not (np.isfinite(x) and np.isfinite(y) and _inside(x, y, rows, cols)):
            return back, ST_OUTSIDE
        vs, us = np.meshgrid(np.arange(-r, r + 1, dtype=np.int64), np.arange(-r, r + 1, dtype=np.int64), indexing="ij")
        w = (r + 1 - np.abs(us)) * (r + 1 - np.abs(vs))
        assert int(w.sum()) == (r + 1) ** 4
        tau = float(f32(min_eigen)) * 1024.0 * float((r + 1) ** 4)
        eps2 = f32(f32(epsilon) * f32(epsilon))
        shift = f32(max_shift)
        cx, cy = x, y
        for _ in range(max_iters):
            if not _inside(cx, cy, rows, cols):
                return back, ST_OUTSIDE
            gx = (_raw_sum(img, cx, cy, us + 1, vs) - _raw_sum(img, cx, cy, us - 1, vs) + 2 ** 15) >> 16
            gy = (_raw_sum(img, cx, cy, us, vs + 1) - _raw_sum(img, cx, cy, us, vs - 1) + 2 ** 15) >> 16
            terms = (w * gx * gx, w * gx * gy, w * gy * gy, w * (gx * gx * us + gx * gy * vs), w * (gx * gy * us + gy * gy * vs))
            i11, i12, i22, ib1, ib2 = (int(t.sum()) for t in terms)  # int64: every total is below 2^42
            if trace is not None:
                trace.append(((i11, i12, i22, ib1, ib2), max(int(np.abs(t).max()) for t in terms)))
            g11, g12, g22, b1, b2 = float(i11), float(i12), float(i22), float(ib1), float(ib2)
            e11, e22 = g11 - tau, g22 - tau
            det = g11 * g22 - g12 * g12
            if not (det > 0 and e11 > 0 and e22 > 0 and e11 * e22 - g12 * g12 >= 0):
                return back, ST_FLAT
            sx = (g22 * b1 - g12 * b2) / det
            sy = (g11 * b2 - g12 * b1) / det
            fx, fy = f32(sx), f32(sy)
            cx, cy = f32(cx + fx), f32(cy + fy)
            if not (np.abs(f32(cx - x)) <= shift and np.abs(f32(cy - y)) <= shift):
                return back, ST_DIVERGED
            if f32(f32(fx * fx) + f32(fy * fy)) <= eps2:
                break
        return np.array([cx, cy], f32), ST_REFINED


def refine_ref(frames, xy, counts=None, valid=None, half_window=5, max_iters=20, epsilon=0.01, min_eigen=1e-3,
               max_shift=None, init=None):
    """fd_points_refine for a frame batch uint8 [B, rows, cols] and xy float32 [B, S, 2]. Returns (out_xy [B, S, 2]
    float32, status [B, S] uint8, counts [B] int32); slots the call does not write keep `init` = (xy, status)
    arrays (default: zeros)."""
    frames = np.asarray(frames, np.uint8)
    if frames.ndim == 2:
        frames = frames[None]
    xy = np.asarray(xy, np.float32)
    if xy.ndim == 2:
        xy = xy[None]
    b, s = xy.shape[:2]
    if init is None:
        o_xy, o_st = np.zeros((b, s, 2), f32), np.zeros((b, s), np.uint8)
    else:
        o_xy, o_st = (np.array(a, copy=True) for a in init)
    o_cnt = np.zeros(b, np.int32)
    shift = float(half_window) if max_shift is None else max_shift
    for f in range(b):
        img = frames[f].astype(np.int64)
        n = s if counts is None else min(int(np.uint32(counts[f]) & np.uint32(0x01FFFFFF)), s)
        for i in range(n):
            if valid is not None and not valid[f][i]:
                o_xy[f, i], o_st[f, i] = xy[f, i], ST_INVALID
                continue
            o_xy[f, i], o_st[f, i] = refine_one(img, xy[f, i], half_window, max_iters, epsilon, min_eigen, shift)
            o_cnt[f] += o_st[f, i] == ST_REFINED
    return o_xy, o_st, o_cnt
