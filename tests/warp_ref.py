"""numpy restatement of fd_frames_warp's contract (include/fd_hip.h): float64 ufuncs one operation at a time,
astype(float32) for the conversion, integer arithmetic for the raw bilinear sum S. The yardstick of the warp
tests: nothing of the code under test feeds it.
"""
import numpy as np

HOMOGRAPHY, CAMERA = 0, 1
PARAMS = {HOMOGRAPHY: 9, CAMERA: 22}


def camera_params_ref(new_K, K, dist, R=None):
    """The 22 doubles of FD_WARP_CAMERA from 3 x 3 intrinsics, (k1, k2, p1, p2, k3) and a rotation."""
    new_K, K = np.asarray(new_K, np.float64), np.asarray(K, np.float64)
    R = np.eye(3) if R is None else np.asarray(R, np.float64)
    d = np.zeros(5)
    d[: len(dist)] = dist
    return np.concatenate([[new_K[0, 0], new_K[1, 1], new_K[0, 2], new_K[1, 2]], R.reshape(9),
                           [K[0, 0], K[1, 1], K[0, 2], K[1, 2]], d])


def source_positions(p, model, out_rows, out_cols):
    """(sx, sy) float64 [out_rows, out_cols] of one frame's parameters p, every operation rounded once."""
    p = np.asarray(p, np.float64)
    x = np.broadcast_to(np.arange(out_cols, dtype=np.float64)[None, :], (out_rows, out_cols))
    y = np.broadcast_to(np.arange(out_rows, dtype=np.float64)[:, None], (out_rows, out_cols))
    with np.errstate(all="ignore"):
        if model == HOMOGRAPHY:
            X = (p[0] * x + p[1] * y) + p[2]
            Y = (p[3] * x + p[4] * y) + p[5]
            W = (p[6] * x + p[7] * y) + p[8]
            return X / W, Y / W
        fxn, fyn, cxn, cyn = p[0:4]
        r = p[4:13]
        fx, fy, cx, cy = p[13:17]
        k1, k2, p1, p2, k3 = p[17:22]
        a = (x - cxn) / fxn
        b = (y - cyn) / fyn
        X = (r[0] * a + r[1] * b) + r[2]
        Y = (r[3] * a + r[4] * b) + r[5]
        W = (r[6] * a + r[7] * b) + r[8]
        xn = X / W
        yn = Y / W
        q2 = xn * xn + yn * yn
        q4 = q2 * q2
        q6 = q4 * q2
        rad = ((1.0 + k1 * q2) + k2 * q4) + k3 * q6
        m = 2.0 * (xn * yn)
        xd = (xn * rad + p1 * m) + p2 * (q2 + 2.0 * (xn * xn))
        yd = (yn * rad + p1 * (q2 + 2.0 * (yn * yn))) + p2 * m
        return fx * xd + cx, fy * yd + cy


def sample(frame, sx, sy, fill):
    """(out, mask) uint8 of one frame [rows, cols] at the float64 positions (sx, sy)."""
    rows, cols = frame.shape
    with np.errstate(all="ignore"):
        px, py = sx.astype(np.float32), sy.astype(np.float32)
        has = (px >= 0) & (px <= np.float32(cols - 1)) & (py >= 0) & (py <= np.float32(rows - 1))
    px, py = np.where(has, px, np.float32(0)), np.where(has, py, np.float32(0))
    fx, fy = np.floor(px), np.floor(py)
    qx = ((px - fx) * np.float32(1024)).astype(np.int64)
    qy = ((py - fy) * np.float32(1024)).astype(np.int64)
    ix, iy = np.minimum(fx.astype(np.int64), cols - 1), np.minimum(fy.astype(np.int64), rows - 1)
    ix1, iy1 = np.minimum(ix + 1, cols - 1), np.minimum(iy + 1, rows - 1)
    f = frame.astype(np.int64)
    S = ((1024 - qx) * (1024 - qy) * f[iy, ix] + qx * (1024 - qy) * f[iy, ix1]
         + (1024 - qx) * qy * f[iy1, ix] + qx * qy * f[iy1, ix1])
    out = np.where(has, (S + (1 << 19)) >> 20, fill).astype(np.uint8)
    return out, has.astype(np.uint8)


def warp_ref(frames, params, out_shape=None, model=HOMOGRAPHY, fill=0):
    """(out, mask) uint8 [B, out_rows, out_cols] of frames uint8 [B, rows, cols]; params [P] (shared) or [B, P]."""
    frames = np.asarray(frames)
    if frames.ndim == 2:
        frames = frames[None]
    params = np.asarray(params, np.float64)
    out_rows, out_cols = frames.shape[1:] if out_shape is None else out_shape
    out = np.empty((frames.shape[0], out_rows, out_cols), np.uint8)
    mask = np.empty_like(out)
    for b in range(frames.shape[0]):
        p = params if params.ndim == 1 else params[b]
        assert p.shape == (PARAMS[model],)
        sx, sy = source_positions(p, model, out_rows, out_cols)
        out[b], mask[b] = sample(frames[b], sx, sy, fill)
    return out, mask
