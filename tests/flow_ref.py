"""numpy restatement of fd_pyr_build / fd_flow_lk as include/fd_hip.h states them: the yardstick of
tests/test_flow_host.py, tests/test_gpu_flow.py and tests/test_cpp_flow.py.

Written unlike the kernel on purpose: one feature at a time, plain loops over levels and iterations, whole
windows as int64 arrays, np.float32 scalars for the float steps and Python floats for the double steps.
"""
import numpy as np

f32 = np.float32

ST_INVALID, ST_TRACKED, ST_OUT_OF_FRAME, ST_FLAT, ST_STEP, ST_FB, ST_ERROR = 0, 1, 2, 3, 4, 5, 6


def pyr_layout(batch, rows, cols, levels):
    """Byte offsets of the levels in the packed pyramid; the last entry is the size of the whole."""
    off = [0]
    for l in range(levels):
        end = off[-1] + batch * (rows >> l) * (cols >> l)
        off.append((end + 255) // 256 * 256)
    return off


def pyr_ref(frames, levels):
    """frames uint8 [B, rows, cols] -> list of `levels` uint8 arrays [B, rows >> l, cols >> l]."""
    frames = np.asarray(frames, np.uint8)
    if frames.ndim == 2:
        frames = frames[None]
    out = [frames.copy()]
    for _ in range(1, levels):
        a = out[-1].astype(np.int64)
        r, c = a.shape[1] >> 1, a.shape[2] >> 1
        a = a[:, :2 * r, :2 * c]
        s = a[:, 0::2, 0::2] + a[:, 0::2, 1::2] + a[:, 1::2, 0::2] + a[:, 1::2, 1::2]
        out.append(((s + 2) >> 2).astype(np.uint8))
    return out


def pyr_pack(levels_list):
    """The packed byte image of a pyramid (padding bytes 0)."""
    b, rows, cols = levels_list[0].shape
    off = pyr_layout(b, rows, cols, len(levels_list))
    buf = np.zeros(off[-1], np.uint8)
    for l, a in enumerate(levels_list):
        buf[off[l]:off[l] + a.size] = a.reshape(-1)
    return buf


def _raw_sum(img, x, y, us, vs):
    """S(u, v) of the contract for every (u, v) of the integer arrays us, vs; img int64 [rows, cols]."""
    rows, cols = img.shape
    fx, fy = np.floor(x), np.floor(y)
    ix, iy = int(fx), int(fy)
    qx, qy = int(f32(f32(x - fx) * f32(1024.0))), int(f32(f32(y - fy) * f32(1024.0)))

    def at(yy, xx):
        return img[np.clip(yy, 0, rows - 1), np.clip(xx, 0, cols - 1)]

    xx, yy = ix + us, iy + vs
    return ((1024 - qx) * (1024 - qy) * at(yy, xx) + qx * (1024 - qy) * at(yy, xx + 1)
            + (1024 - qx) * qy * at(yy + 1, xx) + qx * qy * at(yy + 1, xx + 1))


def _finite(v):
    return bool(np.isfinite(v))


def track_one(prev_levels, next_levels, xy, guess, rows, cols, r, max_iters, epsilon, min_eigen, max_error, trace=None):
    """One feature through the forward tracker. prev_levels / next_levels: int64 [rows_l, cols_l] per level.
    Returns (out_xy float32 [2], status, err float32). trace (a list) receives (level, usable, iterations)."""
    with np.errstate(all="ignore"):
        x, y = f32(xy[0]), f32(xy[1])
        lost = (np.array([x, y], f32), f32(-1.0))
        if not (_finite(x) and _finite(y) and f32(0) <= x <= f32(cols - 1) and f32(0) <= y <= f32(rows - 1)):
            return lost[0], ST_OUT_OF_FRAME, lost[1]
        levels = len(prev_levels)
        top = levels - 1
        n = (2 * r + 1) ** 2
        vs, us = np.meshgrid(np.arange(-r, r + 1), np.arange(-r, r + 1), indexing="ij")
        dx = dy = f32(0.0)
        if guess is not None:
            dx = f32(f32(f32(guess[0]) - x) * f32(2.0 ** -top))
            dy = f32(f32(f32(guess[1]) - y) * f32(2.0 ** -top))
        eps2 = f32(f32(epsilon) * f32(epsilon))
        tau = float(f32(min_eigen)) * 1024.0 * n
        e_sum = -1
        for l in range(top, -1, -1):
            prev, nxt = prev_levels[l], next_levels[l]
            px, py = f32(x * f32(2.0 ** -l)), f32(y * f32(2.0 ** -l))
            iq = (_raw_sum(prev, px, py, us, vs) + 2 ** 14) >> 15
            gx = (_raw_sum(prev, px, py, us + 1, vs) - _raw_sum(prev, px, py, us - 1, vs) + 2 ** 15) >> 16
            gy = (_raw_sum(prev, px, py, us, vs + 1) - _raw_sum(prev, px, py, us, vs - 1) + 2 ** 15) >> 16
            a11, a12, a22 = float(int((gx * gx).sum())), float(int((gx * gy).sum())), float(int((gy * gy).sum()))
            e11, e22 = a11 - tau, a22 - tau
            det = a11 * a22 - a12 * a12
            usable = det > 0 and e11 > 0 and e22 > 0 and e11 * e22 - a12 * a12 >= 0
            iters = 0
            if not usable:
                if l == 0:
                    if trace is not None:
                        trace.append((l, False, 0))
                    return lost[0], ST_FLAT, lost[1]
            else:
                scale = f32(2.0 ** l)
                for _ in range(max_iters):
                    qx, qy = f32(px + dx), f32(py + dy)
                    fx0, fy0 = f32(qx * scale), f32(qy * scale)
                    if not (f32(0) <= fx0 <= f32(cols - 1) and f32(0) <= fy0 <= f32(rows - 1)):
                        return lost[0], ST_OUT_OF_FRAME, lost[1]
                    jq = (_raw_sum(nxt, qx, qy, us, vs) + 2 ** 14) >> 15
                    d = iq - jq
                    b1, b2, e_it = float(int((d * gx).sum())), float(int((d * gy).sum())), int(np.abs(d).sum())
                    if l == 0:
                        e_sum = e_it
                    iters += 1
                    sx = (a22 * b1 - a12 * b2) / det
                    sy = (a11 * b2 - a12 * b1) / det
                    fx, fy = f32(sx), f32(sy)
                    if not (_finite(fx) and _finite(fy)):
                        return lost[0], ST_STEP, lost[1]
                    dx, dy = f32(dx + fx), f32(dy + fy)
                    if f32(f32(fx * fx) + f32(fy * fy)) <= eps2:
                        break
            if trace is not None:
                trace.append((l, usable, iters))
            if l > 0:
                dx, dy = f32(dx * f32(2.0)), f32(dy * f32(2.0))
        out = np.array([f32(x + dx), f32(y + dy)], f32)
        err = f32(float(e_sum) / (32.0 * n))
        if f32(max_error) >= 0 and err > f32(max_error):
            return out, ST_ERROR, err
        return out, ST_TRACKED, err


def _levels_i64(frames, levels):
    return [[a[b].astype(np.int64) for a in pyr_ref(frames, levels)] for b in range(np.asarray(frames).shape[0])]


def flow_ref(prev, nxt, xy, counts=None, valid=None, guess=None, levels=3, half_window=7, max_iters=30, epsilon=0.01,
             min_eigen=1e-3, fb_max_dist=-1.0, max_error=-1.0, init=None):
    """fd_flow_lk for frame batches prev / nxt uint8 [B, rows, cols] and xy float32 [B, S, 2].
    Returns (out_xy [B, S, 2] float32, status [B, S] uint8, err [B, S] float32, counts [B] int32); slots the
    call does not write keep `init` = (xy, status, err) arrays (default: zeros)."""
    prev, nxt = np.asarray(prev, np.uint8), np.asarray(nxt, np.uint8)
    if prev.ndim == 2:
        prev, nxt = prev[None], nxt[None]
    xy = np.asarray(xy, np.float32)
    if xy.ndim == 2:
        xy = xy[None]
    b, s = xy.shape[:2]
    rows, cols = prev.shape[1:]
    if init is None:
        o_xy, o_st, o_err = np.zeros((b, s, 2), f32), np.zeros((b, s), np.uint8), np.zeros((b, s), f32)
    else:
        o_xy, o_st, o_err = (np.array(a, copy=True) for a in init)
    o_cnt = np.zeros(b, np.int32)
    pl, nl = _levels_i64(prev, levels), _levels_i64(nxt, levels)
    kw = dict(rows=rows, cols=cols, r=half_window, max_iters=max_iters, epsilon=epsilon, min_eigen=min_eigen)
    fb = f32(fb_max_dist)
    for f in range(b):
        n = s if counts is None else min(int(np.uint32(counts[f]) & np.uint32(0x01FFFFFF)), s)
        for i in range(n):
            if valid is not None and not valid[f][i]:
                o_xy[f, i], o_st[f, i] = xy[f, i], ST_INVALID
                continue
            g = None if guess is None else guess[f][i]
            out, st, err = track_one(pl[f], nl[f], xy[f, i], g, max_error=max_error, **kw)
            if st == ST_TRACKED and fb >= 0:
                back, bst, _ = track_one(nl[f], pl[f], out, xy[f, i], max_error=-1.0, **kw)
                with np.errstate(all="ignore"):
                    bx, by = f32(back[0] - xy[f, i, 0]), f32(back[1] - xy[f, i, 1])
                    if bst != ST_TRACKED or f32(f32(bx * bx) + f32(by * by)) > f32(fb * fb):
                        st = ST_FB
            o_xy[f, i], o_st[f, i], o_err[f, i] = out, st, err
            o_cnt[f] += st == ST_TRACKED
    return o_xy, o_st, o_err, o_cnt
