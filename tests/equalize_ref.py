"""numpy restatement of fd_frames_equalize's contract (include/fd_hip.h), the yardstick of the equalization
tests: tile edges, per-tile histogram, clip and single redistribution pass, LUT, separable 1/1024 blend. Written
from the header text, tile by tile and with Python integers where a product could overflow; it shares nothing
with the kernels."""
import numpy as np


def edges(n, tiles):
    return [(i * n) // tiles for i in range(tiles + 1)]


def tile_lut(tile, clip_milli):
    """(lut uint8 [256], info) of one tile's pixels; info = dict(A, lim, E, r) (lim None without clipping)."""
    A = int(tile.size)
    h = np.bincount(tile.reshape(-1), minlength=256).astype(np.int64)
    lim, E, r = None, 0, 0
    if clip_milli > 0:
        lim = max(1, (int(clip_milli) * A) // 256000)
        E = int(np.maximum(h - lim, 0).sum())
        h = np.minimum(h, lim) + E // 256
        r = E % 256
        if r > 0:
            step = 256 // r
            v = np.arange(256)
            h = h + ((v % step == 0) & (v // step < r))
    assert int(h.sum()) == A
    cdf = np.cumsum(h)
    lut = (cdf * 255 + A // 2) // A
    return lut.astype(np.uint8), dict(A=A, lim=lim, E=E, r=r)


def axis_table(n, tiles):
    """(i0, i1, f) arrays over the n pixels of an axis."""
    e = edges(n, tiles)
    c2 = [e[i] + e[i + 1] for i in range(tiles)]
    i0, i1, f = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    for x in range(n):
        p = 2 * x + 1
        if p < c2[0]:
            continue
        if p >= c2[tiles - 1]:
            i0[x] = i1[x] = tiles - 1
            continue
        i = max(k for k in range(tiles) if c2[k] <= p)
        i0[x], i1[x] = i, i + 1
        f[x] = ((p - c2[i]) * 1024) // (c2[i + 1] - c2[i])
        assert 0 <= f[x] < 1024
    return i0, i1, f


def frame_luts(frame, tiles_x, tiles_y, clip_milli):
    """(luts uint8 [tiles_y, tiles_x, 256], infos [tiles_y][tiles_x]) of one frame."""
    rows, cols = frame.shape
    ex, ey = edges(cols, tiles_x), edges(rows, tiles_y)
    luts = np.zeros((tiles_y, tiles_x, 256), np.uint8)
    infos = []
    for j in range(tiles_y):
        infos.append([])
        for i in range(tiles_x):
            luts[j, i], info = tile_lut(frame[ey[j]:ey[j + 1], ex[i]:ex[i + 1]], clip_milli)
            infos[-1].append(info)
    return luts, infos


def equalize_ref(frames, tiles=(8, 8), clip_milli=3000, with_info=False):
    """out uint8 of the frames' shape ([B, H, W] or [H, W]); with_info: (out, infos [B][tiles_y][tiles_x])."""
    frames = np.asarray(frames)
    assert frames.dtype == np.uint8
    batch = frames if frames.ndim == 3 else frames[None]
    tiles_x, tiles_y = (tiles, tiles) if isinstance(tiles, int) else tiles
    _, rows, cols = batch.shape
    assert 1 <= tiles_x <= min(32, cols) and 1 <= tiles_y <= min(32, rows) and clip_milli >= 0
    i0, i1, fx = axis_table(cols, tiles_x)
    j0, j1, fy = axis_table(rows, tiles_y)
    out = np.zeros_like(batch)
    infos = []
    for b, frame in enumerate(batch):
        luts, info = frame_luts(frame, tiles_x, tiles_y, clip_milli)
        infos.append(info)
        L = luts.astype(np.int64)
        v = frame.astype(np.int64)
        J0, J1, I0, I1 = j0[:, None], j1[:, None], i0[None, :], i1[None, :]
        FX, FY = fx[None, :], fy[:, None]
        top = L[J0, I0, v] * (1024 - FX) + L[J0, I1, v] * FX
        bot = L[J1, I0, v] * (1024 - FX) + L[J1, I1, v] * FX
        s = top * (1024 - FY) + bot * FY + (1 << 19)
        assert s.max() < 1 << 32
        out[b] = (s >> 20).astype(np.uint8)
    out = out if frames.ndim == 3 else out[0]
    return (out, infos) if with_info else out
