"""Frames and feature sets shared by the refinement tests (tests/test_refine_host.py on the CPU,
tests/test_gpu_refine.py and tests/test_cpp_refine.py on the GPU). Pixel centres are at integer coordinates."""
import numpy as np

ROWS, COLS = 96, 128
COUNTS = np.array([40, 17], np.int32)


def render_corners(rows, cols, corners, seed=0, noise=2.0, reach=14):
    """Two-tone (60 / 200) rotated corners (x, y, angle): opposite quadrants bright within `reach` pixels of each
    corner. 8 x supersampling, box average, 3 x 3 binomial blur, N(0, noise) noise, rounding."""
    ss = 8
    big = np.full((rows * ss, cols * ss), 60.0)
    yy, xx = np.mgrid[0:rows * ss, 0:cols * ss]
    yy, xx = (yy + 0.5) / ss - 0.5, (xx + 0.5) / ss - 0.5
    for cx, cy, ang in corners:
        dx, dy = xx - cx, yy - cy
        m = (np.abs(dx) < reach) & (np.abs(dy) < reach)
        u, v = np.cos(ang) * dx[m] + np.sin(ang) * dy[m], -np.sin(ang) * dx[m] + np.cos(ang) * dy[m]
        big[m] = np.where((u > 0) ^ (v > 0), 200.0, 60.0)
    img = big.reshape(rows, ss, cols, ss).mean((1, 3))
    p = np.pad(img, 1, mode="edge")
    k = np.array([0.25, 0.5, 0.25])
    img = sum(k[i] * k[j] * p[i:i + rows, j:j + cols] for i in range(3) for j in range(3))
    if noise:
        img = img + np.random.default_rng(seed).normal(0.0, noise, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def grid_corners(nx, ny, x0=20.0, y0=20.0, pitch=30.0, seed=1):
    """nx x ny corners on a grid, each jittered by U(-0.5, 0.5) px per axis and rotated by U(0, pi / 2)."""
    rng = np.random.default_rng(seed)
    return [(x0 + pitch * i + rng.uniform(-0.5, 0.5), y0 + pitch * j + rng.uniform(-0.5, 0.5), rng.uniform(0, np.pi / 2))
            for j in range(ny) for i in range(nx)]


def corner_scene():
    """The 100 x 130 guard scene: (frame, the 12 true corners)."""
    corners = grid_corners(4, 3)
    return render_corners(100, 130, corners), corners


def _box(a, k):
    p = np.pad(a, k // 2, mode="edge")
    c = np.cumsum(np.cumsum(np.pad(p, ((1, 0), (1, 0))), 0), 1)
    return (c[k:, k:] - c[:-k, k:] - c[k:, :-k] + c[:-k, :-k]) / (k * k)


def texture(seed, rows=ROWS, cols=COLS):
    """Noise plus blobs, the tracker tests' kind of texture."""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, 256, (rows // 8 + 1, cols // 8 + 1)).astype(np.float64)
    blobs = _box(np.kron(coarse, np.ones((8, 8)))[:rows, :cols], 7)
    fine = rng.integers(0, 256, (rows, cols)).astype(np.float64)
    return np.clip(np.rint(0.85 * blobs + 0.15 * fine), 0, 255).astype(np.uint8)


def main_frames():
    """[2, ROWS, COLS]: frame 0 rendered corners (a 4 x 3 grid from (18, 18), pitch 28), frame 1 texture; and
    frame 0's true corners."""
    corners = grid_corners(4, 3, 18.0, 18.0, 28.0, seed=2)
    return np.stack([render_corners(ROWS, COLS, corners, seed=3, reach=13), texture(7)]), corners


def main_features(corners):
    """[2, 40, 2] float32: frame 0 around its corners (integer starts, then fractional ones up to 2 px off), frame 1
    anywhere at least 12 px inside (integer and fractional)."""
    rng = np.random.default_rng(11)
    c = np.array([(x, y) for x, y, _ in corners])
    xy0 = np.concatenate([np.rint(c), np.rint(c) + [1, -1], c + rng.uniform(-2, 2, c.shape), c[:4] + rng.uniform(-1, 1, (4, 2))])
    xy1 = np.stack([rng.uniform(12, COLS - 13, 40), rng.uniform(12, ROWS - 13, 40)], -1)
    xy1[:12] = np.rint(xy1[:12])
    return np.stack([xy0, xy1]).astype(np.float32)
