"""Inputs the line band descriptor's tests share (test_line_desc_host.py, test_gpu_line_desc.py,
test_cpp_line_desc.py): seeded frames, line sets, and the two crops of the detect -> describe -> match chain."""
import numpy as np

F32 = np.float32


def noise_frame(rows, cols, seed):
    return np.random.default_rng(seed).integers(0, 256, (rows, cols), dtype=np.uint8)


def step_frame(rows=16, cols=16, edge=8, level=100):
    """Columns >= edge are `level`, the others 0: a vertical step edge."""
    f = np.zeros((rows, cols), np.uint8)
    f[:, edge:] = level
    return f


def geometry_lines():
    """Lines for a 48 x 64 frame whose support regions (63 rows across at the default options) stay mostly
    inside it: horizontal, vertical, at 45 degrees and at arbitrary angles, integer and fractional endpoints,
    each also with its endpoints swapped."""
    base = [
        (10, 24, 50, 24), (12.5, 30.25, 47.75, 30.25),          # horizontal
        (32, 6, 32, 40), (20.5, 8.125, 20.5, 39.5),             # vertical
        (12, 8, 42, 38), (45.25, 9.75, 20.25, 34.75),           # 45 degrees, both diagonals
        (8, 12, 55, 31), (14.3, 40.9, 50.1, 11.2), (30.7, 5.2, 36.4, 41.9), (5.5, 20.0, 58.0, 26.5),
        (40, 20, 43, 24),                                        # short: N = 5
        (22.0, 22.0, 23.0, 22.5),                                # N == 1
    ]
    return np.array(base + [(ex, ey, sx, sy) for sx, sy, ex, ey in base], F32)


def border_lines():
    """For a 48 x 64 frame: support regions that leave it on the left, the right, the top and the bottom (the
    line itself inside), a line that crosses a corner, and a line wholly outside."""
    return np.array([(2, 10, 2, 40), (61.5, 8, 61.5, 38), (10, 1.5, 50, 1.5), (12, 46, 52, 46), (-10, -8, 30, 20),
                     (200, 100, 260, 130), (-80, 10, -40, 12)], F32)


# The chain: two crops of tests/golden/image.png (480 x 752), the second shifted by CHAIN_SHIFT (x, y) pixels,
# lsd_lines with min_length 12. On the oracle's lines and the restatement (test_line_desc_host.py): 54 and 39
# segments; nn_match with cross-check and ratio 0.8 accepts 28, 26 of them consistent with the shift; the
# guided form (radius 8 about the midpoint moved by the shift) accepts 32, 30 consistent.
CHAIN_SHAPE = (400, 560)
CHAIN_SHIFT = (40, 24)
CHAIN_MIN_LENGTH = 12.0
CHAIN_RATIO = 0.8
CHAIN_RADIUS = 8.0


def chain_crops(image):
    h, w = CHAIN_SHAPE
    dx, dy = CHAIN_SHIFT
    return np.ascontiguousarray(image[:h, :w]), np.ascontiguousarray(image[dy:dy + h, dx:dx + w])


def chain_sane(idx, q_xy, t_xy):
    """The chain's sanity condition on one frame's match indices and midpoints: (accepted, consistent, ok): at
    least 10 accepted, more than half of them joining midpoints that agree with the shift within 3 pixels."""
    acc = np.flatnonzero(idx >= 0)
    shift = np.array(CHAIN_SHIFT, F32)
    good = sum(1 for q in acc if np.abs(q_xy[q] - t_xy[idx[q]] - shift).max() <= 3.0)
    return len(acc), good, len(acc) >= 10 and 2 * good > len(acc)
