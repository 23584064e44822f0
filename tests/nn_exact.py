"""Exact inputs and the exact reference for the SuperPoint layer kernels (K9 k_conv3x3_c1_bias_relu, K10
k_conv3x3_c64_pp, k_bias_relu / k_bias_relu_pool), on the CPU.

The builders give seeded integer-valued fp16 tensors whose products are integers times one power of two with
|sum| < 2^24 in those units, so every float32 sum is exact in any order and the kernels' documented rounding
sequence -- half(sum), then half(half(sum) + bias), then the ReLU (a NaN gives +0, so does -0) and the 2x2 max
pool -- has one right answer per output, compared on bit patterns. Subnormal halves are out of scope."""
import functools

import numpy as np

REGIMES = {  # name: (x high (0..), |w| max, bias integer range, bias unit)
    "rounding": (63, 31, 2048, 16),  # |sum| <= 576 * 63 * 31 = 1,124,928: most sums need the half rounding
    "exact": (2, 1, 8, 1),           # |sum + b| < 2048: no rounding at all (the permutation check)
    "k9": (255, 31, 2048, 16),       # one input channel: |sum| <= 9 * 255 * 31 = 71,145
}
SUM_BOUND = {"rounding": 576 * 63 * 31, "exact": 576 * 2 * 1, "k9": 9 * 255 * 31}
X_SCALE, W_SCALE = 2.0 ** -6, 2.0 ** -5  # the scaled copies: other exponents, still exact
TINY = 2.0 ** -14  # the smallest normal half: TINY * -TINY = -2^-28 rounds to -0 in half


def build(regime, n, h, w, co, seed, scaled=False):
    """(x [n, ci, h, w], weight [co, ci, 3, 3], bias [co]) as float16 arrays; ci = 1 for "k9", else 64."""
    xmax, wmax, bmax, bunit = REGIMES[regime]
    ci = 1 if regime == "k9" else 64
    rng = np.random.default_rng(seed)
    x = rng.integers(0, xmax + 1, (n, ci, h, w)).astype(np.float64)
    wt = rng.integers(-wmax, wmax + 1, (co, ci, 3, 3)).astype(np.float64)
    b = rng.integers(-bmax, bmax + 1, co).astype(np.float64) * bunit
    if scaled:
        assert regime != "exact"
        x, wt, b = x * X_SCALE, wt * W_SCALE, b * (X_SCALE * W_SCALE)
    out = tuple(a.astype(np.float16) for a in (x, wt, b))
    assert all(np.array_equal(a, o.astype(np.float64)) for a, o in zip((x, wt, b), out))  # (every value is a half)
    return out


def plant_specials(x, wt, b):
    """Plant the special values into an unscaled rounding-regime (or K9) case, in place: n >= 3 frames of at
    least 7 x 14, co >= 8. Returns {name: (frame, channel, y, x)} of the outputs the values are planted for:
      pos_inf / neg_inf   a 3x3 block of the largest x under an all-(+max) / all-(-max) filter: the sum overflows half
      nan_zero            a +inf pixel under a zero weight (inf * 0), beside weights of both signs (+inf, -inf)
      nan_cancel          two +inf inputs under weights of opposite sign (inf - inf)
      cancel              a sum of exactly -bias: +0 before the ReLU
      neg_zero            the product TINY * -TINY = -2^-28 alone in its window, bias -0: a -0 reaches the ReLU"""
    n, ci, h, w = x.shape
    co = wt.shape[0]
    assert n >= 3 and h >= 7 and w >= 14 and co >= 8
    xmax, wmax = float(x[np.isfinite(x)].max()), float(np.abs(wt).max())
    at = {}
    x[0, :, 1:4, 1:4] = xmax
    wt[0], wt[1] = wmax, -wmax
    at["pos_inf"], at["neg_inf"] = (0, 0, 2, 2), (0, 1, 2, 2)
    # frame 1: +inf at (3, 5) (and, for inf - inf, a second one: the next channel, or the next pixel for K9).
    # Output (3, 6) has it under tap (1, 0), weight 0 in filter 2; outputs (3, 5) and (3, 4) under +5 and -5.
    x[1, 0, 3, 5] = np.inf
    wt[2, 0] = np.array([[3, -3, 0], [0, 5, -5], [-7, 0, 7]], wt.dtype)
    at["nan_zero"] = (1, 2, 3, 6)
    if ci > 1:
        x[1, 1, 3, 5] = np.inf
        wt[3, 0], wt[3, 1] = 1, -1
        at["nan_cancel"] = (1, 3, 3, 5)
    else:
        x[1, 0, 5, 9] = x[1, 0, 5, 10] = np.inf
        wt[3, 0] = np.array([[1, -1, 1], [-1, 1, -1], [1, -1, 1]], wt.dtype)
        at["nan_cancel"] = (1, 3, 5, 9)  # taps (1, 1) = +1 and (1, 2) = -1 on the two infs
    # frame 2: a zero 5x5 block holding one input: every sum of its inner 3x3 is that input times one weight
    x[2, :, 1:6, 1:6] = 0
    x[2, 0, 3, 3] = 16
    wt[4, 0, 1, 1], b[4] = -3, 48
    at["cancel"] = (2, 4, 3, 3)
    x[2, :, 1:6, 8:13] = 0
    x[2, 0, 3, 10] = TINY
    wt[5] = 0  # (alone in its filter: TINY times the other inputs must not meet integer sums)
    wt[5, 0, 1, 1], b[5] = -TINY, -0.0
    at["neg_zero"] = (2, 5, 3, 10)
    return at


def conv_sum(x, wt, dtype="float64"):
    """The 3x3, padding-1 convolution's sums on the CPU, as a torch tensor [n, co, h, w] of dtype."""
    import torch

    dt = getattr(torch, dtype)
    return torch.nn.functional.conv2d(torch.from_numpy(x.astype(np.float32)).to(dt),
                                      torch.from_numpy(wt.astype(np.float32)).to(dt), None, 1, 1)


def half(a):
    """One round-to-nearest-even from float64 to half (overflow gives inf)."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(a, np.float64).astype(np.float16)


def round_twice(s, b):
    """The contract before the ReLU: h2 = half(half(s) + b), the add in float64. s [n, c, h, w], b [c]."""
    with np.errstate(invalid="ignore"):
        return half(half(s).astype(np.float64) + np.asarray(b, np.float64).reshape(1, -1, 1, 1))


def round_once(s, b):
    """What a kernel that adds the bias before its only rounding would give: half(s + b)."""
    with np.errstate(invalid="ignore"):
        return half(np.asarray(s, np.float64) + np.asarray(b, np.float64).reshape(1, -1, 1, 1))


def relu_pool_bits(h2, pool):
    """ReLU (+0 where h2 is NaN or <= 0, so a -0 gives +0) and the 2x2 max pool of the ReLU'd values (equal to
    the kernels' max-then-ReLU for everything but NaN, which counts as 0) -> uint16 bit patterns."""
    with np.errstate(invalid="ignore"):
        r = np.where(np.isnan(h2) | (h2 <= 0), np.float16(0.0), h2).astype(np.float16)
    if pool:
        n, c, h, w = r.shape
        r = r.reshape(n, c, h // 2, 2, w // 2, 2).max(axis=(3, 5))
    return np.ascontiguousarray(r).view(np.uint16)


def conv_bias_relu_ref(x, wt, b, pool=False, s=None):
    """The contract's result [n, co, h(/2), w(/2)] as uint16 half bit patterns: the exact sum (float64 conv2d
    on the CPU, or s if given), h1 = half(sum), h2 = half(h1 + b), ReLU, pool."""
    if s is None:
        s = conv_sum(x, wt).numpy()
    return relu_pool_bits(round_twice(s, b), pool)


def bias_relu_ref(x, b, pool=False):
    """fd_nn_bias_relu's rule on a half activation x [n, c, h, w]: half(x + b), ReLU, pool -> uint16 bits."""
    with np.errstate(invalid="ignore"):
        h2 = half(x.astype(np.float64) + np.asarray(b, np.float64).reshape(1, -1, 1, 1))
    return relu_pool_bits(h2, pool)


@functools.lru_cache(maxsize=4)
def cached_case(regime, n, h, w, seed, scaled=False):
    """build(..., co = 128) and its exact sums, shared by the tests of one shape (treat as read-only)."""
    x, wt, b = build(regime, n, h, w, 128, seed, scaled)
    return x, wt, b, conv_sum(x, wt).numpy()
