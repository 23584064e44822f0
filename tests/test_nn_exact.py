"""The exact NN-layer inputs and reference (tests/nn_exact.py) and the restated launch geometry
(tests/nn_geometry.py) checked on the CPU: the reference against a plain-loop restatement, the builders against
their exactness bounds, order independence of the float32 sum, the share of outputs on which the documented
rounding sequence differs from a single rounding (so that a GPU comparison can tell the two apart), the planted
special values, and the K multisets the GPU tests rely on."""
import math

import numpy as np
import pytest

import nn_exact as E
import nn_geometry as G


def loop_ref(x, wt, b, pool):
    """conv_bias_relu_ref restated with plain loops: int64 sums where the inputs are integers, Python floats
    (doubles: inf * 0 and inf - inf give NaN) otherwise."""
    n, ci, h, w = x.shape
    co = wt.shape[0]
    integral = bool(np.isfinite(x).all() and (x == np.round(x)).all() and (wt == np.round(wt)).all())
    xs = x.astype(np.int64) if integral else x.astype(np.float64)
    ws = wt.astype(np.int64) if integral else wt.astype(np.float64)
    r = np.zeros((n, co, h, w), np.float16)
    for f in range(n):
        for o in range(co):
            for y in range(h):
                for c in range(w):
                    s = 0 if integral else 0.0
                    for k in range(ci):
                        for dy in range(3):
                            for dx in range(3):
                                yy, cc = y + dy - 1, c + dx - 1
                                if 0 <= yy < h and 0 <= cc < w:
                                    s += (int if integral else float)(ws[o, k, dy, dx]) * (int if integral else float)(xs[f, k, yy, cc])
                    h1 = E.half(float(s))
                    h2 = E.half(float(h1) + float(b[o]))
                    r[f, o, y, c] = np.float16(0.0) if (math.isnan(float(h2)) or float(h2) <= 0) else h2
    if pool:
        p = np.zeros((n, co, h // 2, w // 2), np.float16)
        for y in range(h // 2):
            for c in range(w // 2):
                p[:, :, y, c] = np.maximum(np.maximum(r[:, :, 2 * y, 2 * c], r[:, :, 2 * y, 2 * c + 1]),
                                           np.maximum(r[:, :, 2 * y + 1, 2 * c], r[:, :, 2 * y + 1, 2 * c + 1]))
        r = p
    return r.view(np.uint16)


@pytest.mark.parametrize("regime,scaled", [("rounding", False), ("rounding", True), ("exact", False), ("k9", False),
                                           ("k9", True)])
def test_reference_equals_plain_loops(regime, scaled):
    x, wt, b = E.build(regime, 2, 4, 6, 8, 5, scaled)
    x, wt = x[:, :6], wt[:, :6]  # (6 input channels keep the loops short; the reference takes any count)
    for pool in (False, True):
        assert np.array_equal(E.conv_bias_relu_ref(x, wt, b, pool), loop_ref(x, wt, b, pool)), pool


def test_reference_equals_plain_loops_on_specials():
    """Around each planted value (inf * 0, inf - inf, overflow, cancellation, -0) the float64 convolution gives
    what plain double arithmetic gives."""
    for regime in ("rounding", "k9"):
        x, wt, b = E.build(regime, 3, 8, 14, 8, 9)
        E.plant_specials(x, wt, b)
        x, wt = x[:, :4], wt[:, :4]  # (the planted values sit in input channels 0 and 1)
        for pool in (False, True):
            assert np.array_equal(E.conv_bias_relu_ref(x, wt, b, pool), loop_ref(x, wt, b, pool)), (regime, pool)


@pytest.mark.parametrize("regime", ["rounding", "exact", "k9"])
def test_builders_stay_exact(regime):
    """Integer inputs inside the stated ranges, every extreme drawn, |sum| within the regime's bound and below
    2^24 in the products' unit (also for the scaled copy, whose values are the same integers times 2^-11)."""
    xmax, wmax, bmax, bunit = E.REGIMES[regime]
    x, wt, b = E.build(regime, 3, 10, 34, 64, 1)
    for a, lo, hi in ((x, 0, xmax), (wt, -wmax, wmax), (b / bunit, -bmax, bmax)):
        a = a.astype(np.float64)
        assert np.array_equal(a, np.round(a)) and a.min() >= lo and a.max() <= hi
    assert x.min() == 0 and x.max() == xmax and wt.min() == -wmax and wt.max() == wmax
    assert x.shape[1] == wt.shape[1] == (1 if regime == "k9" else 64)
    bound = 9 * x.shape[1] * xmax * wmax
    assert bound == E.SUM_BOUND[regime] < 1 << 24
    s = E.conv_sum(x, wt).numpy()
    assert np.abs(s).max() <= bound and np.array_equal(s, np.round(s))
    if regime == "exact":  # no rounding anywhere: |sum + b| < 2048
        assert bound + bmax * bunit < 2048
        assert np.array_equal(E.round_twice(s, b).astype(np.float64), s + b.astype(np.float64).reshape(1, -1, 1, 1))
    else:
        xs, ws, bs = E.build(regime, 3, 10, 34, 64, 1, scaled=True)
        k = E.X_SCALE * E.W_SCALE
        assert np.array_equal(xs.astype(np.float64), x * E.X_SCALE) and np.array_equal(ws.astype(np.float64), wt * E.W_SCALE)
        assert np.array_equal(bs.astype(np.float64), b.astype(np.float64) * k)
        assert np.array_equal(E.conv_sum(xs, ws).numpy(), s * k)
        # the same roundings at other exponents (no result is subnormal: the smallest non-zero one is 2^-11),
        # wherever the unscaled values stay below half's overflow
        fin = np.isfinite(E.half(s)) & np.isfinite(E.round_twice(s, b))
        assert fin.mean() > 0.9
        assert np.array_equal(E.round_twice(s * k, bs).astype(np.float64)[fin], E.round_twice(s, b).astype(np.float64)[fin] * k)


@pytest.mark.parametrize("regime,shape", [("rounding", (4, 10, 34)), ("k9", (4, 10, 34)), ("exact", (4, 10, 34))])
def test_float32_sum_is_order_independent(regime, shape):
    """The float32 convolution (another summation order, and FMA or not) equals the float64 one: every partial
    sum is an integer below 2^24, so any order gives the exact sum."""
    for scaled in ((False, True) if regime != "exact" else (False,)):
        x, wt, _ = E.build(regime, *shape, 64, 3, scaled)
        assert np.array_equal(E.conv_sum(x, wt, "float32").numpy().astype(np.float64), E.conv_sum(x, wt).numpy())


@pytest.mark.parametrize("n,h,w,co", [(4, 10, 34, 64), (130, 10, 34, 128)])
def test_rounding_orders_differ_often_enough(n, h, w, co):
    """In the rounding regime at least half of the outputs need the first rounding and at least 10 % differ
    between half(half(s) + b) and half(s + b) (19-22 % measured on the reference): a kernel that rounds once, or
    adds the bias first, cannot pass a bit comparison on these tensors."""
    x, wt, b, s = E.cached_case("rounding", n, h, w, 11) if co == 128 else (*E.build("rounding", n, h, w, co, 11), None)
    if s is None:
        s = E.conv_sum(x, wt).numpy()
    needs = float((E.half(s).astype(np.float64) != s).mean())
    two, one = E.round_twice(s, b), E.round_once(s, b)
    differ = float((two.view(np.uint16) != one.view(np.uint16)).mean())
    differ_out = float((E.relu_pool_bits(two, False) != E.relu_pool_bits(one, False)).mean())
    print(f"first rounding needed {needs:.3f}, orders differ {differ:.3f} (after the ReLU {differ_out:.3f})")
    assert needs >= 0.5 and differ >= 0.10
    assert differ_out >= 0.05  # (the ReLU zeroes about half of them)


def test_k9_rounding_orders_differ():
    x, wt, b = E.build("k9", 3, 3, 257, 64, 2)
    s = E.conv_sum(x, wt).numpy()
    differ = float((E.round_twice(s, b).view(np.uint16) != E.round_once(s, b).view(np.uint16)).mean())
    print(f"K9 regime: orders differ {differ:.3f}")
    assert differ >= 0.05


@pytest.mark.parametrize("regime", ["rounding", "k9"])
def test_planted_values(regime):
    x, wt, b = E.build(regime, 3, 8, 14, 8, 4)
    at = E.plant_specials(x, wt, b)
    s = E.conv_sum(x, wt).numpy()
    h1, h2 = E.half(s), E.round_twice(s, b)
    out = E.conv_bias_relu_ref(x, wt, b, False, s)
    assert s[at["pos_inf"]] == E.SUM_BOUND[regime] and h1[at["pos_inf"]] == np.inf
    assert out[at["pos_inf"]] == 0x7C00  # +inf passes the ReLU
    assert s[at["neg_inf"]] == -E.SUM_BOUND[regime] and h1[at["neg_inf"]] == -np.inf and out[at["neg_inf"]] == 0
    f, c, y, xx = at["nan_zero"]
    assert np.isnan(s[f, c, y, xx]) and s[f, c, y, xx - 1] == np.inf and s[f, c, y, xx - 2] == -np.inf
    assert out[f, c, y, xx] == 0 and out[f, c, y, xx - 1] == 0x7C00 and out[f, c, y, xx - 2] == 0
    assert np.isnan(s[at["nan_cancel"]]) and np.isnan(h2[at["nan_cancel"]]) and out[at["nan_cancel"]] == 0
    assert s[at["cancel"]] == -float(b[at["cancel"][1]]) != 0 and h2.view(np.uint16)[at["cancel"]] == 0
    assert s[at["neg_zero"]] == -2.0 ** -28 and h1.view(np.uint16)[at["neg_zero"]] == 0x8000
    assert h2.view(np.uint16)[at["neg_zero"]] == 0x8000 and out[at["neg_zero"]] == 0  # -0 before the ReLU, +0 after
    assert not (out & 0x8000).any()
    pooled = E.conv_bias_relu_ref(x, wt, b, True, s)
    assert not (pooled & 0x8000).any() and not np.isnan(pooled.view(np.float16)).any()
    assert pooled[0, 0, 1, 1] == 0x7C00


def test_bias_relu_rule():
    x = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 3.0, -3.0, 65504.0], np.float16).reshape(1, 8, 1, 1)
    x = np.ascontiguousarray(np.broadcast_to(x, (1, 8, 2, 2)))
    got = E.bias_relu_ref(x, np.array([1, 1, 1, -0.0, -0.0, -3, 3, 65504], np.float16))
    assert got[0, :, 0, 0].tolist() == [0, 0x7C00, 0, 0, 0, 0, 0, 0x7C00]


def test_k10_depth_multisets():
    """The pipeline depths the GPU tests assert: one-tile frames at each tile count, the ragged multi-tile
    frames, and the lone 24 x 96 frame."""
    one = lambda t: G.k10_depth_counts(t, 8, 32)
    assert one(1) == {1: 1} and one(2) == {1: 2} and one(255) == {1: 255} and one(256) == {1: 256}
    assert one(257) == {2: 1, 1: 255} and G.k10_depths(257, 8, 32)[0] == 2
    assert one(512) == {2: 256} and one(513) == {3: 1, 2: 255} and one(769) == {4: 1, 3: 255}
    assert one(1025) == {5: 1, 4: 255} and one(1537) == {7: 1, 6: 255}
    for h, w in ((6, 18), (2, 2), (1, 1), (5, 17)):
        assert G.k10_tiles(3, h, w) == (1, 1, 3)
    # the XCD remap is a permutation of the 256 first tiles, and switches on at 256 tiles only
    assert sorted(G.k10_first_tile(b, 256) for b in range(256)) == list(range(256))
    assert [G.k10_first_tile(b, 255) for b in (0, 1, 8, 254)] == [0, 1, 8, 254]
    assert [G.k10_first_tile(b, 256) for b in (0, 1, 8, 255)] == [0, 32, 1, 255]
    for n, h, w, tiles in ((130, 9, 33, 520), (130, 10, 34, 520), (130, 16, 64, 520), (60, 17, 65, 540), (60, 18, 66, 540)):
        assert G.k10_tiles(n, h, w)[2] == tiles and set(G.k10_depth_counts(n, h, w)) == {2, 3}
    assert G.k10_tiles(1, 24, 96) == (3, 3, 9) and G.k10_depth_counts(1, 24, 96) == {1: 9}
    # the existing tolerance test's shapes reach K = 1, 4 and 5 only
    assert set(G.k10_depth_counts(1, 480, 640)) == {4, 5} and set(G.k10_depth_counts(2, 120, 160)) == {1}


def test_other_geometry():
    assert G.k9_geometry(1, 480, 640, 64) == dict(grid=480, trips=1, per=32, steps=20)
    assert G.k9_geometry(2800, 3, 5, 8) == dict(grid=8192, trips=2, per=256, steps=1)
    assert [G.k9_geometry(1, 1, 257, c)["per"] for c in G.K9_CHANNELS] == [256, 128, 64, 32, 16, 8]
    assert G.bias_relu_geometry(3, 34, 50, 256, False)["trips"] == 1
    assert G.bias_relu_geometry(1, 2050, 2050, 8, False) == dict(vectors=4202500, grid=16384, trips=2)
    assert G.bias_relu_geometry(1, 4100, 4100, 8, True) == dict(vectors=4202500, grid=16384, trips=2)
    assert G.bias_relu_geometry(1, 2048, 2048, 8, False)["trips"] == 1
    assert [G.heat_groups(wc) for wc in (31, 32, 33, 65)] == [(1, 31), (1, 32), (2, 1), (3, 1)]
    assert [(G.desc_geometry(10, c)["span"], G.desc_geometry(10, c)["rounds"]) for c in (8, 128, 256, 512, 1024)] == \
        [(8, 1), (16, 1), (32, 1), (64, 1), (64, 2)]
    assert G.desc_geometry(37, 8) == dict(span=8, per_wave=8, rounds=1, waves=5, idle=3)
