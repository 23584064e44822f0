"""CPU: the numpy restatement of fd_lines_describe (tests/line_desc_ref.py) against a hand-computed case and
the properties the contract promises (endpoint order, unit norm), and the chain's sanity condition on the oracle's
lines, so that the GPU chain test (test_gpu_line_desc.py) is known not to be vacuous before it runs."""
import numpy as np

import line_desc_cases as C
import line_desc_ref as R
import match_guided_ref as GR
import nn_match_ref as NR


def test_hand_computed_step_edge():
    """16 x 16, columns >= 8 are 100; the line (8, 3) -> (8, 13); bands 1, band_width 1, so H = 1, b = 0.
    L = 10, N = 10, c = (8, 8), dL = (0, 1), n = (-1, 0), dLq = (0, 16384), nq = (-16384, 0). Sample i sits at
    x = 8, y = 8 + (i - 4.5): pixels (8, 4) .. (8, 13), all inside. gx = I(y, 9) - I(y, 7) = 100, gy = 0, so
    gp = -1638400 and gl = 0 at each: v = (0, 16384000, 0, 0), S = -16384000 < 0: flipped, r = (16384000, 0, 0, 0).
    G[0] = 1; band 0 has the one row at t = 1, l = 3: u = 49152000 = mean, std = 0. The means' norm is the mean:
    1 clamps to 0.4; the final norm is 0.4: the descriptor is (1, 0, 0, 0, 0, 0, 0, 0)."""
    f = C.step_frame()
    v, n, c = R.row_sums(f, 8, 3, 8, 13, 1, 1)
    assert n == 10 and c == (8.0, 8.0) and v.tolist() == [[0, 16384000, 0, 0]]
    d = R.describe_line(f, (8, 3, 8, 13), 1, 1)
    assert d["flip"] and d["S"] == -16384000 and d["N"] == 10 and d["valid"] == 1
    assert d["desc"].tolist() == [1, 0, 0, 0, 0, 0, 0, 0] and d["xy"].tolist() == [8, 8]
    assert R.bands_of(np.array([[16384000, 0, 0, 0]]), 1, 1) == [49152000.0, 0, 0, 0, 0, 0, 0, 0]
    back = R.describe_line(f, (8, 13, 8, 3), 1, 1)
    assert not back["flip"] and back["S"] == 16384000 and np.array_equal(back["desc"], d["desc"])
    # one row further from the edge sees nothing: a flat support region is invalid
    flat = R.describe_line(f, (12, 3, 12, 13), 1, 1)
    assert flat["valid"] == 0 and not flat["desc"].any() and flat["N"] == 10


def test_endpoint_swap_gives_identical_bits():
    f = C.noise_frame(48, 64, 11)
    lines = C.geometry_lines()
    half = len(lines) // 2
    for bands, w in ((9, 7), (2, 3), (32, 16)):
        fwd = [R.describe_line(f, l, bands, w) for l in lines[:half]]
        rev = [R.describe_line(f, l, bands, w) for l in lines[half:]]
        for a, b in zip(fwd, rev):
            assert a["S"] != 0 and a["S"] == -b["S"] and a["flip"] != b["flip"] and a["N"] == b["N"]
            assert a["valid"] == 1 and np.array_equal(a["desc"].view(np.uint32), b["desc"].view(np.uint32))
            assert np.array_equal(a["xy"].view(np.uint32), b["xy"].view(np.uint32))
        assert {a["flip"] for a in fwd} == {False, True}


def test_unit_norm_or_zero():
    f = C.noise_frame(48, 64, 12)
    f[:, 40:] = 77  # a flat part
    lines = np.concatenate([C.geometry_lines(), C.border_lines(),
                            np.array([(50, 20, 58, 20.5), (20, 20, 20.5, 20), (np.nan, 1, 5, 5), (1, 1, np.inf, 5)], np.float32)])
    desc, xy, valid, info = R.describe(f[None], lines[None])
    norms = np.sqrt((desc[0].astype(np.float64) ** 2).sum(1))
    assert set(valid[0].tolist()) == {0, 1}
    for s in range(len(lines)):
        if valid[0, s]:
            assert abs(norms[s] - 1.0) < 1e-6 and (desc[0, s] >= 0).all()
        else:
            assert not desc[0, s].any()
    assert not valid[0, -3:].any() and not xy[0, -2:].any()
    assert xy[0, -3].tolist() == [20.25, 20.0]  # shorter than a pixel: invalid, its midpoint stands


def test_chain_is_not_vacuous_on_the_oracle_lines(image_png, oracle):
    a, b = C.chain_crops(image_png)
    la, lb = (oracle.lsd_lines(x, min_length=C.CHAIN_MIN_LENGTH) for x in (a, b))
    assert (len(la), len(lb)) == (54, 39)
    da, db = R.describe(a[None], la[None]), R.describe(b[None], lb[None])
    idx, _, _ = NR.nn_match_ref(da[0], db[0], q_valid=da[2], t_valid=db[2], max_ratio=C.CHAIN_RATIO, cross_check=True)
    assert C.chain_sane(idx[0], da[1][0], db[1][0]) == (28, 26, True)
    moved = da[1] - np.array(C.CHAIN_SHIFT, np.float32)
    idx, _, _ = GR.nn_match_guided_ref(da[0], db[0], moved, db[1], C.CHAIN_RADIUS, q_valid=da[2], t_valid=db[2],
                                       max_ratio=C.CHAIN_RATIO, cross_check=True)
    assert C.chain_sane(idx[0], da[1][0], db[1][0]) == (32, 30, True)
