"""CPU: the yardstick of the float matcher tests (tests/nn_match_ref.py) checked on its own, and the one
fd_nn_match argument check that needs no context.

The other FD_ERR_INVALID cases need a context to carry the message (fd_ctx_create opens the GPU), so they
are in tests/test_gpu_nn_match.py.
"""
import ctypes

import numpy as np

import nn_match_ref as R

F32 = np.float32


def _libm_fmaf():
    m = ctypes.CDLL("libm.so.6")
    m.fmaf.restype = ctypes.c_float
    m.fmaf.argtypes = [ctypes.c_float] * 3
    return m.fmaf


def _triples():
    rng = np.random.default_rng(20261)
    parts = []
    # random mantissas over a wide exponent range, the addend near the product's magnitude or far from it
    n = 60000
    a = (rng.standard_normal(n) * np.exp2(rng.integers(-40, 40, n))).astype(F32)
    b = (rng.standard_normal(n) * np.exp2(rng.integers(-40, 40, n))).astype(F32)
    c = (a.astype(np.float64) * b * rng.standard_normal(n) * np.exp2(rng.integers(-30, 30, n))).astype(F32)
    parts.append((a, b, c))
    # cancellation: c close to -a * b
    a = rng.standard_normal(20000).astype(F32)
    b = rng.standard_normal(20000).astype(F32)
    c = (-(a * b)).astype(F32)
    parts.append((a, b, c))
    # subnormal results
    a = (rng.standard_normal(5000) * 2.0 ** -80).astype(F32)
    b = (rng.standard_normal(5000) * 2.0 ** -60).astype(F32)
    c = (rng.standard_normal(5000) * 2.0 ** -140).astype(F32)
    parts.append((a, b, c))
    # constructed halfway cases. c = +-(1 + j 2^-23) 2^e has ulp 2^(e-23); the product is half of it,
    #   exactly: a = 1, b = 2^(e-24): a * b + c is the midpoint of two floats (ties to even), or
    #   short of it by m^2 2^(e-70) (< one float64 ulp of the sum for m < 2^8): a = 1 + m 2^-23,
    #   b = (1 - 2m 2^-24) 2^(e-24), a * b = 2^(e-24) (1 - m^2 2^-46); with c of the other sign the exact sum
    #   is past the midpoint below |c| by the same amount.
    # A float64 sum rounded to nearest lands on the midpoint and the cast then ties to even: wrong for odd j.
    k = 20000
    e = rng.integers(-20, 20, k)
    j = rng.integers(0, 1 << 23, k)
    m = rng.integers(0, 200, k)  # m = 0: the exact tie
    cs = np.where(rng.random(k) < 0.5, 1.0, -1.0)
    ps = np.where(rng.random(k) < 0.5, 1.0, -1.0)
    c = (cs * (1.0 + j * 2.0 ** -23) * np.exp2(e)).astype(F32)
    a = (ps * (1.0 + m * 2.0 ** -23)).astype(F32)
    b = ((1.0 - 2.0 * m * 2.0 ** -24) * np.exp2(e - 24.0)).astype(F32)
    parts.append((a, b, c))
    return tuple(np.concatenate(x) for x in zip(*parts)), slice(-k, None)


def test_fmaf_emulation_equals_libm():
    (a, b, c), half = _triples()
    assert len(a) >= 100000
    got = R.fmaf32(a, b, c)
    fmaf = _libm_fmaf()
    exp = np.array([fmaf(x, y, z) for x, y, z in zip(a.tolist(), b.tolist(), c.tolist())], F32)
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))
    # the constructed cases do what they are for: a float64 sum cast to float32 gets some of them wrong
    naive = (a[half].astype(np.float64) * b[half] + c[half]).astype(F32)
    assert (naive.view(np.uint32) != exp[half].view(np.uint32)).sum() > 1000


def test_integer_regime_is_exact_integer_arithmetic():
    rng = np.random.default_rng(5)
    for dim in (4, 128, 256):
        q = rng.integers(-7, 8, (23, dim))
        t = rng.integers(-7, 8, (31, dim))
        exact = ((q[:, None, :] - t[None, :, :]) ** 2).sum(-1)
        assert exact.max() < 1 << 24
        D = R.distances(q.astype(F32), t.astype(F32))
        assert D.dtype == F32 and np.array_equal(D.astype(np.int64), exact)
        assert np.array_equal(R.norm_chain(q.astype(F32)).astype(np.int64), (q * q).sum(-1))


def test_distance_sequence_by_hand():
    # one pair, dim 4, worked with libm: chain order and the combine
    fmaf = _libm_fmaf()
    q = np.array([[0.1, 0.7, -0.3, 1e-3]], F32)
    t = np.array([[0.2, -0.6, 0.3, 5.0]], F32)

    def chain(x, y):
        acc = 0.0
        for k in range(4):
            acc = fmaf(float(x[k]), float(y[k]), acc)
        return F32(acc)

    d = max(F32(0.0), F32(F32(chain(q[0], q[0]) + chain(t[0], t[0])) - F32(F32(2.0) * chain(q[0], t[0]))))
    assert R.distances(q, t)[0, 0].view(np.uint32) == F32(d).view(np.uint32)


def test_scan_rules_on_hand_written_matrices():
    D = np.array([[5, 3, 3, 9],    # tie of the best: lowest index, second = best
                  [2, 2, 2, 2],    # all equal
                  [7, 1, 4, 1],    # tie later in the row
                  [8, 8, 8, 0]], F32)
    rows = R.accept_from_distances(D, [0, 1, 2, 3], [0, 1, 2, 3])
    assert [(i, float(a), float(b)) for i, a, b in rows] == [(1, 3, 3), (0, 2, 2), (1, 1, 1), (3, 0, 8)]
    # an invalid train column is no candidate; an invalid query row gets -1s
    rows = R.accept_from_distances(D, [0, 2, 3], [0, 2, 3])
    assert [(i, float(a), float(b)) for i, a, b in rows] == [(2, 3, 5), (-1, -1, -1), (3, 1, 4), (3, 0, 8)]
    # one candidate: no second, and the ratio test is skipped
    rows = R.accept_from_distances(D, [0, 1], [2], max_ratio=0.1)
    assert [(i, float(a), float(b)) for i, a, b in rows] == [(2, 3, -1), (2, 2, -1), (-1, -1, -1), (-1, -1, -1)]
    # no candidate at all
    rows = R.accept_from_distances(D, [0], [])
    assert [(i, float(a), float(b)) for i, a, b in rows][0] == (-1, -1, -1)


def test_acceptance_rules_on_hand_written_matrices():
    D = np.array([[1, 4, 9],
                  [1, 6, 2],
                  [3, 3, 0.5]], F32)
    ok = [0, 1, 2]
    idx = lambda **kw: [r[0] for r in R.accept_from_distances(D, ok, ok, **kw)]  # noqa: E731
    assert idx() == [0, 0, 2]
    assert idx(max_distance=1.0) == [0, 0, 2] and idx(max_distance=0.75) == [-1, -1, 2]
    # ratio on squared distances: d1 < r^2 d2. row 0: 1 < r^2 4 <=> r > 0.5; row 1: 1 < r^2 2; row 2: .5 < r^2 3
    assert idx(max_ratio=0.5) == [-1, -1, 2] and idx(max_ratio=0.51) == [0, -1, 2] and idx(max_ratio=0.75) == [0, 0, 2]
    # cross-check: column 0's best query is the lower of the tied rows 0 and 1; column 2's is row 2
    assert idx(cross_check=True) == [0, -1, 2]
    # all-equal matrix: every row picks column 0, column 0 picks row 0
    E = np.full((3, 3), 2, F32)
    rows = R.accept_from_distances(E, ok, ok, cross_check=True, max_ratio=1.0)
    assert [r[0] for r in rows] == [-1, -1, -1]  # d1 < 1 * d2 fails on the tie
    rows = R.accept_from_distances(E, ok, ok, cross_check=True)
    assert [r[0] for r in rows] == [0, -1, -1]


def test_geometry_helper():
    assert R.instance(4) == R.instance(128) == (128, 64) and R.instance(132) == R.instance(256) == (256, 32)
    assert [R.a_tiles(s) for s in (1, 64, 65, 128, 129)] == [1, 1, 2, 2, 3]
    assert [R.b_tiles(128, n) for n in (0, 1, 64, 65, 129)] == [0, 1, 1, 2, 3]
    assert [R.b_tiles(256, n) for n in (0, 31, 32, 33, 65)] == [0, 1, 1, 2, 3]
    assert R.k_steps(124) == (31, 32) and R.k_steps(132) == (33, 64)


def test_null_context_is_invalid():
    from feature_detector_amd import _lib

    L = _lib.load()
    z = np.zeros((1, 4, 4), F32)
    idx = np.zeros((1, 4), np.int32)
    opts = _lib.fd_nn_match_opts(4, -1.0, 0.0, 0)
    p = lambda x: ctypes.c_void_p(x.ctypes.data)  # noqa: E731
    rc = L.fd_nn_match(None, 1, ctypes.byref(opts), p(z), None, None, 4, p(z), None, None, 4, p(idx), None, None, 0)
    assert rc == _lib.FD_ERR_INVALID
