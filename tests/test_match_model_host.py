"""CPU: the model-gated matchers' rules (fd_brief_match_model / fd_nn_match_model, include/fd_hip.h) on
hand-written cases of the numpy restatement tests/match_model_ref.py, the exported symbols, the argument
errors that need no device, and the condition that keeps tests/test_gpu_match_model.py honest: on every
random fixture it uses, the gate changes the reference's answer for most queries, so a kernel that ignores
the model cannot pass there.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import match_guided_ref as G
import match_model_ref as MM
from match_guided_ref import match_guided_ref, nn_match_guided_ref
from match_model_ref import FUNDAMENTAL, HOMOGRAPHY, OPEN, match_model_ref, model_mask, nn_match_model_ref, pair_mask
from match_ref import match_ref
from nn_match_ref import nn_match_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64
NAN = float("nan")
ZERO = np.zeros(9)
# F = [t]x of a sideways translation: e = v - y, the bound t*t * 2: rows of equal y, Sampson distance |v - y| / sqrt 2
F_ROWS = np.array([0, 0, 0, 0, 0, -1, 0, 1, 0], F64)
# H = a shift by (3, -2)
H_SHIFT = np.array([1, 0, 3, 0, 1, -2, 0, 0, 1], F64)


def xy(*pairs):
    return np.array(pairs, F32).reshape(-1, 2)


def words(*rows):
    """Descriptors of 32 bits: one word each."""
    return np.array(rows, np.uint32).reshape(1, -1, 1)


def same(got, exp):
    for g, e in zip(got, exp):
        assert g.dtype == e.dtype
        assert np.array_equal(g.view(np.uint32) if g.dtype == F32 else g, e.view(np.uint32) if e.dtype == F32 else e)


def test_bound_is_inclusive_and_the_next_threshold_down_excludes():
    down = lambda t: np.nextafter(F32(t), F32(0), dtype=F32)  # noqa: E731
    # H_SHIFT sends query (5, 7) to (8, 5); train (8 + 3, 5 + 4) is exactly 5 px away: 25 <= t*t
    q, t = xy((5, 7)), xy((11, 9))
    assert model_mask(q, t, H_SHIFT, HOMOGRAPHY, F32(5.0))[0, 0]
    assert not model_mask(q, t, H_SHIFT, HOMOGRAPHY, down(5.0))[0, 0]
    # a 3 x 3 with l = (0, -1, 1) and m = (0, 0) (the gate takes any nine doubles): e = 1 - v, the bound t*t * 1;
    # train row 4 gives e*e = 9
    M = np.array([0, 0, 0, 0, 0, -1, 0, 0, 1], F64)
    q, t = xy((0, 0)), xy((0, 4))
    assert model_mask(q, t, M, FUNDAMENTAL, F32(3.0))[0, 0]
    assert not model_mask(q, t, M, FUNDAMENTAL, down(3.0))[0, 0]
    # F_ROWS, rows 4 apart: e*e = 16 against t*t * 2, and t*t = 8 has no float32 root: the two floats around
    # sqrt 8 fall on either side of the bound as their float64 squares say
    q, t = xy((5, 0)), xy((9, 4))
    up = F32(np.sqrt(8.0))
    for thr in (up, down(up), np.nextafter(up, F32(9), dtype=F32)):
        assert model_mask(q, t, F_ROWS, FUNDAMENTAL, thr)[0, 0] == (16.0 <= (F64(thr) * F64(thr)) * 2.0)
    assert model_mask(q, t, F_ROWS, FUNDAMENTAL, np.nextafter(up, F32(9), dtype=F32))[0, 0]
    assert not model_mask(q, t, F_ROWS, FUNDAMENTAL, down(down(up)))[0, 0]


def test_grouping_is_the_headers():
    """The bound's sum is (l0*l0 + l1*l1) + (m0*m0 + m1*m1) and e = (u*l0 + v*l1) + l2, in float64: a pair
    exists (found here by search over a real model) where the left-to-right sum decides otherwise."""
    M = MM.fundamental(0)
    rng = np.random.default_rng(0)
    q = rng.uniform(0, 64, (400, 2)).astype(F32)
    t = rng.uniform(0, 64, (400, 2)).astype(F32)
    x, y, u, v = (a.astype(F64) for a in (q[:, 0], q[:, 1], t[:, 0], t[:, 1]))
    l0, l1 = (M[0] * x + M[1] * y) + M[2], (M[3] * x + M[4] * y) + M[5]
    m0, m1 = (M[0] * u + M[3] * v) + M[6], (M[1] * u + M[4] * v) + M[7]
    grouped = (l0 * l0 + l1 * l1) + (m0 * m0 + m1 * m1)
    serial = ((l0 * l0 + l1 * l1) + m0 * m0) + m1 * m1
    assert (grouped != serial).any()  # the two orders differ in the last bit somewhere: the contract names one
    got = model_mask(q, t, M, FUNDAMENTAL, 1.5)
    e = (u * l0 + v * l1) + (M[6] * x + M[7] * y + M[8])
    assert np.array_equal(np.diag(got), e * e <= (F64(1.5) * F64(1.5)) * grouped)


def test_nan_position_or_model_entry_never_matches():
    t_xy = xy((0, 0), (NAN, 0), (0, NAN), (np.inf, 0), (1, 1))
    for M, kind in ((F_ROWS, FUNDAMENTAL), (H_SHIFT, HOMOGRAPHY), (ZERO, FUNDAMENTAL), (ZERO, HOMOGRAPHY)):
        for qp in ((0, 0), (NAN, 0), (0, NAN), (np.inf, 0)):
            m = model_mask(xy(qp), t_xy, M, kind, 1.0e6)[0]
            assert not m[1] and not m[2] and not m[3], (kind, qp)
            if not np.isfinite(qp).all():
                assert not m.any(), (kind, qp)
    for k in range(9):
        for M0, kind in ((F_ROWS, FUNDAMENTAL), (H_SHIFT, HOMOGRAPHY)):
            M = M0.copy()
            M[k] = NAN
            # entries that never meet the positions: F's M8 enters l2 only, every F entry enters e or the bound
            hit = model_mask(xy((3, 4)), xy((5, 6), (7, 8)), M, kind, 1.0e6)
            assert not hit.any(), (kind, k)
    q, t = words(0x0, 0x0), words(0x0, 0x1, 0x3)
    idx, dist, _ = match_model_ref(q, t, xy((0, 0), (NAN, 0)), xy((0, NAN), (0, 0), (0, 0)), F_ROWS, FUNDAMENTAL, 1.0, length=32)
    assert idx.tolist() == [[1, -1]] and dist.tolist() == [[[1, 2], [-1, -1]]]
    bad = F_ROWS.copy()
    bad[5] = NAN
    idx, dist, cnt = match_model_ref(q, t, xy((0, 0), (1, 0)), xy((0, 0), (0, 0), (0, 0)), bad, FUNDAMENTAL, 1.0, length=32)
    assert (idx == -1).all() and (dist == -1).all() and cnt.tolist() == [0]


@pytest.mark.parametrize("kind", [FUNDAMENTAL, HOMOGRAPHY])
def test_zero_model_is_the_window_alone(kind):
    c = G.brief_case(65, 257, flags=True, radius=8.0)
    kw = dict(max_distance=100, max_ratio=0.95, cross_check=True)
    got = match_model_ref(c["q"], c["t"], c["q_xy"], c["t_xy"], ZERO, kind, 0.5, 8.0, None, None, c["qv"], c["tv"], **kw)
    same(got, match_guided_ref(c["q"], c["t"], c["q_xy"], c["t_xy"], 8.0, None, None, c["qv"], c["tv"], **kw))
    c = G.nn_case(33, 65, dim=16, regime="round", flags=True)
    kw = dict(max_distance=1.5, max_ratio=0.95, cross_check=True)
    got = nn_match_model_ref(c["q"], c["t"], c["q_xy"], c["t_xy"], ZERO, kind, 0.5, 8.0, None, None, c["qv"], c["tv"], **kw)
    same(got, nn_match_guided_ref(c["q"], c["t"], c["q_xy"], c["t_xy"], 8.0, None, None, c["qv"], c["tv"], **kw))


@pytest.mark.parametrize("kind", [FUNDAMENTAL, HOMOGRAPHY])
def test_open_radius_and_zero_model_is_the_unguided_reference(kind):
    c = G.brief_case(65, 257, flags=True)
    kw = dict(max_distance=100, max_ratio=0.95, cross_check=True)
    got = match_model_ref(c["q"], c["t"], c["q_xy"], c["t_xy"], ZERO, kind, 2.0, OPEN, None, None, c["qv"], c["tv"], **kw)
    same(got, match_ref(c["q"], c["t"], None, None, c["qv"], c["tv"], **kw))
    c = G.nn_case(33, 65, dim=16, regime="round", flags=True)
    kw = dict(max_distance=1.5, max_ratio=0.95, cross_check=True)
    got = nn_match_model_ref(c["q"], c["t"], c["q_xy"], c["t_xy"], ZERO, kind, 2.0, OPEN, None, None, c["qv"], c["tv"], **kw)
    same(got, nn_match_ref(c["q"], c["t"], None, None, c["qv"], c["tv"], **kw))


def test_homography_is_directional():
    """H_SHIFT sends (5, 7) to (8, 5). The pair (query (5, 7), train (8, 5)) passes; the swapped pair does not
    (query (8, 5) goes to (11, 3)), and the cross-check's reverse search still judges (query, train)."""
    a, b = xy((5, 7)), xy((8, 5))
    assert model_mask(a, b, H_SHIFT, HOMOGRAPHY, 0.5)[0, 0] and not model_mask(b, a, H_SHIFT, HOMOGRAPHY, 0.5)[0, 0]
    # two queries, one train: train 0's best query in the reverse search is taken over the queries whose forward
    # predicate holds. Query 1 is the closer descriptor but fails the forward predicate, so query 0 is kept.
    q, t = words(0x3, 0x1), words(0x1)
    q_xy, t_xy = xy((5, 7), (8, 5)), xy((8, 5))
    idx, dist, cnt = match_model_ref(q, t, q_xy, t_xy, H_SHIFT, HOMOGRAPHY, 0.5, length=32, cross_check=True)
    assert idx.tolist() == [[0, -1]] and dist.tolist() == [[[1, -1], [-1, -1]]] and cnt.tolist() == [1]
    # a reverse search by the inverse homography would judge (train, query) pairs instead: train 0 maps back onto
    # query 0's position too, but a predicate applied to the swapped pair (query 1 at (8, 5) as the source) differs
    assert not model_mask(q_xy[1:], t_xy, H_SHIFT, HOMOGRAPHY, 0.5)[0, 0]


def test_empty_band_single_candidate_and_tie_inside():
    # F_ROWS, t = 1: the band of a query is the rows within sqrt 2 of its own
    q_xy = xy((10, 10), (10, 30), (10, 50), (10, 70))
    t_xy = xy((40, 20), (50, 10), (60, 11), (20, 30), (30, 51), (40, 49), (50, 50.5))
    q = words(0x0, 0x0, 0xFF00, 0x0)
    t = words(0x0, 0x1, 0x2, 0xFF, 0xFF01, 0xFF03, 0xFF00FF)
    m = model_mask(q_xy, t_xy, F_ROWS, FUNDAMENTAL, 1.0)
    assert m.sum(axis=1).tolist() == [2, 1, 3, 0]
    plain = match_ref(q, t, length=32)
    assert plain[0].tolist() == [[0, 0, 4, 0]]  # query 0's exact copy (train 0) lies outside its band
    # query 0: trains 1 and 2 tie inside, the lowest index wins, the ratio test rejects a tie;
    # query 1: one candidate, 8 bits away, no second: the ratio test is skipped; query 3: an empty band
    idx, dist, cnt = match_model_ref(q, t, q_xy, t_xy, F_ROWS, FUNDAMENTAL, 1.0, length=32)
    assert idx.tolist() == [[1, 3, 4, -1]] and dist.tolist() == [[[1, 1], [8, -1], [1, 2], [-1, -1]]] and cnt.tolist() == [3]
    idx, dist, cnt = match_model_ref(q, t, q_xy, t_xy, F_ROWS, FUNDAMENTAL, 1.0, length=32, max_ratio=0.6)
    assert idx.tolist() == [[-1, 3, 4, -1]] and cnt.tolist() == [2]
    d = np.array([[0, 0, 0, 0]], F32).repeat(4, 0)[None]
    td = np.array([[0, 0, 0, 0], [1, 0, 0, 0], [0, 1, 0, 0], [3, 0, 0, 0], [1, 0, 0, 0], [1, 1, 0, 0], [2, 2, 0, 0]], F32)[None]
    idx, dist, cnt = nn_match_model_ref(d, td, q_xy, t_xy, F_ROWS, FUNDAMENTAL, 1.0, max_ratio=0.9)
    assert idx.tolist() == [[-1, 3, 4, -1]]
    assert dist.tolist() == [[[1.0, 1.0], [9.0, -1.0], [1.0, 2.0], [-1.0, -1.0]]] and cnt.tolist() == [2]


@pytest.mark.parametrize("which,kind", [("brief", FUNDAMENTAL), ("brief", HOMOGRAPHY), ("nn", FUNDAMENTAL), ("nn", HOMOGRAPHY)])
def test_cross_check_equals_the_transposed_problem(which, kind):
    """q -> t is accepted under the cross-check iff t's best query over the queries whose (query, train) pair
    passes the gate is q: the transposed problem with the transposed forward mask."""
    if which == "brief":
        c = MM.brief_case(40, 60, kind=kind, threshold=4.0, length=6, flags=True, seed=5)
    else:
        c = MM.nn_case(40, 60, kind=kind, threshold=4.0, dim=8, regime="int", flags=True, seed=5)
    fwd = MM.ref(which, c)
    mask = pair_mask(c["q_xy"][0], c["t_xy"][0], c["model"][0], kind, 4.0) & c["tv"][0].astype(bool)[None] & c["qv"][0].astype(bool)[:, None]
    exp = np.full((1, 40), -1, np.int32)
    for qi, ti in enumerate(fwd[0][0]):
        if ti < 0:
            continue
        cand = np.flatnonzero(mask[:, ti])
        if which == "brief":
            back = match_ref(c["t"][:, ti:ti + 1], c["q"], t_valid=mask[:, ti].astype(np.uint8)[None], length=6)[0][0, 0]
        else:
            import nn_match_ref as R
            back = R.scan(R.distances(c["q"][0], c["t"][0])[:, ti], cand.tolist())[0]
        exp[0, qi] = ti if back == qi else -1
    got = MM.ref(which, c, cross_check=True)
    assert np.array_equal(got[0], exp) and np.array_equal(got[1], fwd[1])
    assert 0 < (exp >= 0).sum() < (fwd[0] >= 0).sum()


# ---- the honesty condition -----------------------------------------------------------------------------------------
def _plain(which, c):
    if which == "brief":
        return match_ref(c["q"], c["t"], c["qc"], c["tc"], c["qv"], c["tv"], length=c["length"])
    return nn_match_ref(c["q"], c["t"], c["qc"], c["tc"], c["qv"], c["tv"])


@pytest.mark.parametrize("kw", MM.BRIEF_CASES, ids=MM.case_id)
def test_gate_decides_the_brief_fixtures(kw):
    c = MM.brief_case(**kw)
    plain = _plain("brief", c)
    assert (plain[0] >= 0).sum() >= 1
    assert G.changed_fraction(MM.ref("brief", c), plain) > 0.75


@pytest.mark.parametrize("kw", MM.NN_CASES, ids=MM.case_id)
def test_gate_decides_the_nn_fixtures(kw):
    c = MM.nn_case(**kw)
    plain = _plain("nn", c)
    assert (plain[0] >= 0).sum() >= 1
    assert G.changed_fraction(MM.ref("nn", c), plain) > 0.75


def test_fixtures_have_every_kind_of_band():
    """Over the fixture sets: gates that are empty, hold exactly one candidate, and hold several; per kind."""
    for cases, make in ((MM.BRIEF_CASES, MM.brief_case), (MM.NN_CASES, MM.nn_case)):
        kinds = {FUNDAMENTAL: set(), HOMOGRAPHY: set()}
        for kw in cases:
            c = make(**kw)
            if not np.isfinite(c["model"][0]).all():
                continue
            n = pair_mask(c["q_xy"][0], c["t_xy"][0], c["model"][0], c["kind"], c["threshold"], c["radius"]).sum(axis=1)
            kinds[c["kind"]] |= {min(int(k), 2) for k in n}
        assert kinds == {FUNDAMENTAL: {0, 1, 2}, HOMOGRAPHY: {0, 1, 2}}


def test_second_pass_recovers_what_the_first_pass_lost():
    """The chain's fixture (tests/test_gpu_match_model.py::test_device_chain) allows a gain: under the scene's own
    homography the model-gated pass accepts strictly more matches than the first pass, all of them true pairs."""
    s = MM.two_view_scene()
    kw = dict(max_ratio=0.8, cross_check=True)
    first = match_ref(s["q"], s["t"], **kw)
    second = match_model_ref(s["q"], s["t"], s["q_xy"], s["t_xy"], s["H"], HOMOGRAPHY, 2.0, **kw)
    n = s["n"]
    assert int(first[2][0]) <= n - n // 3 and int(second[2][0]) > int(first[2][0])
    assert int(second[2][0]) >= n - 2
    hit = second[0][0] >= 0
    assert np.array_equal(second[0][0][hit], s["perm"][:n][hit])


# ---- the libraries and the binding, without a device -----------------------------------------------------------
def test_both_libraries_export_the_model_entries():
    import feature_detector_amd as fd
    from feature_detector_amd import _lib

    L = fd.load()
    assert hasattr(L, "fd_brief_match_model") and hasattr(L, "fd_nn_match_model")
    assert L.fd_abi_version() == 6
    assert ctypes.sizeof(_lib.fd_match_model_gate) == 16
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "feature_detector_amd", "api")])
    lib = os.path.join(ROOT, "feature_detector_amd", "lib", "libfeature_detector.so")
    nm = subprocess.run(["nm", "-DC", lib], capture_output=True, text=True).stdout
    assert "feature_detector::BriefMatcher::MatchModel" in nm
    assert "feature_detector::NNDescriptorMatcher::MatchModel" in nm


def test_null_context_is_invalid():
    import feature_detector_amd as fd
    from feature_detector_amd import _lib

    L = fd.load()
    gate = _lib.fd_match_model_gate(0, 1.0, 3.0e38, 3.0e38)
    z = np.zeros((1, 4, 8), np.uint32)
    p = xy(*[(0, 0)] * 4)
    m = np.zeros(9)
    idx = np.zeros((1, 4), np.int32)
    v = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    o = _lib.fd_match_opts(256, -1, 0.0, 0)
    assert L.fd_brief_match_model(None, 1, ctypes.byref(o), ctypes.byref(gate), v(m), v(z), None, None, 4, v(p), v(z), None,
                                  None, 4, v(p), v(idx), None, None, 0) == _lib.FD_ERR_INVALID
    o = _lib.fd_nn_match_opts(8, -1.0, 0.0, 0)
    assert L.fd_nn_match_model(None, 1, ctypes.byref(o), ctypes.byref(gate), v(m), v(z), None, None, 4, v(p), v(z), None, None,
                               4, v(p), v(idx), None, None, 0) == _lib.FD_ERR_INVALID


@pytest.mark.parametrize("which", ["brief", "nn"])
def test_python_model_needs_positions_and_a_known_kind(which):
    import feature_detector_amd as fd

    fn = fd.brief_match if which == "brief" else fd.nn_match
    z = np.zeros((1, 4, 8), np.uint32 if which == "brief" else F32)
    p = np.zeros((1, 4, 2), F32)
    m = np.zeros((1, 9))
    for kw in (dict(), dict(q_xy=p), dict(t_xy=p), dict(radius=2.0), dict(q_xy=p, radius=2.0)):
        with pytest.raises(ValueError, match="model-gated matching needs q_xy and t_xy"):
            fn(z, z, model=m, **kw)
    with pytest.raises(ValueError, match="model_kind"):
        fn(z, z, model=m, q_xy=p, t_xy=p, model_kind="affine")
