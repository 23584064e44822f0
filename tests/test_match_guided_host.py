"""CPU: the guided matchers' rules (fd_brief_match_guided / fd_nn_match_guided, include/fd_hip.h) on
hand-written cases of the numpy restatement tests/match_guided_ref.py, the exported symbols, the argument
errors that need no device, and the condition that keeps tests/test_gpu_match_guided.py honest: on every
random fixture it uses, the gate changes the reference's answer for most queries, so a kernel that
ignores the gate cannot pass there.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import match_guided_ref as G
from match_guided_ref import gate_mask, match_guided_ref, nn_match_guided_ref
from match_ref import match_ref
from nn_match_ref import nn_match_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
INF, NAN = F32(np.inf), F32(np.nan)


def xy(*pairs):
    return np.array(pairs, F32).reshape(-1, 2)


def words(*rows):
    """Descriptors of 32 bits: one word each."""
    return np.array(rows, np.uint32).reshape(1, -1, 1)


def test_bound_is_inclusive_and_the_next_float_is_outside():
    for r in (F32(3.0), F32(0.1), F32(1.0e-3), F32(2.5e7)):
        up = np.nextafter(r, INF, dtype=F32)
        q = xy((0.0, 0.0))
        t = xy((r, 0.0), (up, 0.0), (-r, 0.0), (-up, 0.0), (0.0, r), (0.0, up), (0.0, -r), (0.0, -up), (r, r), (up, r))
        assert gate_mask(q, t, r)[0].tolist() == [True, False, True, False, True, False, True, False, True, False]
    # the offset that counts is the rounded float32 difference, not the exact one: 0.1f * 3 - 0.1f * 2
    a, b = F32(0.1) * F32(3), F32(0.1) * F32(2)
    d = F32(a - b)
    assert d != F32(0.1)
    assert gate_mask(xy((b, 0)), xy((a, 0)), d)[0, 0] and not gate_mask(xy((b, 0)), xy((a, 0)), np.nextafter(d, -INF, dtype=F32))[0, 0]


def test_radius_zero_keeps_only_coincident_keypoints():
    q = xy((5, 7), (5.5, 7))
    t = xy((5, 7), (5, 7.0000005), (5.5, 7), (6, 7))
    assert gate_mask(q, t, 0.0).tolist() == [[True, False, False, False], [False, False, True, False]]
    idx, dist, cnt = match_guided_ref(words(0xF, 0xF0), words(0xFFFF, 0xF, 0xF0FF, 0xF0), q, t, 0.0, length=32)
    assert idx.tolist() == [[0, 2]] and dist.tolist() == [[[12, -1], [8, -1]]] and cnt.tolist() == [2]


def test_empty_window_is_absent_and_one_candidate_skips_the_ratio_test():
    q_xy, t_xy = xy((10, 10), (40, 40), (100, 100)), xy((11, 10), (12, 10), (41, 40))
    q, t = words(0x1, 0x1, 0x1), words(0x3, 0x7, 0xFF)
    # query 0 sees trains 0 and 1 (1 against 2: the ratio 0.4 rejects), query 1 only train 2 (no second: the
    # ratio test is skipped, and 7 bits away is accepted), query 2 nothing
    idx, dist, cnt = match_guided_ref(q, t, q_xy, t_xy, 3.0, max_ratio=0.4, length=32)
    assert idx.tolist() == [[-1, 2, -1]]
    assert dist.tolist() == [[[1, 2], [7, -1], [-1, -1]]] and cnt.tolist() == [1]
    d = np.array([[1, 0, 0, 0]], F32).repeat(3, 0)[None]
    td = np.array([[1, 1, 0, 0], [1, 2, 0, 0], [4, 0, 0, 0]], F32)[None]
    idx, dist, cnt = nn_match_guided_ref(d, td, q_xy, t_xy, 3.0, max_ratio=0.4)
    assert idx.tolist() == [[-1, 2, -1]]
    assert dist.tolist() == [[[1.0, 4.0], [9.0, -1.0], [-1.0, -1.0]]] and cnt.tolist() == [1]


def test_nan_and_inf_positions_never_match():
    t_xy = xy((0, 0), (NAN, 0), (0, NAN), (INF, 0), (-INF, 0), (0, INF), (1, 1))
    for q in ((0, 0), (NAN, 0), (0, NAN), (INF, 0), (-INF, INF), (NAN, NAN)):
        m = gate_mask(xy(q), t_xy, 3.0e38)[0].tolist()
        finite = bool(np.isfinite(q).all())
        assert m == [finite, False, False, False, False, False, finite], q
    # inf - inf is NaN: a train keypoint at +inf is not a candidate of a query at +inf
    assert not gate_mask(xy((INF, 0)), xy((INF, 0)), 3.0e38)[0, 0]
    # a query with a NaN position is absent, a train entry with one is neither best nor second
    q, t = words(0x0, 0x0), words(0x0, 0x1, 0x3)
    idx, dist, _ = match_guided_ref(q, t, xy((0, 0), (NAN, 0)), xy((0, NAN), (0, 0), (0, 0)), 1.0, length=32)
    assert idx.tolist() == [[1, -1]] and dist.tolist() == [[[1, 2], [-1, -1]]]


def test_unequal_radii_do_not_swap_axes():
    q_xy = xy((50, 50))
    t_xy = xy((58, 52), (52, 58), (53, 61), (54, 50), (50, 62))
    assert gate_mask(q_xy, t_xy, (3.0, 11.0))[0].tolist() == [False, True, True, False, False]
    assert gate_mask(q_xy, t_xy, (11.0, 3.0))[0].tolist() == [True, False, False, True, False]
    q, t = words(0x0), words(0x0, 0x1, 0x3, 0x7, 0xF)
    assert match_guided_ref(q, t, q_xy, t_xy, (3.0, 11.0), length=32)[0].tolist() == [[1]]
    assert match_guided_ref(q, t, q_xy, t_xy, (11.0, 3.0), length=32)[0].tolist() == [[0]]
    assert match_guided_ref(q, t, q_xy, t_xy, 11.0, length=32)[0].tolist() == [[0]]


def test_ties_and_best_outside_the_window():
    # query 0: trains 0, 2, 4 tie at distance 1; 0 is outside the window, so 2 wins and 4 is the second.
    # query 1: its exact copy (train 1) is outside; the gated best is train 3, the second train 5
    q, t = words(0x0, 0xFF00), words(0x1, 0xFF00, 0x2, 0xFF01, 0x4, 0xFF07)
    q_xy = xy((10, 10), (30, 30))
    t_xy = xy((20, 10), (30, 39), (12, 10), (31, 30), (10, 13), (28, 30))
    plain = match_ref(q, t, length=32)
    assert plain[0].tolist() == [[0, 1]] and plain[1].tolist() == [[[1, 1], [0, 1]]]
    idx, dist, _ = match_guided_ref(q, t, q_xy, t_xy, 8.0, length=32)
    assert idx.tolist() == [[2, 3]] and dist.tolist() == [[[1, 1], [1, 3]]]


@pytest.mark.parametrize("which", ["brief", "nn"])
def test_cross_check_equals_the_transposed_problem(which):
    """q -> t is accepted under the cross-check iff t's best query, found by the same guided search with the
    two sets (and their positions) swapped, is q."""
    if which == "brief":
        c = G.brief_case(40, 60, length=6, flags=True, seed=5)  # 6 bits: ties everywhere, in both directions
        run = lambda a, b, axy, bxy, av, bv, **kw: match_guided_ref(a, b, axy, bxy, c["radius"], None, None, av, bv, length=6, **kw)  # noqa: E731
    else:
        c = G.nn_case(40, 60, dim=8, regime="int", flags=True, seed=5)
        run = lambda a, b, axy, bxy, av, bv, **kw: nn_match_guided_ref(a, b, axy, bxy, c["radius"], None, None, av, bv, **kw)  # noqa: E731
    fwd = run(c["q"], c["t"], c["q_xy"], c["t_xy"], c["qv"], c["tv"])
    rev = run(c["t"], c["q"], c["t_xy"], c["q_xy"], c["tv"], c["qv"])
    exp = np.array([[t if t >= 0 and rev[0][0, t] == q else -1 for q, t in enumerate(fwd[0][0])]], np.int32)
    got = run(c["q"], c["t"], c["q_xy"], c["t_xy"], c["qv"], c["tv"], cross_check=True)
    assert np.array_equal(got[0], exp) and np.array_equal(got[1], fwd[1])
    assert 0 < (exp >= 0).sum() < (fwd[0] >= 0).sum()  # the cross-check rejects some and keeps some


def test_huge_radius_is_the_unguided_reference():
    c = G.brief_case(65, 257, flags=True)
    kw = dict(max_distance=100, max_ratio=0.95, cross_check=True)
    got = match_guided_ref(c["q"], c["t"], c["q_xy"], c["t_xy"], 3.0e38, None, None, c["qv"], c["tv"], **kw)
    for g, e in zip(got, match_ref(c["q"], c["t"], None, None, c["qv"], c["tv"], **kw)):
        assert np.array_equal(g, e)
    c = G.nn_case(33, 65, dim=16, regime="round", flags=True)
    kw = dict(max_distance=1.5, max_ratio=0.95, cross_check=True)
    got = nn_match_guided_ref(c["q"], c["t"], c["q_xy"], c["t_xy"], 3.0e38, None, None, c["qv"], c["tv"], **kw)
    for g, e in zip(got, nn_match_ref(c["q"], c["t"], None, None, c["qv"], c["tv"], **kw)):
        assert np.array_equal(g.view(np.uint32) if g.dtype == F32 else g, e.view(np.uint32) if e.dtype == F32 else e)


@pytest.mark.parametrize("kw", G.BRIEF_CASES, ids=G.case_id)
def test_gate_decides_the_brief_fixtures(kw):
    """A kernel that ignores the gate cannot pass the GPU test of this fixture: of the queries the unguided
    reference matches, the gated reference answers more than 3 in 4 differently (the bar is 1 in 2)."""
    c = G.brief_case(**kw)
    guided = match_guided_ref(c["q"], c["t"], c["q_xy"], c["t_xy"], c["radius"], c["qc"], c["tc"], c["qv"], c["tv"],
                              length=c["length"])
    plain = match_ref(c["q"], c["t"], c["qc"], c["tc"], c["qv"], c["tv"], length=c["length"])
    assert (plain[0] >= 0).sum() >= 1
    assert G.changed_fraction(guided, plain) > 0.75


@pytest.mark.parametrize("kw", G.NN_CASES, ids=G.case_id)
def test_gate_decides_the_nn_fixtures(kw):
    c = G.nn_case(**kw)
    guided = nn_match_guided_ref(c["q"], c["t"], c["q_xy"], c["t_xy"], c["radius"], c["qc"], c["tc"], c["qv"], c["tv"])
    plain = nn_match_ref(c["q"], c["t"], c["qc"], c["tc"], c["qv"], c["tv"])
    assert (plain[0] >= 0).sum() >= 1
    assert G.changed_fraction(guided, plain) > 0.75


def test_fixtures_have_every_kind_of_window():
    """Over the radius cases, windows that are empty, hold exactly one candidate, and hold several."""
    for cases, make in ((G.BRIEF_CASES, G.brief_case), (G.NN_CASES, G.nn_case)):
        kinds = set()
        for kw in cases:
            if "variant" in kw:
                c = make(**kw)
                n = gate_mask(c["q_xy"][0], c["t_xy"][0], c["radius"]).sum(axis=1)
                kinds |= {min(int(k), 2) for k in n}
        assert kinds == {0, 1, 2}


# ---- the libraries and the binding, without a device -------------------------------------------------------
def test_both_libraries_export_the_guided_entries():
    import feature_detector_amd as fd

    L = fd.load()
    assert hasattr(L, "fd_brief_match_guided") and hasattr(L, "fd_nn_match_guided")
    assert L.fd_abi_version() == 6
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "feature_detector_amd", "api")])
    lib = os.path.join(ROOT, "feature_detector_amd", "lib", "libfeature_detector.so")
    nm = subprocess.run(["nm", "-DC", lib], capture_output=True, text=True).stdout
    assert "feature_detector::BriefMatcher::MatchGuided" in nm
    assert "feature_detector::NNDescriptorMatcher::MatchGuided" in nm


def test_null_context_is_invalid():
    import feature_detector_amd as fd
    from feature_detector_amd import _lib

    L = fd.load()
    gate = _lib.fd_match_gate(1.0, 1.0)
    z = np.zeros((1, 4, 8), np.uint32)
    p = xy(*[(0, 0)] * 4)
    idx = np.zeros((1, 4), np.int32)
    v = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    o = _lib.fd_match_opts(256, -1, 0.0, 0)
    assert L.fd_brief_match_guided(None, 1, ctypes.byref(o), ctypes.byref(gate), v(z), None, None, 4, v(p), v(z), None, None,
                                   4, v(p), v(idx), None, None, 0) == _lib.FD_ERR_INVALID
    o = _lib.fd_nn_match_opts(8, -1.0, 0.0, 0)
    assert L.fd_nn_match_guided(None, 1, ctypes.byref(o), ctypes.byref(gate), v(z), None, None, 4, v(p), v(z), None, None, 4,
                                v(p), v(idx), None, None, 0) == _lib.FD_ERR_INVALID


@pytest.mark.parametrize("which", ["brief", "nn"])
def test_python_needs_all_three_or_none(which):
    import feature_detector_amd as fd

    fn = fd.brief_match if which == "brief" else fd.nn_match
    z = np.zeros((1, 4, 8), np.uint32 if which == "brief" else F32)
    p = np.zeros((1, 4, 2), F32)
    for kw in (dict(q_xy=p), dict(t_xy=p), dict(radius=2.0), dict(q_xy=p, t_xy=p), dict(q_xy=p, radius=2.0),
               dict(t_xy=p, radius=(1.0, 2.0))):
        with pytest.raises(ValueError, match="q_xy, t_xy and radius together"):
            fn(z, z, **kw)
