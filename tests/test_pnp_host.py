"""The restatement of fd_pnp_ransac / fd_pnp_refit (tests/pnp_ref.py) on the CPU: against an independent solution
(np.linalg.svd DLT on the same samples, a plain dense Gauss-Newton), the refit guard, the Jacobi sweep count, and
the pieces it shares with the other geometry restatements. No GPU.

Accuracy margins (stated before the restatement was run against them; the reasoning, not its results):
* after RANSAC both poses are unrefined minimal-sample winners. A winner is only held to reproject its inliers
  within the threshold, so two valid winners may differ by the angle the threshold subtends, A = threshold / fx
  (2 px / 500 = 0.23 deg), and by the translation that angle moves the scene's mean depth (6.5 * A = 0.026):
      error <= 2 * independent + 2 * A        (rotation),   <= 2 * independent + 2 * 6.5 * A   (translation)
* after refinement both are least-squares optima over nearly the same inliers, so they agree up to the estimate's
  own noise, E = sigma / (fx * sqrt(inliers)) radians (and 6.5 * E of translation):
      error <= 2 * independent + 2 * E        (rotation),   <= 2 * independent + 2 * 6.5 * E   (translation)
"""
import functools

import numpy as np
import pytest

import pnp_ref as P
import ransac_ref as R

# (seed, points, outlier fraction, image noise in px)
SCENES = [(0, 40, 0.2, 0.3), (1, 80, 0.3, 0.5), (2, 120, 0.35, 0.5), (3, 200, 0.4, 0.6), (4, 300, 0.5, 0.7), (5, 500, 0.3, 0.5)]
HYPOTHESES, ROUNDS, DEPTH = 256, 4, 6.5


@functools.lru_cache(maxsize=None)
def solved(k):
    """Scene k through the restatement and through the independent solution."""
    seed, n, out, noise = SCENES[k]
    sc = P.scene(seed, n=n, outliers=out, noise=noise)
    c = P.case(sc, hypotheses=HYPOTHESES, seed=seed)
    detail, trace = [], []
    ran = P.run_ransac(c, detail=detail)
    fit = P.run_refit(c, ran[0], ran[1], ROUNDS, trace=trace)
    iR, it, iinl = P.independent_ransac(sc, HYPOTHESES, seed, P.THRESHOLD)
    jR, jt, jinl = P.independent_refine(sc, iR, it, iinl, ROUNDS, P.THRESHOLD)
    ind = (np.concatenate([iR.reshape(9), it]), np.concatenate([jR.reshape(9), jt]), int(iinl.sum()), int(jinl.sum()))
    return sc, c, ran, fit, detail[0], trace[0], ind


@pytest.mark.parametrize("k", range(len(SCENES)))
def test_accuracy_against_the_independent_solution(k):
    sc, c, ran, fit, _, _, ind = solved(k)
    noise = SCENES[k][3]
    assert ran[3][0] >= 0 and fit[3][0] >= 1
    A = P.THRESHOLD / sc["cam"][0]
    E = noise / (sc["cam"][0] * np.sqrt(max(ind[3], 1)))
    r0, t0 = P.pose_errors(ran[0][0], sc)
    r1, t1 = P.pose_errors(fit[0][0], sc)
    ir0, it0 = P.pose_errors(ind[0], sc)
    ir1, it1 = P.pose_errors(ind[1], sc)
    true = int(sc["planted"].sum())
    print(f"scene {k}: n {len(sc['p'])} true inliers {true} | RANSAC {ran[2][0]} inl {r0:.3f} deg {t0:.4f} "
          f"(independent {ind[2]} inl {ir0:.3f} deg {it0:.4f}) | refined {fit[2][0]} inl {r1:.4f} deg {t1:.5f} "
          f"(independent {ind[3]} inl {ir1:.4f} deg {it1:.5f})")
    assert r0 <= 2 * ir0 + 2 * np.degrees(A) and t0 <= 2 * it0 + 2 * DEPTH * A
    assert r1 <= 2 * ir1 + 2 * np.degrees(E) and t1 <= 2 * it1 + 2 * DEPTH * E
    # the refined inliers reach or come close to the planted ones (an outlier may land within the threshold)
    assert fit[2][0] >= 0.95 * true


@pytest.mark.parametrize("k", range(len(SCENES)))
def test_refit_guard_never_loses_inliers(k):
    _, _, ran, fit, _, trace, _ = solved(k)
    assert all(b >= a for a, b in zip(trace, trace[1:])), trace
    assert fit[3][0] >= 1 and len(trace) == fit[3][0] + 1 and fit[2][0] == trace[-1]
    # c_0 is what the orthonormalised pose classifies, not the projective winner's count
    assert trace[0] <= ran[2][0]


def _winners():
    """The winning camera matrix of every frame of every scene of this file and of tests/test_gpu_pnp.py."""
    out = [solved(k)[4][2][np.argmax(np.where(solved(k)[4][1], solved(k)[4][0], -1))] for k in range(len(SCENES))]
    for name, c in P.all_cases():
        if name == "hyp-4096":
            continue  # the scene of hyp-64 with more samples
        detail = []
        best = P.run_ransac(c, detail=detail)[3]
        out += [d[2][np.argmax(np.where(d[1], d[0], -1))] for d, b in zip(detail, best) if d[1].any()]
    return out


def test_sweep_count_rule():
    """FD_POSE_SWEEPS's rule: the diagonal and V of M^T M change no bit after FD_POSE_SWEEPS - 2 sweeps."""
    winners = _winners()
    assert len(winners) >= 20
    for Pw in winners:
        trace = []
        P.to_pose(Pw, (0.0, 0.0, 0.0), 1.0, sweeps=P.SWEEPS + 2, trace=trace)
        d5, V5 = trace[P.SWEEPS - 3]
        for d, V in trace[P.SWEEPS - 2:]:
            assert np.array_equal(d.view(np.uint64), d5.view(np.uint64)) and np.array_equal(V.view(np.uint64), V5.view(np.uint64))


def test_pose_is_a_rotation():
    for k in range(len(SCENES)):
        for pose in (solved(k)[2][0][0], solved(k)[3][0][0]):
            Rm = pose[:9].reshape(3, 3)
            assert np.allclose(Rm @ Rm.T, np.eye(3), atol=1e-12) and np.linalg.det(Rm) > 0.999999


def test_elimination_is_fd_ransacs_at_8_rows():
    rng = np.random.default_rng(2)
    A = rng.standard_normal((40, 8, 9))
    A[3, 2] = A[3, 1]   # a singular system
    A[5, 0, 0] = np.nan
    a, av = R.null_vector(A)
    b, bv = P.null_vector(A)
    assert np.array_equal(av, bv) and not bv[3] and not bv[5] and bv.sum() == 38
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_conditioning_is_undone():
    """The pose does not depend on the conditioning beyond the data's rounding: centre and scale of the scene against none."""
    sc = P.scene(1, n=80, outliers=0.0, noise=0.0)
    a = P.run_ransac(P.case(sc, hypotheses=8))
    b = P.run_ransac(P.case(sc, hypotheses=8, center=(0.0, 0.0, 0.0), scale=1.0))
    assert a[3][0] == b[3][0] >= 0 and a[2][0] == b[2][0] == 80
    for pose in (a[0][0], b[0][0]):  # exact data but for the float32 rounding of the positions
        rot, tr = P.pose_errors(pose, sc)
        assert rot < 1e-2 and tr < 1e-3
    assert np.allclose(a[0][:, :9], b[0][:, :9], atol=1e-6)


def test_degenerate_cases_have_no_pose():
    cases = dict(P.all_cases())
    for name in ("coplanar", "duplicate", "n-0", "n-5"):
        pose, inl, cnt, best = P.run_ransac(cases[name], fill=7)
        assert best[0] == -1 and cnt[0] == 0 and not pose.any(), name
    detail = []
    pose, inl, cnt, best = P.run_ransac(cases["behind"], detail=detail)
    assert best[0] >= 0 and cnt[0] == 0 and detail[0][0].max() == 0
    c = cases["few-distinct"]
    gave_up = R.exhausted(c["seed"], 0, 6, P.M, c["hypotheses"])
    assert 0 < len(gave_up) < c["hypotheses"]
    detail = []
    assert P.run_ransac(c, detail=detail)[3][0] not in gave_up and not detail[0][1][gave_up].any()


def test_refit_rejections():
    """A support set of fewer than three points has a singular system; a pose already at the optimum of a noise
    free scene is kept bit for bit when the round loses an inlier or cannot be solved."""
    sc = P.scene(6, n=50, outliers=0.2)
    c = P.case(sc)
    ran = P.run_ransac(c)
    two = np.zeros_like(ran[1])
    two[0, np.flatnonzero(ran[1][0])[:2]] = 1
    out = P.run_refit(c, ran[0], two, 8)
    assert out[3][0] == 0 and out[2][0] == 2 and np.array_equal(out[0].view(np.uint64), ran[0].view(np.uint64))
    assert np.array_equal(out[1], two)
