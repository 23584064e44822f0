"""The restatement of fd_align_ransac / fd_align_refit / fd_align_apply (tests/align_ref.py) on the CPU: against an
independent solution (an SVD Umeyama with the determinant fix on the same samples and members), the refit guard, the
Jacobi sweep count, and transform_poses. No GPU.

Accuracy margins (stated before the restatement was run against them; the reasoning, not its results). th is the
threshold, sigma the noise per coordinate, rho the RMS distance of the planted source points from their centroid c:
* after RANSAC both models are unrefined 3-point winners. A winner is only held to map its inliers within th, so two
  valid winners may differ by what th subtends over the scene's radius: the angle A = th / rho, the relative scale
  th / rho, and the translation th * (1 + |c| / rho) (the offset itself, plus the angle's lever over the centroid):
      error <= 2 * independent + 2 * A    (angle, relative scale),   <= 2 * independent + 2 * th * (1 + |c| / rho)
* after the refit both are least-squares optima over nearly the same members, so they agree up to the estimate's own
  noise, E = sigma / (rho * sqrt(inliers)) of angle and relative scale, and sigma / sqrt(inliers) * (1 + |c| / rho) of
  translation:
      error <= 2 * independent + 2 * E,   <= 2 * independent + 2 * sigma / sqrt(inliers) * (1 + |c| / rho)
"""
import ctypes
import functools

import numpy as np
import pytest

import align_ref as A

# (seed, points, outlier fraction, planar)
SCENES = [(0, 40, 0.2, False), (1, 80, 0.3, False), (2, 120, 0.35, True), (3, 200, 0.4, False), (4, 300, 0.5, False),
          (5, 500, 0.3, True)]
KINDS = (A.SIMILARITY, A.RIGID)
HYPOTHESES, ROUNDS = 256, 4
@functools.lru_cache(maxsize=None)
def solved(k, kind):
    """Scene k through the restatement and through the independent solution."""
    seed, n, out, planar = SCENES[k]
    sc = A.scene(seed, n=n, outliers=out, noise=A.NOISE, planar=planar, rigid=kind == A.RIGID)
    c = A.case(sc, kind=kind, hypotheses=HYPOTHESES, seed=seed)
    trace = []
    ran = A.run_ransac(c)
    fit = A.run_refit(c, ran[0], ran[1], ROUNDS, trace=trace)
    i = A.independent_ransac(sc, HYPOTHESES, seed, A.THRESHOLD, kind)
    j = A.independent_refine(sc, i[3], ROUNDS, A.THRESHOLD, kind)
    pack = lambda r: np.concatenate([r[0].reshape(9), r[1], [r[2]]])  # noqa: E731
    return sc, c, ran, fit, trace[0], (pack(i), pack(j), int(i[3].sum()), int(j[3].sum()))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k", range(len(SCENES)))
def test_accuracy_against_the_independent_solution(k, kind):
    sc, c, ran, fit, _, ind = solved(k, kind)
    assert ran[3][0] >= 0 and fit[3][0] >= 1
    rho, lever = sc["radius"], 1.0 + np.linalg.norm(sc["centroid"]) / sc["radius"]
    th, sigma = A.THRESHOLD, A.NOISE
    E = sigma / (rho * np.sqrt(max(ind[3], 1)))
    e0, e1 = A.model_errors(ran[0][0], sc), A.model_errors(fit[0][0], sc)
    i0, i1 = A.model_errors(ind[0], sc), A.model_errors(ind[1], sc)
    true = int(sc["planted"].sum())
    print(f"scene {k} kind {kind}: n {len(sc['q'])} planted {true} | RANSAC {ran[2][0]} inl {e0} (independent {ind[2]} inl {i0}) | "
          f"refined {fit[2][0]} inl {e1} (independent {ind[3]} inl {i1})")
    assert e0[0] <= 2 * i0[0] + 2 * th / rho and e0[1] <= 2 * i0[1] + 2 * th / rho and e0[2] <= 2 * i0[2] + 2 * th * lever
    assert e1[0] <= 2 * i1[0] + 2 * E and e1[1] <= 2 * i1[1] + 2 * E and e1[2] <= 2 * i1[2] + 2 * E * rho * lever
    assert fit[2][0] >= 0.95 * true
    if kind == A.RIGID:
        assert ran[0][0, 12] == 1.0 and fit[0][0, 12] == 1.0


# The largest differences measured over the twelve (scene, kind) pairs of this file between one round of the refit
# and umeyama() on identical members: 1.33e-15 in R (entrywise), 6.22e-15 in t, 2.22e-16 in s (relative). A cyclic
# Jacobi in double on a 4 x 4 matrix leaves the eigenvector a few units in the last place off, and t carries R's error
# over the centroid's distance (about 5.5 here). The bounds are 100 times the measured values.
REFIT_BOUNDS = (1.33e-13, 6.22e-13, 2.22e-14)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k", range(len(SCENES)))
def test_refit_equals_umeyama_on_identical_members(k, kind):
    sc, c, ran, _, _, _ = solved(k, kind)
    _, _, corr, slots = next(A._frames(c["q"], c["t"], None, None, None, None, None))
    member = ran[1][0, slots] == 1
    m = A.horn_fit(corr, member, kind)
    R, t, s = A.umeyama(corr[member, :3], corr[member, 3:], kind == A.SIMILARITY)
    dR, dt, ds = np.abs(m[:9].reshape(3, 3) - R).max(), np.abs(m[9:12] - t).max(), abs(m[12] / s - 1.0)
    print(f"scene {k} kind {kind}: members {member.sum()} dR {dR:.2e} dt {dt:.2e} ds {ds:.2e}")
    assert dR <= REFIT_BOUNDS[0] and dt <= REFIT_BOUNDS[1] and ds <= REFIT_BOUNDS[2]


@pytest.mark.parametrize("kind", KINDS)
def test_mirrored_target_still_gives_a_proper_rotation(kind):
    sc = A.scene(7, n=60, outliers=0.0, mirror=True)
    c = A.case(sc, kind=kind, threshold=100.0)  # wide enough that the refit runs on every correspondence
    ran = A.run_ransac(c)
    fit = A.run_refit(c, ran[0], ran[1], 2)
    assert ran[3][0] >= 0 and fit[3][0] >= 1 and fit[2][0] == 60
    for model in (ran[0][0], fit[0][0]):
        Rm = model[:9].reshape(3, 3)
        assert np.allclose(Rm @ Rm.T, np.eye(3), atol=1e-12) and abs(np.linalg.det(Rm) - 1.0) < 1e-12 and model[12] > 0
    # the unconstrained SVD solution of the same members is a reflection: the determinant fix is what umeyama adds
    X, Y = sc["q"].astype(np.float64), sc["t"].astype(np.float64)
    U, _, Vt = np.linalg.svd((Y - Y.mean(0)).T @ (X - X.mean(0)))
    assert np.linalg.det(U @ Vt) < 0
    R, _, _ = A.umeyama(X, Y)
    assert np.abs(fit[0][0, :9].reshape(3, 3) - R).max() < 1e-9


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k", range(len(SCENES)))
def test_refit_guard_never_loses_inliers(k, kind):
    _, _, _, fit, trace, _ = solved(k, kind)
    assert all(b >= a for a, b in zip(trace, trace[1:])), trace
    assert fit[3][0] >= 1 and len(trace) == fit[3][0] + 1 and fit[2][0] == trace[-1]


def test_refit_guard_stops_early():
    c = A.stopped_case()
    ran = A.run_ransac(c)
    trace = []
    eight = A.run_refit(c, ran[0], ran[1], 8, trace=trace)
    done = int(eight[3][0])
    assert done == 3 and len(trace[0]) == done + 1
    same = A.run_refit(c, ran[0], ran[1], done)
    for a, b in zip(same, eight):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    # the round after the last accepted one would lose an inlier
    more = A.refit_frame(*_list(c), eight[1][0] == 1, eight[0][0], 1, c["kind"], _tt(c))
    assert more[2] == 0
    # no accepted round: the model comes back bit for bit, with S_0's count
    for inl in (np.zeros_like(ran[1]), np.eye(1, 64, 3, dtype=np.uint8) + np.eye(1, 64, 5, dtype=np.uint8)):
        out = A.run_refit(c, ran[0], inl, 8)
        assert out[3][0] == 0 and np.array_equal(out[0].view(np.uint64), ran[0].view(np.uint64)) and out[2][0] == inl.sum()


def _tt(c):
    t = np.float64(np.float32(c["threshold"]))
    return t * t


def _list(c):
    _, _, corr, slots = next(A._frames(c["q"], c["t"], c["counts"], c["idx"], c["valid"], c["q_valid"], c["t_valid"]))
    return (corr,)


def _member_sets():
    """(corr, members, kind) of every refit round of every scene of this file and of tests/test_gpu_align.py."""
    cases = [solved(k, kind)[1] for k in range(len(SCENES)) for kind in KINDS] + [A.stopped_case()]
    cases += [c for name, c in A.all_cases() if name != "hyp-4096"]  # hyp-4096: the scene of hyp-64 with more samples
    for c in cases:
        ran = A.run_ransac(c)
        tt = _tt(c)
        for b, _, corr, slots in A._frames(c["q"], c["t"], c["counts"], c["idx"], c["valid"], c["q_valid"], c["t_valid"]):
            member = ran[1][b, slots] == 1
            for _ in range(A.SWEEPS + 1):
                m = A.horn_fit(corr, member, c["kind"])
                if m is None:
                    break
                yield corr, member, c["kind"]
                member = A.inliers(m[None], corr, tt)[0]


def test_sweep_count_rule():
    """FD_ALIGN_SWEEPS's rule: the diagonal of Horn's matrix and q change no bit after FD_ALIGN_SWEEPS - 2 sweeps."""
    sets = 0
    for corr, member, kind in _member_sets():
        trace = []
        A.horn_fit(corr, member, kind, sweeps=A.SWEEPS + 2, trace=trace)
        d5, q5 = trace[A.SWEEPS - 3]
        for d, q in trace[A.SWEEPS - 2:]:
            assert np.array_equal(d.view(np.uint64), d5.view(np.uint64)) and np.array_equal(q.view(np.uint64), q5.view(np.uint64))
        sets += 1
    assert sets >= 60


def test_degenerate_samples_and_small_lists():
    for name in ("collinear", "duplicate", "n-0", "n-2"):
        c = dict(A.all_cases())[name]
        detail = []
        ran = A.run_ransac(c, detail=detail)
        assert not detail[0][1].any() and ran[3][0] == -1 and not ran[0].any() and not ran[1].any()
    ran = A.run_ransac(dict(A.all_cases())["n-3"])
    assert ran[3][0] >= 0 and ran[2][0] == 3


def test_apply_restatement():
    sc = A.scene(11, n=30, outliers=0.0, noise=0.0)
    model = np.concatenate([sc["R"].reshape(9), sc["t_vec"], [sc["s"]]])[None]
    valid = np.ones((1, 30), np.uint8)
    valid[0, ::4] = 2
    out = A.align_apply_ref(model, sc["q"][None], valid, np.array([25], np.int32))
    moved = (valid[0] == 1) & (np.arange(30) < 25)
    assert np.array_equal(out[0][~moved], sc["q"][~moved]) and np.allclose(out[0][moved], sc["t"][moved], atol=1e-5)


def test_transform_poses_against_reprojection():
    """A camera of the source frame sees the transformed points, under its transformed pose, where it saw the points:
    the camera coordinates scale by s, the image positions do not move."""
    import feature_detector_amd as fd

    rng = np.random.default_rng(3)
    R, t, s = A.planted(21)
    model = np.concatenate([R.reshape(9), t, [s]])
    X = rng.uniform(-2, 2, (50, 3)) + np.array([0.0, 0.0, 6.0])
    Y = s * X @ R.T + t
    poses = np.stack([np.concatenate([A.rotation(*rng.uniform(-0.2, 0.2, 3)).reshape(9), rng.uniform(-0.5, 0.5, 3)]) for _ in range(3)])
    for shaped in (poses[0], poses, poses[None]):
        new = fd.transform_poses(model, shaped)
        assert new.shape == shaped.shape and new.dtype == np.float64
        for old, cur in zip(shaped.reshape(-1, 12), new.reshape(-1, 12)):
            xc = X @ old[:9].reshape(3, 3).T + old[9:]
            yc = Y @ cur[:9].reshape(3, 3).T + cur[9:]
            assert np.allclose(yc, s * xc, atol=1e-12) and np.allclose(yc[:, :2] / yc[:, 2:], xc[:, :2] / xc[:, 2:], atol=1e-12)
            Rn = cur[:9].reshape(3, 3)
            assert np.allclose(Rn @ Rn.T, np.eye(3), atol=1e-12)
    batch = fd.transform_poses(np.stack([model, model]), np.stack([poses, poses]))
    assert np.array_equal(batch[0], fd.transform_poses(model, poses)) and np.array_equal(batch[0], batch[1])
    with pytest.raises(ValueError):
        fd.transform_poses(model[:12], poses)


def test_null_context_and_exports():
    """Without a GPU there is no context: a NULL one is FD_ERR_INVALID whatever else is passed
    (tests/test_gpu_align.py::test_rejected_arguments tells the rejected arguments apart with a real context)."""
    import feature_detector_amd as fd
    from feature_detector_amd._lib import fd_align_opts

    L = fd.load()
    buf = np.zeros(64, np.float64)
    p = ctypes.c_void_p(buf.ctypes.data)
    opts = fd_align_opts(0, 4, 0, 2, 1.0)
    assert L.fd_align_ransac(None, 1, ctypes.byref(opts), p, None, None, 4, p, None, 4, None, None, p, None, None, None, 0) == fd._lib.FD_ERR_INVALID
    assert L.fd_align_refit(None, 1, ctypes.byref(opts), p, None, None, 4, p, None, 4, None, None, p, p, p, None, None, None, 0) == fd._lib.FD_ERR_INVALID
    assert L.fd_align_apply(None, 1, p, p, None, None, 4, p, 0) == fd._lib.FD_ERR_INVALID
    assert ctypes.sizeof(fd_align_opts) == 20 and L.fd_abi_version() == 6
    assert fd._lib.FD_ALIGN_SIMILARITY == 0 and fd._lib.FD_ALIGN_RIGID == 1 and fd._lib.FD_ALIGN_MAX_ROUNDS == 8
    for name in ("fd_align_ransac", "fd_align_refit", "fd_align_apply"):
        assert name in fd._lib.EXPORTS
    for name in ("align_points", "refine_alignment", "transform_points", "transform_poses", "AlignResult", "AlignRefineResult"):
        assert hasattr(fd, name) and name in fd.__all__
