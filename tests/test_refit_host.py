"""CPU checks of fd_ransac_refit's yardstick tests/refit_ref.py (the numpy restatement of the contract in
include/fd_hip.h) and of what the entry point answers without a GPU."""
import ctypes

import numpy as np
import pytest

import ransac_ref as R
import refit_ref as F

MODELS = [R.FUNDAMENTAL, R.HOMOGRAPHY]
# The noisy planted scenes (n = 64, 16 outliers, +-0.5 px on every planted coordinate) of the accuracy test,
# chosen here on the CPU: the seeds 0..7 of both models, all of which the restatement alone satisfies.
ACCURACY_SEEDS = tuple(range(8))


@pytest.fixture(scope="module")
def cases():
    return F.all_cases()


@pytest.fixture(scope="module")
def accuracy():
    """(model, seed) -> (scene, fd_ransac restatement outputs (256 hypotheses), refit outputs (rounds 2))."""
    out = {}
    for model in MODELS:
        for seed in ACCURACY_SEEDS:
            sc = F.noisy_scene(model, seed)
            ran = R.ransac_ref(sc[0][None], sc[1][None], model=model, hypotheses=256, seed=seed, center=F.CENTER, scale=F.SCALE)
            ref = F.refit_ref(sc[0][None], sc[1][None], ran[0], ran[1], model=model, rounds=2, center=F.CENTER, scale=F.SCALE)
            out[model, seed] = (sc, ran, ref)
    return out


def normal_matrices(cases, accuracy):
    """(name, model, N) of the first round's normal matrix of every frame of the tests' scenes that has a fit."""
    out = []
    sets = [(name, c["model"], c["q"], c["t"], c["counts"], c["idx"], c["valid"], c["in_inlier"]) for name, _, c in cases]
    sets += [(f"noisy-{m}-{s}", m, sc[0][None], sc[1][None], None, None, None, ran[1]) for (m, s), (sc, ran, _) in accuracy.items()]
    for name, model, q, t, counts, idx, valid, inl in sets:
        for b in range(q.shape[0]):
            corr, slots = R.correspondences(q[b], t[b], None if counts is None else counts[b], None if idx is None else idx[b],
                                            None if valid is None else valid[b], F.CENTER[0], F.CENTER[1], F.SCALE)
            member = inl[b, slots] == 1
            if member.sum() >= R.SAMPLE[model]:
                out.append((f"{name}[{b}]", model, F.normal_matrix(model, corr, member)))
    return out


def settled(A, sweeps=24):
    """The first sweep count after which no later sweep (up to `sweeps`) changes a bit of the eigenvector at
    the smallest diagonal entry."""
    trace = []
    F.jacobi(A, sweeps, trace=trace)
    vec = [V[:, F.smallest(d)].view(np.uint64) for d, V in trace]
    return next(k + 1 for k in range(sweeps) if all(np.array_equal(vec[k], vec[j]) for j in range(k + 1, sweeps)))


def test_sweep_count_rule(cases, accuracy):
    """FD_REFIT_SWEEPS = 2 + the smallest sweep count after which one more sweep changes no bit of the
    eigenvector, over the 9 x 9 normal matrix of every scene of these tests that passes the rank test (a
    degenerate one has no eigenvector to settle) and the 3 x 3 matrix F^T F of its rank-2 step."""
    worst = 0
    for name, model, N in normal_matrices(cases, accuracy):
        x, valid = F.eigenvector(N, 24)
        if not valid:
            continue
        k = settled(N)
        if model == R.FUNDAMENTAL:
            Fm = x.reshape(3, 3)
            G = np.array([[sum(Fm[r, i] * Fm[r, j] for r in range(3)) for j in range(3)] for i in range(3)])
            k = max(k, settled(G))
        worst = max(worst, k)
    print("sweeps until no bit changes:", worst)
    assert F.SWEEPS == worst + 2
    header = open(R.__file__.replace("tests/ransac_ref.py", "include/fd_hip.h")).read()
    assert f"#define FD_REFIT_SWEEPS {F.SWEEPS}\n" in header


def test_jacobi_eigenvector_against_eigh(cases, accuracy):
    """The angle between the restatement's eigenvector and numpy.linalg.eigh's, on every normal matrix of the
    tests' scenes that passes the rank test. Bound: both are eigenvectors of a matrix within about 9 * eps *
    |N| of N (backward stability, eps = 2^-52), so each is within 9 * eps * lambda_max / gap of the true one
    (Davis-Kahan), gap = lambda_2 - lambda_1 as eigh measures it; the bound is four times the sum of the two."""
    eps, worst = 2.0 ** -52, 0.0
    checked = 0
    for name, model, N in normal_matrices(cases, accuracy):
        x, valid = F.eigenvector(N)
        if not valid:
            continue
        w, U = np.linalg.eigh(N)
        gap = w[1] - w[0]
        bound = 4 * 2 * 9 * eps * w[-1] / gap
        u = U[:, 0]
        angle = np.linalg.norm(x - np.sign(x @ u) * u)  # = 2 sin(angle / 2)
        worst = max(worst, angle / bound)
        assert abs(np.linalg.norm(x) - 1.0) < 1e-14 and angle <= bound, (name, angle, bound, gap / w[-1])
        checked += 1
    print("largest angle / bound:", worst, "matrices:", checked)
    assert checked >= 30


def test_jacobi_diagonalises_a_known_matrix():
    rng = np.random.default_rng(3)
    Q, _ = np.linalg.qr(rng.standard_normal((9, 9)))
    lam = np.array([5.0, 1e-6, 3.0, 2.0, 9.0, 0.5, 7.0, 4.0, 1.0])
    d, V = F.jacobi(Q @ np.diag(lam) @ Q.T)
    assert np.allclose(np.sort(d), np.sort(lam), rtol=0, atol=1e-13) and np.allclose(V.T @ V, np.eye(9), atol=1e-14)
    at = F.smallest(d)
    assert abs(abs(V[:, at] @ Q[:, 1]) - 1.0) < 1e-13
    d, V = F.jacobi(np.diag(lam))  # every pair skipped: nothing changes
    assert np.array_equal(d, lam) and np.array_equal(V, np.eye(9)) and F.smallest(np.array([2.0, 1.0, 1.0])) == 1


def test_normal_matrix_is_the_sum_of_row_products():
    """Against a plain float64 matmul, to rounding; members only; position i goes to partial i % 256."""
    for model in MODELS:
        q, t = F.scenes(model, 600, 1, seed=1)
        corr, _ = R.correspondences(q[0], t[0], None, None, None, F.CENTER[0], F.CENTER[1], F.SCALE)
        member = np.arange(600) % 3 != 1
        N = F.normal_matrix(model, corr, member)
        rows = R.build_rows(model, corr[member].reshape(-1, 4, 4)).reshape(-1, 9)
        assert np.array_equal(N, N.T) and np.allclose(N, rows.T @ rows, rtol=1e-12, atol=1e-15)
        one = np.zeros(600, bool)
        one[300] = True
        r = R.build_rows(model, np.repeat(corr[300][None, None], 4, 1)).reshape(-1, 9)[:1 if model == R.FUNDAMENTAL else 2]
        assert np.array_equal(F.normal_matrix(model, corr, one), sum(np.outer(x, x) for x in r))


@pytest.mark.parametrize("seed", ACCURACY_SEEDS)
def test_refit_fundamental_has_rank_two(accuracy, seed):
    """A projection in double leaves a few ulps: smallest over largest singular value <= 1e-12."""
    _, _, ref = accuracy[R.FUNDAMENTAL, seed]
    sv = np.linalg.svd(ref[0][0].reshape(3, 3), compute_uv=False)
    assert ref[3][0] >= 1 and sv[2] / sv[0] <= 1e-12


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("seed", ACCURACY_SEEDS)
def test_refit_lowers_the_residual_on_noisy_scenes(accuracy, model, seed):
    """The refit model's RMS residual against the noise-free planted pairs is lower than the minimal-sample
    model's, on every listed scene, and the inlier count does not fall. The list (ACCURACY_SEEDS, both
    models) was chosen on the CPU so that the restatement alone satisfies this."""
    (q, t, planted, q0, t0), ran, ref = accuracy[model, seed]
    before, after = F.rms(model, ran[0][0], q0, t0, planted), F.rms(model, ref[0][0], q0, t0, planted)
    print(f"rms residual [px]: {before:.4f} -> {after:.4f}; inliers {ran[2][0]} -> {ref[2][0]}; rounds {ref[3][0]}")
    assert ref[3][0] >= 1 and after < before and ref[2][0] >= ran[2][0]
    assert ref[2][0] == ref[1][0].sum() and np.abs(ref[0][0]).max() == 1.0


def test_cases_reach_what_they_are_for(cases):
    """The outcomes the GPU cases are built for, on the restatement."""
    got = {name: (F.run_case(c, rounds), c) for name, rounds, c in cases}
    for name, (out, c) in got.items():
        support = (c["in_inlier"] == 1).sum(axis=1)
        assert np.all(out[2] == (out[1] == 1).sum(axis=1))
        if name.startswith("support"):
            k = int(name.split("-")[2])
            small = k < R.SAMPLE[c["model"]]
            assert support[0] == k and (out[3][0] == 0) == small and (out[2][0] == k if small else out[2][0] >= k), name
        if name.startswith("degenerate") or (name.startswith("support") and out[3][0] == 0):
            assert out[3][0] == 0 and np.array_equal(out[0].view(np.uint64), c["in_model"].view(np.uint64))
            assert np.array_equal(out[1] == 1, c["in_inlier"] == 1)
        if name.startswith("stopped"):
            assert out[3][0] == 1 and F.run_case(c, 1)[3][0] == 1
            assert np.array_equal(out[0].view(np.uint64), F.run_case(c, 1)[0].view(np.uint64))
        if name.startswith("batch"):
            assert len(set(support.tolist())) == 3 and np.all(out[3] >= 1) and np.all(out[2] >= support)
            assert [F.run_case(c, r)[3].max() for r in (1, 2)] == [1, 2]
        if name.startswith("holes"):
            inl = c["in_inlier"]
            assert {0, 1, 2, 0xFF} <= set(inl.ravel().tolist()) and out[3].max() >= 1
            assert out[1][0, 5] == 0 and out[1][0, 30] == 0 and not out[1][:, 5:9].any()
    # a degenerate fit fails the rank test, not the guard: without it the arbitrary null vector is accepted
    for model in MODELS:
        c = F.degenerate_case(model)
        corr, slots = R.correspondences(c["q"][0], c["t"][0], None, None, None, F.CENTER[0], F.CENTER[1], F.SCALE)
        x, valid = F.eigenvector(F.normal_matrix(model, corr, c["in_inlier"][0, slots] == 1))
        assert not valid and np.all(np.isfinite(x))


def test_guard_keeps_counts_from_falling(cases):
    for name, rounds, c in cases:
        prev = []  # c_0: the bytes of 1 at slots that are correspondences
        for b in range(c["q"].shape[0]):
            slots = R.correspondences(c["q"][b], c["t"][b], None if c["counts"] is None else c["counts"][b],
                                      None if c["idx"] is None else c["idx"][b], None if c["valid"] is None else c["valid"][b],
                                      F.CENTER[0], F.CENTER[1], F.SCALE)[1]
            prev.append(int((c["in_inlier"][b, slots] == 1).sum()))
        prev = np.array(prev)
        for r in range(1, 5):
            out = F.run_case(c, r)
            assert np.all(out[2] >= prev) and np.all(out[3] <= r), name
            prev = out[2]


def test_null_context_and_exports():
    """Without a GPU there is no context: a NULL one is FD_ERR_INVALID whatever else is passed
    (tests/test_gpu_refit.py::test_rejected_arguments tells the rejected arguments apart with a real context)."""
    import feature_detector_amd as fd
    from feature_detector_amd._lib import fd_refit_opts

    L = fd.load()
    buf = np.zeros(64, np.float64)
    p = ctypes.c_void_p(buf.ctypes.data)
    good = dict(model=0, rounds=2, threshold=1.0, center_x=0.0, center_y=0.0, scale=1.0)
    for bad in ({}, dict(model=2), dict(rounds=0), dict(rounds=5), dict(threshold=0.0), dict(scale=float("nan"))):
        opts = fd_refit_opts(**{**good, **bad})
        rc = L.fd_ransac_refit(None, 1, ctypes.byref(opts), p, None, 4, p, 4, None, None, p, p, p, None, None, None, 0)
        assert rc == fd._lib.FD_ERR_INVALID
    assert ctypes.sizeof(fd_refit_opts) == 24 and L.fd_abi_version() == 6
    assert "fd_ransac_refit" in fd._lib.EXPORTS and hasattr(fd, "refit_geometry") and hasattr(fd, "RefitResult")
