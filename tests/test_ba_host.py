"""The restatement of fd_bundle_adjust (tests/ba_ref.py) on the CPU against an independent solver written here: dense
Levenberg-Marquardt over the full Jacobian and the full damped normal equations, without the Schur complement, with
np.linalg.solve and whole-array numpy sums; it shares no code with ba_ref. No GPU.

Scenes: planted, fixed seeds, cameras 2 / 3 / 5 / 8, 40 to 300 points, 0.3 to 0.7 px image noise, 10 to 20 % gross
outliers, the given poses and points perturbed from the planted ones, cameras 0 and 1 held (the scale is pinned).
They were chosen so that the independent solver alone, in 8 trials, brings the cost below 1.5 times the cost at the
planted state (measured: 1.091, 1.035, 1.000, 0.996): a condition on the inputs, asserted below.

Margins (the reasoning, stated before the restatement was run against them):
* Final cost. The Schur step and the dense step are algebraically the same, so both walk the same states up to
  rounding. The independent solver's own spread is measured by re-running it with the points permuted (three
  permutations per scene), relative to its cost; the restatement is allowed twice that. A spread of exactly 0 (four
  runs equal to the last bit, which another BLAS may give) is the one case handled apart: it counts as one ulp of the
  cost, the smallest spread a double can show. Measured, scenes 0..3: spread 1.3e-16, 1.9e-16, 1.8e-16, 2.0e-16
  (one ulp of the cost each); the restatement's difference 1.3e-16, 0, 0, 2.0e-16, i.e. ratios 1.0, 0, 0, 1.0 of
  the spread.
* Pose and point error against the planted state. Both solvers end at the optimum of the same cost over nearly the
  same active set, so they agree up to the estimate's own noise: E = sigma / (fx * sqrt(active observations of the
  camera)) radians of rotation, 6.5 * E of translation (6.5: the scenes' mean depth), and for a point
  Z^2 * sigma / (fx * B) with Z = 6.5 and B the distance between the outermost cameras:
      error <= 2 * independent + 2 * noise.
  And the adjustment must help: the error after is below the error before, on every scene.
* Motion-only. With every point held and lambda -> 0 the first step is fd_pnp_refit's Gauss-Newton step. Two things
  separate them, both measured on pnp_ref alone: the damping (pnp_ref's system with its diagonal scaled by
  1 + lambda against the plain one) and the order of the sums (pnp_ref on the correspondences reversed); the tolerance
  is twice their sum (measured: damping 4.1e-13, order 0; bundle adjustment differs from pnp_ref by 4.1e-13: it is
  the damped step).
"""
import functools

import numpy as np
import pytest

import ba_ref as B
import pnp_ref as P

# (seed, cameras, points, image noise px, outlier fraction, baseline)
SCENES = [(0, 2, 40, 0.3, 0.10, 1.6), (1, 3, 100, 0.5, 0.15, 0.8), (2, 5, 200, 0.6, 0.20, 0.45), (3, 8, 300, 0.7, 0.15, 0.3)]
ROUNDS, THRESHOLD, LAM, UP, DOWN, DEPTH = 8, 20.0, 1e-3, 10.0, 0.1, 6.5


def _exp(w):
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) + (np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K if th > 0 else K)


def ind_cost(Rs, ts, X, obs, cam, thr):
    """The truncated cost and the active mask [C, n] of a state, by whole-array numpy."""
    fx, fy, cx, cy = cam
    y = np.einsum("cij,nj->cni", Rs, X) + ts[:, None, :]
    with np.errstate(all="ignore"):
        e = (fx * y[..., 0] / y[..., 2] + cx - obs[..., 0]) ** 2 + (fy * y[..., 1] / y[..., 2] + cy - obs[..., 1]) ** 2
    act = (y[..., 2] > 0) & (e <= thr * thr)
    return float(np.sum(np.where(act, e, thr * thr))), act


def independent(poses, X, obs, cam, free, thr, rounds, lam, up, down, trace=None):
    """Dense Levenberg-Marquardt without the Schur complement: the full Jacobian of the active observations over the
    free cameras and the points with two or more of them, the normal equations with their diagonal scaled by
    1 + lambda, np.linalg.solve. Shares no code with ba_ref. Returns (Rs, ts, X, cost, accepted)."""
    fx, fy, cx, cy = cam
    Rs, ts, X = poses[:, :9].reshape(-1, 3, 3).copy(), poses[:, 9:].copy(), np.array(X, np.float64)
    obs = np.asarray(obs, np.float64)
    C, n = obs.shape[:2]
    cost, _ = ind_cost(Rs, ts, X, obs, cam, thr)
    done = 0
    for _ in range(rounds):
        _, act = ind_cost(Rs, ts, X, obs, cam, thr)
        pfree = np.flatnonzero(act.sum(0) >= 2)
        pcol = -np.ones(n, int)
        pcol[pfree] = 6 * len(free) + 3 * np.arange(len(pfree))
        ccol = {c: 6 * f for f, c in enumerate(free)}
        rows, res = [], []
        for c in range(C):
            for i in np.flatnonzero(act[c]):
                y = Rs[c] @ X[i] + ts[c]
                a, b, iz = y[0] / y[2], y[1] / y[2], 1.0 / y[2]
                dpi = np.array([[fx * iz, 0, -fx * a * iz], [0, fy * iz, -fy * b * iz]])  # d residual / d y
                row = np.zeros((2, 6 * len(free) + 3 * len(pfree)))
                if c in ccol:  # y' = y + w x y + delta
                    yx = np.array([[0, -y[2], y[1]], [y[2], 0, -y[0]], [-y[1], y[0], 0]])
                    row[:, ccol[c]:ccol[c] + 3] = dpi @ (-yx)
                    row[:, ccol[c] + 3:ccol[c] + 6] = dpi
                if pcol[i] >= 0:
                    row[:, pcol[i]:pcol[i] + 3] = dpi @ Rs[c]
                rows.append(row)
                res.append([fx * a + cx - obs[c, i, 0], fy * b + cy - obs[c, i, 1]])
        ok = False
        if rows and rows[0].shape[1]:
            J, r = np.concatenate(rows), np.array(res).reshape(-1)
            H = J.T @ J
            H[np.diag_indices_from(H)] *= 1.0 + lam
            try:
                step = np.linalg.solve(H, -J.T @ r)
                ok = bool(np.all(np.isfinite(step)))
            except np.linalg.LinAlgError:
                ok = False
        if ok:
            R2, t2, X2 = Rs.copy(), ts.copy(), X.copy()
            for c, k in ccol.items():
                E = _exp(step[k:k + 3])
                R2[c], t2[c] = E @ Rs[c], E @ ts[c] + step[k + 3:k + 6]
            X2[pfree] += step[6 * len(free):].reshape(-1, 3)
            c2, _ = ind_cost(R2, t2, X2, obs, cam, thr)
            ok = c2 < cost
        if trace is not None:
            trace.append((ok, lam))
        if ok:
            Rs, ts, X, cost, done = R2, t2, X2, c2, done + 1
            lam *= down
        else:
            lam *= up
    return Rs, ts, X, cost, done


@functools.lru_cache(maxsize=None)
def solved(k):
    seed, cams, n, noise, out, base = SCENES[k]
    sc = B.scene(1000 + seed, cams=cams, n=n, noise=noise, outliers=out, baseline=base, point_noise=0.06, rot=0.008, trans=0.04)
    c = B.case(sc, rounds=ROUNDS, threshold=THRESHOLD, lam=LAM, up=UP, down=DOWN)
    trace = []
    ref = B.run(c, trace=trace)
    free = list(range(2, cams))
    args = (sc["cam"], free, THRESHOLD, ROUNDS, LAM, UP, DOWN)
    X0 = sc["points0"].astype(np.float64)
    ind = independent(sc["poses0"], X0, sc["obs"], *args)
    costs = [ind[3]]
    for s in range(3):
        perm = np.random.default_rng(70 + s).permutation(n)
        costs.append(independent(sc["poses0"], X0[perm], sc["obs"][:, perm], *args)[3])
    planted = ind_cost(sc["poses"][:, :9].reshape(-1, 3, 3), sc["poses"][:, 9:], sc["points"], sc["obs"].astype(np.float64), sc["cam"], THRESHOLD)[0]
    return dict(sc=sc, case=c, ref=ref, trace=trace[0], ind=ind, ind_cost=ind[3], ind_rounds=ind[4], spread=(max(costs) - min(costs)) / ind[3],
                planted_cost=planted, free=free)


def _rot_err(Ra, Rb):
    return float(np.arccos(np.clip((np.trace(Ra @ Rb.T) - 1) / 2, -1, 1)))


def errors(r):
    """(rotation radians, translation, point RMS) errors against the planted state, summed over the free cameras
    and over the points with two or more planted-good observations: before, restatement, independent."""
    sc, free = r["sc"], r["free"]
    use = sc["good"].sum(0) >= 2
    def of(Rs, ts, X):
        rot = sum(_rot_err(Rs[c], sc["poses"][c, :9].reshape(3, 3)) for c in free)
        tr = sum(float(np.linalg.norm(ts[c] - sc["poses"][c, 9:])) for c in free)
        return rot, tr, float(np.sqrt(np.mean(np.sum((X[use] - sc["points"][use]) ** 2, 1))))
    p0 = sc["poses0"]
    before = of(p0[:, :9].reshape(-1, 3, 3), p0[:, 9:], sc["points0"].astype(np.float64))
    pr = r["ref"][0][0]
    ref = of(pr[:, :9].reshape(-1, 3, 3), pr[:, 9:], r["ref"][1][0].astype(np.float64))
    ind = of(r["ind"][0], r["ind"][1], r["ind"][2])
    return before, ref, ind


def _tolerance(spread, cost):
    """Twice the measured spread; a spread of exactly 0 counts as one ulp of the cost."""
    return 2.0 * (spread if spread > 0.0 else float(np.spacing(cost)) / cost)


@pytest.mark.parametrize("k", range(len(SCENES)))
def test_scene_condition_and_final_cost(k):
    r = solved(k)
    diff = abs(r["ref"][4][0, 1] - r["ind_cost"]) / r["ind_cost"]
    print(f"scene {k}: planted cost {r['planted_cost']:.3f} independent {r['ind_cost']:.6f} ({r['ind_cost'] / r['planted_cost']:.3f} x) "
          f"restatement {r['ref'][4][0, 1]:.6f} spread {r['spread']:.3e} difference {diff:.3e}")
    assert r["ind_cost"] < 1.5 * r["planted_cost"]          # the condition on the inputs
    assert diff <= _tolerance(r["spread"], r["ind_cost"])


@pytest.mark.parametrize("k", range(len(SCENES)))
def test_errors_against_the_planted_state(k):
    r = solved(k)
    seed, cams, n, noise, out, base = SCENES[k]
    before, ref, ind = errors(r)
    print(f"scene {k}: (rotation rad, translation, point RMS) before {before} restatement {ref} independent {ind}")
    active = max(int(r["ref"][2][0].sum()) // cams, 1)
    E = noise / (r["sc"]["cam"][0] * np.sqrt(active))
    nfree = len(r["free"])
    Ep = DEPTH * DEPTH * noise / (r["sc"]["cam"][0] * base * (cams - 1))
    assert ref[0] <= 2 * ind[0] + 2 * nfree * E and ref[1] <= 2 * ind[1] + 2 * nfree * DEPTH * E and ref[2] <= 2 * ind[2] + 2 * Ep
    assert ref[2] < before[2]
    if nfree:
        assert ref[0] < before[0] and ref[1] < before[1]


@pytest.mark.parametrize("k", range(len(SCENES)))
def test_cost_never_rises(k):
    r = solved(k)
    cost = r["ref"][4][0]
    assert cost[1] <= cost[0]
    last = cost[0]
    for valid, accepted, c, _ in r["trace"]:
        if accepted:
            assert valid and c < last
            last = c
    assert last == cost[1] and r["ref"][5][0] == sum(1 for t in r["trace"] if t[1])


def test_rejected_trials_leave_the_state():
    """The trailing rejected trials of a run change nothing: its poses and points are, bit for bit, those of the run
    that stops after the last accepted trial; and a run whose only trial is rejected returns the given state."""
    c = dict(B.all_cases())["rounds-16"]
    trace = []
    full = B.run(c, trace=trace)
    acc = [t[1] for t in trace[0]]
    last = max(i for i, a in enumerate(acc) if a) + 1
    assert last < len(acc) and not any(acc[last:])
    short = B.run(dict(c, rounds=last))
    for a, b in zip(full[:5], short[:5]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    g = dict(B.all_cases())["reject"]
    one = B.run(dict(g, rounds=1))
    assert one[5][0] == 0 and np.array_equal(one[0].view(np.uint64), g["poses"].view(np.uint64))
    assert np.array_equal(one[1].view(np.uint32), g["p"].view(np.uint32)) and one[4][0, 0] == one[4][0, 1]


def test_structure_only_equals_per_point_refinement():
    """Every camera held: the restatement against the independent solver with no free camera, within the margin of
    the final cost (the spread measured on this configuration)."""
    seed, cams, n, noise, out, base = SCENES[1]
    sc = B.scene(1000 + seed, cams=cams, n=n, noise=noise, outliers=out, baseline=base, point_noise=0.06, rot=0.0, trans=0.0)
    c = B.case(sc, fixed=np.ones((1, cams), np.uint8), rounds=ROUNDS, threshold=THRESHOLD, lam=LAM, up=UP, down=DOWN)
    ref = B.run(c)
    args = (sc["cam"], [], THRESHOLD, ROUNDS, LAM, UP, DOWN)
    X0 = sc["points0"].astype(np.float64)
    ind = independent(sc["poses0"], X0, sc["obs"], *args)
    costs = [ind[3]]
    for s in range(3):
        perm = np.random.default_rng(80 + s).permutation(n)
        costs.append(independent(sc["poses0"], X0[perm], sc["obs"][:, perm], *args)[3])
    spread = (max(costs) - min(costs)) / ind[3]
    diff = abs(ref[4][0, 1] - ind[3]) / ind[3]
    print(f"structure-only: independent {ind[3]:.6f} restatement {ref[4][0, 1]:.6f} spread {spread:.3e} difference {diff:.3e}")
    assert ref[5][0] >= 1 and np.array_equal(ref[0].view(np.uint64), c["poses"].view(np.uint64))
    assert diff <= _tolerance(spread, ind[3])
    assert np.max(np.abs(ref[1][0].astype(np.float64) - ind[2])) <= 1e-5  # float32 points: half an ulp at depth 9 is 5e-7


def test_motion_only_first_step_is_pnp_gauss_newton():
    """Every point held (one observation each, all of camera 1, the only free camera) and lambda -> 0: the accepted
    first trial moves camera 1 by fd_pnp_refit's Gauss-Newton step."""
    lam = 1e-12
    sc = P.scene(7, n=80, outliers=0.0, noise=0.5)
    rng = np.random.default_rng(3)
    pose0 = B.perturb_pose(rng, B.pose12(sc["R"], sc["t_vec"]), 0.002, 0.01)
    poses = np.stack([B.IDENTITY, pose0])[None]
    obs = np.stack([np.zeros_like(sc["t"]), sc["t"]])[None]
    ov = np.stack([np.zeros(80, np.uint8), np.ones(80, np.uint8)])[None]
    out = B.bundle_adjust_ref(poses, sc["p"][None], obs, fixed=np.array([[1, 0]], np.uint8), obs_valid=ov, cam=sc["cam"], rounds=1,
                              threshold=50.0, lam=lam)
    assert out[5][0] == 1 and np.array_equal(out[1].view(np.uint32), sc["p"][None].view(np.uint32))
    corr, _ = P.correspondences(sc["p"], sc["t"], None, None, None, None, sc["cam"], (0.0, 0.0, 0.0), 1.0)
    member = np.ones(len(corr), bool)

    def pnp_step(corr, damp):
        A = P.gn_system(pose0, corr, member, sc["cam"])
        A[np.arange(6), np.arange(6)] *= damp
        x, valid = P.null_vector(A[None])
        assert valid[0]
        return P.cayley_update(pose0, x[0])[0]

    plain = pnp_step(corr, 1.0)
    damping = np.max(np.abs(pnp_step(corr, 1.0 + lam) - plain))
    order = np.max(np.abs(pnp_step(corr[::-1].copy(), 1.0) - plain))
    got = np.max(np.abs(out[0][0, 1] - plain))
    print(f"motion-only: damping {damping:.3e} order {order:.3e} bundle adjustment {got:.3e}")
    assert got <= 2.0 * (damping + order)
