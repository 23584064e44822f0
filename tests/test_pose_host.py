"""CPU checks of fd_pose_recover's and fd_triangulate's yardstick tests/pose_ref.py (the numpy restatement of
the contract in include/fd_hip.h) and of what the entry points answer without a GPU."""
import ctypes

import numpy as np
import pytest

import pose_ref as P
import ransac_ref as R
import refit_ref as F

ACCURACY_SEEDS = tuple(range(6))  # scene(seed, n=96, outliers=24), F estimated by the fd_ransac and refit restatements
PLANTED_SEEDS = tuple(range(16))  # noise-free scene(seed) with the planted pose's own F


@pytest.fixture(scope="module")
def cases():
    return P.all_cases()


@pytest.fixture(scope="module")
def estimated():
    """seed -> (scene, refit restatement outputs (model, inliers, ...)) of the accuracy scenes."""
    out = {}
    for seed in ACCURACY_SEEDS:
        sc = P.scene(seed, n=96, outliers=24)
        q, t = sc["q"][None], sc["t"][None]
        ran = R.ransac_ref(q, t, model=R.FUNDAMENTAL, hypotheses=F.HYP, seed=seed, center=F.CENTER, scale=F.SCALE)
        out[seed] = (sc, F.refit_ref(q, t, ran[0], ran[1], model=R.FUNDAMENTAL, rounds=2, center=F.CENTER, scale=F.SCALE))
    return out


def every_case(cases, estimated):
    """Every scene of the pose tests, as case dicts: the GPU cases, the planted scenes, the estimated ones."""
    out = list(cases) + [(f"planted-{s}", P.case(P.scene(s))) for s in PLANTED_SEEDS]
    out += [(f"estimated-{s}", P.case(sc, in_model=fit[0], in_inlier=fit[1])) for s, (sc, fit) in estimated.items()]
    return out


# ---- the contract once more, in plain loops over float64 scalars ---------------------------------------------
def plain_jacobi(A, sweeps):
    n = len(A)
    A = [[np.float64(v) for v in row] for row in A]
    V = [[np.float64(1.0 if i == k else 0.0) for k in range(n)] for i in range(n)]
    for _ in range(sweeps):
        for p in range(n - 1):
            for q in range(p + 1, n):
                apq = A[p][q]
                if apq == 0.0:
                    continue
                app, aqq = A[p][p], A[q][q]
                theta = (aqq - app) / (np.float64(2.0) * apq)
                t = np.float64(-1.0 if theta < 0 else 1.0) / (abs(theta) + np.sqrt(theta * theta + np.float64(1.0)))
                c = np.float64(1.0) / np.sqrt(t * t + np.float64(1.0))
                s = t * c
                for k in range(n):
                    if k != p and k != q:
                        akp, akq = A[k][p], A[k][q]
                        A[k][p] = A[p][k] = c * akp - s * akq
                        A[k][q] = A[q][k] = s * akp + c * akq
                A[p][p], A[q][q] = app - t * apq, aqq + t * apq
                A[p][q] = A[q][p] = np.float64(0.0)
                for k in range(n):
                    vkp, vkq = V[k][p], V[k][q]
                    V[k][p], V[k][q] = c * vkp - s * vkq, s * vkp + c * vkq
    return [A[i][i] for i in range(n)], V


def plain_step(Rm, tv, ax, ay, bx, by, D, m):
    one = np.float64(1.0)
    r = [Rm[i][0] * ax + Rm[i][1] * ay + Rm[i][2] for i in range(3)]
    pr = [bx, by, one]
    dot = lambda a, b: a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
    rr, pp, rp, rt, pt = dot(r, r), dot(pr, pr), dot(r, pr), dot(r, tv), dot(pr, tv)
    det = rr * pp - rp * rp
    z1 = (rp * pt - pp * rt) / det
    z2 = (rr * pt - rp * rt) / det
    front = bool(det > (m * m) * (rr * pp)) and bool(z1 > 0) and bool(z2 > 0) and bool(z1 <= D) and bool(z2 <= D)
    return front, [np.float32(z1 * ax), np.float32(z1 * ay), np.float32(z1)]


def plain_frame(c, b, sweeps):
    """One frame of fd_pose_recover: (pose [12], choice, {slot: point}, counts of the four candidates or None)."""
    f64 = np.float64
    q, t = c["q"][b], c["t"][b]
    S, T = q.shape[0], t.shape[0]
    nq = S if c["counts"] is None else min(int(c["counts"][b]) & R.COUNT_MASK, S)
    (fxq, fyq, cxq, cyq), (fxt, fyt, cxt, cyt) = [[f64(v) for v in cam] for cam in (c["cam_q"], c["cam_t"])]
    D, m = f64(np.float32(c["max_depth"])), f64(np.float32(c["min_parallax"]))
    pairs = []
    for i in range(nq):
        j = i if c["idx"] is None else int(c["idx"][b, i])
        if (c["valid"] is not None and c["valid"][b, i] != 1) or not 0 <= j < T or c["in_inlier"][b, i] != 1:
            continue
        x, y, u, v = f64(q[i, 0]), f64(q[i, 1]), f64(t[j, 0]), f64(t[j, 1])
        if np.isfinite(x) and np.isfinite(y) and np.isfinite(u) and np.isfinite(v):
            pairs.append((i, (x - cxq) / fxq, (y - cyq) / fyq, (u - cxt) / fxt, (v - cyt) / fyt))
    Fm = [[f64(c["in_model"][b, 3 * i + k]) for k in range(3)] for i in range(3)]
    z, one = f64(0.0), f64(1.0)
    Kq, KtT = [[fxq, z, cxq], [z, fyq, cyq], [z, z, one]], [[fxt, z, z], [z, fyt, z], [cxt, cyt, one]]

    def mul(a, bm):
        out = [[z] * 3 for _ in range(3)]
        for i in range(3):
            for k in range(3):
                acc = f64(0.0)
                for l in range(3):
                    acc = acc + a[i][l] * bm[l][k]
                out[i][k] = acc
        return out

    E = mul(KtT, mul(Fm, Kq))
    G = [[z] * 3 for _ in range(3)]
    for i in range(3):
        for k in range(3):
            acc = f64(0.0)
            for l in range(3):
                acc = acc + E[l][i] * E[l][k]
            G[i][k] = acc
    d, V = plain_jacobi(G, sweeps)
    j = 0
    for i in range(1, 3):
        if d[i] < d[j]:
            j = i
    a, bb = [i for i in range(3) if i != j]
    v1, v2 = [V[k][a] for k in range(3)], [V[k][bb] for k in range(3)]
    w1 = [E[i][0] * v1[0] + E[i][1] * v1[1] + E[i][2] * v1[2] for i in range(3)]
    w2 = [E[i][0] * v2[0] + E[i][1] * v2[1] + E[i][2] * v2[2] for i in range(3)]
    n1 = np.sqrt(w1[0] * w1[0] + w1[1] * w1[1] + w1[2] * w1[2])
    n2 = np.sqrt(w2[0] * w2[0] + w2[1] * w2[1] + w2[2] * w2[2])
    u1, u2 = [w / n1 for w in w1], [w / n2 for w in w2]
    cross = lambda p, r: [p[1] * r[2] - p[2] * r[1], p[2] * r[0] - p[0] * r[2], p[0] * r[1] - p[1] * r[0]]
    u3, v3 = cross(u1, u2), cross(v1, v2)
    Ra = [[(u2[i] * v1[k] - u1[i] * v2[k]) + u3[i] * v3[k] for k in range(3)] for i in range(3)]
    Rb = [[(u1[i] * v2[k] - u2[i] * v1[k]) + u3[i] * v3[k] for k in range(3)] for i in range(3)]
    used = d + v1 + v2 + u3 + [x for row in Ra + Rb for x in row]
    none = (np.zeros(12), -1, {}, None)
    if not all(np.isfinite(x) for x in used) or not min(d[a], d[bb]) > f64(1e-12) * max(d):
        return none
    four = [(Ra, u3), (Ra, [-x for x in u3]), (Rb, u3), (Rb, [-x for x in u3])]
    counts = [sum(plain_step(Rm, tv, *p[1:], D, m)[0] for p in pairs) for Rm, tv in four]
    best = 0
    for k in range(1, 4):
        if counts[k] > counts[best]:
            best = k
    if counts[best] == 0:
        return none[:3] + (counts,)
    Rm, tv = four[best]
    pts = {}
    for p in pairs:
        front, pt = plain_step(Rm, tv, *p[1:], D, m)
        if front:
            pts[p[0]] = pt
    return np.array([x for row in Rm for x in row] + list(tv), np.float64), best, pts, counts


def test_restatement_equals_plain_loops(cases, estimated):
    """Every output of pose_ref on every scene of these tests, bit for bit, against the contract written once
    more as plain loops over float64 scalars; triangulate_ref with the winner's pose gives the same points."""
    with np.errstate(all="ignore"):
        for name, c in every_case(cases, estimated):
            det = []
            pose, choice, pts, val, cnt = P.run_pose(c, detail=det)
            for b in range(c["q"].shape[0]):
                ppose, pchoice, ppts, pcounts = plain_frame(c, b, P.SWEEPS)
                assert pchoice == choice[b] and pcounts == det[b], (name, b)
                assert np.array_equal(ppose.view(np.uint64), pose[b].view(np.uint64)), (name, b)
                assert sorted(ppts) == np.flatnonzero(val[b]).tolist() and cnt[b] == len(ppts), (name, b)
                for s, pt in ppts.items():
                    assert np.array_equal(np.array(pt, np.float32).view(np.uint32), pts[b, s].view(np.uint32)), (name, b, s)
                assert not pts[b][val[b] == 0].any()
            if np.all(choice >= 0):
                tri = P.run_triangulate(c, pose)
                assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(tri, (pts, val, cnt))), name


def test_sweep_count_rule(cases, estimated):
    """FD_POSE_SWEEPS = 2 + the smallest sweep count after which no later sweep changes a bit of the diagonal or
    of V, over E^T E of every frame of these tests' scenes that has pose candidates."""
    worst, frames = 0, 0
    for name, c in every_case(cases, estimated):
        for b in range(c["q"].shape[0]):
            trace = []
            if P.candidates(c["in_model"][b], c["cam_q"], c["cam_t"], 24, trace=trace) is None:
                continue
            bits = [np.concatenate([d.view(np.uint64), V.view(np.uint64).ravel()]) for d, V in trace]
            k = next(k + 1 for k in range(24) if all(np.array_equal(bits[k], bits[j]) for j in range(k + 1, 24)))
            worst, frames = max(worst, k), frames + 1
    print("sweeps until no bit changes:", worst, "frames:", frames)
    assert frames >= 40 and P.SWEEPS == worst + 2
    header = open(R.__file__.replace("tests/ransac_ref.py", "include/fd_hip.h")).read()
    assert f"#define FD_POSE_SWEEPS {P.SWEEPS}\n" in header


@pytest.mark.parametrize("seed", PLANTED_SEEDS)
def test_planted_pose_is_chosen_and_every_inlier_valid(seed):
    """Noise-free scene, the planted pose's own F: of the four candidates the restatement picks the one nearest
    the planted pose, marks every planted inlier valid and no other slot, and the points are the planted ones
    at the scale |t| = 1."""
    sc = P.scene(seed)
    c = P.case(sc)
    pose, choice, pts, val, cnt = P.run_pose(c)
    Ra, Rb, u3 = P.candidates(sc["model"], sc["cam_q"], sc["cam_t"])
    four = [(Ra, u3), (Ra, [-v for v in u3]), (Rb, u3), (Rb, [-v for v in u3])]
    dist = [P.rotation_angle(np.array(Rm), sc["R"]) + P.direction_angle(tv, sc["t_vec"]) for Rm, tv in four]
    assert choice[0] == int(np.argmin(dist)) and dist[choice[0]] < 1e-6
    assert np.array_equal(val[0] == 1, sc["planted"]) and cnt[0] == sc["planted"].sum()
    X = sc["X"][sc["planted"]] / np.linalg.norm(sc["t_vec"])
    # float32 pixels are off by up to 2^-24 * 640 px = 7.6e-8 rad per ray at f = 500; the rays of the farthest
    # point (depth 9 / 0.3 baselines) meet at 1 / 30 rad: 2 * 7.6e-8 * 30 = 4.6e-6 of the point's distance
    err = np.linalg.norm(pts[0][sc["planted"]] - X, axis=1) / np.linalg.norm(X, axis=1)
    assert err.max() < 1e-5 and abs(np.linalg.norm(pose[0, 9:]) - 1.0) < 1e-14
    Rm = pose[0, :9].reshape(3, 3)
    assert np.allclose(Rm.T @ Rm, np.eye(3), atol=1e-14) and abs(np.linalg.det(Rm) - 1.0) < 1e-14


def test_every_choice_wins():
    for k, seed in P.CHOICE_SEEDS.items():
        assert P.run_pose(P.case(P.scene(seed)))[1][0] == k


def test_cases_reach_what_they_are_for(cases):
    """The outcomes the GPU cases are built for, on the restatement."""
    C = dict(cases)
    det = []
    tie = P.run_pose(C["tie"], detail=det)
    assert sorted(det[0]) == [0, 0, 32, 32] and tie[1][0] == det[0].index(32) and tie[4][0] == 32
    assert not tie[3][0, 32:].any() or not tie[3][0, :32].any()  # one half of the scene, whole
    det = []
    none = P.run_pose(C["count0"], detail=det)
    assert det[0] == [0, 0, 0, 0] and none[1][0] == -1 and not none[0].any()
    det = []
    rot = P.run_pose(C["rotation"], detail=det)
    assert det[0] == [0, 0, 0, 0] and rot[1][0] == -1  # rank 2, candidates exist, no ray pair has parallax
    assert P.candidates(np.zeros(9), P.CAM, P.CAM) is None
    rank1 = np.outer([1.0, 2.0, 3.0], [0.5, -1.0, 2.0]).reshape(9)
    assert P.candidates(rank1, P.CAM, P.CAM) is None
    for name in ("depth", "parallax"):
        c = C[name]
        got, free = P.run_pose(c), P.run_pose(dict(c, max_depth=P.MAX_DEPTH, min_parallax=0.0))
        assert 0 < got[4][0] < free[4][0] == c["in_inlier"].sum(), name
    batch = P.run_pose(C["batch"])
    assert batch[1][0] == -1 and batch[1][1] >= 0 and batch[1][2] >= 0 and batch[4][1] < batch[4][2]
    holes = C["holes"]
    assert {0, 1, 2, 0xFF} <= set(holes["in_inlier"].ravel().tolist()) and P.run_pose(holes)[4].min() >= 20
    assert sorted({P.run_pose(C[f"stride-{s}"])[1][0] >= 0 for s in (8, 255, 256, 257, 513)}) == [True]


def test_accuracy_against_an_independent_solution(estimated):
    """Rotation angle and translation-direction angle to the planted pose, and the largest relative depth error
    over the planted inliers the restatement marks valid, of the restatement and of an independent
    np.linalg.svd decomposition of E with linear (DLT) triangulation in float64, on the same float32 pixels and
    the same estimated F (fd_ransac and refit restatements, 96 pairs, 24 outliers). Both are dominated by the
    float32 rounding of the pixels; the restatement may be up to ten times the independent solution's error.
    Measured over the six scenes (restatement / independent): rotation 2.2e-08..1.9e-04 rad, translation
    direction 9.8e-08..2.4e-03 rad, both equal to the independent solution's to four digits on every scene;
    relative depth 4.9e-07..1.3e-03 / 4.9e-07..1.4e-03, the largest ratio 1.28. The upper ends are scene 1,
    whose refit keeps one outlier (73 inliers of 72 planted)."""
    for seed, (sc, fit) in estimated.items():
        c = P.case(sc, in_model=fit[0], in_inlier=fit[1])
        pose, choice, pts, val, cnt = P.run_pose(c)
        assert choice[0] >= 0
        use = (val[0] == 1) & sc["planted"]
        Ri, ti, zi = P.independent_solution(fit[0][0], sc["q"], sc["t"], sc["cam_q"], sc["cam_t"])
        truth = sc["X"][:, 2] / np.linalg.norm(sc["t_vec"])
        mine = (P.rotation_angle(pose[0, :9], sc["R"]), P.direction_angle(pose[0, 9:], sc["t_vec"]),
                float(np.max(np.abs(pts[0][use, 2].astype(np.float64) - truth[use]) / truth[use])))
        other = (P.rotation_angle(Ri, sc["R"]), P.direction_angle(ti, sc["t_vec"]),
                 float(np.max(np.abs(zi[use] - truth[use]) / truth[use])))
        print(f"seed {seed}: rotation {mine[0]:.3e} / {other[0]:.3e} rad, direction {mine[1]:.3e} / {other[1]:.3e} rad, "
              f"depth {mine[2]:.3e} / {other[2]:.3e}, valid {cnt[0]}")
        assert use.sum() >= 60 and all(a <= 10.0 * b for a, b in zip(mine, other)), (seed, mine, other)


def test_null_context_struct_size_and_exports():
    import feature_detector_amd as fd
    from feature_detector_amd._lib import fd_pose_opts

    L = fd.load()
    buf = np.zeros(64, np.float64)
    p = ctypes.c_void_p(buf.ctypes.data)
    opts = fd_pose_opts(500.0, 500.0, 320.0, 240.0, 500.0, 500.0, 320.0, 240.0, 10.0, 0.0)
    assert L.fd_pose_recover(None, 1, ctypes.byref(opts), p, None, 4, p, 4, None, None, p, p, p, None, None, None, None, 0) == \
        fd._lib.FD_ERR_INVALID
    assert L.fd_triangulate(None, 1, ctypes.byref(opts), p, None, 4, p, 4, None, None, p, None, None, None, None, 0) == \
        fd._lib.FD_ERR_INVALID
    assert ctypes.sizeof(fd_pose_opts) == 72 and fd_pose_opts.max_depth.offset == 64 and L.fd_abi_version() == 6
    assert {"fd_pose_recover", "fd_triangulate"} <= set(fd._lib.EXPORTS)
    assert all(hasattr(fd, n) for n in ("recover_pose", "triangulate", "PoseResult", "PointsResult"))
    assert fd.geometry.intrinsics(np.array([[500.0, 0, 320], [0, 510, 240], [0, 0, 1]])) == (500.0, 510.0, 320.0, 240.0)
    for bad in (np.array([[500.0, 1e-9, 320], [0, 510, 240], [0, 0, 1]]), (0.0, 500.0, 1.0, 1.0), (500.0, 500.0, float("nan"), 1.0),
                np.eye(4)):
        with pytest.raises(ValueError):
            fd.geometry.intrinsics(bad)
