"""numpy restatement of fd_bundle_adjust (include/fd_hip.h): windowed bundle adjustment by Levenberg-Marquardt with
the points eliminated by the Schur complement, the contract's arithmetic sequence in elementwise float64 numpy
(IEEE, one rounding per operation), vectorised over the points where the contract's order allows. The GPU tests
compare every output with it bit for bit.

Every ordered sum is explicit: a sum over the points in ascending order is np.add.accumulate (sequential, unlike
the pairwise np.sum) over terms that are 0.0 where the contract skips one. Adding +0.0 is exact here: a sum that
starts at +0.0 is never -0.0, so x + 0.0 == x bit for bit.

Also the planted scenes of the tests (scene) and the cases the GPU tests run (all_cases).
"""
import numpy as np

from pnp_ref import cayley_update
from pose_ref import CAM, kmat, planted_pose, rotation_angle  # noqa: F401
from ransac_ref import COLS, COUNT_MASK, ROWS

LANES = 256
REG_EPS = 1e-12
IDENTITY = np.array([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0, 0, 0, 0], np.float64)


def _f(x):
    return np.float64(x)


def seq_sum(terms):
    """Sum over axis 0 from 0.0 in ascending order, one rounding per addition."""
    terms = np.asarray(terms, np.float64)
    if terms.shape[0] == 0:
        return np.zeros(terms.shape[1:], np.float64)
    return np.add.accumulate(np.concatenate([np.zeros((1,) + terms.shape[1:]), terms], 0), axis=0)[-1]


def tree_sum(P):
    """The contract's tree over 256 partials."""
    P = np.array(P, np.float64)
    step = LANES // 2
    while step >= 1:
        P[:step] = P[:step] + P[step:2 * step]
        step //= 2
    return P[0]


# ---- projection, cost ------------------------------------------------------------------------------------------
def project(pose, X):
    """y [n, 3] of the points X [n, 3] under pose [12], each row summed left to right."""
    R, t = pose[:9], pose[9:]
    return np.stack([((R[3 * k] * X[:, 0] + R[3 * k + 1] * X[:, 1]) + R[3 * k + 2] * X[:, 2]) + t[k] for k in range(3)], 1)


def terms(pose, X, ray, cam, tt):
    """(term [n], active [n], y [n, 3]) of one camera's observations."""
    fx, fy = _f(cam[0]), _f(cam[1])
    with np.errstate(all="ignore"):
        y = project(pose, X)
        front = y[:, 2] > 0.0
        a, b = y[:, 0] / y[:, 2], y[:, 1] / y[:, 2]
        dx, dy = fx * (a - ray[:, 0]), fy * (b - ray[:, 1])
        e = dx * dx + dy * dy
        active = front & (e <= tt)
    return np.where(active, e, tt), active, y


def state_cost(poses, X, rays, exists, cam, tt):
    """(cost, active [C, n]) of a state."""
    C, n = exists.shape
    T, A = np.zeros((C, n)), np.zeros((C, n), bool)
    for c in range(C):
        T[c], A[c], _ = terms(poses[c], X, rays[c], cam, tt)
    A &= exists
    P = np.zeros(LANES, np.float64)
    for base in range(0, n, LANES):
        m = min(LANES, n - base)
        for c in range(C):
            P[:m] = np.where(exists[c, base:base + m], P[:m] + T[c, base:base + m], P[:m])
    return tree_sum(P), A


# ---- the elimination at run-time size ----------------------------------------------------------------------------
def solve(A):
    """The step of the R x (R + 1) system [S | rhs] by Gaussian elimination with complete pivoting (fd_ransac's
    rules), back substitution with the columns descending, x[j] / x[R]. Returns (step [R], valid)."""
    A = np.array(A, np.float64)
    R = A.shape[0]
    if R == 0:
        return np.zeros(0), True
    C = R + 1
    perm = np.arange(C)
    valid, p0 = True, None
    with np.errstate(all="ignore"):
        for k in range(R):
            mag = np.abs(A[k:, k:])
            mag = np.where(np.isnan(mag), -2.0, mag).reshape(-1)  # a NaN never wins
            arg = int(np.argmax(mag))                             # first of the largest: strict >
            best = mag[arg]
            if best < 0.0:                                        # nothing beat -1: the pivot stays (k, k)
                best, arg = _f(-1.0), 0
            pr, pc = k + arg // (C - k), k + arg % (C - k)
            if k == 0:
                p0 = best
            valid = valid and bool(best > _f(REG_EPS) * p0)
            A[[k, pr], k:] = A[[pr, k], k:]
            A[:, [k, pc]] = A[:, [pc, k]]
            perm[[k, pc]] = perm[[pc, k]]
            f = A[k + 1:, k] / A[k, k]
            A[k + 1:, k + 1:] = A[k + 1:, k + 1:] - f[:, None] * A[k, k + 1:][None, :]
        y = np.zeros(C)
        y[R] = 1.0
        s = np.zeros(R)
        for c in range(R, 0, -1):
            s[:c] = s[:c] + A[:c, c] * y[c]
            y[c - 1] = (0.0 - s[c - 1]) / A[c - 1, c - 1]
        x = np.zeros(C)
        x[perm] = y
        step = x[:R] / x[R]
    valid = valid and bool(np.all(np.isfinite(x))) and bool(np.all(np.isfinite(step)))
    return step, valid


# ---- one trial's linearisation -----------------------------------------------------------------------------------
def linearise(poses, X, rays, exists, cam, tt, damp, free):
    """Steps 1 to 3 of the contract: dict with the system A [R, R + 1] and what the update needs."""
    fx, fy = _f(cam[0]), _f(cam[1])
    C, n = exists.shape
    one = _f(1.0)
    act = np.zeros((C, n), bool)
    JX, JY, PX, PY = (np.zeros((C, n, k)) for k in (7, 7, 3, 3))
    with np.errstate(all="ignore"):
        for c in range(C):
            _, a_, y = terms(poses[c], X, rays[c], cam, tt)
            act[c] = a_ & exists[c]
            Rm = poses[c][:9]
            iz = one / y[:, 2]
            a, b = y[:, 0] * iz, y[:, 1] * iz
            zero = np.zeros(n)
            JX[c] = np.stack([fx * -(a * b), fx * (one + a * a), fx * -b, fx * iz, zero, fx * -(a * iz), fx * (a - rays[c][:, 0])], 1)
            JY[c] = np.stack([fy * -(one + b * b), fy * (a * b), fy * a, zero, fy * iz, fy * -(b * iz), fy * (b - rays[c][:, 1])], 1)
            PX[c] = np.stack([(fx * iz) * (Rm[k] - a * Rm[6 + k]) for k in range(3)], 1)
            PY[c] = np.stack([(fy * iz) * (Rm[3 + k] - b * Rm[6 + k]) for k in range(3)], 1)
        # point blocks
        V, g = np.zeros((n, 3, 3)), np.zeros((n, 3))
        for c in range(C):
            m = act[c]
            for k in range(3):
                for l in range(k, 3):
                    acc = V[:, k, l] + PX[c][:, k] * PX[c][:, l]
                    acc = acc + PY[c][:, k] * PY[c][:, l]
                    V[:, k, l] = np.where(m, acc, V[:, k, l])
                acc = g[:, k] + PX[c][:, k] * JX[c][:, 6]
                acc = acc + PY[c][:, k] * JY[c][:, 6]
                g[:, k] = np.where(m, acc, g[:, k])
        nact = act.sum(0)
        d0, d1, d2 = V[:, 0, 0] * damp, V[:, 1, 1] * damp, V[:, 2, 2] * damp
        V01, V02, V12 = V[:, 0, 1], V[:, 0, 2], V[:, 1, 2]
        c00, c01, c02 = d1 * d2 - V12 * V12, V02 * V12 - V01 * d2, V01 * V12 - V02 * d1
        c11, c12, c22 = d0 * d2 - V02 * V02, V01 * V02 - d0 * V12, d0 * d1 - V01 * V01
        det = (d0 * c00 + V01 * c01) + V02 * c02
        elim = (nact >= 2) & np.isfinite(det) & (det > _f(REG_EPS) * ((d0 * d1) * d2))
        I = np.zeros((n, 3, 3))
        for (k, l), ckl in (((0, 0), c00), ((0, 1), c01), ((0, 2), c02), ((1, 1), c11), ((1, 2), c12), ((2, 2), c22)):
            I[:, k, l] = I[:, l, k] = ckl / det
        F = len(free)
        W, Y = np.zeros((F, n, 6, 3)), np.zeros((F, n, 6, 3))
        for f, c in enumerate(free):
            W[f] = JX[c][:, :6, None] * PX[c][:, None, :] + JY[c][:, :6, None] * PY[c][:, None, :]
            Y[f] = (W[f][:, :, 0:1] * I[:, None, 0, :] + W[f][:, :, 1:2] * I[:, None, 1, :]) + W[f][:, :, 2:3] * I[:, None, 2, :]
        # the Schur system: every entry two sums over the points in ascending order
        R = 6 * F
        A = np.zeros((R, R + 1))
        for f, c in enumerate(free):
            m = act[c][:, None, None]
            tx = np.where(m, JX[c][:, :6, None] * JX[c][:, None, :], 0.0)
            ty = np.where(m, JY[c][:, :6, None] * JY[c][:, None, :], 0.0)
            U = seq_sum(np.stack([tx, ty], 1).reshape(2 * n, 6, 7))
            me = (act[c] & elim)[:, None]
            Eg = seq_sum(np.where(me, (Y[f][:, :, 0] * g[:, None, 0] + Y[f][:, :, 1] * g[:, None, 1]) + Y[f][:, :, 2] * g[:, None, 2], 0.0))
            for f2 in range(f, F):
                both = (act[c] & act[free[f2]] & elim)[:, None, None]
                t3 = (Y[f][:, :, None, 0] * W[f2][:, None, :, 0] + Y[f][:, :, None, 1] * W[f2][:, None, :, 1]) \
                    + Y[f][:, :, None, 2] * W[f2][:, None, :, 2]
                E = seq_sum(np.where(both, t3, 0.0))
                for r in range(6):
                    for s in range(6):
                        ra, cb = 6 * f + r, 6 * f2 + s
                        if ra > cb:
                            continue
                        u = U[r, s] if f2 == f else _f(0.0)
                        if ra == cb:
                            u = u * damp
                        A[ra, cb] = A[cb, ra] = u - E[r, s]
            for r in range(6):
                A[6 * f + r, R] = U[r, 6] - Eg[r]
    return dict(A=A, act=act, elim=elim, W=W, I=I, g=g)


def trial(poses, X, rays, exists, cam, tt, lam, free):
    """One trial's candidate: (poses', X', valid)."""
    damp = _f(1.0) + lam
    L = linearise(poses, X, rays, exists, cam, tt, damp, free)
    step, valid = solve(L["A"])
    if not valid:
        return poses, X, False
    cand = poses.copy()
    for f, c in enumerate(free):
        cand[c], fin = cayley_update(poses[c], step[6 * f:6 * f + 6])
        valid = valid and fin
    with np.errstate(all="ignore"):
        v = L["g"].copy()
        for f, c in enumerate(free):
            m = L["act"][c]
            for r in range(6):
                for k in range(3):
                    v[:, k] = np.where(m, v[:, k] + L["W"][f][:, r, k] * step[6 * f + r], v[:, k])
        I = L["I"]
        Xn = np.stack([X[:, k] - ((I[:, k, 0] * v[:, 0] + I[:, k, 1] * v[:, 1]) + I[:, k, 2] * v[:, 2]) for k in range(3)], 1)
    Xn = np.where(L["elim"][:, None], Xn, X)
    valid = valid and bool(np.all(np.isfinite(Xn[L["elim"]])))
    return cand, Xn, valid


def adjust_problem(poses, fixed, p, p_valid, count, obs, obs_valid, cam, rounds, threshold, lam, up, down, trace=None):
    """One problem. Returns (poses [C, 12], X [n, 3] float64, participates [n], inlier [C, n], (cost0, cost), accepted).
    trace (a list) receives per trial (valid, accepted, cost', lambda)."""
    poses = np.array(poses, np.float64).reshape(-1, 12)
    C = poses.shape[0]
    p = np.asarray(p, np.float32)
    S = p.shape[0]
    n = S if count is None else min(int(count) & COUNT_MASK, S)
    obs = np.asarray(obs, np.float32)
    t = _f(np.float32(threshold))
    tt = t * t
    fx, fy, cx, cy = (_f(v) for v in cam)
    pf = p[:n].astype(np.float64)
    pok = np.all(np.isfinite(pf), axis=1)
    if p_valid is not None:
        pok &= np.asarray(p_valid)[:n] == 1
    exists, rays = np.zeros((C, n), bool), np.zeros((C, n, 2))
    with np.errstate(all="ignore"):
        for c in range(C):
            uv = obs[c, :n].astype(np.float64)
            exists[c] = pok & np.all(np.isfinite(uv), axis=1)
            if obs_valid is not None:
                exists[c] &= np.asarray(obs_valid)[c, :n] == 1
            rays[c] = np.stack([(uv[:, 0] - cx) / fx, (uv[:, 1] - cy) / fy], 1)
    free = [c for c in range(C) if (c != 0 if fixed is None else int(fixed[c]) == 0)]
    X = pf.copy()
    cost0, _ = state_cost(poses, X, rays, exists, cam, tt)
    cost, lam, done = cost0, _f(lam), 0
    for _ in range(rounds):
        cp, cX, valid = trial(poses, X, rays, exists, cam, tt, lam, free)
        accept, cn = False, None
        if valid:
            cn, _ = state_cost(cp, cX, rays, exists, cam, tt)
            accept = bool(cn < cost)
        if trace is not None:
            trace.append((valid, accept, cn, float(lam)))
        if accept:
            poses, X, cost, done = cp, cX, cn, done + 1
            lam = lam * _f(down)
        else:
            lam = lam * _f(up)
    _, inl = state_cost(poses, X, rays, exists, cam, tt)
    return poses, X, exists.any(0), inl, (cost0, cost), done


def bundle_adjust_ref(poses, p, obs, fixed=None, p_valid=None, counts=None, obs_valid=None, cam=CAM, rounds=8, threshold=2.0,
                      lam=1e-3, up=10.0, down=0.1, fill_points=0.0, fill_inlier=0, trace=None):
    """fd_bundle_adjust. Returns (poses float64 [B, C, 12], points float32 [B, S, 3], inlier uint8 [B, C, O], counts int32
    [B], cost float64 [B, 2], rounds int32 [B]); slots the call does not write hold the fills."""
    poses = np.array(poses, np.float64)
    B, C = poses.shape[0], poses.shape[1]
    p, obs = np.asarray(p, np.float32), np.asarray(obs, np.float32)
    S, O = p.shape[1], obs.shape[2]
    out_p = np.full((B, S, 3), fill_points, np.float32)
    out_i = np.full((B, C, O), fill_inlier, np.uint8)
    out_c, out_cost, out_r = np.zeros(B, np.int32), np.zeros((B, 2), np.float64), np.zeros(B, np.int32)
    if S == 0:
        return poses, out_p, out_i, out_c, out_cost, out_r
    for b in range(B):
        tr = [] if trace is not None else None
        ps, X, part, inl, cost, done = adjust_problem(
            poses[b], None if fixed is None else fixed[b], p[b], None if p_valid is None else p_valid[b],
            None if counts is None else counts[b], obs[b], None if obs_valid is None else obs_valid[b], cam, rounds, threshold,
            lam, up, down, trace=tr)
        if trace is not None:
            trace.append(tr)
        n = X.shape[0]
        poses[b] = ps
        with np.errstate(all="ignore"):
            out_p[b, :n] = np.where(part[:, None], X.astype(np.float32), p[b, :n])
        keep = ~part
        out_p[b, :n].view(np.uint32)[keep] = p[b, :n].view(np.uint32)[keep]  # the input's bits, a NaN's payload included
        out_i[b, :, :n] = inl
        out_c[b], out_cost[b], out_r[b] = int(inl.sum()), cost, done
    return poses, out_p, out_i, out_c, out_cost, out_r


# ---- planted scenes ----------------------------------------------------------------------------------------------
def pose12(R, t):
    return np.concatenate([np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64).reshape(3)])


def perturb_pose(rng, pose, rot, trans):
    """pose [12] with a small rotation (radians, per axis sigma) and translation noise applied on the left."""
    w = rng.normal(0.0, rot, 3)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    E = np.eye(3) + (np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K if th > 0 else K)
    R, t = pose[:9].reshape(3, 3), pose[9:]
    return pose12(E @ R, E @ t + rng.normal(0.0, trans, 3))


def scene(seed, cams=3, n=64, noise=0.5, outliers=0.15, rot=0.0015, trans=0.006, point_noise=0.008, baseline=0.45, cam=CAM):
    """n seeded points seen by `cams` cameras on a short arc, `baseline` apart (camera 0 the identity), image noise of `noise` px, a
    fraction `outliers` of the observations replaced by uniform positions; the given poses (cameras 2.. only: 0 and
    1 keep the planted ones, which pins the scale) and points are perturbed from the planted ones. Returns a dict:
    poses0 / points0 (given), poses / points (planted), obs float32 [cams, n, 2], good bool [cams, n], cam."""
    rng = np.random.default_rng(52000 + seed)
    K = np.array(kmat(cam), np.float64)
    planted = [IDENTITY.copy()]
    for c in range(1, cams):
        ang = 0.05 * c
        Rm = np.array([[np.cos(ang), 0, -np.sin(ang)], [0, 1, 0], [np.sin(ang), 0, np.cos(ang)]])
        w = rng.normal(0.0, 0.01, 3)
        Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        planted.append(pose12((np.eye(3) + Kx) @ Rm, [-baseline * c + rng.normal(0, 0.03), rng.normal(0, 0.03), 0.05 * c]))
    for c in range(1, cams):  # a proper rotation
        U, _, Vt = np.linalg.svd(planted[c][:9].reshape(3, 3))
        planted[c][:9] = (U @ Vt).reshape(9)
    planted = np.array(planted)
    X = []
    while len(X) < n:
        x = np.array([rng.uniform(-2.5, 2.5), rng.uniform(-1.8, 1.8), rng.uniform(4.0, 9.0)])
        ok = True
        for c in range(cams):
            y = K @ (planted[c][:9].reshape(3, 3) @ x + planted[c][9:])
            ok = ok and y[2] > 1.0 and 0 <= y[0] / y[2] <= COLS - 1 and 0 <= y[1] / y[2] <= ROWS - 1
        if ok:
            X.append(x)
    X = np.array(X)
    obs, good = np.zeros((cams, n, 2)), np.ones((cams, n), bool)
    for c in range(cams):
        y = (X @ planted[c][:9].reshape(3, 3).T + planted[c][9:]) @ K.T
        obs[c] = y[:, :2] / y[:, 2:3] + rng.normal(0.0, noise, (n, 2))
        bad = rng.choice(n, int(round(outliers * n)), replace=False)
        good[c, bad] = False
        obs[c, bad] = np.stack([rng.uniform(0, COLS - 1, len(bad)), rng.uniform(0, ROWS - 1, len(bad))], 1)
    poses0 = planted.copy()
    for c in range(2, cams):
        poses0[c] = perturb_pose(rng, planted[c], rot, trans)
    points0 = (X + rng.normal(0.0, point_noise, X.shape)).astype(np.float32)
    return dict(poses0=poses0, points0=points0, poses=planted, points=X, obs=obs.astype(np.float32), good=good, cam=tuple(cam))


# ---- the cases of the GPU tests ----------------------------------------------------------------------------------
def case(sc, **kw):
    """A case dict of one scene (batch 1): cameras 0 and 1 held."""
    C = sc["poses0"].shape[0]
    fixed = np.zeros((1, C), np.uint8)
    fixed[0, :2] = 1
    d = dict(poses=sc["poses0"][None].copy(), fixed=fixed, p=sc["points0"][None].copy(), p_valid=None, counts=None,
             obs=sc["obs"][None].copy(), obs_valid=None, cam=sc["cam"], rounds=4, threshold=2.0, lam=1e-3, up=10.0, down=0.1)
    d.update(kw)
    return d


def stack(cases, **kw):
    d = dict(cases[0])
    for k in ("poses", "fixed", "p", "obs"):
        d[k] = np.concatenate([c[k] for c in cases], 0)
    d.update(kw)
    return d


def run(c, fill_points=0.0, fill_inlier=0, trace=None):
    return bundle_adjust_ref(c["poses"], c["p"], c["obs"], c["fixed"], c["p_valid"], c["counts"], c["obs_valid"], cam=c["cam"],
                             rounds=c["rounds"], threshold=c["threshold"], lam=c["lam"], up=c["up"], down=c["down"],
                             fill_points=fill_points, fill_inlier=fill_inlier, trace=trace)


def n_case(n):
    """Three cameras, n points of a stride of max(n, 1)."""
    return case(scene(100 + n, cams=3, n=max(n, 1)), counts=np.array([n], np.int32), rounds=3)


def cams_case(kind):
    if kind == "1-held":
        return case(scene(200, cams=1, n=40), fixed=np.ones((1, 1), np.uint8))
    if kind == "2":
        return case(scene(201, cams=2, n=40), fixed=np.array([[1, 0]], np.uint8))
    if kind == "7-free":
        return case(scene(202, cams=8, n=70), fixed=np.array([[1, 0, 0, 0, 0, 0, 0, 0]], np.uint8), rounds=3)
    if kind == "8-free":  # R = 48, the largest system: no camera held, the gauge left to the damping
        return case(scene(205, cams=8, n=70), fixed=np.zeros((1, 8), np.uint8), rounds=3)
    if kind == "8-held":
        return case(scene(203, cams=8, n=70), fixed=np.ones((1, 8), np.uint8), rounds=3)
    return case(scene(204, cams=8, n=70), fixed=None, rounds=3)  # "8-null"


def reject_case():
    """A tiny lambda far from the optimum: the first trial overshoots and is rejected, a later, damped one is accepted
    (tests/test_gpu_ba.py asserts both from the restatement's trace)."""
    return case(scene(300, cams=4, n=60, rot=0.05, trans=0.25, point_noise=0.3), lam=1e-9, up=1e3, rounds=6, threshold=8.0)


def gauge_case():
    """One held camera, down = 1 and a tiny lambda: the scale gauge is all but undamped (whatever the pivot test says
    of it, the restatement and the kernel agree)."""
    return case(scene(301, cams=3, n=48, noise=0.0, outliers=0.0, point_noise=0.0, rot=0.0, trans=0.0),
                fixed=np.array([[1, 0, 0]], np.uint8), lam=1e-300, down=1.0, rounds=2)


def held_points_case():
    """Slot 0: seen once. Slot 1: every observation behind its camera. Slot 2: two parallel rays (the point on the
    common optical axis of cameras 0 and 1, camera 2 not seeing it)."""
    sc = scene(302, cams=3, n=40)
    sc["poses0"][1] = pose12(np.eye(3), [0.0, 0.0, -1.0])
    sc["poses0"][1][:9] = IDENTITY[:9]
    d = case(sc)
    ov = np.ones((1, 3, 40), np.uint8)
    ov[0, 1:, 0] = 0
    d["p"][0, 1] = (0.3, -0.2, -5.0)
    d["p"][0, 2] = (0.0, 0.0, 5.0)
    ov[0, 2, 2] = 0
    cx, cy = sc["cam"][2], sc["cam"][3]
    d["obs"][0, 0, 2] = (cx + 0.25, cy - 0.5)
    d["obs"][0, 1, 2] = (cx - 0.5, cy + 0.25)
    d["obs_valid"] = ov
    return d


def all_held_case():
    """Every point held: each has one valid observation (camera i mod 3); cameras 1 and 2 free (motion-only)."""
    d = case(scene(303, cams=3, n=60, outliers=0.0), fixed=np.array([[1, 0, 0]], np.uint8))
    ov = np.zeros((1, 3, 60), np.uint8)
    ov[0, np.arange(60) % 3, np.arange(60)] = 1
    d["obs_valid"] = ov
    return d


def masks_case():
    """p_valid and obs_valid bytes 0..6, a NaN / inf in each of the five coordinate places, counts below the stride with
    the flag bits 25..31 set, o_stride > p_stride."""
    rng = np.random.default_rng(17)
    S, O = 90, 101
    sc = scene(304, cams=4, n=S)
    d = case(sc)
    obs = np.full((1, 4, O, 2), np.nan, np.float32)
    obs[0, :, :S] = sc["obs"]
    pv = np.where(rng.random((1, S)) < 0.2, rng.integers(0, 7, (1, S)), 1).astype(np.uint8)
    ov = np.where(rng.random((1, 4, O)) < 0.2, rng.integers(0, 7, (1, 4, O)), 1).astype(np.uint8)
    p = d["p"]
    p[0, 30, 0], p[0, 31, 1], p[0, 32, 2], obs[0, 1, 33, 0], obs[0, 2, 34, 1] = np.nan, np.inf, -np.inf, np.nan, np.inf
    hi = sum(1 << k for k in range(25, 32))
    d.update(obs=obs, p_valid=pv, obs_valid=ov, counts=np.array([77 | hi], np.uint32).view(np.int32))
    return d


def batch_case():
    """Batch 5 of three cameras, stride 70: a plain problem, counts 0, every camera held, the rejecting damping of
    reject_case's kind, and a short count."""
    frames = [case(scene(400 + k, cams=3, n=70, rot=0.03 if k == 3 else 0.0015, trans=0.2 if k == 3 else 0.006)) for k in range(5)]
    d = stack(frames, counts=np.array([70, 0, 70, 70, 9], np.int32))
    d["fixed"][2] = 1
    return d


def all_cases():
    """(name, case) of every scene the GPU tests compare with the restatement."""
    out = [(f"n-{n}", n_case(n)) for n in (0, 1, 2, 255, 256, 257, 600)]
    out += [(f"cams-{k}", cams_case(k)) for k in ("1-held", "2", "7-free", "8-free", "8-held", "8-null")]
    out += [("rounds-1", case(scene(500, cams=3, n=50), rounds=1)), ("rounds-16", case(scene(500, cams=3, n=50), rounds=16)),
            ("reject", reject_case()), ("gauge", gauge_case()), ("held-points", held_points_case()), ("all-held", all_held_case()),
            ("masks", masks_case()), ("batch", batch_case())]
    return out
