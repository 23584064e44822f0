"""numpy restatement of fd_pnp_ransac and fd_pnp_refit (include/fd_hip.h): the camera pose from 3-D - 2-D
correspondences, the contract's arithmetic sequence in scalar and elementwise float64 numpy (IEEE, one rounding
per operation), vectorised over the hypotheses. The GPU tests compare every output with it bit for bit. The
sampler is fd_ransac's (tests/ransac_ref.py), the Jacobi routine fd_ransac_refit's (tests/refit_ref.py); the
elimination is ransac_ref.null_vector generalised from 8 x 9 to R x (R + 1).

Also the planted scenes of the tests (scene), an independent solution (np.linalg.svd DLT and a dense
Gauss-Newton) and the cases the GPU tests run (all_cases).
"""
import numpy as np

from pose_ref import CAM, direction_angle, kmat, planted_pose, rotation_angle  # noqa: F401
from ransac_ref import COLS, COUNT_MASK, ROWS, sample
from refit_ref import jacobi

SWEEPS = 7        # FD_POSE_SWEEPS: tests/test_pnp_host.py::test_sweep_count_rule confirms it for these scenes
RANK_EPS = 1e-12
LANES = 256
M = 6             # picks per hypothesis
R_PNP = 11        # rows of the DLT system
GN = [(i, j) for i in range(6) for j in range(i, 7)]  # the 27 summed entries of [N | g], in this order


def _f(x):
    return np.float64(x)


# ---- the correspondence list --------------------------------------------------------------------------------
def correspondences(p_xyz, t_xy, count, match_idx, pair_valid, p_valid, cam, center, scale):
    """([n, 5] float64 (Xc, Yc, Zc, bx, by), slot index [n]) of one frame."""
    p_xyz, t_xy = np.asarray(p_xyz, np.float32), np.asarray(t_xy, np.float32)
    s, ts = p_xyz.shape[0], t_xy.shape[0]
    nq = s if count is None else min(int(count) & COUNT_MASK, s)
    fx, fy, cx, cy = (_f(v) for v in cam)
    c, sc = [_f(v) for v in center], _f(scale)
    rows, slots = [], []
    with np.errstate(all="ignore"):
        for i in range(nq):
            if pair_valid is not None and int(pair_valid[i]) != 1:
                continue
            if p_valid is not None and int(p_valid[i]) != 1:
                continue
            j = i if match_idx is None else int(match_idx[i])
            if not 0 <= j < ts:
                continue
            v = np.array([p_xyz[i, 0], p_xyz[i, 1], p_xyz[i, 2], t_xy[j, 0], t_xy[j, 1]], np.float64)
            if not np.all(np.isfinite(v)):
                continue
            rows.append([(v[0] - c[0]) * sc, (v[1] - c[1]) * sc, (v[2] - c[2]) * sc, (v[3] - cx) / fx, (v[4] - cy) / fy])
            slots.append(i)
    return np.array(rows, np.float64).reshape(-1, 5), np.array(slots, np.int64)


# ---- the elimination, R x (R + 1) ---------------------------------------------------------------------------
def null_vector(A):
    """Null vectors of the systems A [H, R, R + 1] by Gaussian elimination with complete pivoting
    (ransac_ref.null_vector with R for 8). Returns (x [H, R + 1], valid [H])."""
    A = np.array(A, np.float64)
    nh, R = A.shape[0], A.shape[1]
    C = R + 1
    hh = np.arange(nh)
    perm = np.tile(np.arange(C), (nh, 1))
    valid = np.ones(nh, bool)
    p0 = None
    with np.errstate(all="ignore"):
        for k in range(R):
            mag = np.abs(A[:, k:, k:])
            mag = np.where(np.isnan(mag), -2.0, mag).reshape(nh, -1)  # a NaN never wins
            arg = np.argmax(mag, axis=1)                               # first of the largest: strict >
            best = mag[hh, arg]
            none = best < 0.0                                          # nothing beat -1: the pivot stays (k, k)
            best = np.where(none, -1.0, best)
            arg = np.where(none, 0, arg)
            pr, pc = k + arg // (C - k), k + arg % (C - k)
            if k == 0:
                p0 = best
            valid &= best > 1e-12 * p0
            rk, rp = A[hh, k, :].copy(), A[hh, pr, :].copy()
            A[hh, k, :], A[hh, pr, :] = rp, rk
            ck, cp = A[hh, :, k].copy(), A[hh, :, pc].copy()
            A[hh, :, k], A[hh, :, pc] = cp, ck
            a, b = perm[hh, k].copy(), perm[hh, pc].copy()
            perm[hh, k], perm[hh, pc] = b, a
            for r in range(k + 1, R):
                f = A[:, r, k] / A[:, k, k]
                for c in range(k + 1, C):
                    A[:, r, c] = A[:, r, c] - f * A[:, k, c]
        x = np.zeros((nh, C))
        x[:, R] = 1.0
        for k in range(R - 1, -1, -1):
            s = np.zeros(nh)
            for c in range(k + 1, C):
                s = s + A[:, k, c] * x[:, c]
            x[:, k] = (0.0 - s) / A[:, k, k]
    out = np.zeros((nh, C))
    for c in range(C):
        out[hh, perm[:, c]] = x[:, c]
    valid &= np.all(np.isfinite(out), axis=1)
    return out, valid


# ---- fd_pnp_ransac ------------------------------------------------------------------------------------------
def build_rows(pts):
    """pts [H, 6, 5] -> the 11 x 12 systems [H, 11, 12]."""
    X, Y, Z, bx, by = (pts[..., i] for i in range(5))
    one, zero = np.ones_like(X), np.zeros_like(X)
    with np.errstate(all="ignore"):
        r0 = np.stack([X, Y, Z, one, zero, zero, zero, zero, -(bx * X), -(bx * Y), -(bx * Z), -bx], axis=-1)
        r1 = np.stack([zero, zero, zero, zero, X, Y, Z, one, -(by * X), -(by * Y), -(by * Z), -by], axis=-1)
    return np.stack([r0, r1], axis=2).reshape(pts.shape[0], 12, 12)[:, :R_PNP, :]


def fix_sign(P, valid):
    """det of the left block in the contract's order; (P with det < 0 negated, valid and det usable)."""
    p = [P[:, i] for i in range(12)]
    with np.errstate(all="ignore"):
        det = (p[0] * (p[5] * p[10] - p[6] * p[9]) - p[1] * (p[4] * p[10] - p[6] * p[8])) + p[2] * (p[4] * p[9] - p[5] * p[8])
    ok = valid & (det != 0.0) & np.isfinite(det)
    return np.where((det < 0.0)[:, None], -P, P), ok


def inliers(P, corr, cam, tt):
    """P [H, 12], corr [n, 5] -> bool [H, n] by the contract's test (a NaN fails the compare)."""
    fx, fy = _f(cam[0]), _f(cam[1])
    p = [P[:, i][:, None] for i in range(12)]
    X, Y, Z, bx, by = (corr[:, i][None, :] for i in range(5))
    with np.errstate(all="ignore"):
        y0 = ((p[0] * X + p[1] * Y) + p[2] * Z) + p[3]
        y1 = ((p[4] * X + p[5] * Y) + p[6] * Z) + p[7]
        w = ((p[8] * X + p[9] * Y) + p[10] * Z) + p[11]
        dx = fx * (y0 - bx * w)
        dy = fy * (y1 - by * w)
        return (w > 0.0) & (dx * dx + dy * dy <= tt * (w * w))


def hypotheses_ref(corr, b, hypotheses, seed):
    """(P [H, 12], valid [H]) of one frame's correspondences."""
    n = corr.shape[0]
    picks = [sample(seed, b, h, n, M) for h in range(hypotheses)]
    ok = np.array([p is not None for p in picks], bool)
    pts = np.zeros((hypotheses, M, 5))
    for h, p in enumerate(picks):
        if p is not None:
            pts[h] = corr[p]
    P, valid = null_vector(build_rows(pts))
    return fix_sign(P, valid & ok)


def gram(P12):
    """G = M^T M of the left block, sums from 0.0 with k ascending."""
    Mm = [[_f(P12[4 * i + j]) for j in range(3)] for i in range(3)]
    G = np.zeros((3, 3), np.float64)
    with np.errstate(all="ignore"):
        for i in range(3):
            for j in range(3):
                acc = _f(0.0)
                for k in range(3):
                    acc = acc + Mm[k][i] * Mm[k][j]
                G[i, j] = acc
    return Mm, G


def to_pose(P12, center, scale, sweeps=SWEEPS, trace=None):
    """The winner's pose [12] (R row-major, then t), or None."""
    c, sc = [_f(v) for v in center], _f(scale)
    Mm, G = gram(P12)
    with np.errstate(all="ignore"):
        d, V = jacobi(G, sweeps, trace=trace)
        dmin, dmax = d[0], d[0]
        for k in range(1, 3):
            if d[k] < dmin:
                dmin = d[k]
            if d[k] > dmax:
                dmax = d[k]
        ok = bool(np.all(np.isfinite(d))) and bool(dmin > _f(RANK_EPS) * dmax)
        sd = [np.sqrt(d[k]) for k in range(3)]
        W = [[_f(0.0)] * 3 for _ in range(3)]
        for i in range(3):
            for j in range(3):
                acc = _f(0.0)
                for k in range(3):
                    acc = acc + Mm[i][k] * V[k, j]
                W[i][j] = acc
        ks = ((sd[0] + sd[1]) + sd[2]) / _f(3.0)
        R, t = np.zeros((3, 3), np.float64), np.zeros(3, np.float64)
        for i in range(3):
            for k in range(3):
                acc = _f(0.0)
                for j in range(3):
                    acc = acc + (W[i][j] / sd[j]) * V[k, j]
                R[i, k] = acc
            tc = _f(P12[4 * i + 3]) / ks
            t[i] = tc / sc - ((R[i, 0] * c[0] + R[i, 1] * c[1]) + R[i, 2] * c[2])
    if not (ok and np.all(np.isfinite(V)) and np.all(np.isfinite(R)) and np.all(np.isfinite(t))):
        return None
    return np.concatenate([R.reshape(9), t])


def pose_matrix(pose):
    """[R | t] row-major [12] of a pose stored R, then t."""
    pose = np.asarray(pose, np.float64)
    return np.concatenate([np.concatenate([pose[3 * i:3 * i + 3], pose[9 + i:10 + i]]) for i in range(3)])


def _frames(p_xyz, t_xy, q_counts, match_idx, pair_valid, p_valid, cam, center, scale):
    p_xyz, t_xy = np.asarray(p_xyz, np.float32), np.asarray(t_xy, np.float32)
    B, S = p_xyz.shape[0], p_xyz.shape[1]
    for b in range(B):
        cnt = None if q_counts is None else q_counts[b]
        nq = S if cnt is None else min(int(cnt) & COUNT_MASK, S)
        corr, slots = correspondences(p_xyz[b], t_xy[b], cnt, None if match_idx is None else match_idx[b],
                                      None if pair_valid is None else pair_valid[b], None if p_valid is None else p_valid[b],
                                      cam, center, scale)
        yield b, nq, corr, slots


def pnp_ransac_ref(p_xyz, t_xy, p_valid=None, q_counts=None, match_idx=None, pair_valid=None, cam=CAM, hypotheses=256, seed=0,
                   threshold=2.0, center=(0.0, 0.0, 0.0), scale=1.0, fill=0, sweeps=SWEEPS, detail=None):
    """fd_pnp_ransac. Returns (pose float64 [B, 12], inlier uint8 [B, S], counts int32 [B], best int32 [B]); inlier
    slots the call does not write hold `fill`. detail (a list) receives per frame (scores [H], valid [H], P [H, 12])."""
    p_xyz = np.asarray(p_xyz, np.float32)
    B, S = p_xyz.shape[0], p_xyz.shape[1]
    t = _f(np.float32(threshold))
    tt = t * t
    out_pose, out_inl = np.zeros((B, 12), np.float64), np.full((B, S), fill, np.uint8)
    out_cnt, out_best = np.zeros(B, np.int32), np.full(B, -1, np.int32)
    for b, nq, corr, slots in _frames(p_xyz, t_xy, q_counts, match_idx, pair_valid, p_valid, cam, center, scale):
        out_inl[b, :nq] = 0
        P, valid = hypotheses_ref(corr, b, hypotheses, seed)
        inl = inliers(P, corr, cam, tt) if corr.shape[0] else np.zeros((hypotheses, 0), bool)
        score = inl.sum(axis=1)
        if detail is not None:
            detail.append((score, valid, P))
        if not valid.any():
            continue
        best = int(np.argmax(np.where(valid, score, -1)))  # first of the largest: the lowest index
        pose = to_pose(P[best], center, scale, sweeps)
        if pose is None:
            continue
        out_best[b], out_pose[b] = best, pose
        out_inl[b, slots[inl[best]]] = 1
        out_cnt[b] = int(score[best])
    return out_pose, out_inl, out_cnt, out_best


# ---- fd_pnp_refit -------------------------------------------------------------------------------------------
def gn_system(pose, corr, member, cam):
    """The 6 x 7 system [N | g] of the members of corr [n, 5] under pose [12], in the contract's order: 256
    partials by list position modulo 256, ascending, then the tree."""
    fx, fy = _f(cam[0]), _f(cam[1])
    R, t = [_f(v) for v in pose[:9]], [_f(v) for v in pose[9:]]
    n = corr.shape[0]
    P = np.zeros((LANES, len(GN)), np.float64)
    one = _f(1.0)
    with np.errstate(all="ignore"):
        for base in range(0, n, LANES):
            pts, take = np.zeros((LANES, 5), np.float64), np.zeros(LANES, bool)
            m = min(LANES, n - base)
            pts[:m], take[:m] = corr[base:base + m], member[base:base + m]
            X, Y, Z, bx, by = (pts[:, i] for i in range(5))
            y = [((R[3 * i] * X + R[3 * i + 1] * Y) + R[3 * i + 2] * Z) + t[i] for i in range(3)]
            iz = one / y[2]
            a, b = y[0] * iz, y[1] * iz
            zero = np.zeros(LANES)
            jx = [fx * -(a * b), fx * (one + a * a), fx * -b, fx * iz, zero, fx * -(a * iz), fx * (a - bx)]
            jy = [fy * -(one + b * b), fy * (a * b), fy * a, zero, fy * iz, fy * -(b * iz), fy * (b - by)]
            for e, (i, j) in enumerate(GN):
                acc = P[:, e] + jx[i] * jx[j]
                acc = acc + jy[i] * jy[j]
                P[:, e] = np.where(take, acc, P[:, e])
        step = LANES // 2
        while step >= 1:
            P[:step] = P[:step] + P[step:2 * step]
            step //= 2
    A = np.zeros((6, 7), np.float64)
    for e, (i, j) in enumerate(GN):
        A[i, j] = P[0, e]
        if j < 6:
            A[j, i] = P[0, e]
    return A


def cayley_update(pose, x):
    """The pose after the step x = (w, delta): (pose [12], finite)."""
    R, t = [_f(v) for v in pose[:9]], [_f(v) for v in pose[9:]]
    two, one, zero = _f(2.0), _f(1.0), _f(0.0)
    with np.errstate(all="ignore"):
        h = [_f(x[i]) / two for i in range(3)]
        hh = (h[0] * h[0] + h[1] * h[1]) + h[2] * h[2]
        f = two / (one + hh)
        K = [[zero, -h[2], h[1]], [h[2], zero, -h[0]], [-h[1], h[0], zero]]
        C = [[(one if i == j else zero) + f * (K[i][j] + (h[i] * h[j] - (hh if i == j else zero))) for j in range(3)]
             for i in range(3)]
        out = np.zeros(12, np.float64)
        for i in range(3):
            for j in range(3):
                acc = zero
                for k in range(3):
                    acc = acc + C[i][k] * R[3 * k + j]
                out[3 * i + j] = acc
            out[9 + i] = ((C[i][0] * t[0] + C[i][1] * t[1]) + C[i][2] * t[2]) + _f(x[3 + i])
    return out, bool(np.all(np.isfinite(out)))


def refit_frame(corr, member, pose, rounds, cam, tt, trace=None):
    """The rounds of one frame: (pose [12] or None when no round was accepted, member bool [n], c, accepted rounds).
    trace (a list) receives c_0 and every accepted c_r."""
    none = np.zeros(0, bool)
    cls = lambda p: inliers(pose_matrix(p)[None], corr, cam, tt)[0] if corr.shape[0] else none  # noqa: E731
    cur, count, done = np.asarray(pose, np.float64), int(cls(pose).sum()), 0
    if trace is not None:
        trace.append(count)
    for _ in range(rounds):
        x, valid = null_vector(gn_system(cur, corr, member, cam)[None])
        cand, finite = cayley_update(cur, x[0])
        if not (bool(valid[0]) and finite):
            break
        inl = cls(cand)
        if int(inl.sum()) < count:
            break
        cur, member, count, done = cand, inl, int(inl.sum()), done + 1
        if trace is not None:
            trace.append(count)
    return (cur if done else None), member, count, done


def pnp_refit_ref(p_xyz, t_xy, in_pose, in_inlier, p_valid=None, q_counts=None, match_idx=None, pair_valid=None, cam=CAM,
                  rounds=4, threshold=2.0, fill=0, trace=None):
    """fd_pnp_refit. Returns (pose float64 [B, 12], inlier uint8 [B, S], counts int32 [B], rounds int32 [B]); inlier
    slots the call does not write hold `fill`. trace (a list) receives every frame's [c_0, c_1, ...]."""
    p_xyz = np.asarray(p_xyz, np.float32)
    B, S = p_xyz.shape[0], p_xyz.shape[1]
    t = _f(np.float32(threshold))
    tt = t * t
    out_pose = np.array(in_pose, np.float64).reshape(B, 12).copy()
    out_inl = np.full((B, S), fill, np.uint8)
    out_cnt, out_rounds = np.zeros(B, np.int32), np.zeros(B, np.int32)
    in_inlier = np.asarray(in_inlier, np.uint8).reshape(B, S)
    for b, nq, corr, slots in _frames(p_xyz, t_xy, q_counts, match_idx, pair_valid, p_valid, cam, (0.0, 0.0, 0.0), 1.0):
        out_inl[b, :nq] = 0
        member = in_inlier[b, slots] == 1
        tr = [] if trace is not None else None
        pose, member, _, done = refit_frame(corr, member, out_pose[b].copy(), rounds, cam, tt, trace=tr)
        if trace is not None:
            trace.append(tr)
        out_inl[b, slots[member]] = 1
        out_cnt[b], out_rounds[b] = int(member.sum()), done
        if done:
            out_pose[b] = pose
    return out_pose, out_inl, out_cnt, out_rounds


# ---- planted scenes ---------------------------------------------------------------------------------------
def scene(seed, n=64, outliers=0.25, noise=0.5, cam=CAM, depth=(4.0, 9.0), planar=False, point_noise=0.0):
    """n seeded 3-D points (float32, the world frame) seen by a camera with a planted pose (R, t), X_t = R X + t:
    image positions with Gaussian noise of `noise` px, a fraction `outliers` of them (random slots) replaced by
    uniform random positions. Returns a dict: p float32 [n, 3], t float32 [n, 2], planted bool [n], R, t_vec, cam."""
    rng = np.random.default_rng(41000 + seed)
    R, tv = planted_pose(seed)
    K = np.array(kmat(cam), np.float64)
    p, t = [], []
    while len(p) < n:
        X = np.array([rng.uniform(-3, 3), rng.uniform(-2.2, 2.2), rng.uniform(*depth)])
        if planar == "tilted":
            X[2] = 6.0 + 0.3 * X[0] - 0.2 * X[1]
        elif planar:
            X[2] = 6.0
        X = X.astype(np.float32).astype(np.float64)
        y = K @ (R @ X + tv)
        if y[2] < 1.0:
            continue
        uv = y[:2] / y[2]
        if 0 <= uv[0] <= COLS - 1 and 0 <= uv[1] <= ROWS - 1:
            p.append(X)
            t.append(uv)
    p, t = np.array(p), np.array(t) + rng.normal(0.0, noise, (n, 2))
    k = int(round(outliers * n))
    planted = np.ones(n, bool)
    bad = rng.choice(n, k, replace=False)
    planted[bad] = False
    t[bad] = np.stack([rng.uniform(0, COLS - 1, k), rng.uniform(0, ROWS - 1, k)], axis=1)
    return dict(p=p.astype(np.float32), t=t.astype(np.float32), planted=planted, R=R, t_vec=tv, cam=tuple(cam))


def conditioning(p):
    """A fixed conditioning of a scene's points: (centre, scale) = (their mean, 1 / their RMS distance from it),
    rounded to float32 values so that every caller passes the same doubles."""
    p = np.asarray(p, np.float64).reshape(-1, 3)
    c = p.mean(0)
    spread = np.sqrt(np.mean(np.sum((p - c) ** 2, axis=1)))
    s = 1.0 / spread if spread > 0 else 1.0
    return tuple(float(np.float32(v)) for v in c), float(np.float32(s))


def pose_errors(pose, sc):
    """(rotation angle in degrees, |t - t_planted|) of a pose [12] against the scene's."""
    return np.degrees(rotation_angle(pose[:9], sc["R"])), float(np.linalg.norm(np.asarray(pose[9:]) - sc["t_vec"]))


# ---- an independent solution: np.linalg.svd DLT on the same samples, a dense Gauss-Newton ---------------------
def _reproject(R, t, X, cam):
    y = X @ R.T + t
    return np.stack([cam[0] * y[:, 0] / y[:, 2] + cam[2], cam[1] * y[:, 1] / y[:, 2] + cam[3]], 1), y[:, 2]


def independent_ransac(sc, hypotheses, seed, threshold, b=0):
    """The same samples (fd_ransac's sampler), each solved by an SVD of the full 12 x 12 DLT system on
    normalised rays and centred points, scored by the reprojection error in pixels: (R, t, inlier bool [n])."""
    X, uv, cam = sc["p"].astype(np.float64), sc["t"].astype(np.float64), sc["cam"]
    n = len(X)
    c = X.mean(0)
    Xc = X - c
    rays = np.stack([(uv[:, 0] - cam[2]) / cam[0], (uv[:, 1] - cam[3]) / cam[1]], 1)
    best = (-1, None, None, None)
    for h in range(hypotheses):
        pk = sample(seed, b, h, n, M)
        if pk is None:
            continue
        A = []
        for i in pk:
            Xh = np.append(Xc[i], 1.0)
            A.append(np.concatenate([Xh, np.zeros(4), -rays[i, 0] * Xh]))
            A.append(np.concatenate([np.zeros(4), Xh, -rays[i, 1] * Xh]))
        _, sv, Vt = np.linalg.svd(np.array(A))
        if sv[10] < 1e-9 * sv[0]:
            continue
        P = Vt[-1].reshape(3, 4)
        if np.linalg.det(P[:, :3]) < 0:
            P = -P
        U, s, Wt = np.linalg.svd(P[:, :3])
        if s[2] < 1e-6 * s[0]:
            continue
        R = U @ Wt
        t = P[:, 3] / s.mean() - R @ c
        # score the projective matrix like the kernel, then keep the orthonormalised pose
        y = np.concatenate([Xc, np.ones((n, 1))], 1) @ P.T
        with np.errstate(all="ignore"):
            err = np.hypot(cam[0] * (y[:, 0] / y[:, 2] - rays[:, 0]), cam[1] * (y[:, 1] / y[:, 2] - rays[:, 1]))
        inl = (y[:, 2] > 0) & (err <= threshold)
        if inl.sum() > best[0]:
            best = (int(inl.sum()), R, t, inl)
    return best[1], best[2], best[3]


def independent_refine(sc, R, t, inl, rounds, threshold):
    """Plain dense Gauss-Newton (numerical SO(3) exponential, np.linalg.solve) on the inliers, which are
    classified again after every round."""
    X, uv, cam = sc["p"].astype(np.float64), sc["t"].astype(np.float64), sc["cam"]
    for _ in range(rounds):
        Xi, ui = X[inl], uv[inl]
        y = Xi @ R.T + t
        a, b, iz = y[:, 0] / y[:, 2], y[:, 1] / y[:, 2], 1.0 / y[:, 2]
        r = np.concatenate([cam[0] * a + cam[2] - ui[:, 0], cam[1] * b + cam[3] - ui[:, 1]])
        z = np.zeros_like(a)
        Jx = cam[0] * np.stack([-a * b, 1 + a * a, -b, iz, z, -a * iz], 1)
        Jy = cam[1] * np.stack([-(1 + b * b), a * b, a, z, iz, -b * iz], 1)
        J = np.concatenate([Jx, Jy])
        step = np.linalg.solve(J.T @ J, -J.T @ r)
        w, th = step[:3], np.linalg.norm(step[:3])
        Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        E = np.eye(3) + (np.sin(th) / th * Kx + (1 - np.cos(th)) / th ** 2 * Kx @ Kx if th > 0 else Kx)
        R, t = E @ R, E @ t + step[3:]
        proj, z2 = _reproject(R, t, X, cam)
        inl = (z2 > 0) & (np.hypot(*(proj - uv).T) <= threshold)
    return R, t, inl


# ---- the cases of the GPU tests -----------------------------------------------------------------------------
THRESHOLD = 2.0
HYP = 64


def case(sc, **kw):
    """A case dict of one scene (batch 1), conditioned by its points."""
    c, s = conditioning(sc["p"])
    d = dict(p=sc["p"][None].copy(), t=sc["t"][None].copy(), p_valid=None, counts=None, idx=None, valid=None, cam=sc["cam"],
             hypotheses=HYP, seed=3, threshold=THRESHOLD, center=c, scale=s)
    d.update(kw)
    return d


def stack(cases, **kw):
    d = dict(cases[0])
    for k in ("p", "t"):
        d[k] = np.concatenate([c[k] for c in cases], 0)
    d.update(kw)
    return d


def run_ransac(c, fill=0, detail=None, sweeps=SWEEPS):
    return pnp_ransac_ref(c["p"], c["t"], c["p_valid"], c["counts"], c["idx"], c["valid"], cam=c["cam"], hypotheses=c["hypotheses"],
                          seed=c["seed"], threshold=c["threshold"], center=c["center"], scale=c["scale"], fill=fill, detail=detail,
                          sweeps=sweeps)


def run_refit(c, in_pose, in_inlier, rounds, fill=0, trace=None):
    return pnp_refit_ref(c["p"], c["t"], in_pose, in_inlier, c["p_valid"], c["counts"], c["idx"], c["valid"], cam=c["cam"],
                         rounds=rounds, threshold=c["threshold"], fill=fill, trace=trace)


def n_case(n):
    """One frame of n correspondences, no outliers (small n must still give a pose from few samples)."""
    return case(scene(500 + n, n=max(n, 1), outliers=0.0 if n < 40 else 0.25), counts=np.array([n], np.int32))


def batch_case():
    """Batch 3, stride 90, a different n per frame; counts with the bits 25..31 set."""
    frames = [case(scene(600 + k, n=90)) for k in range(3)]
    hi = sum(1 << k for k in range(25, 32))
    return stack(frames, counts=np.array([90 | hi, 60 | hi, 7 | hi], np.uint32).view(np.int32))


def holes_case():
    """Batch 3: match_idx with -1, out-of-range and repeated entries, t_stride != q_stride, p_valid and pair_valid
    bytes 0..6, and a NaN / inf in each of the five coordinate places."""
    rng = np.random.default_rng(13)
    S, T = 90, 75
    d = stack([case(scene(700 + k, n=S)) for k in range(3)])
    idx = np.tile(np.arange(S, dtype=np.int32), (3, 1))
    idx[:, T:] = np.arange(S - T, dtype=np.int32) * 3
    d["t"] = np.ascontiguousarray(d["t"][:, :T])
    idx[:, 5], idx[:, 6], idx[:, 7], idx[:, 8] = -1, T, -2 ** 31, 2 ** 31 - 1
    idx[1, 20:30] = 3
    valid, pv = np.ones((3, S), np.uint8), np.ones((3, S), np.uint8)
    valid[0, 10:24] = np.arange(14) % 7
    valid[2] = np.where(rng.random(S) < 0.2, rng.integers(0, 7, S), 1)
    pv[1] = np.where(rng.random(S) < 0.2, rng.integers(0, 7, S), 1)
    pv[0, 40:47] = np.arange(7)
    p, t = d["p"], d["t"]
    p[0, 30, 0], p[0, 31, 1], p[0, 32, 2], t[0, 33, 0], t[0, 34, 1] = np.nan, np.inf, -np.inf, np.nan, np.inf
    d.update(idx=idx, valid=valid, p_valid=pv, counts=np.array([S, 70, 77], np.int32))
    return d


def coplanar_case(tilted=False):
    """Every point on one plane. Z = 6 is a plane in float32 too: the Z column is a multiple of the ones column,
    the elimination cancels exactly and every hypothesis fails the pivot test. A tilted plane is one only up to
    the points' float32 rounding: the pivots pass, the matrix fits the points, and its pose is arbitrary."""
    return case(scene(800, n=64, planar="tilted" if tilted else True, outliers=0.0))


def duplicate_case():
    """Every slot the same point and image position: no sample has 6 distinct rows, every pivot test fails."""
    sc = scene(801, n=12, outliers=0.0)
    sc["p"][:], sc["t"][:] = sc["p"][0], sc["t"][0]
    return case(sc)


def few_distinct_case():
    """n = 6 with hypotheses whose sampler finds no 6 distinct indices within 32 tries (tests/test_pnp_host.py
    confirms that some give up and some do not)."""
    return case(scene(802, n=6, outliers=0.0), hypotheses=256, seed=0)


def behind_case():
    """Every point behind the camera (the scene mirrored through the camera centre keeps its image positions)."""
    sc = scene(803, n=64, outliers=0.0, noise=0.0)
    Xc = sc["p"].astype(np.float64) @ sc["R"].T + sc["t_vec"]
    sc["p"] = ((-Xc - sc["t_vec"]) @ sc["R"]).astype(np.float32)
    return case(sc)


def all_cases():
    """(name, case) of every scene the GPU tests compare with the restatement."""
    out = [(f"n-{n}", n_case(n)) for n in (0, 5, 6, 7, 255, 256, 257, 600)]
    out += [(f"hyp-{h}", case(scene(900, n=48), hypotheses=h, seed=11)) for h in (1, 63, 64, 65, 4096)]
    out += [("batch", batch_case()), ("holes", holes_case()), ("coplanar", coplanar_case()), ("near-coplanar", coplanar_case(True)), ("duplicate", duplicate_case()),
            ("few-distinct", few_distinct_case()), ("behind", behind_case()),
            ("unconditioned", case(scene(901, n=80), center=(0.0, 0.0, 0.0), scale=1.0)),
            ("conditioned", case(scene(901, n=80), center=(0.25, -0.5, 6.0), scale=0.375))]
    return out
