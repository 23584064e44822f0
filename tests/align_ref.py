"""numpy restatement of fd_align_ransac, fd_align_refit and fd_align_apply (include/fd_hip.h): the similarity or
rigid transform Y = s R X + t between two 3-D point sets, the contract's arithmetic sequence in scalar and elementwise
float64 numpy (IEEE, one rounding per operation), vectorised over the hypotheses. The GPU tests compare every output
with it bit for bit. The sampler is fd_ransac's (tests/ransac_ref.py), the Jacobi routine fd_ransac_refit's
(tests/refit_ref.py).

Also the planted scenes of the tests (scene), an independent solution (an SVD Umeyama with the determinant fix on
the same samples and members) and the cases the GPU tests run (all_cases).
"""
import numpy as np

from pose_ref import rotation, rotation_angle  # noqa: F401
from ransac_ref import COUNT_MASK, sample
from refit_ref import jacobi

SIMILARITY, RIGID = 0, 1
SWEEPS = 7        # FD_ALIGN_SWEEPS: tests/test_align_host.py::test_sweep_count_rule confirms it for these scenes
FRAME_EPS = 1e-12
LANES = 256
M = 3             # picks per hypothesis
MODEL = 13        # R row-major, t, s


def _f(x):
    return np.float64(x)


def dot(a, b):
    """a.b of [..., 3] arrays, left to right."""
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


# ---- the correspondence list --------------------------------------------------------------------------------
def correspondences(q_xyz, t_xyz, count, match_idx, pair_valid, q_valid, t_valid):
    """([n, 6] float64 (X, Y), slot index [n]) of one frame."""
    q_xyz, t_xyz = np.asarray(q_xyz, np.float32), np.asarray(t_xyz, np.float32)
    s, ts = q_xyz.shape[0], t_xyz.shape[0]
    nq = s if count is None else min(int(count) & COUNT_MASK, s)
    rows, slots = [], []
    for i in range(nq):
        if pair_valid is not None and int(pair_valid[i]) != 1:
            continue
        if q_valid is not None and int(q_valid[i]) != 1:
            continue
        j = i if match_idx is None else int(match_idx[i])
        if not 0 <= j < ts:
            continue
        if t_valid is not None and int(t_valid[j]) != 1:
            continue
        v = np.concatenate([q_xyz[i], t_xyz[j]]).astype(np.float64)
        if not np.all(np.isfinite(v)):
            continue
        rows.append(v)
        slots.append(i)
    return np.array(rows, np.float64).reshape(-1, 6), np.array(slots, np.int64)


# ---- the model's map and the inlier test ----------------------------------------------------------------------
def apply_model(m, X):
    """z = s * (R X) + t for models m [..., 13] and points X [..., 3] (broadcast), the contract's expression."""
    with np.errstate(all="ignore"):
        return np.stack([m[..., 12] * ((m[..., 3 * i] * X[..., 0] + m[..., 3 * i + 1] * X[..., 1]) + m[..., 3 * i + 2] * X[..., 2])
                         + m[..., 9 + i] for i in range(3)], axis=-1)


def inliers(models, corr, tt):
    """models [H, 13], corr [n, 6] -> bool [H, n] (a NaN fails the compare)."""
    with np.errstate(all="ignore"):
        z = apply_model(models[:, None, :], corr[None, :, :3])
        e = corr[None, :, 3:] - z
        return (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2] <= tt


# ---- fd_align_ransac ----------------------------------------------------------------------------------------
def side_frame(u, v):
    """The frames (e1, e2, e3 [H, 3] each) of the sides u, v [H, 3] and their validity."""
    with np.errstate(all="ignore"):
        uu = dot(u, u)
        e1 = u / np.sqrt(uu)[:, None]
        d = dot(v, e1)
        w = v - d[:, None] * e1
        ww = dot(w, w)
        e2 = w / np.sqrt(ww)[:, None]
        e3 = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                       e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
        valid = (uu > 0.0) & (ww > _f(FRAME_EPS) * dot(v, v))
    return e1, e2, e3, valid


def side_lengths(u, v):
    g = v - u
    return (dot(u, u) + dot(v, v)) + dot(g, g)


def models_of(pts, kind):
    """pts [H, 3, 6] -> (models [H, 13], valid [H])."""
    Xa, Ya = pts[:, 0, :3], pts[:, 0, 3:]
    with np.errstate(all="ignore"):
        u, v = pts[:, 1, :3] - Xa, pts[:, 2, :3] - Xa
        U, V = pts[:, 1, 3:] - Ya, pts[:, 2, 3:] - Ya
        e1, e2, e3, ok_e = side_frame(u, v)
        f1, f2, f3, ok_f = side_frame(U, V)
        m = np.zeros((pts.shape[0], MODEL), np.float64)
        for i in range(3):
            for j in range(3):
                m[:, 3 * i + j] = (f1[:, i] * e1[:, j] + f2[:, i] * e2[:, j]) + f3[:, i] * e3[:, j]
        m[:, 12] = 1.0 if kind == RIGID else np.sqrt(side_lengths(U, V) / side_lengths(u, v))
        Xm = Xa + (u + v) / _f(3.0)
        Ym = Ya + (U + V) / _f(3.0)
        for i in range(3):
            m[:, 9 + i] = Ym[:, i] - m[:, 12] * ((m[:, 3 * i] * Xm[:, 0] + m[:, 3 * i + 1] * Xm[:, 1]) + m[:, 3 * i + 2] * Xm[:, 2])
        valid = ok_e & ok_f & np.all(np.isfinite(m), axis=1) & (m[:, 12] > 0.0)
    return m, valid


def hypotheses_ref(corr, b, hypotheses, seed, kind):
    """(models [H, 13], valid [H]) of one frame's correspondences."""
    n = corr.shape[0]
    picks = [sample(seed, b, h, n, M) for h in range(hypotheses)]
    ok = np.array([p is not None for p in picks], bool)
    pts = np.zeros((hypotheses, M, 6))
    for h, p in enumerate(picks):
        if p is not None:
            pts[h] = corr[p]
    m, valid = models_of(pts, kind)
    return m, valid & ok


def _frames(q_xyz, t_xyz, q_counts, match_idx, pair_valid, q_valid, t_valid):
    q_xyz, t_xyz = np.asarray(q_xyz, np.float32), np.asarray(t_xyz, np.float32)
    B, S = q_xyz.shape[0], q_xyz.shape[1]
    pick = lambda a, b: None if a is None else a[b]  # noqa: E731
    for b in range(B):
        cnt = pick(q_counts, b)
        nq = S if cnt is None else min(int(cnt) & COUNT_MASK, S)
        corr, slots = correspondences(q_xyz[b], t_xyz[b], cnt, pick(match_idx, b), pick(pair_valid, b), pick(q_valid, b),
                                      pick(t_valid, b))
        yield b, nq, corr, slots


def align_ransac_ref(q_xyz, t_xyz, q_valid=None, t_valid=None, q_counts=None, match_idx=None, pair_valid=None, kind=SIMILARITY,
                     hypotheses=256, seed=0, threshold=0.1, fill=0, detail=None):
    """fd_align_ransac. Returns (model float64 [B, 13], inlier uint8 [B, S], counts int32 [B], best int32 [B]); inlier
    slots the call does not write hold `fill`. detail (a list) receives per frame (scores [H], valid [H], models)."""
    q_xyz = np.asarray(q_xyz, np.float32)
    B, S = q_xyz.shape[0], q_xyz.shape[1]
    t = _f(np.float32(threshold))
    tt = t * t
    out_model, out_inl = np.zeros((B, MODEL), np.float64), np.full((B, S), fill, np.uint8)
    out_cnt, out_best = np.zeros(B, np.int32), np.full(B, -1, np.int32)
    for b, nq, corr, slots in _frames(q_xyz, t_xyz, q_counts, match_idx, pair_valid, q_valid, t_valid):
        out_inl[b, :nq] = 0
        m, valid = hypotheses_ref(corr, b, hypotheses, seed, kind)
        inl = inliers(m, corr, tt) if corr.shape[0] else np.zeros((hypotheses, 0), bool)
        score = inl.sum(axis=1)
        if detail is not None:
            detail.append((score, valid, m))
        if not valid.any():
            continue
        best = int(np.argmax(np.where(valid, score, -1)))  # first of the largest: the lowest index
        out_best[b], out_model[b] = best, m[best]
        out_inl[b, slots[inl[best]]] = 1
        out_cnt[b] = int(score[best])
    return out_model, out_inl, out_cnt, out_best


# ---- fd_align_refit -----------------------------------------------------------------------------------------
def tree_sums(vals, member):
    """The sums of the columns of vals [n, k] over the members, in the contract's order: 256 partials by list position
    modulo 256, ascending, then the tree."""
    n, k = vals.shape
    P = np.zeros((LANES, k), np.float64)
    with np.errstate(all="ignore"):
        for base in range(0, n, LANES):
            m = min(LANES, n - base)
            take = member[base:base + m]
            P[:m] = np.where(take[:, None], P[:m] + vals[base:base + m], P[:m])
        step = LANES // 2
        while step >= 1:
            P[:step] = P[:step] + P[step:2 * step]
            step //= 2
    return P[0].copy()


def horn_matrix(A):
    """Horn's symmetric 4 x 4 matrix of the cross sums A [9] (row-major, source row and target column)."""
    Sxx, Sxy, Sxz, Syx, Syy, Syz, Szx, Szy, Szz = (_f(v) for v in A)
    with np.errstate(all="ignore"):
        return np.array([[Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx],
                         [Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz],
                         [Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy],
                         [Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz]], np.float64)


def largest(d):
    """Index of the largest diagonal entry: a strict > from entry 0."""
    at = 0
    for i in range(1, len(d)):
        if d[i] > d[at]:
            at = i
    return at


def quaternion_rotation(q):
    """The nine entries of the rotation of q = (a, b, c, d), each divided by q.q."""
    a, b, c, d = (_f(v) for v in q)
    two = _f(2.0)
    with np.errstate(all="ignore"):
        qq = a * a + b * b + c * c + d * d
        return [(a * a + b * b - c * c - d * d) / qq, (two * (b * c - a * d)) / qq, (two * (b * d + a * c)) / qq,
                (two * (b * c + a * d)) / qq, (a * a - b * b + c * c - d * d) / qq, (two * (c * d - a * b)) / qq,
                (two * (b * d - a * c)) / qq, (two * (c * d + a * b)) / qq, (a * a - b * b - c * c + d * d) / qq]


def horn_fit(corr, member, kind, sweeps=SWEEPS, trace=None):
    """One round's model [13] on the members of corr [n, 6], or None for an invalid round. trace (a list) receives
    (diagonal, q) after every sweep."""
    m = int(member.sum())
    if m < 3:
        return None
    with np.errstate(all="ignore"):
        mean = tree_sums(corr, member) / _f(m)
        Xb, Yb = mean[:3], mean[3:]
        xc, yc = corr[:, :3] - Xb, corr[:, 3:] - Yb
        cols = [xc[:, i] * yc[:, j] for i in range(3) for j in range(3)]
        cols.append((xc[:, 0] * xc[:, 0] + xc[:, 1] * xc[:, 1]) + xc[:, 2] * xc[:, 2])
        S = tree_sums(np.stack(cols, axis=1), member)
        A, Sx = S[:9], S[9]
        tr = [] if trace is not None else None
        d, V = jacobi(horn_matrix(A), sweeps, trace=tr)
        if trace is not None:
            trace.extend((dd, VV[:, largest(dd)].copy()) for dd, VV in tr)
        R = quaternion_rotation(V[:, largest(d)])
        s = _f(1.0)
        if kind != RIGID:
            acc = _f(0.0)
            for i in range(3):
                for j in range(3):
                    acc = acc + R[3 * i + j] * A[3 * j + i]
            s = acc / Sx
        t = [Yb[i] - s * ((R[3 * i] * Xb[0] + R[3 * i + 1] * Xb[1]) + R[3 * i + 2] * Xb[2]) for i in range(3)]
        model = np.array(R + t + [s], np.float64)
        if not (Sx > 0.0 and np.all(np.isfinite(model)) and s > 0.0):
            return None
    return model


def refit_frame(corr, member, model, rounds, kind, tt, sweeps=SWEEPS, trace=None):
    """The rounds of one frame: (model [13] or None when no round was accepted, member bool [n], accepted rounds).
    trace (a list) receives c_0 and every accepted c_r."""
    none = np.zeros(0, bool)
    cls = lambda m: inliers(np.asarray(m, np.float64)[None], corr, tt)[0] if corr.shape[0] else none  # noqa: E731
    cur, count, done = None, int(cls(model).sum()), 0
    if trace is not None:
        trace.append(count)
    for _ in range(rounds):
        cand = horn_fit(corr, member, kind, sweeps)
        if cand is None:
            break
        inl = cls(cand)
        if int(inl.sum()) < count:
            break
        cur, member, count, done = cand, inl, int(inl.sum()), done + 1
        if trace is not None:
            trace.append(count)
    return cur, member, done


def align_refit_ref(q_xyz, t_xyz, in_model, in_inlier, q_valid=None, t_valid=None, q_counts=None, match_idx=None, pair_valid=None,
                    kind=SIMILARITY, rounds=4, threshold=0.1, fill=0, sweeps=SWEEPS, trace=None):
    """fd_align_refit. Returns (model float64 [B, 13], inlier uint8 [B, S], counts int32 [B], rounds int32 [B]); inlier
    slots the call does not write hold `fill`. trace (a list) receives every frame's [c_0, c_1, ...]."""
    q_xyz = np.asarray(q_xyz, np.float32)
    B, S = q_xyz.shape[0], q_xyz.shape[1]
    t = _f(np.float32(threshold))
    tt = t * t
    out_model = np.array(in_model, np.float64).reshape(B, MODEL).copy()
    out_inl = np.full((B, S), fill, np.uint8)
    out_cnt, out_rounds = np.zeros(B, np.int32), np.zeros(B, np.int32)
    in_inlier = np.asarray(in_inlier, np.uint8).reshape(B, S)
    for b, nq, corr, slots in _frames(q_xyz, t_xyz, q_counts, match_idx, pair_valid, q_valid, t_valid):
        out_inl[b, :nq] = 0
        member = in_inlier[b, slots] == 1
        tr = [] if trace is not None else None
        model, member, done = refit_frame(corr, member, out_model[b].copy(), rounds, kind, tt, sweeps, trace=tr)
        if trace is not None:
            trace.append(tr)
        out_inl[b, slots[member]] = 1
        out_cnt[b], out_rounds[b] = int(member.sum()), done
        if done:
            out_model[b] = model
    return out_model, out_inl, out_cnt, out_rounds


# ---- fd_align_apply -----------------------------------------------------------------------------------------
def align_apply_ref(model, xyz, valid=None, counts=None, out=None):
    """fd_align_apply into a copy of `out` (None: of xyz, the in-place call): float32 [B, S, 3]."""
    xyz = np.asarray(xyz, np.float32)
    B, S = xyz.shape[0], xyz.shape[1]
    model = np.asarray(model, np.float64).reshape(B, MODEL)
    res = np.array(xyz if out is None else out, np.float32).reshape(B, S, 3).copy()
    for b in range(B):
        n = S if counts is None else min(int(counts[b]) & COUNT_MASK, S)
        take = np.zeros(S, bool)
        take[:n] = True
        if valid is not None:
            take &= np.asarray(valid[b]) == 1
        with np.errstate(all="ignore"):
            z = apply_model(model[b][None, :], xyz[b].astype(np.float64))
            res[b][take] = z[take].astype(np.float32)
    return res


# ---- planted scenes ---------------------------------------------------------------------------------------
def planted(seed):
    """A seeded similarity (R, t, s): a rotation of up to 60 degrees about each axis, a scale in 0.5..2."""
    rng = np.random.default_rng(51000 + seed)
    R = rotation(*rng.uniform(-1.0, 1.0, 3))
    return R, rng.uniform(-3.0, 3.0, 3), float(rng.uniform(0.5, 2.0))


def scene(seed, n=64, outliers=0.25, noise=0.01, planar=False, rigid=False, radius=2.0, offset=(1.0, -2.0, 5.0), mirror=False):
    """n seeded source points (float32) within `radius` of `offset` (planar: on the plane z = offset z) and their
    targets Y = s R X + t with Gaussian noise of `noise` per coordinate; a fraction `outliers` of the targets (random
    slots) replaced by uniform random points of the target's box; mirror: every target reflected in x (no proper
    rotation fits). Returns a dict: q, t float32 [n, 3], planted bool [n], R, t_vec, s, radius (the RMS distance of the
    planted sources from their centroid), centroid."""
    rng = np.random.default_rng(52000 + seed)
    R, tv, s = planted(seed)
    if rigid:
        s = 1.0
    X = rng.uniform(-radius, radius, (n, 3))
    if planar:
        X[:, 2] = 0.0
    X = (X + np.asarray(offset)).astype(np.float32).astype(np.float64)
    Y = s * X @ R.T + tv
    if mirror:
        Y[:, 0] = -Y[:, 0]
    Y = Y + rng.normal(0.0, noise, (n, 3))
    k = int(round(outliers * n))
    good = np.ones(n, bool)
    bad = rng.choice(n, k, replace=False)
    good[bad] = False
    lo, hi = Y.min(0), Y.max(0)
    Y[bad] = rng.uniform(lo, hi, (k, 3))
    c = X[good].mean(0)
    rho = float(np.sqrt(np.mean(np.sum((X[good] - c) ** 2, axis=1))))
    return dict(q=X.astype(np.float32), t=Y.astype(np.float32), planted=good, R=R, t_vec=tv, s=s, radius=rho, centroid=c,
                noise=noise)


def model_errors(model, sc):
    """(rotation angle in radians, |s / s_planted - 1|, |t - t_planted|) of a model [13] against the scene's."""
    model = np.asarray(model, np.float64)
    return (rotation_angle(model[:9], sc["R"]), abs(float(model[12]) / sc["s"] - 1.0),
            float(np.linalg.norm(model[9:12] - sc["t_vec"])))


# ---- an independent solution: SVD Umeyama on the same samples and members ------------------------------------
def umeyama(X, Y, with_scale=True):
    """(R, t, s) minimising sum |Y - (s R X + t)|^2 by the SVD of the cross covariance, with the determinant fix."""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    mx, my = X.mean(0), Y.mean(0)
    xc, yc = X - mx, Y - my
    U, D, Vt = np.linalg.svd(yc.T @ xc)
    sg = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        sg[2] = -1.0
    R = U @ np.diag(sg) @ Vt
    s = float((D * sg).sum() / (xc ** 2).sum()) if with_scale else 1.0
    return R, my - s * R @ mx, s


def independent_ransac(sc, hypotheses, seed, threshold, kind=SIMILARITY, b=0):
    """The same samples (fd_ransac's sampler), each solved by umeyama on its three points and scored by the distance
    in the target's units: (R, t, s, inlier bool [n])."""
    X, Y = sc["q"].astype(np.float64), sc["t"].astype(np.float64)
    n = len(X)
    best = (-1, None, None, None, None)
    for h in range(hypotheses):
        pk = sample(seed, b, h, n, M)
        if pk is None:
            continue
        if np.linalg.matrix_rank(X[pk] - X[pk].mean(0), tol=1e-9) < 2 or np.linalg.matrix_rank(Y[pk] - Y[pk].mean(0), tol=1e-9) < 2:
            continue
        R, t, s = umeyama(X[pk], Y[pk], kind == SIMILARITY)
        inl = np.linalg.norm(Y - (s * X @ R.T + t), axis=1) <= threshold
        if inl.sum() > best[0]:
            best = (int(inl.sum()), R, t, s, inl)
    return best[1:]


def independent_refine(sc, inl, rounds, threshold, kind=SIMILARITY):
    """umeyama on the inliers, which are classified again after every round."""
    X, Y = sc["q"].astype(np.float64), sc["t"].astype(np.float64)
    R = t = s = None
    for _ in range(rounds):
        R, t, s = umeyama(X[inl], Y[inl], kind == SIMILARITY)
        inl = np.linalg.norm(Y - (s * X @ R.T + t), axis=1) <= threshold
    return R, t, s, inl


# ---- the cases of the GPU tests -----------------------------------------------------------------------------
NOISE = 0.01
THRESHOLD = 4 * NOISE
HYP = 64


def case(sc, **kw):
    """A case dict of one scene (batch 1)."""
    d = dict(q=sc["q"][None].copy(), t=sc["t"][None].copy(), q_valid=None, t_valid=None, counts=None, idx=None, valid=None,
             kind=SIMILARITY, hypotheses=HYP, seed=3, threshold=THRESHOLD)
    d.update(kw)
    return d


def stack(cases, **kw):
    d = dict(cases[0])
    for k in ("q", "t"):
        d[k] = np.concatenate([c[k] for c in cases], 0)
    d.update(kw)
    return d


def run_ransac(c, fill=0, detail=None):
    return align_ransac_ref(c["q"], c["t"], c["q_valid"], c["t_valid"], c["counts"], c["idx"], c["valid"], kind=c["kind"],
                            hypotheses=c["hypotheses"], seed=c["seed"], threshold=c["threshold"], fill=fill, detail=detail)


def run_refit(c, in_model, in_inlier, rounds, fill=0, trace=None, sweeps=SWEEPS):
    return align_refit_ref(c["q"], c["t"], in_model, in_inlier, c["q_valid"], c["t_valid"], c["counts"], c["idx"], c["valid"],
                           kind=c["kind"], rounds=rounds, threshold=c["threshold"], fill=fill, trace=trace, sweeps=sweeps)


def n_case(n):
    """One frame of n correspondences (small n without outliers: the few samples must still give a model)."""
    return case(scene(500 + n, n=max(n, 1), outliers=0.0 if n < 40 else 0.25), counts=np.array([n], np.int32))


def batch_case():
    """Batch 3, stride 90, a different n per frame, one of them empty; counts with the bits 25..31 set."""
    frames = [case(scene(600 + k, n=90)) for k in range(3)]
    hi = sum(1 << k for k in range(25, 32))
    return stack(frames, counts=np.array([90 | hi, 0 | hi, 37 | hi], np.uint32).view(np.int32))


def holes_case():
    """Batch 3: match_idx with -1, out-of-range and repeated entries, t_stride != q_stride, q_valid, t_valid and
    pair_valid bytes 0..6, and a NaN / inf in each of the six coordinate places."""
    rng = np.random.default_rng(13)
    S, T = 90, 75
    d = stack([case(scene(700 + k, n=S)) for k in range(3)])
    idx = np.tile(np.arange(S, dtype=np.int32), (3, 1))
    idx[:, T:] = np.arange(S - T, dtype=np.int32) * 3
    d["t"] = np.ascontiguousarray(d["t"][:, :T])
    idx[:, 5], idx[:, 6], idx[:, 7], idx[:, 8] = -1, T, -2 ** 31, 2 ** 31 - 1
    idx[1, 20:30] = 3
    valid, qv, tv = np.ones((3, S), np.uint8), np.ones((3, S), np.uint8), np.ones((3, T), np.uint8)
    valid[0, 10:24] = np.arange(14) % 7
    valid[2] = np.where(rng.random(S) < 0.2, rng.integers(0, 7, S), 1)
    qv[1] = np.where(rng.random(S) < 0.2, rng.integers(0, 7, S), 1)
    qv[0, 40:47] = np.arange(7)
    tv[0, 50:57] = np.arange(7)
    tv[2] = np.where(rng.random(T) < 0.15, rng.integers(0, 3, T) * 2, 1)  # 0, 2 or 4 at the partner
    q, t = d["q"], d["t"]
    q[0, 30, 0], q[0, 31, 1], q[0, 32, 2], t[0, 33, 0], t[0, 34, 1], t[0, 35, 2] = np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf
    d.update(idx=idx, valid=valid, q_valid=qv, t_valid=tv, counts=np.array([S, 70, 77], np.int32))
    return d


def collinear_case():
    """Every source point on one line, every target on its image: each sample's second side lies along its first."""
    sc = scene(800, n=48, outliers=0.0, noise=0.0)
    k = np.arange(48, dtype=np.float64)[:, None]
    X = np.array([1.0, -2.0, 5.0]) + k * np.array([0.25, 0.5, -0.125])  # exact in float32: the differences are parallel
    sc["q"], sc["t"] = X.astype(np.float32), (2.0 * X + np.array([1.0, 2.0, 3.0])).astype(np.float32)
    return case(sc)


def duplicate_case():
    """Every slot the same pair of points: u = 0 in every sample."""
    sc = scene(801, n=12, outliers=0.0)
    sc["q"][:], sc["t"][:] = sc["q"][0], sc["t"][0]
    return case(sc)


def planar_case():
    """Source and target exactly planar in float32 (z constant in both: a rotation about z, scale 2): the 3-point
    frames and Horn's quaternion both take a plane."""
    rng = np.random.default_rng(802)
    X = np.concatenate([np.round(rng.uniform(-4, 4, (80, 2)) * 64) / 64, np.full((80, 1), 5.0)], axis=1)
    Rz = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    Y = 2.0 * X @ Rz.T + np.array([0.5, -1.25, 3.0])
    noise = np.round(rng.normal(0.0, NOISE, (80, 2)) * 1024) / 1024
    Y[:, :2] += noise
    Y[::5] = rng.uniform(-8, 8, (16, 3))
    return case(dict(q=X.astype(np.float32), t=Y.astype(np.float32)))


def rigid_scaled_case():
    """The rigid kind on a target scaled by 1.5: s stays exactly 1.0 and few correspondences fit."""
    sc = scene(803, n=64, outliers=0.2)
    sc["t"] = (1.5 * sc["t"].astype(np.float64)).astype(np.float32)
    return case(sc, kind=RIGID)


# of the seeds 1000..1199 of scene(seed, n=64, outliers=0.3, noise=0.02) at threshold 0.05 and 32 hypotheses one whose
# refit stops at round 3 of 8 (tests/test_align_host.py::test_refit_guard_stops_early confirms it)
STOPPED_SEED = 1026


def stopped_case():
    return case(scene(STOPPED_SEED, n=64, outliers=0.3, noise=0.02), threshold=0.05, hypotheses=32)


def all_cases():
    """(name, case) of every scene the GPU tests compare with the restatement."""
    out = [(f"n-{n}", n_case(n)) for n in (0, 2, 3, 4, 255, 256, 257, 513)]
    out += [(f"hyp-{h}", case(scene(900, n=48), hypotheses=h, seed=11)) for h in (1, 64, 65, 4096)]
    out += [("batch", batch_case()), ("holes", holes_case()), ("collinear", collinear_case()), ("duplicate", duplicate_case()),
            ("planar", planar_case()), ("rigid-scaled", rigid_scaled_case()),
            ("rigid", case(scene(901, n=80, rigid=True), kind=RIGID)), ("similarity", case(scene(901, n=80)))]
    return out
