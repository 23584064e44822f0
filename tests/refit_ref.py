"""numpy restatement of fd_ransac_refit (include/fd_hip.h): the least-squares refit of fd_ransac's model on
its inliers, the contract's arithmetic sequence in elementwise float64 numpy (IEEE, one rounding per
operation). The GPU tests compare every output with it bit for bit. The correspondence list, the rows, the
inlier test and the denormalisation are fd_ransac's and come from tests/ransac_ref.py.

Also the noisy variant of the planted scenes (noisy_scene) of the accuracy tests.
"""
import numpy as np

from ransac_ref import (COLS, COUNT_MASK, FUNDAMENTAL, HOMOGRAPHY, ROWS, SAMPLE, build_rows, conditioning,  # noqa: F401
                        correspondences, denormalise, inliers, pixel_residual, planted_scene, ransac_ref)

LANES = 256   # partial sums of the normal matrix: list position i goes to partial i % 256
SWEEPS = 8    # FD_REFIT_SWEEPS: tests/test_refit_host.py::test_sweep_count_rule derives it
RANK_EPS = 1e-12
PAIRS = [(a, b) for a in range(9) for b in range(a, 9)]  # the 45 summed entries, in this order


def normal_matrix(model, corr, member):
    """N = sum of row^T row over the members of corr [n, 4] (member bool [n]), in the contract's order:
    256 partials by list position modulo 256, ascending, then the tree."""
    n = corr.shape[0]
    P = np.zeros((LANES, 45), np.float64)
    with np.errstate(all="ignore"):
        for base in range(0, n, LANES):
            pts = np.zeros((LANES, 4), np.float64)
            take = np.zeros(LANES, bool)
            m = min(LANES, n - base)
            pts[:m], take[:m] = corr[base:base + m], member[base:base + m]
            # build_rows takes picks in fours: [64, 4, 4] -> per position one row (F) or two in pick order (H)
            rows = build_rows(model, pts.reshape(LANES // 4, 4, 4)).reshape(LANES, -1, 9)
            for r in range(1 if model == FUNDAMENTAL else 2):
                row = rows[:, r, :]
                for e, (a, b) in enumerate(PAIRS):
                    P[:, e] = np.where(take, P[:, e] + row[:, a] * row[:, b], P[:, e])
        step = LANES // 2
        while step >= 1:
            P[:step] = P[:step] + P[step:2 * step]
            step //= 2
    N = np.zeros((9, 9), np.float64)
    for e, (a, b) in enumerate(PAIRS):
        N[a, b] = N[b, a] = P[0, e]
    return N


def jacobi(A, sweeps=SWEEPS, trace=None):
    """Cyclic Jacobi on the symmetric A [n, n] with V accumulated from the identity: (diagonal [n], V [n, n]).
    trace (a list) receives (diagonal, V) copies after every sweep."""
    A = np.array(A, np.float64)
    n = A.shape[0]
    V = np.eye(n, dtype=np.float64)
    one, two = np.float64(1.0), np.float64(2.0)
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for p in range(n):
                for q in range(p + 1, n):
                    apq = A[p, q]
                    if apq == 0.0:
                        continue
                    app, aqq = A[p, p], A[q, q]
                    theta = (aqq - app) / (two * apq)
                    t = (-one if theta < 0 else one) / (np.abs(theta) + np.sqrt(theta * theta + one))
                    c = one / np.sqrt(t * t + one)
                    s = t * c
                    xp, xq = A[:, p].copy(), A[:, q].copy()
                    np_, nq = c * xp - s * xq, s * xp + c * xq
                    np_[p], nq[p] = app - t * apq, 0.0
                    np_[q], nq[q] = 0.0, aqq + t * apq
                    A[:, p], A[:, q] = np_, nq
                    A[p, :], A[q, :] = np_, nq
                    vp, vq = V[:, p].copy(), V[:, q].copy()
                    V[:, p], V[:, q] = c * vp - s * vq, s * vp + c * vq
            if trace is not None:
                trace.append((np.diag(A).copy(), V.copy()))
    return np.diag(A).copy(), V


def smallest(d):
    """Index of the smallest diagonal entry: a strict < from entry 0, so the lowest index among equals."""
    at = 0
    for i in range(1, len(d)):
        if d[i] < d[at]:
            at = i
    return at


def eigenvector(N, sweeps=SWEEPS):
    """(x [9], valid): the column of V at N's smallest diagonal entry after the sweeps; invalid for a
    non-finite entry, or unless the second smallest diagonal entry exceeds 1e-12 times the largest."""
    d, V = jacobi(N, sweeps)
    at = smallest(d)
    x = V[:, at].copy()
    d2, dmax = np.float64(np.inf), d[0]
    for i in range(9):
        if i != at and d[i] < d2:
            d2 = d[i]
        if d[i] > dmax:
            dmax = d[i]
    with np.errstate(all="ignore"):
        valid = bool(np.all(np.isfinite(x))) and bool(d2 > np.float64(RANK_EPS) * dmax)
    return x, valid


def rank2(x, sweeps=SWEEPS):
    """F <- F - (F v) v^T with v the eigenvector of F^T F at its smallest diagonal entry: (x [9], valid)."""
    F = np.array(x, np.float64).reshape(3, 3)
    with np.errstate(all="ignore"):
        G = np.zeros((3, 3), np.float64)
        for i in range(3):
            for j in range(3):
                acc = np.float64(0.0)
                for k in range(3):
                    acc = acc + F[k, i] * F[k, j]
                G[i, j] = acc
        d, V = jacobi(G, sweeps)
        v = V[:, smallest(d)]
        out = np.zeros((3, 3), np.float64)
        for i in range(3):
            w = np.float64(0.0)
            for j in range(3):
                w = w + F[i, j] * v[j]
            for j in range(3):
                out[i, j] = F[i, j] - w * v[j]
    out = out.reshape(9)
    return out, bool(np.all(np.isfinite(out)))


def fit(model, corr, member, sweeps=SWEEPS):
    """One least-squares fit of the conditioned model on the members: (x [9], valid)."""
    if int(member.sum()) < SAMPLE[model]:
        return np.zeros(9), False
    x, valid = eigenvector(normal_matrix(model, corr, member), sweeps)
    if model == FUNDAMENTAL:
        x, ok = rank2(x, sweeps)
        valid = valid and ok
    return x, valid


def refit_frame(model, corr, member, rounds, tt, sweeps=SWEEPS):
    """The rounds of one frame: (conditioned model or None, member bool [n], count, accepted rounds)."""
    x, count, done = None, int(member.sum()), 0
    for _ in range(rounds):
        cand, valid = fit(model, corr, member, sweeps)
        if not valid:
            break
        inl = inliers(model, cand[None], corr, tt)[0] if corr.shape[0] else np.zeros(0, bool)
        if int(inl.sum()) < count:
            break
        x, member, count, done = cand, inl, int(inl.sum()), done + 1
    return x, member, count, done


def refit_ref(q_xy, t_xy, in_model, in_inlier, q_counts=None, match_idx=None, pair_valid=None, model=FUNDAMENTAL, rounds=2,
              threshold=1.0, center=(0.0, 0.0), scale=1.0 / 256, fill=0, sweeps=SWEEPS):
    """fd_ransac_refit for [B, S, 2] / [B, T, 2] float32 positions. Returns (model float64 [B, 9], inlier
    uint8 [B, S], counts int32 [B], rounds int32 [B]); inlier slots the call does not write hold `fill`."""
    q_xy, t_xy = np.asarray(q_xy, np.float32), np.asarray(t_xy, np.float32)
    B, S = q_xy.shape[0], q_xy.shape[1]
    cx, cy = center
    t = np.float64(np.float32(threshold)) * np.float64(np.float32(scale))
    tt = t * t
    out_model = np.array(in_model, np.float64).reshape(B, 9).copy()
    out_inl = np.full((B, S), fill, np.uint8)
    out_cnt, out_rounds = np.zeros(B, np.int32), np.zeros(B, np.int32)
    in_inlier = np.asarray(in_inlier, np.uint8).reshape(B, S)
    for b in range(B):
        cnt = None if q_counts is None else q_counts[b]
        nq = S if cnt is None else min(int(cnt) & COUNT_MASK, S)
        out_inl[b, :nq] = 0
        corr, slots = correspondences(q_xy[b], t_xy[b], cnt, None if match_idx is None else match_idx[b],
                                      None if pair_valid is None else pair_valid[b], cx, cy, scale)
        member = in_inlier[b, slots] == 1
        x, member, count, done = refit_frame(model, corr, member, rounds, tt, sweeps)
        out_inl[b, slots[member]] = 1
        out_cnt[b], out_rounds[b] = count, done
        if done:
            out_model[b] = denormalise(model, x, cx, cy, scale)
    return out_model, out_inl, out_cnt, out_rounds


# ---- noisy planted scenes ---------------------------------------------------------------------------------
def noisy_scene(model, seed, n=64, outliers=16, noise=0.5):
    """planted_scene with every planted inlier's query and train position moved by a seeded offset uniform in
    [-noise, noise] px per coordinate: (q, t float32 noisy, planted flags, q0, t0 float32 noise-free)."""
    q0, t0, planted = planted_scene(model, seed, n=n, outliers=outliers)
    rng = np.random.default_rng(77000 + 1000 * model + seed)
    dq, dt = rng.uniform(-noise, noise, q0.shape), rng.uniform(-noise, noise, t0.shape)
    q = np.where(planted[:, None], q0.astype(np.float64) + dq, q0).astype(np.float32)
    t = np.where(planted[:, None], t0.astype(np.float64) + dt, t0).astype(np.float32)
    return q, t, planted, q0, t0


CENTER, SCALE = conditioning((ROWS, COLS))
HYP = 64  # hypotheses of the fd_ransac restatement that supplies the cases' in_model and in_inlier
ANY_MODEL = np.array([0.25, -3.0, 7.5, 1.0, 0.125, -2.0, 1e-3, -1e-3, 1.0])


def scenes(model, stride, batch, seed=0, outliers=None, noise=0.5):
    """[batch, stride, 2] noisy query and train positions (a quarter of each frame outliers)."""
    q, t = zip(*(noisy_scene(model, 50 * seed + b, n=stride, outliers=stride // 4 if outliers is None else outliers,
                             noise=noise)[:2] for b in range(batch)))
    return np.stack(q), np.stack(t)


def from_ransac(model, q, t, counts=None, idx=None, valid=None, seed=0):
    """A case dict whose in_model / in_inlier are the fd_ransac restatement's outputs."""
    m, inl, _, _ = ransac_ref(q, t, counts, idx, valid, model=model, hypotheses=HYP, seed=seed, center=CENTER, scale=SCALE)
    return dict(model=model, q=q, t=t, counts=counts, idx=idx, valid=valid, in_model=m, in_inlier=inl)


SUPPORT_NOISE = 0.05  # px: small enough that every support set below keeps its members


def support_case(model, k):
    """One frame without outliers whose support is its first k slots (3 more slots are correspondences
    outside the support); in_model is an arbitrary matrix."""
    q, t = scenes(model, k + 3, 1, seed=k, outliers=0, noise=SUPPORT_NOISE)
    inl = np.zeros((1, k + 3), np.uint8)
    inl[0, :k] = 1
    return dict(model=model, q=q, t=t, counts=None, idx=None, valid=None, in_model=ANY_MODEL[None].copy(), in_inlier=inl)


def batch_case(model):
    """Batch 3, stride 90, a different count per frame (one with flag bits), supports from fd_ransac."""
    q, t = scenes(model, 90, 3, seed=2)
    counts = np.array([90, 60 | (1 << 25) | (1 << 31), 77], np.uint32).view(np.int32)
    return from_ransac(model, q, t, counts=counts, seed=5)


def degenerate_case(model):
    """A support set that leaves more than one direction free: collinear query points (H), a pure
    translation (F). The first fit is invalid, so the frame passes through."""
    rng = np.random.default_rng(5 + model)
    n = 40
    if model == HOMOGRAPHY:
        q, t, _, _, _ = noisy_scene(model, 9, n=n, outliers=0, noise=0.0)
        x = rng.uniform(20, 250, 24)
        line = np.stack([x, 0.75 * x + 40.0, np.ones(24)], 0)
        Hm = np.array([[1.02, 0.01, 5.0], [-0.02, 0.98, -3.0], [1e-5, 2e-5, 1.0]])
        p = Hm @ line
        q[:24], t[:24] = line[:2].T.astype(np.float32), (p[:2] / p[2]).T.astype(np.float32)
        inl = np.zeros((1, n), np.uint8)
        inl[0, :24] = 1
    else:
        q = np.stack([rng.uniform(0, COLS - 10, n), rng.uniform(0, ROWS - 10, n)], -1).astype(np.float32)
        t = q + np.array([5.0, 3.0], np.float32)
        inl = np.ones((1, n), np.uint8)
    return dict(model=model, q=q[None], t=t[None], counts=None, idx=None, valid=None, in_model=ANY_MODEL[None].copy(), in_inlier=inl)


STOPPED_H = 51  # of the seeds 0..79 of scenes(HOMOGRAPHY, 64, 1, seed) the one whose round 2 loses an inlier


def stopped_case(model):
    """Round 1 accepted, round 2 rejected by the guard. H: a scene found by search on the restatement. F: none
    of 80 such scenes stops, but the support of exactly 8 does (the fit through 8 points, then rank 2)."""
    if model == FUNDAMENTAL:
        return support_case(FUNDAMENTAL, 8)
    q, t = scenes(model, 64, 1, seed=STOPPED_H)
    return from_ransac(model, q, t, seed=STOPPED_H)


def holes_case(model):
    """Batch 3: match_idx with -1, out-of-range and repeated train indices, pair_valid bytes 0..6, non-finite
    coordinates, and in_inlier bytes 0, 2 and 0xFF where fd_ransac had written 1."""
    rng = np.random.default_rng(11)
    S, T = 90, 75
    q, t = scenes(model, S, 3, seed=3)
    t = np.ascontiguousarray(t[:, :T])
    idx = np.tile(np.arange(S, dtype=np.int32) % T, (3, 1))
    idx[:, 5], idx[:, 6], idx[:, 7], idx[:, 8] = -1, T, -2 ** 31, 2 ** 31 - 1
    idx[1, 20:30] = 3
    valid = np.ones((3, S), np.uint8)
    valid[0, 10:24] = np.arange(14) % 7
    valid[2] = np.where(rng.random(S) < 0.2, rng.integers(0, 7, S), 1)
    q[0, 30, 0], q[0, 31, 1], t[0, 32, 0], t[0, 33, 1] = np.nan, np.inf, -np.inf, np.nan
    case = from_ransac(model, q, t, counts=np.array([S, 70, 77], np.int32), idx=idx, valid=valid, seed=5)
    inl = case["in_inlier"]
    for b in range(3):
        ones = np.flatnonzero(inl[b] == 1)
        inl[b, ones[1::9]], inl[b, ones[2::9]], inl[b, ones[4::9]] = 2, 0xFF, 0
        inl[b, 5], inl[b, 30 + b] = 1, 1  # bytes of 1 at slots that are no correspondences (frame 0) or may be none
    return case


def all_cases():
    """(name, rounds, case) of every scene the GPU tests compare with the restatement."""
    out = []
    for model, ks in ((HOMOGRAPHY, (3, 4, 5)), (FUNDAMENTAL, (7, 8, 9))):
        out += [(f"support-{model}-{k}", 2, support_case(model, k)) for k in ks + (255, 256, 257, 513)]
    for model in (FUNDAMENTAL, HOMOGRAPHY):
        out += [(f"batch-{model}", 4, batch_case(model)), (f"degenerate-{model}", 2, degenerate_case(model)),
                (f"stopped-{model}", 2, stopped_case(model)), (f"holes-{model}", 2, holes_case(model))]
    return out


def run_case(case, rounds, fill=0, sweeps=SWEEPS):
    return refit_ref(case["q"], case["t"], case["in_model"], case["in_inlier"], case["counts"], case["idx"], case["valid"],
                     model=case["model"], rounds=rounds, center=CENTER, scale=SCALE, fill=fill, sweeps=sweeps)


def rms(model, m9, q, t, planted):
    """RMS pixel residual of a pixel-coordinate model on the planted pairs of (q, t)."""
    r = pixel_residual(model, m9, q[planted], t[planted])
    return float(np.sqrt(np.mean(r * r)))
