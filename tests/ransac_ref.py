"""numpy restatement of fd_ransac (include/fd_hip.h): the contract's arithmetic sequence in elementwise
float64 numpy (IEEE, one rounding per operation) and Python integers for the sampler, vectorised over the
hypotheses. The GPU tests compare every output with it bit for bit.

Also the planted scenes of the property tests (planted_scene) and their pixel-space residuals, which do
not use the restatement.
"""
import numpy as np

FUNDAMENTAL, HOMOGRAPHY = 0, 1
SAMPLE = {FUNDAMENTAL: 8, HOMOGRAPHY: 4}
M32 = 0xFFFFFFFF
COUNT_MASK = 0x01FFFFFF


def mix(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def sample_trace(seed, b, h, n, m):
    """The sampler step by step: (picks, tries). picks are the distinct indices found, in order; tries[k] is
    the number of draws pick k took (1..32). The sampler stops at the first pick that finds no new index in 32
    draws, so an exhausted hypothesis has len(picks) < m. n < m gives ([], [])."""
    picks, tries = [], []
    if n < m:
        return picks, tries
    base = mix(mix(seed + 0x9E3779B9 * b) + h)
    for k in range(m):
        for a in range(32):
            idx = (mix(base + 32 * k + a) * n) >> 32
            if idx not in picks:
                picks.append(idx)
                tries.append(a + 1)
                break
        else:
            break
    return picks, tries


def sample(seed, b, h, n, m):
    """The m distinct picks of hypothesis h of frame b among n correspondences, or None."""
    picks = sample_trace(seed, b, h, n, m)[0]
    return picks if len(picks) == m and n >= m else None


def exhausted(seed, b, n, m, hypotheses):
    """The hypotheses of frame b whose sampler gives up (n >= m, a pick found no new index in 32 draws)."""
    return [h for h in range(hypotheses) if n >= m and sample(seed, b, h, n, m) is None]


# Pinned sampler cases of the tests, all with n equal to the sample size (tests/test_ransac_host.py confirms
# each on the CPU). EXHAUSTING: (model, seed, hypotheses) whose frame 0 has exhausted hypotheses: for F the
# hypotheses 70, 99, 220 and 250; for H, of the seeds below 64, the one whose first exhausted hypothesis (34)
# comes earliest. EDGE_SEEDS: (model, seed, what hypothesis 0 does). With no outlier every valid hypothesis
# counts all n, so the lowest valid index wins and hypothesis 0 decides `best`:
#   "last draw": a pick of hypothesis 0 succeeds on its 32nd draw and 0 wins; a sampler that stops a draw early loses it;
#   "dead": hypothesis 0 gives up while index 0, what an unfilled pick holds, is still free; a sampler that forgets
#   the failure gives the solver distinct rows, a valid model, and 0 wins where it must not.
EXHAUSTING = [(FUNDAMENTAL, 0, 256), (HOMOGRAPHY, 45, 1024)]
EDGE_SEEDS = [(FUNDAMENTAL, 544, "last draw"), (FUNDAMENTAL, 99, "dead"), (HOMOGRAPHY, 853, "last draw"),
              (HOMOGRAPHY, 71484, "dead")]


def correspondences(q_xy, t_xy, count, match_idx, pair_valid, cx, cy, scale):
    """(conditioned [n, 4] float64 (x, y, u, v), slot index [n]) of one frame."""
    q_xy, t_xy = np.asarray(q_xy, np.float32), np.asarray(t_xy, np.float32)
    s, ts = q_xy.shape[0], t_xy.shape[0]
    nq = s if count is None else min(int(count) & COUNT_MASK, s)
    cx, cy, sc = np.float64(np.float32(cx)), np.float64(np.float32(cy)), np.float64(np.float32(scale))
    rows, slots = [], []
    for i in range(nq):
        if pair_valid is not None and int(pair_valid[i]) != 1:
            continue
        j = i if match_idx is None else int(match_idx[i])
        if not 0 <= j < ts:
            continue
        c = np.array([q_xy[i, 0], q_xy[i, 1], t_xy[j, 0], t_xy[j, 1]], np.float64)
        if not np.all(np.isfinite(c)):
            continue
        rows.append([(c[0] - cx) * sc, (c[1] - cy) * sc, (c[2] - cx) * sc, (c[3] - cy) * sc])
        slots.append(i)
    return np.array(rows, np.float64).reshape(-1, 4), np.array(slots, np.int64)


def build_rows(model, pts):
    """pts [H, m, 4] -> the 8 x 9 systems [H, 8, 9]."""
    x, y, u, v = (pts[..., i] for i in range(4))
    one, zero = np.ones_like(x), np.zeros_like(x)
    if model == FUNDAMENTAL:
        return np.stack([u * x, u * y, u, v * x, v * y, v, x, y, one], axis=-1)
    r0 = np.stack([x, y, one, zero, zero, zero, -(u * x), -(u * y), -u], axis=-1)
    r1 = np.stack([zero, zero, zero, x, y, one, -(v * x), -(v * y), -v], axis=-1)
    return np.stack([r0, r1], axis=2).reshape(pts.shape[0], 8, 9)


def null_vector(A):
    """Null vectors of the systems A [H, 8, 9] by Gaussian elimination with complete pivoting.
    Returns (x [H, 9], valid [H])."""
    A = np.array(A, np.float64)
    nh = A.shape[0]
    hh = np.arange(nh)
    perm = np.tile(np.arange(9), (nh, 1))
    valid = np.ones(nh, bool)
    p0 = None
    with np.errstate(all="ignore"):
        for k in range(8):
            mag = np.abs(A[:, k:, k:])
            mag = np.where(np.isnan(mag), -2.0, mag).reshape(nh, -1)  # a NaN never wins
            arg = np.argmax(mag, axis=1)                               # first of the largest: strict >
            best = mag[hh, arg]
            none = best < 0.0                                          # nothing beat -1: the pivot stays (k, k)
            best = np.where(none, -1.0, best)
            arg = np.where(none, 0, arg)
            pr, pc = k + arg // (9 - k), k + arg % (9 - k)
            if k == 0:
                p0 = best
            valid &= best > 1e-12 * p0
            rk, rp = A[hh, k, :].copy(), A[hh, pr, :].copy()
            A[hh, k, :], A[hh, pr, :] = rp, rk
            ck, cp = A[hh, :, k].copy(), A[hh, :, pc].copy()
            A[hh, :, k], A[hh, :, pc] = cp, ck
            a, b = perm[hh, k].copy(), perm[hh, pc].copy()
            perm[hh, k], perm[hh, pc] = b, a
            for r in range(k + 1, 8):
                f = A[:, r, k] / A[:, k, k]
                for c in range(k + 1, 9):
                    A[:, r, c] = A[:, r, c] - f * A[:, k, c]
        x = np.zeros((nh, 9))
        x[:, 8] = 1.0
        for k in range(7, -1, -1):
            s = np.zeros(nh)
            for c in range(k + 1, 9):
                s = s + A[:, k, c] * x[:, c]
            x[:, k] = (0.0 - s) / A[:, k, k]
    out = np.zeros((nh, 9))
    for c in range(9):
        out[hh, perm[:, c]] = x[:, c]
    valid &= np.all(np.isfinite(out), axis=1)
    return out, valid


def inliers(model, hyp, corr, tt):
    """hyp [H, 9], corr [n, 4] -> bool [H, n] by the contract's test (a NaN fails the compare)."""
    h = [hyp[:, i][:, None] for i in range(9)]
    x, y, u, v = (corr[:, i][None, :] for i in range(4))
    with np.errstate(all="ignore"):
        if model == FUNDAMENTAL:
            l0 = h[0] * x + h[1] * y + h[2]
            l1 = h[3] * x + h[4] * y + h[5]
            l2 = h[6] * x + h[7] * y + h[8]
            m0 = h[0] * u + h[3] * v + h[6]
            m1 = h[1] * u + h[4] * v + h[7]
            e = u * l0 + v * l1 + l2
            return e * e <= tt * (l0 * l0 + l1 * l1 + m0 * m0 + m1 * m1)
        w = h[6] * x + h[7] * y + h[8]
        dx = (h[0] * x + h[1] * y + h[2]) - u * w
        dy = (h[3] * x + h[4] * y + h[5]) - v * w
        return dx * dx + dy * dy <= tt * (w * w)


def _matmul(a, b):
    out = [[np.float64(0.0)] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            acc = np.float64(0.0)
            for k in range(3):
                acc = acc + a[i][k] * b[k][j]
            out[i][j] = acc
    return out


def denormalise(model, hyp, cx, cy, scale):
    """The pixel-coordinate model [9] of a conditioned one, scaled so its largest entry is 1.0."""
    cx, cy, s = np.float64(np.float32(cx)), np.float64(np.float32(cy)), np.float64(np.float32(scale))
    z, one = np.float64(0.0), np.float64(1.0)
    with np.errstate(all="ignore"):
        T = [[s, z, -(s * cx)], [z, s, -(s * cy)], [z, z, one]]
        m = [[np.float64(hyp[3 * i + j]) for j in range(3)] for i in range(3)]
        mt = _matmul(m, T)
        if model == FUNDAMENTAL:
            left = [[T[j][i] for j in range(3)] for i in range(3)]
        else:
            inv = one / s
            left = [[inv, z, cx], [z, inv, cy], [z, z, one]]
        p = [v for row in _matmul(left, mt) for v in row]
        best, at = np.float64(-1.0), 0
        for i, v in enumerate(p):
            if abs(v) > best:
                best, at = abs(v), i
        return np.array([v / p[at] for v in p], np.float64)


def hypotheses_ref(model, corr, b, hypotheses, seed):
    """(hyp [H, 9], valid [H]) of one frame's correspondences."""
    m, n = SAMPLE[model], corr.shape[0]
    picks = [sample(seed, b, h, n, m) for h in range(hypotheses)]
    ok = np.array([p is not None for p in picks], bool)
    pts = np.zeros((hypotheses, m, 4))
    for h, p in enumerate(picks):
        if p is not None:
            pts[h] = corr[p]
    hyp, valid = null_vector(build_rows(model, pts))
    return hyp, valid & ok


def ransac_ref(q_xy, t_xy, q_counts=None, match_idx=None, pair_valid=None, model=FUNDAMENTAL, hypotheses=256, seed=0,
               threshold=1.0, center=(0.0, 0.0), scale=1.0 / 256, fill=0, detail=None):
    """fd_ransac for [B, S, 2] / [B, T, 2] float32 positions. Returns (model float64 [B, 9], inlier uint8
    [B, S], counts int32 [B], best int32 [B]); inlier slots the call does not write hold `fill`.
    detail (a list) receives per frame (hypothesis inlier counts [H], valid [H])."""
    q_xy, t_xy = np.asarray(q_xy, np.float32), np.asarray(t_xy, np.float32)
    B, S = q_xy.shape[0], q_xy.shape[1]
    cx, cy = center
    t = np.float64(np.float32(threshold)) * np.float64(np.float32(scale))
    tt = t * t
    out_model = np.zeros((B, 9), np.float64)
    out_inl = np.full((B, S), fill, np.uint8)
    out_cnt, out_best = np.zeros(B, np.int32), np.full(B, -1, np.int32)
    for b in range(B):
        cnt = None if q_counts is None else q_counts[b]
        nq = S if cnt is None else min(int(cnt) & COUNT_MASK, S)
        out_inl[b, :nq] = 0
        corr, slots = correspondences(q_xy[b], t_xy[b], cnt, None if match_idx is None else match_idx[b],
                                      None if pair_valid is None else pair_valid[b], cx, cy, scale)
        hyp, valid = hypotheses_ref(model, corr, b, hypotheses, seed)
        inl = inliers(model, hyp, corr, tt) if corr.shape[0] else np.zeros((hypotheses, 0), bool)
        score = inl.sum(axis=1)
        if detail is not None:
            detail.append((score, valid))
        if not valid.any():
            continue
        best = int(np.argmax(np.where(valid, score, -1)))  # first of the largest: the lowest index
        out_best[b] = best
        out_inl[b, slots[inl[best]]] = 1
        out_cnt[b] = int(score[best])
        out_model[b] = denormalise(model, hyp[best], cx, cy, scale)
    return out_model, out_inl, out_cnt, out_best


def conditioning(image_size):
    """verify_geometry's (center, scale) of image_size = (rows, cols), as float32 values."""
    if image_size is None:
        return (0.0, 0.0), float(np.float32(1.0 / 256))
    rows, cols = image_size
    return (float(np.float32((cols - 1) / 2)), float(np.float32((rows - 1) / 2))), float(np.float32(2.0 / (rows + cols)))


# ---- planted scenes of the property tests ---------------------------------------------------------------
ROWS, COLS = 480, 640


def planted_scene(model, seed, n=64, outliers=16):
    """A two-view pinhole scene (F) or a plane seen by two cameras (H): (q [n, 2], t [n, 2] float32, planted
    inlier flags [n]). Positions are rounded to float32, no noise; `outliers` train positions (random
    slots) are replaced by uniform random ones."""
    rng = np.random.default_rng(1000 * (model + 1) + seed)
    K = np.array([[500.0, 0, (COLS - 1) / 2], [0, 500.0, (ROWS - 1) / 2], [0, 0, 1]])
    ax, ay, az = 0.04, -0.10, 0.03
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    Rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    R, tr = Rz @ Ry @ Rx, np.array([0.6, 0.05, 0.1])
    q, t = [], []
    while len(q) < n:
        p = np.array([rng.uniform(-3, 3), rng.uniform(-2.2, 2.2), rng.uniform(4, 9)])
        if model == HOMOGRAPHY:
            p[2] = 6.0 + 0.3 * p[0] - 0.2 * p[1]
        a, b = K @ p, K @ (R @ p + tr)
        a, b = a[:2] / a[2], b[:2] / b[2]
        if 0 <= a[0] <= COLS - 1 and 0 <= a[1] <= ROWS - 1 and 0 <= b[0] <= COLS - 1 and 0 <= b[1] <= ROWS - 1:
            q.append(a)
            t.append(b)
    q, t = np.array(q), np.array(t)
    planted = np.ones(n, bool)
    bad = rng.choice(n, outliers, replace=False)
    planted[bad] = False
    t[bad] = np.stack([rng.uniform(0, COLS - 1, outliers), rng.uniform(0, ROWS - 1, outliers)], axis=1)
    return q.astype(np.float32), t.astype(np.float32), planted


def pixel_residual(model, m9, q, t):
    """Sampson distance (F) or forward transfer error (H), in pixels, of a pixel-coordinate model."""
    M = np.asarray(m9, np.float64).reshape(3, 3)
    qh = np.concatenate([np.asarray(q, np.float64), np.ones((len(q), 1))], axis=1)
    th = np.concatenate([np.asarray(t, np.float64), np.ones((len(t), 1))], axis=1)
    if model == FUNDAMENTAL:
        l, mm = qh @ M.T, th @ M
        e = np.sum(th * l, axis=1)
        return np.abs(e) / np.sqrt(l[:, 0] ** 2 + l[:, 1] ** 2 + mm[:, 0] ** 2 + mm[:, 1] ** 2)
    p = qh @ M.T
    return np.hypot(p[:, 0] / p[:, 2] - th[:, 0], p[:, 1] / p[:, 2] - th[:, 1])
