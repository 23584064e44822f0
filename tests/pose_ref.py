"""numpy restatement of fd_pose_recover and fd_triangulate (include/fd_hip.h): the relative camera pose from a
fundamental matrix and the 3-D points of its inliers, the contract's arithmetic sequence in scalar and
elementwise float64 numpy (IEEE, one rounding per operation). The GPU tests compare every output with it bit
for bit. The correspondence list is fd_ransac's (tests/ransac_ref.py, centre 0 and scale 1: exact) and the
Jacobi routine is fd_ransac_refit's (tests/refit_ref.py).

Also the planted two-view scenes of the tests (scene) and the cases the GPU tests run (all_cases).
"""
import numpy as np

from ransac_ref import COLS, COUNT_MASK, ROWS, correspondences
from refit_ref import jacobi, smallest

SWEEPS = 7       # FD_POSE_SWEEPS: tests/test_pose_host.py::test_sweep_count_rule derives it
RANK_EPS = 1e-12
CAM = (500.0, 500.0, (COLS - 1) / 2, (ROWS - 1) / 2)  # fx, fy, cx, cy of the scenes' query camera
CAM_T = (480.0, 510.0, 300.5, 250.25)                 # a different train camera (two-camera cases)
MAX_DEPTH, MIN_PARALLAX = float("inf"), 1e-3          # the defaults of recover_pose / triangulate


def _f(x):
    return np.float64(x)


def kmat(cam):
    fx, fy, cx, cy = (_f(v) for v in cam)
    z, one = _f(0.0), _f(1.0)
    return [[fx, z, cx], [z, fy, cy], [z, z, one]]


def matmul3(a, b):
    """3 x 3 product, every sum from 0.0 with the inner index ascending (fd_ransac's matmul3)."""
    out = [[_f(0.0)] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            acc = _f(0.0)
            for k in range(3):
                acc = acc + a[i][k] * b[k][j]
            out[i][j] = acc
    return out


def essential(F9, cam_q, cam_t):
    """E = K_t^T (F K_q) as a 3 x 3 list of float64."""
    F = [[_f(F9[3 * i + j]) for j in range(3)] for i in range(3)]
    Kq, Kt = kmat(cam_q), kmat(cam_t)
    KtT = [[Kt[j][i] for j in range(3)] for i in range(3)]
    with np.errstate(all="ignore"):
        return matmul3(KtT, matmul3(F, Kq))


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def candidates(F9, cam_q, cam_t, sweeps=SWEEPS, trace=None):
    """Steps 1-4: (Ra, Rb [3][3], u3 [3]) of the model, or None where there is no pose."""
    E = essential(F9, cam_q, cam_t)
    with np.errstate(all="ignore"):
        G = np.zeros((3, 3), np.float64)
        for i in range(3):
            for j in range(3):
                acc = _f(0.0)
                for k in range(3):
                    acc = acc + E[k][i] * E[k][j]
                G[i, j] = acc
        d, V = jacobi(G, sweeps, trace=trace)
        j = smallest(d)
        a, b = (1 if j == 0 else 0), (1 if j == 2 else 2)
        dmax = d[0]
        for i in range(1, 3):
            if d[i] > dmax:
                dmax = d[i]
        dmin = d[b] if d[b] < d[a] else d[a]
        v1, v2 = [V[k, a] for k in range(3)], [V[k, b] for k in range(3)]
        w1 = [_dot(E[i], v1) for i in range(3)]
        w2 = [_dot(E[i], v2) for i in range(3)]
        n1, n2 = np.sqrt(_dot(w1, w1)), np.sqrt(_dot(w2, w2))
        u1, u2 = [w / n1 for w in w1], [w / n2 for w in w2]
        u3, v3 = _cross(u1, u2), _cross(v1, v2)
        Ra = [[(u2[i] * v1[k] - u1[i] * v2[k]) + u3[i] * v3[k] for k in range(3)] for i in range(3)]
        Rb = [[(u1[i] * v2[k] - u2[i] * v1[k]) + u3[i] * v3[k] for k in range(3)] for i in range(3)]
        used = v1 + v2 + u3 + [x for row in Ra + Rb for x in row] + [d[0], d[1], d[2]]
        if not (bool(np.all(np.isfinite(used))) and bool(dmin > _f(RANK_EPS) * dmax)):
            return None
    return Ra, Rb, u3


def rays(corr, cam_q, cam_t):
    """(ax, ay, bx, by) [n] of the pixel correspondences corr [n, 4]."""
    fq, ft = [_f(v) for v in cam_q], [_f(v) for v in cam_t]
    with np.errstate(all="ignore"):
        return ((corr[:, 0] - fq[2]) / fq[0], (corr[:, 1] - fq[3]) / fq[1],
                (corr[:, 2] - ft[2]) / ft[0], (corr[:, 3] - ft[3]) / ft[1])


def step(R, t, ax, ay, bx, by, max_depth, min_parallax):
    """The per-correspondence step, elementwise over [n]: (in front bool [n], points float32 [n, 3])."""
    D, m = _f(np.float32(max_depth)), _f(np.float32(min_parallax))
    R = [[_f(R[i][k]) for k in range(3)] for i in range(3)]
    t = [_f(v) for v in t]
    with np.errstate(all="ignore"):
        r = [(R[i][0] * ax + R[i][1] * ay) + R[i][2] for i in range(3)]
        one = np.ones_like(ax)
        pp_ = [bx, by, one]
        rr, pp, rp = _dot(r, r), _dot(pp_, pp_), _dot(r, pp_)
        rt, pt = _dot(r, t), _dot(pp_, t)
        det = rr * pp - rp * rp
        z1 = (rp * pt - pp * rt) / det
        z2 = (rr * pt - rp * rt) / det
        front = (det > (m * m) * (rr * pp)) & (z1 > 0) & (z2 > 0) & (z1 <= D) & (z2 <= D)
        pts = np.stack([z1 * ax, z1 * ay, z1], axis=-1).astype(np.float32)
    return front, pts


def _frame(q, t, cnt, idx, valid):
    return correspondences(q, t, cnt, idx, valid, 0.0, 0.0, 1.0)


def _write(out_pts, out_val, out_cnt, b, nq, slots, front, pts):
    out_pts[b, :nq], out_val[b, :nq] = 0.0, 0
    out_pts[b, slots[front]] = pts[front]
    out_val[b, slots[front]] = 1
    out_cnt[b] = int(front.sum())


def _cams(cam_q, cam_t):
    return tuple(cam_q), tuple(cam_q if cam_t is None else cam_t)


def triangulate_ref(q_xy, t_xy, pose, in_inlier=None, q_counts=None, match_idx=None, pair_valid=None, cam_q=CAM, cam_t=None,
                    max_depth=MAX_DEPTH, min_parallax=MIN_PARALLAX, fill=(0.0, 0)):
    """fd_triangulate for [B, S, 2] / [B, T, 2] float32 positions and pose float64 [B, 12]: (points float32
    [B, S, 3], valid uint8 [B, S], counts int32 [B]); slots the call does not write hold `fill`."""
    q_xy, t_xy = np.asarray(q_xy, np.float32), np.asarray(t_xy, np.float32)
    B, S = q_xy.shape[0], q_xy.shape[1]
    cam_q, cam_t = _cams(cam_q, cam_t)
    pose = np.asarray(pose, np.float64).reshape(B, 12)
    out_pts, out_val = np.full((B, S, 3), fill[0], np.float32), np.full((B, S), fill[1], np.uint8)
    out_cnt = np.zeros(B, np.int32)
    for b in range(B):
        cnt = None if q_counts is None else q_counts[b]
        nq = S if cnt is None else min(int(cnt) & COUNT_MASK, S)
        corr, slots = _frame(q_xy[b], t_xy[b], cnt, None if match_idx is None else match_idx[b],
                             None if pair_valid is None else pair_valid[b])
        if in_inlier is not None:
            take = np.asarray(in_inlier, np.uint8).reshape(B, S)[b, slots] == 1
            corr, slots = corr[take], slots[take]
        front, pts = step(pose[b, :9].reshape(3, 3), pose[b, 9:], *rays(corr, cam_q, cam_t), max_depth, min_parallax)
        _write(out_pts, out_val, out_cnt, b, nq, slots, front, pts)
    return out_pts, out_val, out_cnt


def pose_ref(q_xy, t_xy, in_model, in_inlier, q_counts=None, match_idx=None, pair_valid=None, cam_q=CAM, cam_t=None,
             max_depth=MAX_DEPTH, min_parallax=MIN_PARALLAX, fill=(0.0, 0), sweeps=SWEEPS, detail=None):
    """fd_pose_recover. Returns (pose float64 [B, 12], choice int32 [B], points float32 [B, S, 3], valid uint8
    [B, S], counts int32 [B]). detail (a list) receives every frame's four candidate counts (None: no candidates)."""
    q_xy, t_xy = np.asarray(q_xy, np.float32), np.asarray(t_xy, np.float32)
    B, S = q_xy.shape[0], q_xy.shape[1]
    cam_q, cam_t = _cams(cam_q, cam_t)
    in_model = np.asarray(in_model, np.float64).reshape(B, 9)
    in_inlier = np.asarray(in_inlier, np.uint8).reshape(B, S)
    out_pose, out_choice = np.zeros((B, 12), np.float64), np.full(B, -1, np.int32)
    out_pts, out_val = np.full((B, S, 3), fill[0], np.float32), np.full((B, S), fill[1], np.uint8)
    out_cnt = np.zeros(B, np.int32)
    for b in range(B):
        cnt = None if q_counts is None else q_counts[b]
        nq = S if cnt is None else min(int(cnt) & COUNT_MASK, S)
        out_pts[b, :nq], out_val[b, :nq] = 0.0, 0
        corr, slots = _frame(q_xy[b], t_xy[b], cnt, None if match_idx is None else match_idx[b],
                             None if pair_valid is None else pair_valid[b])
        take = in_inlier[b, slots] == 1
        corr, slots = corr[take], slots[take]
        cand = candidates(in_model[b], cam_q, cam_t, sweeps)
        if cand is None:
            if detail is not None:
                detail.append(None)
            continue
        Ra, Rb, u3 = cand
        neg = [-v for v in u3]
        four = [(Ra, u3), (Ra, neg), (Rb, u3), (Rb, neg)]
        ry = rays(corr, cam_q, cam_t)
        res = [step(R, t, *ry, max_depth, min_parallax) for R, t in four]
        counts = [int(f.sum()) for f, _ in res]
        if detail is not None:
            detail.append(counts)
        k = int(np.argmax(counts))  # the first of the largest: the lowest k among equals
        if counts[k] == 0:
            continue
        out_choice[b] = k
        out_pose[b, :9], out_pose[b, 9:] = np.array(four[k][0], np.float64).reshape(9), np.array(four[k][1], np.float64)
        _write(out_pts, out_val, out_cnt, b, nq, slots, *res[k])
    return out_pose, out_choice, out_pts, out_val, out_cnt


# ---- planted scenes ---------------------------------------------------------------------------------------
def rotation(rx, ry, rz):
    Rx = np.array([[1, 0, 0], [0, np.cos(rx), -np.sin(rx)], [0, np.sin(rx), np.cos(rx)]])
    Ry = np.array([[np.cos(ry), 0, np.sin(ry)], [0, 1, 0], [-np.sin(ry), 0, np.cos(ry)]])
    Rz = np.array([[np.cos(rz), -np.sin(rz), 0], [np.sin(rz), np.cos(rz), 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def planted_pose(seed):
    """A seeded pose (R, t), X_t = R X_q + t: a rotation of a few degrees, a baseline of 0.3 to 0.8."""
    rng = np.random.default_rng(31000 + seed)
    R = rotation(*rng.uniform(-0.12, 0.12, 3))
    t = rng.standard_normal(3) * np.array([1.0, 0.6, 0.4])
    return R, t / np.linalg.norm(t) * rng.uniform(0.3, 0.8)


def model_of(R, t, cam_q=CAM, cam_t=None):
    """F = K_t^-T [t]x R K_q^-1 of a pose, divided by its entry of largest magnitude (fd_ransac's form)."""
    cam_q, cam_t = _cams(cam_q, cam_t)
    Kq, Kt = np.array(kmat(cam_q), np.float64), np.array(kmat(cam_t), np.float64)
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    F = np.linalg.inv(Kt).T @ tx @ R @ np.linalg.inv(Kq)
    with np.errstate(all="ignore"):  # t = 0: no F
        return (F / F.ravel()[np.argmax(np.abs(F))]).reshape(9)


def scene(seed, n=64, outliers=16, pose=None, cam_q=CAM, cam_t=None, depth=(4.0, 9.0)):
    """A two-view pinhole scene with a planted pose: n random 3-D points in front of both cameras, projected
    to float32 pixels inside the query image; `outliers` train positions (random slots) replaced
    by uniform random ones. Returns a dict: q, t float32 [n, 2], planted bool [n], X float64 [n, 3] (query
    frame), R, t_vec, model float64 [9] (the planted pose's exact F), cam_q, cam_t."""
    cam_q, cam_t = _cams(cam_q, cam_t)
    R, tv = planted_pose(seed) if pose is None else pose
    rng = np.random.default_rng(32000 + seed)
    Kq, Kt = np.array(kmat(cam_q), np.float64), np.array(kmat(cam_t), np.float64)
    q, t, X = [], [], []
    while len(q) < n:
        p = np.array([rng.uniform(-3, 3), rng.uniform(-2.2, 2.2), rng.uniform(*depth)])
        p2 = R @ p + tv
        if p2[2] < 1.0:
            continue
        a, b = Kq @ p, Kt @ p2
        a, b = a[:2] / a[2], b[:2] / b[2]
        if 0 <= a[0] <= COLS - 1 and 0 <= a[1] <= ROWS - 1 and -200 <= b[0] <= COLS + 200 and -200 <= b[1] <= ROWS + 200:
            q.append(a)
            t.append(b)
            X.append(p)
    q, t, X = np.array(q), np.array(t), np.array(X)
    planted = np.ones(n, bool)
    bad = rng.choice(n, outliers, replace=False)
    planted[bad] = False
    t[bad] = np.stack([rng.uniform(0, COLS - 1, outliers), rng.uniform(0, ROWS - 1, outliers)], axis=1)
    return dict(q=q.astype(np.float32), t=t.astype(np.float32), planted=planted, X=X, R=R, t_vec=tv,
                model=model_of(R, tv, cam_q, cam_t), cam_q=cam_q, cam_t=cam_t)


def behind_scene(seed, n=64, behind=32, outliers=0):
    """scene() whose first `behind` points lie behind both cameras and still satisfy the planted epipolar
    geometry (a point X behind the query camera with R X + t behind the train camera projects like any other):
    they are in front for the pose with -t."""
    sc = scene(seed, n=n, outliers=0)
    R, tv = sc["R"], sc["t_vec"]
    rng = np.random.default_rng(33000 + seed)
    Kq, Kt = np.array(kmat(sc["cam_q"]), np.float64), np.array(kmat(sc["cam_t"]), np.float64)
    k = 0
    while k < behind:
        p = -np.array([rng.uniform(-3, 3), rng.uniform(-2.2, 2.2), rng.uniform(4, 9)])
        p2 = R @ p + tv
        if p2[2] > -1.0:
            continue
        a, b = Kq @ p, Kt @ p2
        a, b = a[:2] / a[2], b[:2] / b[2]
        if 0 <= a[0] <= COLS - 1 and 0 <= a[1] <= ROWS - 1 and -200 <= b[0] <= COLS + 200 and -200 <= b[1] <= ROWS + 200:
            sc["q"][k], sc["t"][k], sc["X"][k] = a.astype(np.float32), b.astype(np.float32), p
            k += 1
    if outliers:
        bad = np.arange(n - outliers, n)
        sc["planted"][bad] = False
        sc["t"][bad] = np.stack([rng.uniform(0, COLS - 1, outliers), rng.uniform(0, ROWS - 1, outliers)], axis=1).astype(np.float32)
    return sc


def rotation_scene(seed, n=64):
    """A pure rotation: t = 0, so every pair of rays is parallel. The model is the F of the same rotation with
    an arbitrary translation, which the pairs satisfy exactly: it has rank 2, and no candidate has a point."""
    R, _ = planted_pose(seed)
    sc = scene(seed, n=n, outliers=0, pose=(R, np.zeros(3)))
    sc["model"] = model_of(R, np.array([0.5, 0.1, -0.2]))
    return sc


# Seeds of scene() whose restatement picks candidate 0, 1, 2 and 3: found by a search over the seeds 0..63 on the
# CPU (tests/test_pose_host.py::test_every_choice_wins confirms each).
CHOICE_SEEDS = {0: 0, 1: 3, 2: 1, 3: 2}


def case(sc, **kw):
    """A case dict of one scene (batch 1): the planted model, the planted flags as in_inlier."""
    d = dict(q=sc["q"][None], t=sc["t"][None], counts=None, idx=None, valid=None, in_model=sc["model"][None].copy(),
             in_inlier=sc["planted"].astype(np.uint8)[None], cam_q=sc["cam_q"], cam_t=sc["cam_t"], max_depth=MAX_DEPTH,
             min_parallax=MIN_PARALLAX)
    d.update(kw)
    return d


def stack(cases, **kw):
    """Frames of equal stride into one batch (camera and options of the first)."""
    d = dict(cases[0])
    for k in ("q", "t", "in_model", "in_inlier"):
        d[k] = np.concatenate([c[k] for c in cases], 0)
    d.update(kw)
    return d


def stride_case(stride):
    """One frame of `stride` slots, a quarter outliers, two cameras."""
    return case(scene(100 + stride, n=stride, outliers=stride // 4, cam_t=CAM_T))


def batch_case():
    """Batch 3, stride 90: a zero model, a frame with q_counts below the stride (and flag bits), a full frame."""
    a, b, c = (case(scene(200 + k, n=90, outliers=20)) for k in range(3))
    d = stack([a, b, c], counts=np.array([90, 60 | (1 << 25) | (1 << 31), 90], np.uint32).view(np.int32))
    d["in_model"][0] = 0.0
    return d


def holes_case():
    """Batch 3: match_idx with -1, out-of-range and repeated train indices, pair_valid bytes 0..6, non-finite
    coordinates, and in_inlier bytes 0, 2 and 0xFF beside 1 (a 1 also at slots that are no correspondences)."""
    rng = np.random.default_rng(12)
    S, T = 90, 75
    frames = [case(scene(300 + k, n=S, outliers=20)) for k in range(3)]
    d = stack(frames)
    idx = np.tile(np.arange(S, dtype=np.int32), (3, 1))
    # the train array keeps the first T positions: slots past T pair with an earlier train point (outliers)
    idx[:, T:] = np.arange(S - T, dtype=np.int32) * 3
    d["t"] = np.ascontiguousarray(d["t"][:, :T])
    idx[:, 5], idx[:, 6], idx[:, 7], idx[:, 8] = -1, T, -2 ** 31, 2 ** 31 - 1
    idx[1, 20:30] = 3
    valid = np.ones((3, S), np.uint8)
    valid[0, 10:24] = np.arange(14) % 7
    valid[2] = np.where(rng.random(S) < 0.2, rng.integers(0, 7, S), 1)
    q, t = d["q"], d["t"]
    q[0, 30, 0], q[0, 31, 1], t[0, 32, 0], t[0, 33, 1] = np.nan, np.inf, -np.inf, np.nan
    inl = d["in_inlier"]
    inl[:, T:] = 1
    for b in range(3):
        ones = np.flatnonzero(inl[b] == 1)
        inl[b, ones[1::9]], inl[b, ones[2::9]], inl[b, ones[4::9]] = 2, 0xFF, 0
        inl[b, 5], inl[b, 30 + b] = 1, 1
    d.update(idx=idx, valid=valid, counts=np.array([S, 70, 77], np.int32))
    return d


def tie_case():
    """Half of the points behind both cameras: (R, +t) and (R, -t) have equal counts, and the lower index wins."""
    return case(behind_scene(400, n=64, behind=32))


def count0_case():
    """A valid model whose in_inlier has no byte equal to 1: every candidate counts 0."""
    sc = scene(401, n=32, outliers=8)
    return case(sc, in_inlier=np.where(sc["planted"], 2, 0).astype(np.uint8)[None])


def rotation_case():
    return case(rotation_scene(402))


def depth_case():
    """max_depth (in units of |t|) between the scene's nearest and farthest inlier."""
    return case(scene(403, n=64, outliers=8, depth=(2.0, 12.0)), max_depth=15.0)


def parallax_case():
    """min_parallax between the scene's smallest and largest ray angle."""
    return case(scene(404, n=64, outliers=8, depth=(2.0, 12.0)), min_parallax=0.05)


def nonfinite_model_case():
    sc = scene(405, n=16, outliers=0)
    m = sc["model"].copy()
    m[4] = np.nan
    return case(sc, in_model=m[None])


def all_cases():
    """(name, case) of every scene the GPU tests compare with the restatement."""
    out = [(f"stride-{s}", stride_case(s)) for s in (8, 255, 256, 257, 513)]
    out += [(f"choice-{k}", case(scene(seed))) for k, seed in CHOICE_SEEDS.items()]
    out += [("batch", batch_case()), ("holes", holes_case()), ("tie", tie_case()), ("count0", count0_case()),
            ("rotation", rotation_case()), ("depth", depth_case()), ("parallax", parallax_case()),
            ("nonfinite-model", nonfinite_model_case())]
    return out


def _opts(c):
    return dict(q_counts=c["counts"], match_idx=c["idx"], pair_valid=c["valid"], cam_q=c["cam_q"], cam_t=c["cam_t"],
                max_depth=c["max_depth"], min_parallax=c["min_parallax"])


def run_pose(c, fill=(0.0, 0), sweeps=SWEEPS, detail=None):
    return pose_ref(c["q"], c["t"], c["in_model"], c["in_inlier"], fill=fill, sweeps=sweeps, detail=detail, **_opts(c))


def run_triangulate(c, pose, use_inlier=True, fill=(0.0, 0)):
    return triangulate_ref(c["q"], c["t"], pose, c["in_inlier"] if use_inlier else None, fill=fill, **_opts(c))


# ---- accuracy against the planted pose ----------------------------------------------------------------------
def rotation_angle(Ra, Rb):
    """The angle of Ra^T Rb, from the sine (its skew part) and the cosine: arccos alone resolves no angle
    below 1.5e-8."""
    D = np.asarray(Ra, np.float64).reshape(3, 3).T @ np.asarray(Rb, np.float64).reshape(3, 3)
    s = np.linalg.norm([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]]) / 2.0
    return float(np.arctan2(s, (np.trace(D) - 1.0) / 2.0))


def direction_angle(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.arctan2(np.linalg.norm(np.cross(a, b)), a @ b))


def independent_solution(F9, q, t, cam_q, cam_t):
    """np.linalg.svd decomposition of E and linear (DLT) triangulation in float64, the candidate chosen by the
    number of points with positive depth in both cameras: (R [3, 3], t [3] of unit length, depths [n])."""
    Kq, Kt = np.array(kmat(cam_q), np.float64), np.array(kmat(cam_t), np.float64)
    E = Kt.T @ np.asarray(F9, np.float64).reshape(3, 3) @ Kq
    U, _, Vt = np.linalg.svd(E)
    if np.linalg.det(U) < 0:
        U = -U
    if np.linalg.det(Vt) < 0:
        Vt = -Vt
    W = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    a = np.linalg.solve(Kq, np.concatenate([q.astype(np.float64), np.ones((len(q), 1))], 1).T).T
    b = np.linalg.solve(Kt, np.concatenate([t.astype(np.float64), np.ones((len(t), 1))], 1).T).T
    best = None
    for R in (U @ W @ Vt, U @ W.T @ Vt):
        for tv in (U[:, 2], -U[:, 2]):
            P2 = np.concatenate([R, tv[:, None]], 1)
            z = np.zeros(len(q))
            good = 0
            for i in range(len(q)):
                A = np.stack([np.array([1.0, 0, -a[i, 0], 0]), np.array([0, 1.0, -a[i, 1], 0]),
                              P2[0] - b[i, 0] * P2[2], P2[1] - b[i, 1] * P2[2]])
                X = np.linalg.svd(A)[2][-1]
                X = X[:3] / X[3]
                z[i] = X[2]
                good += X[2] > 0 and (R @ X + tv)[2] > 0
            if best is None or good > best[0]:
                best = (good, R, tv, z)
    return best[1], best[2], best[3]
