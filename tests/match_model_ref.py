"""Helper: a numpy restatement of the model-gated matchers' contract (fd_brief_match_model /
fd_nn_match_model, include/fd_hip.h), the yardstick of the model-gated matching tests.

Not a third matcher: the gate is the contract's float64 expression with its grouping, and it is applied as
a candidate mask to what tests/match_ref.py and tests/nn_match_ref.py already do, exactly as
tests/match_guided_ref.py applies the window (the window's mask, gate_mask, is taken from there). The
cross-check's reverse search uses column t of the same (query, train) mask: a pair is judged by the forward
predicate whichever side is searched.

The module also holds the two-view models and the random fixtures the CPU and the GPU tests share.
"""
import numpy as np

import match_guided_ref as G
import nn_match_ref as R
from match_guided_ref import gate_mask
from match_ref import _count, match_ref

F32, F64, U8 = np.float32, np.float64, np.uint8
FUNDAMENTAL, HOMOGRAPHY = 0, 1
KINDS = {"fundamental": FUNDAMENTAL, "homography": HOMOGRAPHY}
OPEN = 3.0e38


def model_mask(q_xy, t_xy, model, kind, threshold):
    """[Sq, 2], [St, 2] float32, model float64 [9] -> [Sq, St] bool: the model test of include/fd_hip.h in
    float64, one rounding per operation (numpy fuses nothing), the groupings as written there. A NaN fails."""
    q, t = np.asarray(q_xy), np.asarray(t_xy)
    assert q.dtype == F32 and t.dtype == F32
    M = np.asarray(model, F64).reshape(9)
    x, y = q[:, 0].astype(F64)[:, None], q[:, 1].astype(F64)[:, None]
    u, v = t[:, 0].astype(F64)[None, :], t[:, 1].astype(F64)[None, :]
    tt = F64(F32(threshold))
    tt = tt * tt
    with np.errstate(all="ignore"):
        if kind == FUNDAMENTAL:
            l0 = (M[0] * x + M[1] * y) + M[2]
            l1 = (M[3] * x + M[4] * y) + M[5]
            l2 = (M[6] * x + M[7] * y) + M[8]
            m0 = (M[0] * u + M[3] * v) + M[6]
            m1 = (M[1] * u + M[4] * v) + M[7]
            e = (u * l0 + v * l1) + l2
            return e * e <= tt * ((l0 * l0 + l1 * l1) + (m0 * m0 + m1 * m1))
        assert kind == HOMOGRAPHY
        px = (M[0] * x + M[1] * y) + M[2]
        py = (M[3] * x + M[4] * y) + M[5]
        w = (M[6] * x + M[7] * y) + M[8]
        dx = px - u * w
        dy = py - v * w
        return dx * dx + dy * dy <= tt * (w * w)


def pair_mask(q_xy, t_xy, model, kind, threshold, radius=OPEN):
    """The whole gate of one frame: the window of fd_match_gate and the model test."""
    return gate_mask(q_xy, t_xy, radius) & model_mask(q_xy, t_xy, model, kind, threshold)


def _flags(valid, B, S, b, n):
    return np.ones(n, bool) if valid is None else np.asarray(valid).reshape(B, S)[b, :n].astype(bool)


def _gated(B, Sq, St, q_xy, t_xy, mask, q_counts, t_counts, q_valid, t_valid, cross_check, fill, dist_dtype, frame):
    """match_guided_ref._guided with the frame's candidate mask from mask(b, q_xy, t_xy) instead of the window."""
    q_xy = np.asarray(q_xy).reshape(B, Sq, 2)
    t_xy = np.asarray(t_xy).reshape(B, St, 2)
    idx = np.full((B, Sq), fill, np.int32)
    dist = np.full((B, Sq, 2), fill, dist_dtype)
    counts = np.zeros((B,), np.int32)
    for b in range(B):
        nq, nt = _count(q_counts, b, Sq), _count(t_counts, b, St)
        row, back = frame(b, nq, nt)
        M = mask(b, q_xy[b, :nq], t_xy[b, :nt])
        q_ok, t_ok = _flags(q_valid, B, Sq, b, nq), _flags(t_valid, B, St, b, nt)
        seen = {}
        for q in range(nq):
            if not q_ok[q]:
                idx[b, q], dist[b, q] = -1, (-1, -1)
                continue
            i, d1, d2 = row(q, M[q] & t_ok)
            if i >= 0 and cross_check:
                if i not in seen:
                    seen[i] = back(i, M[:, i] & q_ok)
                if seen[i] != q:
                    i = -1
            idx[b, q], dist[b, q, 0], dist[b, q, 1] = i, d1, d2
            counts[b] += int(i >= 0)
    return idx, dist, counts


def _mask_of(model, kind, threshold, radius, B):
    model = np.asarray(model, F64).reshape(B, 9)
    return lambda b, q, t: pair_mask(q, t, model[b], kind, threshold, radius)


def match_model_ref(q_bits, t_bits, q_xy, t_xy, model, kind, threshold, radius=OPEN, q_counts=None, t_counts=None,
                    q_valid=None, t_valid=None, length=256, max_distance=-1, max_ratio=0.0, cross_check=False, fill=-1):
    """fd_brief_match_model: (idx [B, Sq], dist [B, Sq, 2], counts [B]) int32; slots >= q_counts[b] hold `fill`."""
    q_bits, t_bits = np.asarray(q_bits), np.asarray(t_bits)
    if q_bits.ndim == 2:
        q_bits, t_bits = q_bits[None], t_bits[None]
    B, Sq, St = q_bits.shape[0], q_bits.shape[1], t_bits.shape[1]

    def frame(b, nq, nt):
        def row(q, cand):
            i, d, _ = match_ref(q_bits[b, q:q + 1], t_bits[b, :nt], t_valid=cand.astype(U8)[None], length=length,
                                max_distance=max_distance, max_ratio=max_ratio)
            return int(i[0, 0]), int(d[0, 0, 0]), int(d[0, 0, 1])

        def back(t, cand):
            return int(match_ref(t_bits[b, t:t + 1], q_bits[b, :nq], t_valid=cand.astype(U8)[None], length=length)[0][0, 0])

        return row, back

    return _gated(B, Sq, St, q_xy, t_xy, _mask_of(model, kind, threshold, radius, B), q_counts, t_counts, q_valid, t_valid,
                  cross_check, fill, np.int32, frame)


def nn_match_model_ref(q_desc, t_desc, q_xy, t_xy, model, kind, threshold, radius=OPEN, q_counts=None, t_counts=None,
                       q_valid=None, t_valid=None, max_distance=-1.0, max_ratio=0.0, cross_check=False, fill=-1):
    """fd_nn_match_model: (idx [B, Sq] int32, dist [B, Sq, 2] float32, counts [B] int32)."""
    q_desc, t_desc = np.asarray(q_desc, F32), np.asarray(t_desc, F32)
    if q_desc.ndim == 2:
        q_desc, t_desc = q_desc[None], t_desc[None]
    B, Sq, St = q_desc.shape[0], q_desc.shape[1], t_desc.shape[1]

    def frame(b, nq, nt):
        D = R.distances(q_desc[b, :nq], t_desc[b, :nt])

        def row(q, cand):
            return R.accept_from_distances(D[q:q + 1], [0], np.flatnonzero(cand).tolist(), max_distance, max_ratio)[0]

        def back(t, cand):
            return R.scan(D[:, t], np.flatnonzero(cand).tolist())[0]

        return row, back

    return _gated(B, Sq, St, q_xy, t_xy, _mask_of(model, kind, threshold, radius, B), q_counts, t_counts, q_valid, t_valid,
                  cross_check, fill, F32, frame)


# ---- two-view models -------------------------------------------------------------------------------------------
def _normalised(m):
    """Divided by the entry of largest magnitude (the lowest index among equals), as fd_ransac writes a model."""
    m = np.asarray(m, F64).reshape(9)
    return m / m[int(np.argmax(np.abs(m)))]


def fundamental(seed=0, focal=60.0, centre=32.0):
    """F of a small rotation and a sideways-forward translation between two views of focal length ~60 with
    the principal point at the centre of the 64-pixel square: x2^T F x1 = 0 with x1 the query, x2 the train."""
    rng = np.random.default_rng([17, seed])
    ax, ay, az = rng.uniform(-0.04, 0.04, 3)
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    Rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    t = np.array([1.0, rng.uniform(-0.2, 0.2), rng.uniform(0.3, 0.6)])
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Kinv = np.linalg.inv(np.array([[focal, 0, centre], [0, focal, centre], [0, 0, 1.0]]))
    return _normalised(Kinv.T @ tx @ (Rz @ Ry @ Rx) @ Kinv)


def homography(seed=0):
    """H close to the identity: a small rotation, scale, shift and perspective on the 64-pixel square."""
    rng = np.random.default_rng([23, seed])
    a, s = rng.uniform(-0.05, 0.05), 1.0 + rng.uniform(-0.03, 0.03)
    H = np.array([[s * np.cos(a), -s * np.sin(a), rng.uniform(-3, 3)], [s * np.sin(a), s * np.cos(a), rng.uniform(-3, 3)],
                  [rng.uniform(-4e-4, 4e-4), rng.uniform(-4e-4, 4e-4), 1.0]])
    return _normalised(H)


def make_model(kind, seed=0):
    return fundamental(seed) if kind == FUNDAMENTAL else homography(seed)


def plant_on_gate(rng, q_xy, t_xy, model, kind, threshold, share=3):
    """Move 1 in `share` train keypoints of one frame ([Sq, 2], [St, 2]) onto, and just to either side of, the
    gate's boundary of a random query: on the query's epipolar line / transfer point, or off it by about the
    threshold times 0, 0.98, 1.02 (F: times sqrt 2, the Sampson distance being about the line distance over
    sqrt 2 here). float32 positions cannot sit on the boundary exactly; the hand-written cases cover that."""
    M = np.asarray(model, F64).reshape(3, 3)
    if not np.isfinite(M).all() or not M.any():
        return
    Sq, St = q_xy.shape[0], t_xy.shape[0]
    for _ in range(St // share):
        x, y = q_xy[rng.integers(Sq)].astype(F64)
        off = float(threshold) * rng.choice([0.0, 0.98, 1.02, -0.98, -1.02])
        p = M @ np.array([x, y, 1.0])
        if kind == FUNDAMENTAL:
            n = np.hypot(p[0], p[1])
            if not n > 0:
                continue
            nx, ny = p[0] / n, p[1] / n
            s = rng.uniform(-40, 40)  # along the line, from its point closest to the square's centre
            d0 = (p[0] * 32 + p[1] * 32 + p[2]) / n
            u, v = 32 - d0 * nx - s * ny + off * np.sqrt(2) * nx, 32 - d0 * ny + s * nx + off * np.sqrt(2) * ny
        else:
            a = rng.uniform(0, 2 * np.pi)
            u, v = p[0] / p[2] + off * np.cos(a), p[1] / p[2] + off * np.sin(a)
        t_xy[rng.integers(St)] = (u, v)


# ---- shared random fixtures ------------------------------------------------------------------------------------
def _models(kind, B, models, seed):
    """The frames' models [B, 9]. "real": a different model per frame; "mixed": frame 1 all zeros (no model),
    frame 2 with a NaN entry."""
    m = np.stack([make_model(kind, seed + b) for b in range(B)])
    if models == "mixed":
        assert B == 3
        m[1] = 0.0
        m[2, 4] = np.nan
    return m


def _with_model(c, kind, threshold, B, models, seed, radius):
    rng = np.random.default_rng([B, seed, kind, int(threshold * 100)])
    c["model"] = _models(kind, B, models, seed)
    c["kind"], c["threshold"], c["radius"] = kind, threshold, radius
    for b in range(B):
        plant_on_gate(rng, c["q_xy"][b], c["t_xy"][b], c["model"][b], kind, threshold)
    return c


def brief_case(nq, nt, kind=FUNDAMENTAL, threshold=1.5, radius=OPEN, models="real", length=256, B=1, qc=None, tc=None,
               flags=False, seed=0):
    """match_guided_ref.brief_case (integer positions on the 64-pixel square) with a model per frame and a
    share of the train keypoints planted around the gate's boundary."""
    return _with_model(G.brief_case(nq, nt, length=length, B=B, qc=qc, tc=tc, flags=flags, seed=seed), kind, threshold, B,
                       models, seed, radius)


def nn_case(nq, nt, kind=FUNDAMENTAL, threshold=1.5, radius=OPEN, models="real", dim=128, regime="int", B=1, qc=None,
            tc=None, flags=False, seed=0):
    return _with_model(G.nn_case(nq, nt, dim=dim, regime=regime, B=B, qc=qc, tc=tc, flags=flags, seed=seed), kind, threshold,
                       B, models, seed, radius)


# Two thresholds per kind (F stays below about 3 px: a wider band lets the unguided best back in).
GATES = ((FUNDAMENTAL, 0.5), (HOMOGRAPHY, 1.5), (FUNDAMENTAL, 2.5), (HOMOGRAPHY, 4.0))


def _cycle(cases):
    return [dict(kw, kind=GATES[i % 4][0], threshold=GATES[i % 4][1]) for i, kw in enumerate(cases)]


# The random cases of tests/test_gpu_match_model.py as keyword sets of brief_case / nn_case;
# tests/test_match_model_host.py proves on the restatement alone that the gate decides each of them.
# Hamming: the 64-query workgroup and the 256-entry tile at their edges, the four gates cycling over the grid
# (every gate meets every nt); NW 1, 2, 4, 8 and the tail mask under both kinds; window and band together; a
# batch of 3 with different counts, flags and a model per frame, and one with a zero and a NaN model.
BRIEF_CASES = (
    _cycle([dict(nq=nq, nt=nt) for nt in (1, 255, 256, 257, 513) for nq in (1, 63, 64, 65)] + [dict(nq=65, nt=513)])
    + [dict(nq=65, nt=257, length=length, kind=k, threshold=t) for length in (1, 33, 100)
       for k, t in ((FUNDAMENTAL, 1.5), (HOMOGRAPHY, 4.0))]
    + [dict(nq=65, nt=300, kind=k, threshold=t, radius=r) for k, t in GATES[1:3] for r in (8.0, (20.0, 5.0))]
    + [dict(nq=70, nt=300, B=3, qc=[70, 33, 65], tc=[300, 120, 257], flags=True, kind=k, threshold=t, models=m, radius=r,
            length=length)
       for (k, t), m, r, length in ((GATES[0], "real", OPEN, 256), (GATES[1], "mixed", 8.0, 100), (GATES[2], "mixed", 8.0, 256),
                                    (GATES[3], "real", OPEN, 100))]
)
# Float: both K instances and zero padding; the wave's 16 rows and the workgroup's 64; both sides of TB (64 /
# 32); both regimes; the same gates, window cases and batches.
NN_CASES = (
    _cycle([dict(nq=nq, nt=65, dim=dim, regime=reg) for nq in (1, 16, 17, 64, 65) for dim, reg in ((128, "int"), (256, "round"))])
    + _cycle([dict(nq=17, nt=nt, dim=dim, regime=reg) for nt in (31, 32, 33, 64, 65, 129)
              for dim, reg in ((128, "round"), (256, "int"))])
    + [dict(nq=65, nt=129, dim=dim, regime="round", kind=k, threshold=t) for dim in (4, 132)
       for k, t in ((FUNDAMENTAL, 1.5), (HOMOGRAPHY, 4.0))]
    + [dict(nq=65, nt=129, dim=128, kind=k, threshold=t, radius=r) for k, t in GATES[1:3] for r in (8.0, (20.0, 5.0))]
    + [dict(nq=70, nt=130, B=3, qc=[70, 41, 66], tc=[130, 99, 17], flags=True, kind=k, threshold=t, models=m, radius=r, dim=dim,
            regime=reg)
       for (k, t), m, r, dim, reg in ((GATES[0], "real", OPEN, 128, "int"), (GATES[1], "mixed", 8.0, 256, "round"),
                                      (GATES[2], "mixed", 8.0, 128, "round"), (GATES[3], "real", OPEN, 256, "int"))]
)


def case_id(kw):
    return "-".join(f"{k}{v}" for k, v in kw.items() if k not in ("qc", "tc")).replace(" ", "")


def ref(which, c, fill=-1, **kw):
    """The restatement on a case dict of brief_case / nn_case."""
    if which == "brief":
        return match_model_ref(c["q"], c["t"], c["q_xy"], c["t_xy"], c["model"], c["kind"], c["threshold"], c["radius"], c["qc"],
                               c["tc"], c["qv"], c["tv"], length=c["length"], fill=fill, **kw)
    return nn_match_model_ref(c["q"], c["t"], c["q_xy"], c["t_xy"], c["model"], c["kind"], c["threshold"], c["radius"], c["qc"],
                              c["tc"], c["qv"], c["tv"], fill=fill, **kw)


# ---- the chain's scene: planted two-view correspondences -------------------------------------------------------
def two_view_scene(n=160, seed=3, noise=0.15):
    """Keypoints of a homography-related pair of views on a 640 x 480 frame with BRIEF-like descriptors: train
    entry perm[i] is query i moved by the homography (plus sub-pixel noise) with a descriptor a few bits from the
    query's. Every third query also has a decoy: a train entry elsewhere in the frame whose descriptor is exactly
    as close as the true partner's, so the first pass's ratio test rejects the pair (a third of the first-pass
    matches destroyed); the model gate removes the decoy. The other train entries are noise. Returns a dict
    (q, t uint32 [1, n, 8] / [1, 2n, 8]; q_xy, t_xy float32; perm; H)."""
    rng = np.random.default_rng(seed)
    H = np.array([[0.98, -0.03, 14.0], [0.025, 1.01, -9.0], [2e-5, -1e-5, 1.0]])
    q_xy = np.stack([rng.uniform(40, 600, n), rng.uniform(40, 440, n)], 1)
    p = np.c_[q_xy, np.ones(n)] @ H.T
    moved = p[:, :2] / p[:, 2:] + rng.normal(0, noise, (n, 2))
    perm = rng.permutation(2 * n)
    t_xy = np.stack([rng.uniform(0, 640, 2 * n), rng.uniform(0, 480, 2 * n)], 1)
    q = G.rand_words(rng, n, 8)
    t = G.rand_words(rng, 2 * n, 8)

    def flip(w, k):
        w = w.copy()
        for bit in rng.choice(256, k, replace=False):
            w[bit // 32] ^= np.uint32(1 << (bit % 32))
        return w

    for i in range(n):
        t_xy[perm[i]] = moved[i]
        k = int(rng.integers(4, 12))
        t[perm[i]] = flip(q[i], k)
        if i % 3:
            continue
        # the decoy, far from where the model sends the query
        j = perm[n + i]
        while True:
            cand = np.array([rng.uniform(0, 640), rng.uniform(0, 480)])
            if np.hypot(*(cand - moved[i])) > 40:
                break
        t_xy[j] = cand
        t[j] = flip(q[i], k)
    return dict(q=q[None], t=t[None], q_xy=q_xy.astype(F32)[None], t_xy=t_xy.astype(F32)[None], perm=perm, n=n,
                H=_normalised(H))
