"""Helper: a numpy restatement of the guided matchers' contract (fd_brief_match_guided /
fd_nn_match_guided, include/fd_hip.h), the yardstick of the guided-matching tests.

Not a second matcher: the gate is the contract's float32 expression, and it is applied as a candidate
mask to what tests/match_ref.py and tests/nn_match_ref.py already do. A query's row is match_ref on that
one query with the window as the train flags (Hamming), or accept_from_distances on the query's row of
the distance matrix with the window's indices as candidates (float); the cross-check's reverse search is
the same with the roles swapped, which the gate's symmetry allows.

The module also holds the random fixtures the CPU and the GPU tests share (positions, descriptor sets).
"""
import numpy as np

import nn_match_ref as R
from match_ref import _count, match_ref

F32 = np.float32
U8 = np.uint8


def radii(radius):
    """radius (a float or an (rx, ry) pair) -> (rx, ry) as float32."""
    try:
        rx, ry = radius
    except TypeError:
        rx = ry = radius
    return F32(rx), F32(ry)


def gate_mask(q_xy, t_xy, radius):
    """[Sq, 2], [St, 2] float32 -> [Sq, St] bool: fabsf(t.x - q.x) <= rx and fabsf(t.y - q.y) <= ry, each one
    float32 subtraction and one inclusive compare; a NaN (inf - inf included) compares false."""
    q, t = np.asarray(q_xy), np.asarray(t_xy)
    assert q.dtype == F32 and t.dtype == F32
    rx, ry = radii(radius)
    with np.errstate(all="ignore"):
        dx = np.abs(t[None, :, 0] - q[:, None, 0])
        dy = np.abs(t[None, :, 1] - q[:, None, 1])
        assert dx.dtype == F32 and dy.dtype == F32
        return (dx <= rx) & (dy <= ry)


def _flags(valid, B, S, b, n):
    return np.ones(n, bool) if valid is None else np.asarray(valid).reshape(B, S)[b, :n].astype(bool)


def _guided(B, Sq, St, q_xy, t_xy, radius, q_counts, t_counts, q_valid, t_valid, cross_check, fill, dist_dtype, frame):
    """The frame loop both matchers share. frame(b, nq, nt) -> (row, back): row(q, cand) is query q's
    (accepted index, d1, d2) over the train flags `cand` without the cross-check, back(t, cand) train t's
    raw best query over the query flags `cand`."""
    q_xy = np.asarray(q_xy).reshape(B, Sq, 2)
    t_xy = np.asarray(t_xy).reshape(B, St, 2)
    idx = np.full((B, Sq), fill, np.int32)
    dist = np.full((B, Sq, 2), fill, dist_dtype)
    counts = np.zeros((B,), np.int32)
    for b in range(B):
        nq, nt = _count(q_counts, b, Sq), _count(t_counts, b, St)
        row, back = frame(b, nq, nt)
        M = gate_mask(q_xy[b, :nq], t_xy[b, :nt], radius)
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


def match_guided_ref(q_bits, t_bits, q_xy, t_xy, radius, q_counts=None, t_counts=None, q_valid=None, t_valid=None,
                     length=256, max_distance=-1, max_ratio=0.0, cross_check=False, fill=-1):
    """fd_brief_match_guided: (idx [B, Sq], dist [B, Sq, 2], counts [B]) int32; slots >= q_counts[b] hold `fill`."""
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

    return _guided(B, Sq, St, q_xy, t_xy, radius, q_counts, t_counts, q_valid, t_valid, cross_check, fill, np.int32, frame)


def nn_match_guided_ref(q_desc, t_desc, q_xy, t_xy, radius, q_counts=None, t_counts=None, q_valid=None, t_valid=None,
                        max_distance=-1.0, max_ratio=0.0, cross_check=False, fill=-1):
    """fd_nn_match_guided: (idx [B, Sq] int32, dist [B, Sq, 2] float32, counts [B] int32)."""
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

    return _guided(B, Sq, St, q_xy, t_xy, radius, q_counts, t_counts, q_valid, t_valid, cross_check, fill, F32, frame)


# ---- shared fixtures --------------------------------------------------------------------------------------
def rand_words(rng, *shape):
    return rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)


def unit_rows(rng, *shape):
    """L2-normalised Gaussian rows (float32): what SuperPoint / DISK descriptors look like."""
    x = rng.standard_normal(shape)
    return (x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(F32)


def int_rows(rng, *shape):
    """Integer-valued floats in -7..7: every sum of the distance is exact in any order (the integer regime)."""
    return rng.integers(-7, 8, shape).astype(F32)


def positions(rng, B, Sq, St, variant, side=64):
    """(q_xy [B, Sq, 2], t_xy [B, St, 2]) float32 on a side x side pixel square.
    "int": integer pixels, as the detectors write; "tenth": multiples of 0.1f, where the gate's subtraction
    rounds; "far": integer train pixels, and queries predicted up to a quarter of the square outside the
    frame on every edge, so some coordinates are negative."""
    if variant == "int":
        q, t = rng.integers(0, side, (B, Sq, 2)), rng.integers(0, side, (B, St, 2))
        return q.astype(F32), t.astype(F32)
    if variant == "tenth":
        q, t = rng.integers(0, 10 * side, (B, Sq, 2)), rng.integers(0, 10 * side, (B, St, 2))
        return (q.astype(F32) * F32(0.1)).astype(F32), (t.astype(F32) * F32(0.1)).astype(F32)
    assert variant == "far"
    q = rng.integers(-side // 4, side + side // 4, (B, Sq, 2)).astype(F32) + F32(0.5)
    return q, rng.integers(0, side, (B, St, 2)).astype(F32)


def changed_fraction(guided, plain):
    """Of the queries the unguided reference gives a match, the fraction whose index the gate changes."""
    live = plain[0] >= 0
    return float((guided[0][live] != plain[0][live]).mean()) if live.any() else 0.0


def _plant_positions(rng, q_xy, t_xy):
    """Put a third of the train keypoints exactly on a query keypoint, so that radius 0 finds candidates."""
    B, Sq, St = q_xy.shape[0], q_xy.shape[1], t_xy.shape[1]
    for b in range(B):
        for _ in range(min(Sq, St) // 3):
            t_xy[b, rng.integers(St)] = q_xy[b, rng.integers(Sq)]


def _sides(rng, B, Sq, St, qc, tc, flags):
    """Counts and valid flags of a case: None (all of the stride, all valid) unless asked for."""
    qc = None if qc is None else np.asarray(qc, np.int32)
    tc = None if tc is None else np.asarray(tc, np.int32)
    qv = (rng.random((B, Sq)) < 0.85).astype(U8) if flags else None
    tv = (rng.random((B, St)) < 0.85).astype(U8) if flags else None
    return qc, tc, qv, tv


def brief_case(nq, nt, length=256, variant="int", radius=8.0, B=1, qc=None, tc=None, flags=False, seed=0):
    """A random Hamming case: dict of the arrays and keywords match_guided_ref takes. Descriptors are
    random words (garbage above `length`), with near copies of queries planted among the train entries."""
    rng = np.random.default_rng([nq, nt, length, B, seed, sum(map(ord, variant))])
    nw = (length + 31) // 32
    q, t = rand_words(rng, B, nq, nw), rand_words(rng, B, nt, nw)
    for b in range(B):
        for _ in range(nt // 3):  # copies of queries with bit 0 flipped: distance <= 1
            t[b, rng.integers(nt)] = q[b, rng.integers(nq)] ^ np.uint32(1) * (np.arange(nw) == 0).astype(np.uint32)
    q_xy, t_xy = positions(rng, B, nq, nt, variant)
    _plant_positions(rng, q_xy, t_xy)
    qc, tc, qv, tv = _sides(rng, B, nq, nt, qc, tc, flags)
    return dict(q=q, t=t, q_xy=q_xy, t_xy=t_xy, radius=radius, qc=qc, tc=tc, qv=qv, tv=tv, length=length)


def nn_case(nq, nt, dim=128, regime="int", variant="int", radius=8.0, B=1, qc=None, tc=None, flags=False, seed=0):
    """A random float case. regime "int": integer-valued rows (exact sums, many ties and zero distances);
    "round": unit rows with near copies, where every step of the distance rounds."""
    rng = np.random.default_rng([nq, nt, dim, B, seed, sum(map(ord, variant + regime))])
    if regime == "int":
        q, t = int_rows(rng, B, nq, dim), int_rows(rng, B, nt, dim)
        for b in range(B):
            for _ in range(nt // 3):
                t[b, rng.integers(nt)] = q[b, rng.integers(nq)]  # zero distances, tied trains
    else:
        assert regime == "round"
        q, t = unit_rows(rng, B, nq, dim), unit_rows(rng, B, nt, dim)
        for b in range(B):
            for _ in range(nt // 3):
                t[b, rng.integers(nt)] = (q[b, rng.integers(nq)] + F32(0.05) * unit_rows(rng, dim)).astype(F32)
    q_xy, t_xy = positions(rng, B, nq, nt, variant)
    _plant_positions(rng, q_xy, t_xy)
    qc, tc, qv, tv = _sides(rng, B, nq, nt, qc, tc, flags)
    return dict(q=q, t=t, q_xy=q_xy, t_xy=t_xy, radius=radius, qc=qc, tc=tc, qv=qv, tv=tv)


# The random cases of tests/test_gpu_match_guided.py, as keyword sets of brief_case / nn_case;
# tests/test_match_guided_host.py proves on the reference alone that the gate decides each of them.
# K12: the 64-query workgroup and the 256-entry LDS tile with its 4-wave interleave, at their edges; NW 1, 2, 4, 8
# and the tail mask; a batch with different counts and flags; the position variants; the radii.
BRIEF_CASES = (
    [dict(nq=nq, nt=nt) for nq in (1, 63, 64, 65) for nt in (1, 255, 256, 257, 513)]
    + [dict(nq=65, nt=257, length=length) for length in (1, 33, 100)]
    + [dict(nq=70, nt=300, B=3, qc=[70, 0, 65], tc=[300, 5, 257], flags=True, length=length) for length in (256, 100)]
    + [dict(nq=65, nt=300, variant=v, radius=r) for v in ("int", "tenth", "far") for r in (0.0, 1.0, 8.0, (3.0, 11.0))]
)
# K13: both instances and zero padding; the wave's 16 rows and the workgroup's 64; both sides of TB (64 / 32);
# both regimes; a batch with different counts and flags; the position variants; the radii.
NN_CASES = (
    [dict(nq=nq, nt=65, dim=dim, regime=reg) for nq in (1, 16, 17, 64, 65) for dim, reg in ((128, "int"), (256, "round"))]
    + [dict(nq=17, nt=nt, dim=dim, regime=reg) for nt in (31, 32, 33, 64, 65, 129)
       for dim, reg in ((128, "round"), (256, "int"))]
    + [dict(nq=65, nt=129, dim=dim, regime="round") for dim in (4, 132)]
    + [dict(nq=70, nt=130, B=3, qc=[70, 41, 66], tc=[130, 99, 17], flags=True, dim=dim, regime=reg)
       for dim, reg in ((128, "int"), (256, "round"))]
    + [dict(nq=65, nt=129, dim=128, regime="int", variant=v, radius=r) for v in ("int", "tenth", "far")
       for r in (0.0, 1.0, 8.0, (3.0, 11.0))]
)


def case_id(kw):
    return "-".join(f"{k}{v}" for k, v in kw.items() if k not in ("qc", "tc")).replace(" ", "")
