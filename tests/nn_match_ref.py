"""Helper: a numpy restatement of fd_nn_match's contract (include/fd_hip.h), the yardstick of the float
matcher tests. Written unlike the kernel on purpose: distances come from an explicit k loop over
[Sq, St] arrays with an emulated fmaf, and every rule is a serial scan (the shape of match_ref._scan).

fmaf(a, b, c) for float32 is emulated exactly: a * b is exact in float64 (48 significant bits), the sum
with c is taken with TwoSum, the float64 sum is set to round-to-odd when the error term is non-zero, and
the cast to float32 then rounds once (round-to-odd keeps 53 >= 24 + 2 bits, so no double rounding).

The helper also restates the launch geometry of k_nn_match (feature_detector_amd/csrc/fd_nn_match.hip).
"""
import numpy as np

F32 = np.float32


def fmaf32(a, b, c):
    """float32 fmaf(a, b, c), elementwise, one rounding. Finite inputs."""
    a, b, c = (np.asarray(x, F32).astype(np.float64) for x in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b  # exact
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)  # exact: p + c = s + err
    s = np.array(s, np.float64, ndmin=1)
    bits = s.view(np.int64)
    fin = np.isfinite(s) & np.isfinite(err)
    need = fin & (err != 0) & ((bits & 1) == 0)
    away = (err > 0) == (s > 0)  # the exact value lies on the far side of s from zero
    bits += np.where(need, np.where(away, 1, -1), 0)
    with np.errstate(all="ignore"):
        out = s.astype(F32)
    return out.reshape(np.shape(p)) if np.ndim(p) else out[0]


def dot_chain(q, t):
    """[Sq, dim], [St, dim] float32 -> [Sq, St] float32: acc = 0; for k ascending: acc = fmaf(q[k], t[k], acc)."""
    q, t = np.asarray(q, F32), np.asarray(t, F32)
    acc = np.zeros((q.shape[0], t.shape[0]), F32)
    for k in range(q.shape[1]):
        acc = fmaf32(q[:, k, None], t[None, :, k], acc)
    return acc


def norm_chain(x):
    x = np.asarray(x, F32)
    acc = np.zeros((x.shape[0],), F32)
    for k in range(x.shape[1]):
        acc = fmaf32(x[:, k], x[:, k], acc)
    return acc


def preclamp(q, t):
    """(n(q) + n(t)) - 2 * dot(q, t) in float32, before the clamp at zero."""
    nq, nt, dot = norm_chain(q), norm_chain(t), dot_chain(q, t)
    with np.errstate(all="ignore"):
        return (nq[:, None] + nt[None, :]) - F32(2.0) * dot


def distances(q, t):
    """[Sq, St] float32 squared L2 in the contract's sequence."""
    return np.fmax(F32(0.0), preclamp(q, t)).astype(F32)


def _count(counts, b, stride):
    return stride if counts is None else min(int(np.uint32(np.int32(counts[b])) & np.uint32(0x01FFFFFF)), stride)


def scan(dist_row, cand):
    """Serial `<` scan over the candidate indices: (best index, best, second); None where absent."""
    best_i, best, second = -1, None, None
    for t in cand:
        d = dist_row[t]
        if best_i < 0:
            if d == d:  # (a NaN never wins)
                best_i, best = t, d
        elif d < best:
            best_i, best, second = t, d, best
        elif second is None or d < second:
            second = d
    return best_i, best, second


def accept_from_distances(D, q_ok, t_ok, max_distance=-1.0, max_ratio=0.0, cross_check=False):
    """The rules on a distance matrix D [nq, nt] (float32): per query row (idx, d1, d2), -1 where absent /
    rejected; rows not in q_ok get (-1, -1, -1)."""
    D = np.asarray(D, F32)
    nq = D.shape[0]
    back = {t: scan(D[:, t], q_ok)[0] for t in t_ok} if cross_check else {}
    q_set = set(q_ok)
    out = []
    for q in range(nq):
        if q not in q_set:
            out.append((-1, F32(-1), F32(-1)))
            continue
        t, d1, d2 = scan(D[q], t_ok)
        ok = t >= 0
        if ok and F32(max_distance) >= 0 and d1 > F32(max_distance):
            ok = False
        if ok and F32(max_ratio) > 0 and d2 is not None:
            r2 = F32(F32(max_ratio) * F32(max_ratio))
            if not (d1 < F32(r2 * d2)):
                ok = False
        if ok and cross_check and back[t] != q:
            ok = False
        out.append((t if ok else -1, F32(-1) if d1 is None else d1, F32(-1) if d2 is None else d2))
    return out


def nn_match_ref(q_desc, t_desc, q_counts=None, t_counts=None, q_valid=None, t_valid=None, max_distance=-1.0,
                 max_ratio=0.0, cross_check=False, fill=-1):
    """Returns (idx [B, Sq] int32, dist [B, Sq, 2] float32, counts [B] int32); slots >= q_counts[b] hold `fill`."""
    q_desc, t_desc = np.asarray(q_desc, F32), np.asarray(t_desc, F32)
    if q_desc.ndim == 2:
        q_desc, t_desc = q_desc[None], t_desc[None]
    B, Sq, St = q_desc.shape[0], q_desc.shape[1], t_desc.shape[1]
    idx = np.full((B, Sq), fill, np.int32)
    dist = np.full((B, Sq, 2), fill, F32)
    counts = np.zeros((B,), np.int32)
    for b in range(B):
        nq, nt = _count(q_counts, b, Sq), _count(t_counts, b, St)
        D = distances(q_desc[b, :nq], t_desc[b, :nt])
        q_ok = [q for q in range(nq) if q_valid is None or np.asarray(q_valid).reshape(B, Sq)[b, q]]
        t_ok = [t for t in range(nt) if t_valid is None or np.asarray(t_valid).reshape(B, St)[b, t]]
        rows = accept_from_distances(D, q_ok, t_ok, max_distance, max_ratio, cross_check)
        for q, (i, d1, d2) in enumerate(rows):
            idx[b, q], dist[b, q, 0], dist[b, q, 1] = i, d1, d2
            counts[b] += int(i >= 0)
    return idx, dist, counts


# ---- launch geometry of k_nn_match (launch_nn_match) ---------------------------------------------------
A_ROWS = 64  # "a" descriptors per workgroup: 4 waves of 16 rows


def instance(dim):
    """(K, TB): the descriptor length the instance pads dim to, and its "b" rows per LDS tile."""
    return (128, 64) if dim <= 128 else (256, 32)


def a_tiles(stride):
    """Workgroups per frame."""
    return (stride + A_ROWS - 1) // A_ROWS


def b_tiles(dim, count):
    """LDS tiles a workgroup walks for a frame of `count` searched descriptors."""
    tb = instance(dim)[1]
    return (count + tb - 1) // tb


def k_steps(dim):
    """(MFMA K steps that carry data, steps of the instance): the rest multiply zero padding."""
    return dim // 4, instance(dim)[0] // 4
