"""Helper: a numpy restatement of fd_brief_match's semantics (include/fd_hip.h), the yardstick of the
matcher tests. Written differently from the kernel on purpose: descriptors are unpacked to bool arrays
(bits 0..length-1 only), distances are mismatch counts, and every rule is a serial scan."""
import numpy as np


def _bools(words, length):
    """[S, words] int32 / uint32 -> [S, length] bool, bit i = bit i % 32 of word i // 32."""
    w = np.ascontiguousarray(words).view(np.uint32).astype(np.uint64)
    i = np.arange(length)
    return ((w[:, i // 32] >> (i % 32).astype(np.uint64)) & 1).astype(bool)


def _count(counts, b, stride):
    return stride if counts is None else min(int(np.uint32(np.int32(counts[b])) & np.uint32(0x01FFFFFF)), stride)


def _scan(dist_row, cand):
    """Serial `<` scan over the candidate indices: (best index, best, second); -1 where absent."""
    best_i, best, second = -1, -1, -1
    for t, d in zip(cand, dist_row[cand].tolist() if len(cand) else []):
        if best_i < 0:
            best_i, best = t, d
        elif d < best:
            best_i, best, second = t, d, best
        elif second < 0 or d < second:
            second = d
    return best_i, best, second


def match_ref(q_bits, t_bits, q_counts=None, t_counts=None, q_valid=None, t_valid=None, length=256, max_distance=-1,
              max_ratio=0.0, cross_check=False, fill=-1):
    """Returns (idx [B, Sq], dist [B, Sq, 2], counts [B]) int32; slots >= q_counts[b] hold `fill`."""
    q_bits, t_bits = np.asarray(q_bits), np.asarray(t_bits)
    if q_bits.ndim == 2:
        q_bits, t_bits = q_bits[None], t_bits[None]
    B, Sq, St = q_bits.shape[0], q_bits.shape[1], t_bits.shape[1]
    idx = np.full((B, Sq), fill, np.int32)
    dist = np.full((B, Sq, 2), fill, np.int32)
    counts = np.zeros((B,), np.int32)
    for b in range(B):
        nq, nt = _count(q_counts, b, Sq), _count(t_counts, b, St)
        qb, tb = _bools(q_bits[b, :nq], length), _bools(t_bits[b, :nt], length)
        # mismatches = (q set, t clear) + (q clear, t set); sums of at most 256 ones are exact in float32
        qf, tf = qb.astype(np.float32), tb.astype(np.float32)
        D = (qf @ (1 - tf).T + (1 - qf) @ tf.T).astype(np.int64)
        q_ok = [q for q in range(nq) if q_valid is None or np.asarray(q_valid).reshape(B, Sq)[b, q]]
        t_ok = [t for t in range(nt) if t_valid is None or np.asarray(t_valid).reshape(B, St)[b, t]]
        # every valid train descriptor's best query (cross-check)
        back = {t: _scan(D[:, t], q_ok)[0] for t in t_ok} if cross_check else {}
        q_set = set(q_ok)
        for q in range(nq):
            if q not in q_set:
                idx[b, q], dist[b, q] = -1, (-1, -1)
                continue
            t, d1, d2 = _scan(D[q], t_ok)
            dist[b, q] = (d1, d2)
            ok = t >= 0
            if ok and max_distance >= 0 and d1 > max_distance:
                ok = False
            if ok and max_ratio > 0 and d2 >= 0 and not (np.float32(d1) < np.float32(max_ratio) * np.float32(d2)):
                ok = False
            if ok and cross_check and back[t] != q:
                ok = False
            idx[b, q] = t if ok else -1
            counts[b] += int(ok)
    return idx, dist, counts
