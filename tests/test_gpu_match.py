"""GPU: the Hamming matcher (fd_brief_match / fd.brief_match) against tests/match_ref.py.

Bar: every output array equal to the numpy restatement (np.array_equal): accepted indices, both raw
distances, the per-frame counts, and the sentinel in every slot past a frame's query count.
"""
import ctypes

import numpy as np
import pytest

from match_ref import match_ref

pytestmark = pytest.mark.gpu

SENT = -77  # prefill of the output slots that must not be written


@pytest.fixture(scope="module")
def fd():
    import feature_detector_amd as fd

    fd.load()
    return fd


def rand_words(rng, *shape):
    return rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)


def flip(desc, bits):
    """A copy of the descriptor words with the given bit positions inverted."""
    d = desc.copy()
    for i in bits:
        d[i // 32] ^= np.uint32(1 << (i % 32))
    return d


def raw_match(fd, q, t, qc, tc, qv, tv, length, max_distance=-1, max_ratio=0.0, cross_check=0, fill=SENT):
    """fd_brief_match through ctypes on host pointers, the outputs prefilled with `fill`."""
    from feature_detector_amd._lib import fd_match_opts

    L = fd.load()
    ctx = fd.default_context()
    ctx.set_stream(None)
    B, Sq, St = q.shape[0], q.shape[1], t.shape[1]
    idx = np.full((B, Sq), fill, np.int32)
    dist = np.full((B, Sq, 2), fill, np.int32)
    cnt = np.full((B,), fill, np.int32)
    p = lambda x: None if x is None else ctypes.c_void_p(x.ctypes.data)  # noqa: E731
    opts = fd_match_opts(length, max_distance, max_ratio, cross_check)
    rc = L.fd_brief_match(ctx.ptr, B, ctypes.byref(opts), p(q), p(qv), p(qc), Sq, p(t), p(tv), p(tc), St, p(idx), p(dist),
                          p(cnt), 0)
    return rc, ctx, idx, dist, cnt


def assert_same(got, exp):
    for g, e, name in zip(got, exp, ("idx", "dist", "counts")):
        g = g.cpu().numpy() if hasattr(g, "cpu") else g
        assert np.array_equal(g, e), name


def kernel_words(length):
    """(nw, NW): a descriptor's words (the row pitch of the bit arrays) and the words per lane and LDS row of the
    kernel instance launch_brief_match takes for it (1, 2, 4 or 8)."""
    nw = (length + 31) // 32
    return nw, 1 if nw <= 1 else 2 if nw <= 2 else 4 if nw <= 4 else 8


# every nw in 1..8; 65, 96 (nw 3 in NW 4) and 129 .. 224 (nw 5, 6, 7 in NW 8): the row pitch differs from the
# LDS pitch, and the tail mask (none at 96, 160, 192, 224) sits in a word other than the last register
WORDS = {1: (1, 1), 31: (1, 1), 32: (1, 1), 33: (2, 2), 65: (3, 4), 96: (3, 4), 97: (4, 4), 100: (4, 4), 129: (5, 8),
         160: (5, 8), 161: (6, 8), 192: (6, 8), 224: (7, 8), 255: (8, 8), 256: (8, 8)}


@pytest.mark.parametrize("length", [256, 1, 31, 32, 33, 100, 255, 65, 96, 97, 129, 160, 161, 192, 224])
def test_random_counts_and_unwritten_slots(fd, length):
    """Random words (so the bits above `length` in the last word are garbage on both sides), counts that
    cut the frames, random valid flags; the raw C call on host pointers, then fd.brief_match."""
    rng = np.random.default_rng(1000 + length)
    assert kernel_words(length) == WORDS[length]
    nw = (length + 31) // 32
    q, t = rand_words(rng, 3, 70, nw), rand_words(rng, 3, 130, nw)
    qc, tc = np.array([70, 0, 65], np.int32), np.array([130, 5, 1], np.int32)
    qv = (rng.random((3, 70)) < 0.8).astype(np.uint8)
    tv = (rng.random((3, 130)) < 0.8).astype(np.uint8)
    tv[2, 0] = 1
    for kw in ({}, dict(max_distance=int(0.45 * length), max_ratio=0.97, cross_check=True)):
        exp = match_ref(q, t, qc, tc, qv, tv, length, fill=SENT, **kw)
        rc, _, idx, dist, cnt = raw_match(fd, q, t, qc, tc, qv, tv, length, kw.get("max_distance", -1),
                                          kw.get("max_ratio", 0.0), int(kw.get("cross_check", False)))
        assert rc == 0
        assert_same((idx, dist, cnt), exp)
        assert (idx[1] == SENT).all() and (dist[2, 65:] == SENT).all() and (idx[2, 65:] == SENT).all()
        res = fd.brief_match(q, t, qc, tc, qv, tv, length=length, **kw)
        assert_same((res.idx, res.dist, res.counts), match_ref(q, t, qc, tc, qv, tv, length, **kw))
    # without flags and counts: everything valid, `stride` entries each; [S, words] is batch 1
    res = fd.brief_match(q[0].view(np.int32), t[0].view(np.int32), length=length)
    assert_same((res.idx, res.dist, res.counts), match_ref(q[:1], t[:1], length=length))


def test_ties_lowest_index_wins(fd):
    rng = np.random.default_rng(7)
    q, t = rand_words(rng, 1, 6, 8), rand_words(rng, 1, 300, 8)
    # q0: exact duplicates at 9 and 270 (another wave's share of another tile), an equidistant entry at 131
    t[0, 9] = t[0, 270] = flip(q[0, 0], [0, 40, 200])
    t[0, 131] = flip(q[0, 0], [1, 2, 3])
    # q1: duplicates of itself at 299 and 4; q2: equidistant entries in one tile, adjacent
    t[0, 299] = t[0, 4] = q[0, 1]
    t[0, 17] = flip(q[0, 2], [255])
    t[0, 16] = flip(q[0, 2], [0])
    res = fd.brief_match(q, t)
    assert res.idx[0, :3].tolist() == [9, 4, 16]
    assert res.dist[0, :3].tolist() == [[3, 3], [0, 0], [1, 1]]
    assert_same((res.idx, res.dist, res.counts), match_ref(q, t))
    # a short descriptor: almost every distance is tied many times over, in both directions
    q, t = rand_words(rng, 2, 200, 1), rand_words(rng, 2, 300, 1)
    res = fd.brief_match(q, t, length=5, cross_check=True)
    exp = match_ref(q, t, length=5, cross_check=True)
    assert (exp[1][..., 0] == exp[1][..., 1]).all()
    assert_same((res.idx, res.dist, res.counts), exp)


def test_validity(fd):
    rng = np.random.default_rng(8)
    q, t = rand_words(rng, 4, 5, 8), rand_words(rng, 4, 6, 8)
    qv, tv = np.ones((4, 5), np.uint8), np.ones((4, 6), np.uint8)
    # frame 0: t0 equals q0 but is invalid (the nearest is skipped); q3 invalid; all-zero invalid pair
    t[0, 0] = q[0, 0]
    t[0, 3] = flip(q[0, 0], range(20))
    tv[0, 0] = 0
    qv[0, 3] = 0
    q[0, 4] = t[0, 5] = 0
    qv[0, 4] = tv[0, 5] = 0
    tv[1] = 0                                  # frame 1: an all-invalid train set
    tc = np.array([6, 6, 0, 1], np.int32)      # frame 2: no train descriptor; frame 3: exactly one
    res = fd.brief_match(q, t, None, tc, qv, tv, max_ratio=0.5)
    assert res.idx[0].tolist()[0] == 3 and res.dist[0, 0, 0] == 20
    assert res.idx[0, 3:].tolist() == [-1, -1] and (res.dist[0, 3:] == -1).all()
    assert (res.idx[1:3] == -1).all() and (res.dist[1:3] == -1).all() and res.counts[1:3].tolist() == [0, 0]
    # one candidate: the second is absent and the ratio test is skipped, so every query is accepted
    assert (res.idx[3] == 0).all() and (res.dist[3, :, 1] == -1).all() and (res.dist[3, :, 0] >= 0).all()
    assert res.counts[3] == 5
    assert_same((res.idx, res.dist, res.counts), match_ref(q, t, None, tc, qv, tv, max_ratio=0.5))


@pytest.fixture(scope="module")
def proto_sets():
    """Descriptors from prototype words with controlled bit flips (random prototypes differ in ~128 +- 8
    bits, far above every distance built here). Query i, its best and second distance:
      0: 8, 16 (8 == 0.5 * 16 exactly)   1: 4, 16   2: 30, 100   3: 10, 12
      4, 5: both 5 bits from train 8 (equidistant: query 4 keeps it)
      6, 7: 6 and 2 bits from train 9 (query 7 keeps it)"""
    rng = np.random.default_rng(9)
    P = rand_words(rng, 6, 8)
    q = np.stack([P[0], P[1], P[2], P[3], flip(P[4], range(5)), flip(P[4], range(5, 10)), flip(P[5], range(6)),
                  flip(P[5], range(100, 102))])[None]
    t = np.stack([flip(P[0], range(8)), flip(P[0], range(8, 24)), flip(P[1], range(4)), flip(P[1], range(4, 20)),
                  flip(P[2], range(30)), flip(P[2], range(30, 130)), flip(P[3], range(10)), flip(P[3], range(10, 22)),
                  P[4], P[5]])[None]
    return q, t


@pytest.mark.parametrize("kw,accepted", [
    (dict(), [0, 2, 4, 6, 8, 8, 9, 9]),
    (dict(max_distance=20), [0, 2, -1, 6, 8, 8, 9, 9]),
    (dict(max_ratio=0.5), [-1, 2, 4, -1, 8, 8, 9, 9]),
    (dict(cross_check=True), [0, 2, 4, 6, 8, -1, -1, 9]),
    (dict(max_distance=20, max_ratio=0.5, cross_check=True), [-1, 2, -1, -1, 8, -1, -1, 9]),
])
def test_acceptance_tests(fd, proto_sets, kw, accepted):
    q, t = proto_sets
    res = fd.brief_match(q, t, **kw)
    assert res.idx[0].tolist() == accepted
    assert res.dist[0, :4].tolist() == [[8, 16], [4, 16], [30, 100], [10, 12]]  # raw, whatever is accepted
    assert res.counts.tolist() == [sum(a >= 0 for a in accepted)]
    assert_same((res.idx, res.dist, res.counts), match_ref(q, t, **kw))


@pytest.mark.parametrize("length", [256, 12, 70, 200])
@pytest.mark.parametrize("nq,nt", [(63, 65), (64, 64), (65, 63), (255, 257), (256, 256), (257, 255), (1025, 1025)])
def test_tile_edges(fd, nq, nt, length):
    """Counts around the query tile (64), the LDS train tile (256) and several tiles; 12-bit descriptors
    tie constantly, so the tie rule is exercised across waves and tiles, in both directions."""
    rng = np.random.default_rng(nq * 7 + nt + length)
    nw = (length + 31) // 32
    assert kernel_words(length) == {256: (8, 8), 12: (1, 1), 70: (3, 4), 200: (7, 8)}[length]
    q, t = rand_words(rng, 1, nq, nw), rand_words(rng, 1, nt, nw)
    qv, tv = (rng.random((1, nq)) < 0.9).astype(np.uint8), (rng.random((1, nt)) < 0.9).astype(np.uint8)
    kw = dict(length=length, cross_check=True, max_ratio=0.99)
    res = fd.brief_match(q, t, q_valid=qv, t_valid=tv, **kw)
    assert_same((res.idx, res.dist, res.counts), match_ref(q, t, q_valid=qv, t_valid=tv, **kw))


def test_batch_with_different_counts(fd):
    rng = np.random.default_rng(12)
    q, t = rand_words(rng, 2, 300, 8), rand_words(rng, 2, 300, 8)
    qc, tc = np.array([257, 64], np.int32), np.array([65, 256], np.int32)
    rc, _, idx, dist, cnt = raw_match(fd, q, t, qc, tc, None, None, 256, cross_check=1)
    assert rc == 0
    assert_same((idx, dist, cnt), match_ref(q, t, qc, tc, cross_check=True, fill=SENT))


def test_device_chain(fd, image_png):
    """detect -> describe -> match on device tensors: detect's device counts and BRIEF's device valid
    flags are read in place; frame 0 against frame 1 (the same image shifted by 3 rows, 5 columns)."""
    torch = pytest.importorskip("torch")
    host = np.stack([image_png, np.roll(image_png, (3, 5), (0, 1))])
    dev = torch.from_numpy(host).cuda()
    res = fd.detect_points("harris", dev, 200, 15, 30.0)
    bits, valid = fd.brief_compute(dev, res.xy, res.counts, with_valid=True)
    m = fd.brief_match(bits[0:1], bits[1:2], res.counts[0:1], res.counts[1:2], valid[0:1], valid[1:2],
                       cross_check=True, max_distance=64)
    torch.cuda.synchronize()
    b, v, c = bits.cpu().numpy(), valid.cpu().numpy(), res.counts.cpu().numpy()
    exp = match_ref(b[0:1], b[1:2], c[0:1], c[1:2], v[0:1], v[1:2], cross_check=True, max_distance=64)
    assert_same((m.idx, m.dist, m.counts), exp)
    assert int(m.counts[0]) >= 1


def test_graph_capture(fd):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(13)
    B, Sq, St = 2, 90, 140
    q = torch.zeros((B, Sq, 8), dtype=torch.int32, device="cuda")
    t = torch.zeros((B, St, 8), dtype=torch.int32, device="cuda")
    qv = torch.ones((B, Sq), dtype=torch.uint8, device="cuda")
    qc = torch.tensor([90, 77], dtype=torch.int32, device="cuda")
    out = (torch.empty((B, Sq), dtype=torch.int32, device="cuda"), torch.empty((B, Sq, 2), dtype=torch.int32, device="cuda"),
           torch.empty((B,), dtype=torch.int32, device="cuda"))
    kw = dict(max_distance=120, max_ratio=0.98, cross_check=True)
    fd.brief_match(q, t, qc, None, qv, None, out=out, **kw)  # sizes the workspace
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        fd.brief_match(q, t, qc, None, qv, None, out=out, **kw)
    for seed in range(2):  # new contents in the same tensors
        hq, ht = rand_words(rng, B, Sq, 8), rand_words(rng, B, St, 8)
        hv = (rng.random((B, Sq)) < 0.8).astype(np.uint8)
        q.copy_(torch.from_numpy(hq.view(np.int32)))
        t.copy_(torch.from_numpy(ht.view(np.int32)))
        qv.copy_(torch.from_numpy(hv))
        for o in out:
            o.fill_(SENT)
        g.replay()
        torch.cuda.synchronize()
        assert_same(out, match_ref(hq, ht, np.array([90, 77]), None, hv, None, fill=SENT, **kw))
    del g


def test_bad_arguments(fd):
    from feature_detector_amd import _lib

    z = np.zeros((1, 4, 8), np.uint32)
    for kw in ({"length": 0}, {"length": 257}, {"max_ratio": float("nan")}):
        with pytest.raises(fd.FdError):
            fd.brief_match(z, z, **kw)
    for sq, st in ((-1, 4), (4, -1)):
        from feature_detector_amd._lib import fd_match_opts

        ctx = fd.default_context()
        idx = np.zeros((1, 4), np.int32)
        opts = fd_match_opts(256, -1, 0.0, 0)
        rc = fd.load().fd_brief_match(ctx.ptr, 1, ctypes.byref(opts), ctypes.c_void_p(z.ctypes.data), None, None, sq,
                                      ctypes.c_void_p(z.ctypes.data), None, None, st, ctypes.c_void_p(idx.ctypes.data),
                                      None, None, 0)
        with pytest.raises(fd.FdError):
            _lib.check(ctx.ptr, rc)
    # q_stride 0: no work, counts zeroed; t_stride 0: as all train counts 0
    rc, _, idx, dist, cnt = raw_match(fd, np.zeros((2, 0, 8), np.uint32), z.repeat(2, 0), None, None, None, None, 256)
    assert rc == 0 and cnt.tolist() == [0, 0]
    rc, _, idx, dist, cnt = raw_match(fd, z, np.zeros((1, 0, 8), np.uint32), None, None, None, None, 256)
    assert rc == 0 and (idx == -1).all() and (dist == -1).all() and cnt.tolist() == [0]
