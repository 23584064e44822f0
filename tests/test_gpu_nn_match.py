"""GPU: the squared-L2 matcher for NN float descriptors (fd_nn_match / fd.nn_match) against
tests/nn_match_ref.py.

Bar: every output array equal to the numpy restatement (np.array_equal): accepted indices, both raw
distances as bit patterns (.view(np.uint32)), the per-frame counts, and the sentinel in every slot that
must not be written. The rounding-regime cases hold only if the f32-input MFMA is, bit for bit, a
k-ordered fmaf chain with one rounding per product, which is what the contract's distance is.
"""
import ctypes

import numpy as np
import pytest

import nn_match_ref as R
from nn_match_ref import nn_match_ref

pytestmark = pytest.mark.gpu

F32 = np.float32
SENT = -77  # prefill of the output slots that must not be written


@pytest.fixture(scope="module")
def fd():
    import feature_detector_amd as fd

    fd.load()
    return fd


def raw_match(fd, q, t, qc=None, tc=None, qv=None, tv=None, max_distance=-1.0, max_ratio=0.0, cross_check=0, fill=SENT,
              dim=None, strides=None, batch=None):
    """fd_nn_match through ctypes on host pointers, the outputs prefilled with `fill`."""
    from feature_detector_amd._lib import fd_nn_match_opts

    L = fd.load()
    ctx = fd.default_context()
    ctx.set_stream(None)
    B, Sq, St = q.shape[0], q.shape[1], t.shape[1]
    idx = np.full((B, Sq), fill, np.int32)
    dist = np.full((B, Sq, 2), fill, F32)
    cnt = np.full((B,), fill, np.int32)
    p = lambda x: None if x is None else ctypes.c_void_p(x.ctypes.data)  # noqa: E731
    opts = fd_nn_match_opts(q.shape[2] if dim is None else dim, max_distance, max_ratio, int(cross_check))
    sq, st = (Sq, St) if strides is None else strides
    rc = L.fd_nn_match(ctx.ptr, B if batch is None else batch, ctypes.byref(opts), p(q), p(qv), p(qc), sq, p(t), p(tv),
                       p(tc), st, p(idx), p(dist), p(cnt), 0)
    return rc, ctx, idx, dist, cnt


def assert_same(got, exp):
    for g, e, name in zip(got, exp, ("idx", "dist", "counts")):
        g = g.cpu().numpy() if hasattr(g, "cpu") else g
        if name == "dist":
            assert g.dtype == F32 and e.dtype == F32
            g, e = g.view(np.uint32), e.view(np.uint32)
        assert np.array_equal(g, e), name


def unit_rows(rng, *shape):
    """L2-normalised Gaussian rows (float32): what SuperPoint / DISK descriptors look like."""
    x = rng.standard_normal(shape)
    return (x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(F32)


def int_sets(rng, B, Sq, St, dim):
    """Integer-valued floats in -7..7 with planted duplicates: |dot| and the norms are <= 49 * 256 = 12544,
    far below 2^24, so every sum is exact in any order; exact ties and exact zero distances are common."""
    q = rng.integers(-7, 8, (B, Sq, dim)).astype(F32)
    t = rng.integers(-7, 8, (B, St, dim)).astype(F32)
    for b in range(B):
        for _ in range(Sq // 3):
            q[b, rng.integers(Sq)] = t[b, rng.integers(St)]  # zero distances, several queries on one train
        for _ in range(St // 4):
            t[b, rng.integers(St)] = t[b, rng.integers(St)]  # tied trains
    return q, t


OPTS_OFF = dict()
OPTS_ON = dict(max_distance=3000.0, max_ratio=0.95, cross_check=True)


@pytest.mark.parametrize("kw", [OPTS_OFF, OPTS_ON], ids=["off", "on"])
@pytest.mark.parametrize("dim", [256, 128])
def test_integer_regime(fd, kw, dim):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(100 + dim)
    B, Sq, St = 3, 70, 130
    q, t = int_sets(rng, B, Sq, St, dim)
    qc = np.array([70, 41, 66], np.int32)
    tc = np.array([130, 99, 17], np.int32)
    qv = (rng.random((B, Sq)) < 0.8).astype(np.uint8)
    tv = (rng.random((B, St)) < 0.8).astype(np.uint8)
    exp = nn_match_ref(q, t, qc, tc, qv, tv, fill=SENT, **kw)
    assert (exp[1][..., 0] == 0).sum() > 10 and (exp[1][..., 0] == exp[1][..., 1]).sum() > 10  # zeros and ties happen
    if kw:
        assert 0 < exp[2].sum() < (exp[1][..., 0] >= 0).sum()  # some accepted, some rejected
    # the raw C call on host pointers
    rc, _, idx, dist, cnt = raw_match(fd, q, t, qc, tc, qv, tv, **kw)
    assert rc == 0
    assert_same((idx, dist, cnt), exp)
    assert (idx[1, 41:] == SENT).all() and (dist[1, 41:] == SENT).all()
    # the binding on numpy arrays: unwritten slots hold -1
    m = fd.nn_match(q, t, qc, tc, qv, tv, **kw)
    assert_same((m.idx, m.dist, m.counts), nn_match_ref(q, t, qc, tc, qv, tv, fill=-1, **kw))
    # on torch device tensors, and with out= (the sentinel survives past the counts)
    dev = [torch.from_numpy(x).cuda() for x in (q, t, qc, tc, qv, tv)]
    m = fd.nn_match(dev[0], dev[1], dev[2], dev[3], dev[4], dev[5], **kw)
    torch.cuda.synchronize()
    assert m.dist.dtype == torch.float32
    assert_same((m.idx, m.dist, m.counts), nn_match_ref(q, t, qc, tc, qv, tv, fill=-1, **kw))
    out = (torch.full((B, Sq), SENT, dtype=torch.int32, device="cuda"),
           torch.full((B, Sq, 2), SENT, dtype=torch.float32, device="cuda"),
           torch.full((B,), SENT, dtype=torch.int32, device="cuda"))
    m = fd.nn_match(dev[0], dev[1], dev[2], dev[3], dev[4], dev[5], out=out, **kw)
    torch.cuda.synchronize()
    assert m.idx is out[0]
    assert_same(out, exp)


@pytest.mark.parametrize("scale", [1.0, 2.0 ** -6, 37.5])
@pytest.mark.parametrize("dim", [256, 128])
def test_rounding_regime(fd, scale, dim):
    """The float sequence itself: chain order, one rounding per product, the norm combine, the clamp. A
    kernel that splits K over accumulators, or sums in another order, fails here (and passes the integer
    regime)."""
    rng = np.random.default_rng(int(scale * 64) + dim)
    B, Sq, St = 3, 70, 130
    q = (unit_rows(rng, B, Sq, dim) * F32(scale)).astype(F32)
    t = (unit_rows(rng, B, St, dim) * F32(scale)).astype(F32)
    t[:, 20:50] = (q[:, 10:40] + F32(scale) * F32(0.05) * unit_rows(rng, B, 30, dim)).astype(F32)  # near matches
    qc = np.array([70, 70, 33], np.int32)
    qv = (rng.random((B, Sq)) < 0.9).astype(np.uint8)
    tv = (rng.random((B, St)) < 0.9).astype(np.uint8)
    for kw in (OPTS_OFF, dict(max_distance=float(F32(scale) * F32(scale)), max_ratio=0.9, cross_check=True)):
        exp = nn_match_ref(q, t, qc, None, qv, tv, fill=SENT, **kw)
        rc, _, idx, dist, cnt = raw_match(fd, q, t, qc, None, qv, tv, **kw)
        assert rc == 0
        g, e = dist.view(np.uint32).astype(np.int64), exp[1].view(np.uint32).astype(np.int64)
        print(f"dim {dim} scale {scale}: max ulp difference of the distances {np.abs(g - e).max()}, "
              f"idx mismatches {(idx != exp[0]).sum()}")
        assert_same((idx, dist, cnt), exp)
        if kw:
            assert 0 < exp[2].sum() < (exp[1][..., 0] >= 0).sum()


DIM_INSTANCE = {4: (128, 64), 8: (128, 64), 64: (128, 64), 124: (128, 64), 128: (128, 64), 132: (256, 32),
                252: (256, 32), 256: (256, 32)}


@pytest.mark.parametrize("dim", [4, 8, 64, 124, 128, 132, 252, 256])
def test_every_dim_class(fd, dim):
    """Both instances, zero padding in the first K step (4: one step of data) and the last (124, 252), one
    step past the small instance (132), and the DISK (128) and SuperPoint (256) widths."""
    assert R.instance(dim) == DIM_INSTANCE[dim]
    data, total = R.k_steps(dim)
    assert data == dim // 4 and total == DIM_INSTANCE[dim][0] // 4 and data <= total
    rng = np.random.default_rng(dim)
    B, Sq, St = 2, 70, 130
    q, t = unit_rows(rng, B, Sq, dim), unit_rows(rng, B, St, dim)
    t[:, 5:25] = (q[:, 30:50] + F32(0.1) * unit_rows(rng, B, 20, dim)).astype(F32)
    tv = (rng.random((B, St)) < 0.85).astype(np.uint8)
    kw = dict(max_ratio=0.9, cross_check=True)
    exp = nn_match_ref(q, t, None, np.array([130, 77], np.int32), None, tv, fill=SENT, **kw)
    rc, _, idx, dist, cnt = raw_match(fd, q, t, None, np.array([130, 77], np.int32), None, tv, **kw)
    assert rc == 0
    assert_same((idx, dist, cnt), exp)
    # the integer regime at this width too (placement, independent of rounding)
    q, t = int_sets(rng, B, Sq, St, dim)
    rc, _, idx, dist, cnt = raw_match(fd, q, t, cross_check=True)
    assert rc == 0
    assert_same((idx, dist, cnt), nn_match_ref(q, t, cross_check=True, fill=SENT))


@pytest.mark.parametrize("dim", [128, 256])
def test_tile_boundaries(fd, dim):
    """Query counts around the wave's 16 rows and the workgroup's 64; train counts around one and two LDS
    tiles of the instance; empty frames on either side inside a batch; a single train descriptor."""
    tb = R.instance(dim)[1]
    q_counts = [1, 15, 16, 17, 63, 0, 64, 65, 40, 40]
    t_counts = [tb - 1, tb, tb + 1, 2 * tb + 1, 5, 9, tb, tb + 1, 0, 1]
    Sq, St, B = 65, 2 * tb + 1, len(q_counts)
    assert R.a_tiles(Sq) == 2 and [R.a_tiles(max(n, 1)) for n in (63, 64, 65)] == [1, 1, 2]
    assert [R.b_tiles(dim, n) for n in t_counts] == [1, 1, 2, 3, 1, 1, 1, 2, 0, 1]
    rng = np.random.default_rng(7 + dim)
    q, t = unit_rows(rng, B, Sq, dim), unit_rows(rng, B, St, dim)
    t[:, :5] = q[:, :5]  # zero distances in the first tile, also for frames with few train entries
    t[:, St - 1] = q[:, 0]  # and a tie of the best in the last partial tile: the lower index keeps it
    qc, tc = np.array(q_counts, np.int32), np.array(t_counts, np.int32)
    for kw in (OPTS_OFF, dict(max_ratio=0.8, cross_check=True)):
        exp = nn_match_ref(q, t, qc, tc, fill=SENT, **kw)
        rc, _, idx, dist, cnt = raw_match(fd, q, t, qc, tc, **kw)
        assert rc == 0
        assert_same((idx, dist, cnt), exp)
        assert (idx[5] == SENT).all() and cnt[5] == 0  # q_count 0 in the middle of the batch
        assert (idx[8, :40] == -1).all() and (dist[8, :40] == -1).all() and cnt[8] == 0  # t_count 0: all absent
        # t_count 1: no second, the ratio test is skipped, every query takes train 0 (the cross-check keeps one)
        assert (dist[9, :40, 1] == -1).all() and (dist[9, :40, 0] >= 0).all()
        assert cnt[9] == (1 if kw else 40)
    # integer data through the same counts: ties across tiles in both directions
    q, t = int_sets(rng, B, Sq, St, dim)
    rc, _, idx, dist, cnt = raw_match(fd, q, t, qc, tc, cross_check=True)
    assert rc == 0
    assert_same((idx, dist, cnt), nn_match_ref(q, t, qc, tc, cross_check=True, fill=SENT))


def raw_match_dev(fd, torch, q, t, q_off=0, t_off=0, qc=None, tc=None, qv=None, tv=None, max_distance=-1.0, max_ratio=0.0,
                  cross_check=0):
    """fd_nn_match through ctypes on device pointers: the descriptor sets are views q_off / t_off floats into
    their allocations (unaligned.offset_view), the outputs lie between guards. Returns (idx, dist, counts)."""
    from feature_detector_amd._lib import fd_nn_match_opts
    from unaligned import guarded, offset_view, unguard

    L, ctx = fd.load(), fd.default_context()
    ctx.set_stream(torch.cuda.current_stream(ctx.device).cuda_stream)
    B, Sq, St = q.shape[0], q.shape[1], t.shape[1]
    (dq, keep_q), (dt, keep_t) = offset_view(torch, q, q_off), offset_view(torch, t, t_off)
    for d, off in ((dq, q_off), (dt, t_off)):
        assert (d.data_ptr() % 16 != 0) == (off != 0) and d.data_ptr() % 4 == 0
    side = [None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (qv, qc, tv, tc)]
    p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())  # noqa: E731
    shapes = ((B, Sq), (B, Sq, 2), (B,))
    bufs = [guarded(torch, s, SENT, dt_) for s, dt_ in zip(shapes, (torch.int32, torch.float32, torch.int32))]
    opts = fd_nn_match_opts(q.shape[2], max_distance, max_ratio, int(cross_check))
    rc = L.fd_nn_match(ctx.ptr, B, ctypes.byref(opts), p(dq), p(side[0]), p(side[1]), Sq, p(dt), p(side[2]), p(side[3]), St,
                       *(ctypes.c_void_p(ptr) for _, ptr in bufs), 1)
    assert rc == 0, L.fd_last_error(ctx.ptr)
    torch.cuda.synchronize()
    del keep_q, keep_t
    return tuple(unguard(buf, s, SENT) for (buf, _), s in zip(bufs, shapes))


UNALIGNED_COUNTS = dict(qc=np.array([70, 41], np.int32), tc=np.array([130, 77], np.int32))
_unaligned_cache = {}


def unaligned_case(dim, regime):
    """The data of test_every_dim_class (B 2, 70 queries, 130 train entries, counts 130 and 77: the last
    train tile of either instance is partial, also for the reverse pass over 70 and 41 queries), with the
    restatement's answer for the cross-check off and on. Computed once."""
    if (dim, regime) not in _unaligned_cache:
        rng = np.random.default_rng(1000 + dim + (regime == "int"))
        B, Sq, St = 2, 70, 130
        if regime == "int":
            q, t = int_sets(rng, B, Sq, St, dim)
        else:
            q, t = unit_rows(rng, B, Sq, dim), unit_rows(rng, B, St, dim)
            t[:, 5:25] = (q[:, 30:50] + F32(0.1) * unit_rows(rng, B, 20, dim)).astype(F32)
        tv = (rng.random((B, St)) < 0.85).astype(np.uint8)
        # the bare cross-check asks the reverse pass about every query's best, also the random pairs whose
        # mutual status turns on small differences of the reverse distances; with the ratio test only the
        # planted, clear matches get that far
        kws = (dict(), dict(cross_check=True), dict(max_ratio=0.9, cross_check=True))
        exp = [nn_match_ref(q, t, UNALIGNED_COUNTS["qc"], UNALIGNED_COUNTS["tc"], None, tv, fill=SENT, **kw) for kw in kws]
        assert exp[0][2].sum() > exp[1][2].sum() > exp[2][2].sum() > 0  # each test rejects some, keeps some
        _unaligned_cache[dim, regime] = (q, t, tv, kws, exp)
    return _unaligned_cache[dim, regime]


@pytest.mark.parametrize("q_off,t_off", [(1, 0), (0, 2), (3, 1)], ids=["query", "train", "both"])
@pytest.mark.parametrize("regime", ["int", "round"])
@pytest.mark.parametrize("dim", [4, 128, 256])
def test_unaligned_device_descriptors(fd, dim, regime, q_off, t_off):
    """Descriptor bases that are float-aligned but not 16-byte aligned (views into a larger allocation): the
    scalar load4 path of k_nn_norms and of k_nn_match's tile fill. With the cross-check the reverse pass
    searches the query set, so an offset on the query alone reaches the tile fill too. At dim 4 a row is 16
    bytes: every row is misaligned. Equal to the restatement and to the same call on aligned copies."""
    torch = pytest.importorskip("torch")
    q, t, tv, kws, exps = unaligned_case(dim, regime)
    tb = R.instance(dim)[1]
    assert all(int(n) % tb for n in UNALIGNED_COUNTS["tc"]) and all(int(n) % tb for n in UNALIGNED_COUNTS["qc"])
    for kw, exp in zip(kws, exps):
        got = raw_match_dev(fd, torch, q, t, q_off, t_off, tv=tv, **UNALIGNED_COUNTS, **kw)
        assert_same(got, exp)
        assert_same(raw_match_dev(fd, torch, q, t, 0, 0, tv=tv, **UNALIGNED_COUNTS, **kw), got)


@pytest.mark.parametrize("dim", [4, 128, 256])
def test_unaligned_views_through_the_binding(fd, dim):
    """fd.nn_match on sliced torch views: the views are contiguous, so the binding passes their offset
    pointers on as they are (Tensor.contiguous() returns a contiguous tensor itself, no copy)."""
    torch = pytest.importorskip("torch")
    from unaligned import offset_view

    q, t, tv, kws, exps = unaligned_case(dim, "round")
    (dq, keep_q), (dt, keep_t) = offset_view(torch, q, 1), offset_view(torch, t, 2)
    assert dq.data_ptr() % 16 == 4 and dt.data_ptr() % 16 == 8
    assert dq.contiguous().data_ptr() == dq.data_ptr() and dt.contiguous().data_ptr() == dt.data_ptr()
    side = [torch.from_numpy(x).cuda() for x in (UNALIGNED_COUNTS["qc"], UNALIGNED_COUNTS["tc"], tv)]
    for kw, exp in zip(kws, exps):
        out = (torch.full((2, 70), SENT, dtype=torch.int32, device="cuda"),
               torch.full((2, 70, 2), SENT, dtype=torch.float32, device="cuda"),
               torch.full((2,), SENT, dtype=torch.int32, device="cuda"))
        fd.nn_match(dq, dt, side[0], side[1], None, side[2], out=out, **kw)
        torch.cuda.synchronize()
        assert_same(out, exp)


def test_zero_strides(fd):
    z = unit_rows(np.random.default_rng(1), 2, 4, 8)
    # q_stride 0: no work, counts zeroed; t_stride 0: as all train counts 0
    rc, _, idx, dist, cnt = raw_match(fd, np.zeros((2, 0, 8), F32), z)
    assert rc == 0 and cnt.tolist() == [0, 0]
    for kw in (OPTS_OFF, OPTS_ON):
        rc, _, idx, dist, cnt = raw_match(fd, z, np.zeros((2, 0, 8), F32), **kw)
        assert rc == 0 and (idx == -1).all() and (dist == -1).all() and cnt.tolist() == [0, 0]


CLAMP_SEED = 3


def test_clamp_and_cancellation(fd):
    """Copies and near copies in the rounding regime. An exact copy has dot(q, t) = n(q) = n(t) (one and the
    same chain), so its distance is exactly +0.0 before the clamp; the pre-clamp value goes negative for
    near copies (every element moved by one ulp up or down: the true distance, ~1e-14, is far below the
    rounding noise of the three chains), which is where the clamp's +0.0 shows. Zero descriptors: a valid one matches at
    distance n(t); a flagged one is skipped on both sides."""
    dim, Sq, St = 256, 70, 130
    rng = np.random.default_rng(CLAMP_SEED)
    q, t = unit_rows(rng, 1, Sq, dim), unit_rows(rng, 1, St, dim)
    q[0, :20] = t[0, 40:60]  # exact copies
    near = t[0, 60:100]
    up = rng.random(near.shape) < 0.5
    q[0, 20:60] = np.where(up, np.nextafter(near, F32(np.inf)), np.nextafter(near, F32(-np.inf)))
    q[0, 60] = 0  # valid zero query
    q[0, 61] = 0  # flagged zero query
    t[0, 100] = 0  # flagged zero train
    t[0, 101] = 0  # valid zero train
    qv, tv = np.ones((1, Sq), np.uint8), np.ones((1, St), np.uint8)
    qv[0, 61] = 0
    tv[0, 100] = 0
    pre = R.preclamp(q[0], t[0])
    planted = pre[np.arange(20, 60), np.arange(60, 100)]
    assert (planted < 0).sum() >= 1, "choose another CLAMP_SEED"
    assert (pre[np.arange(20), np.arange(40, 60)] == 0).all()
    exp = nn_match_ref(q, t, None, None, qv, tv, fill=SENT)
    neg = 20 + np.flatnonzero(planted < 0)
    assert (exp[1][0, neg, 0].view(np.uint32) == 0).all() and (exp[0][0, neg] == 60 + neg - 20).all()  # +0.0, found
    assert exp[1][0, 60, 0] == R.norm_chain(t[0])[exp[0][0, 60]] and exp[0][0, 60] == 101  # n(zero train) = 0 wins
    assert exp[0][0, 61] == -1 and (exp[1][0, 61] == -1).all()
    assert not (exp[0][0] == 100).any()
    for kw in (OPTS_OFF, dict(cross_check=True)):
        rc, _, idx, dist, cnt = raw_match(fd, q, t, None, None, qv, tv, **kw)
        assert rc == 0
        assert_same((idx, dist, cnt), nn_match_ref(q, t, None, None, qv, tv, fill=SENT, **kw))
    # without the zero train row the zero query's distance is the smallest n(t)
    tv[0, 101] = 0
    rc, _, idx, dist, cnt = raw_match(fd, q, t, None, None, qv, tv)
    nt = R.norm_chain(t[0])
    cand = [i for i in range(St) if tv[0, i]]
    assert dist[0, 60, 0] == min(nt[i] for i in cand) and dist[0, 60, 0] > 0.9
    assert_same((idx, dist, cnt), nn_match_ref(q, t, None, None, qv, tv, fill=SENT))


def test_acceptance_on_the_reported_floats(fd):
    dim, Sq, St = 128, 40, 90
    rng = np.random.default_rng(21)
    q, t = unit_rows(rng, 1, Sq, dim), unit_rows(rng, 1, St, dim)
    t[0, 10:30] = (q[0, 5:25] + F32(0.2) * unit_rows(rng, 20, dim)).astype(F32)
    base = nn_match_ref(q, t)
    # max_distance equal to a reported d1 accepts it; one ulp below rejects it
    d1 = base[1][0, 7, 0]
    assert d1 > 0 and base[0][0, 7] == 12
    for bound, hit in ((d1, 12), (np.nextafter(d1, F32(-1)), -1)):
        rc, _, idx, dist, cnt = raw_match(fd, q, t, max_distance=float(bound), fill=-1)
        assert rc == 0 and idx[0, 7] == hit
        assert_same((idx, dist, cnt), nn_match_ref(q, t, max_distance=float(bound)))
    # d2 exactly d1 (a duplicated train row): rejected by every ratio <= 1, the lower index reported as raw best
    t2 = t.copy()
    t2[0, 70] = t2[0, 12]
    for ratio in (1.0, 0.999, 0.5):
        rc, _, idx, dist, cnt = raw_match(fd, q, t2, max_ratio=ratio, fill=-1)
        assert rc == 0 and idx[0, 7] == -1 and dist[0, 7, 0].view(np.uint32) == dist[0, 7, 1].view(np.uint32) == d1.view(np.uint32)
        assert_same((idx, dist, cnt), nn_match_ref(q, t2, max_ratio=ratio))
    rc, _, idx, dist, cnt = raw_match(fd, q, t2, fill=-1)
    assert idx[0, 7] == 12
    # cross-check: two identical queries share one best train; only the lower query index survives the tie
    q2 = q.copy()
    q2[0, 33] = q2[0, 7]
    rc, _, idx, dist, cnt = raw_match(fd, q2, t, cross_check=True, fill=-1)
    assert rc == 0 and idx[0, 7] == 12 and idx[0, 33] == -1 and dist[0, 33, 0].view(np.uint32) == d1.view(np.uint32)
    assert_same((idx, dist, cnt), nn_match_ref(q2, t, cross_check=True))


def _detector_descriptors(torch, seed=4):
    """nn_descriptors of a seeded map at seeded keypoints, on the device: [B, S, 256], counts [B]."""
    from feature_detector_amd.superpoint import nn_descriptors

    g = torch.Generator().manual_seed(seed)
    B, C, h, w, S = 4, 256, 12, 16, 60
    dmap = torch.nn.functional.normalize(torch.randn((1, C, h, w), generator=g), dim=1).repeat(B, 1, 1, 1).cuda()
    xy = torch.rand((B, S, 2), generator=g) * torch.tensor([8.0 * w - 1, 8.0 * h - 1])
    # one scene: consecutive frames see mostly the same keypoints, moved a little
    for b in range(1, B):
        xy[b, :40] = xy[b - 1, 10:50] + 0.5 * torch.rand((40, 2), generator=g)
    xy = xy.clamp(min=0).cuda()
    counts = torch.tensor([60, 51, 0, 60], dtype=torch.int32, device="cuda")
    return nn_descriptors(dmap, xy, counts), counts


def test_chain_from_the_detector(fd):
    """nn_descriptors output fed straight in on the device, counts as the device tensor, frame i against
    frame i + 1 by pointer advance (batch - 1)."""
    torch = pytest.importorskip("torch")
    desc, counts = _detector_descriptors(torch)
    kw = dict(max_ratio=0.95, cross_check=True)
    m = fd.nn_match(desc[:-1], desc[1:], counts[:-1], counts[1:], **kw)
    torch.cuda.synchronize()
    d, c = desc.cpu().numpy(), counts.cpu().numpy()
    exp = nn_match_ref(d[:-1], d[1:], c[:-1], c[1:], **kw)
    assert_same((m.idx, m.dist, m.counts), exp)
    assert int(m.counts[0]) >= 1 and m.counts.tolist()[1:] == [0, 0]


def test_graph_capture(fd):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(13)
    B, Sq, St, dim = 2, 90, 140, 256
    q = torch.zeros((B, Sq, dim), dtype=torch.float32, device="cuda")
    t = torch.zeros((B, St, dim), dtype=torch.float32, device="cuda")
    qv = torch.ones((B, Sq), dtype=torch.uint8, device="cuda")
    qc = torch.tensor([90, 77], dtype=torch.int32, device="cuda")
    out = (torch.empty((B, Sq), dtype=torch.int32, device="cuda"), torch.empty((B, Sq, 2), dtype=torch.float32, device="cuda"),
           torch.empty((B,), dtype=torch.int32, device="cuda"))
    kw = dict(max_distance=1.9, max_ratio=0.98, cross_check=True)
    fd.nn_match(q, t, qc, None, qv, None, out=out, **kw)  # sizes the workspace
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        fd.nn_match(q, t, qc, None, qv, None, out=out, **kw)
    for seed in range(2):  # new contents in the same tensors
        hq, ht = unit_rows(rng, B, Sq, dim), unit_rows(rng, B, St, dim)
        hv = (rng.random((B, Sq)) < 0.8).astype(np.uint8)
        q.copy_(torch.from_numpy(hq))
        t.copy_(torch.from_numpy(ht))
        qv.copy_(torch.from_numpy(hv))
        for o in out:
            o.fill_(SENT)
        g.replay()
        torch.cuda.synchronize()
        replayed = [o.cpu().numpy().copy() for o in out]
        assert_same(replayed, nn_match_ref(hq, ht, np.array([90, 77]), None, hv, None, fill=SENT, **kw))
        for o in out:
            o.fill_(SENT)
        fd.nn_match(q, t, qc, None, qv, None, out=out, **kw)  # the eager call gives the same
        torch.cuda.synchronize()
        assert_same(out, replayed)
    del g


def test_bad_arguments(fd):
    from feature_detector_amd import _lib

    z = np.zeros((1, 4, 8), F32)
    for dim in (0, 2, 6, 260):
        rc, ctx, *_ = raw_match(fd, np.zeros((1, 4, 264), F32), np.zeros((1, 4, 264), F32), dim=dim)
        assert rc == _lib.FD_ERR_INVALID, dim
        with pytest.raises(fd.FdError):
            _lib.check(ctx.ptr, rc)
    for strides in ((-1, 4), (4, -1)):
        assert raw_match(fd, z, z, strides=strides)[0] == _lib.FD_ERR_INVALID
    assert raw_match(fd, z, z, batch=0)[0] == _lib.FD_ERR_INVALID
    for bad in (float("nan"), float("inf"), float("-inf")):
        assert raw_match(fd, z, z, max_ratio=bad)[0] == _lib.FD_ERR_INVALID
        assert raw_match(fd, z, z, max_distance=bad)[0] == _lib.FD_ERR_INVALID
    for kw in ({"max_ratio": float("nan")}, {"max_distance": float("inf")}):
        with pytest.raises(fd.FdError):
            fd.nn_match(z, z, **kw)
    with pytest.raises(fd.FdError):
        fd.nn_match(np.zeros((1, 4, 6), F32), np.zeros((1, 4, 6), F32))
    # NULL pointers
    L, ctx = fd.load(), fd.default_context()
    opts = _lib.fd_nn_match_opts(8, -1.0, 0.0, 0)
    idx = np.zeros((1, 4), np.int32)
    p = lambda x: ctypes.c_void_p(x.ctypes.data)  # noqa: E731
    good = [ctx.ptr, 1, ctypes.byref(opts), p(z), None, None, 4, p(z), None, None, 4, p(idx), None, None, 0]
    assert L.fd_nn_match(*good) == 0
    for slot in (0, 2, 3, 7, 11):
        args = list(good)
        args[slot] = None
        assert L.fd_nn_match(*args) == _lib.FD_ERR_INVALID, slot
