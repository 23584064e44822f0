"""GPU: guided (position-gated) matching, fd_brief_match_guided (K12) and fd_nn_match_guided (K13), against
tests/match_guided_ref.py.

Bar: every output array equal to the numpy restatement (np.array_equal): accepted indices, both raw
distances (the float ones as bit patterns), the per-frame counts, and the sentinel in every slot that must
not be written. The random fixtures are match_guided_ref.BRIEF_CASES / NN_CASES;
tests/test_match_guided_host.py proves that the gate changes most answers on each of them.
"""
import ctypes

import numpy as np
import pytest

import match_guided_ref as G
from match_guided_ref import match_guided_ref, nn_match_guided_ref
from match_ref import match_ref
from nn_match_ref import nn_match_ref

pytestmark = pytest.mark.gpu

F32 = np.float32
SENT = -77  # prefill of the output slots that must not be written
HUGE = 3.0e38
KINDS = ("brief", "nn")


@pytest.fixture(scope="module")
def fd():
    import feature_detector_amd as fd

    fd.load()
    return fd


def raw_guided(fd, kind, c, radius=None, max_distance=-1, max_ratio=0.0, cross_check=False, fill=SENT, **over):
    """The guided entry through ctypes on host pointers, the outputs prefilled with `fill`. `over` replaces
    positional arguments by name (gate, q, q_xy, t, t_xy, idx, batch, sq, st)."""
    from feature_detector_amd import _lib

    L = fd.load()
    ctx = fd.default_context()
    ctx.set_stream(None)
    q, t = c["q"], c["t"]
    B, Sq, St = q.shape[0], q.shape[1], t.shape[1]
    idx = np.full((B, Sq), fill, np.int32)
    dist = np.full((B, Sq, 2), fill, np.int32 if kind == "brief" else F32)
    cnt = np.full((B,), fill, np.int32)
    p = lambda x: None if x is None else ctypes.c_void_p(x.ctypes.data)  # noqa: E731
    rx, ry = G.radii(c["radius"] if radius is None else radius)
    gate = _lib.fd_match_gate(rx, ry)
    if kind == "brief":
        opts, fn = _lib.fd_match_opts(c["length"], int(max_distance), max_ratio, int(cross_check)), L.fd_brief_match_guided
    else:
        opts, fn = _lib.fd_nn_match_opts(q.shape[2], max_distance, max_ratio, int(cross_check)), L.fd_nn_match_guided
    a = dict(gate=ctypes.byref(gate), q=p(q), q_xy=p(c["q_xy"]), t=p(t), t_xy=p(c["t_xy"]), idx=p(idx), batch=B, sq=Sq, st=St,
             opts=ctypes.byref(opts))
    a.update(over)
    rc = fn(ctx.ptr, a["batch"], a["opts"], a["gate"], a["q"], p(c["qv"]), p(c["qc"]), a["sq"], a["q_xy"], a["t"], p(c["tv"]),
            p(c["tc"]), a["st"], a["t_xy"], a["idx"], p(dist), p(cnt), 0)
    return rc, idx, dist, cnt


def ref(kind, c, radius=None, fill=-1, **kw):
    r = c["radius"] if radius is None else radius
    if kind == "brief":
        return match_guided_ref(c["q"], c["t"], c["q_xy"], c["t_xy"], r, c["qc"], c["tc"], c["qv"], c["tv"],
                                length=c["length"], fill=fill, **kw)
    return nn_match_guided_ref(c["q"], c["t"], c["q_xy"], c["t_xy"], r, c["qc"], c["tc"], c["qv"], c["tv"], fill=fill, **kw)


def bound(fd, kind, c, radius=None, **kw):
    """fd.brief_match / fd.nn_match with the guided keywords, on the case's arrays (or tensors)."""
    r = c["radius"] if radius is None else radius
    if kind == "brief":
        return fd.brief_match(c["q"], c["t"], c["qc"], c["tc"], c["qv"], c["tv"], length=c["length"], q_xy=c["q_xy"],
                              t_xy=c["t_xy"], radius=r, **kw)
    return fd.nn_match(c["q"], c["t"], c["qc"], c["tc"], c["qv"], c["tv"], q_xy=c["q_xy"], t_xy=c["t_xy"], radius=r, **kw)


def assert_same(got, exp):
    for g, e, name in zip(got, exp, ("idx", "dist", "counts")):
        g = g.cpu().numpy() if hasattr(g, "cpu") else g
        assert g.dtype == e.dtype, name
        if g.dtype == F32:
            g, e = g.view(np.uint32), e.view(np.uint32)
        assert np.array_equal(g, e), name


def every_test_on(kind, c):
    """Every acceptance test enabled, at bounds that reject some and keep some."""
    if kind == "brief":
        return dict(max_distance=int(0.45 * c["length"]), max_ratio=0.97, cross_check=True)
    integer = bool((c["q"] == np.rint(c["q"])).all())  # the integer regime: random rows are ~37 dim apart, unit rows ~2
    return dict(max_distance=36.0 * c["q"].shape[2] if integer else 1.9, max_ratio=0.97, cross_check=True)


def run_case(fd, kind, c):
    for kw in ({}, every_test_on(kind, c)):
        exp = ref(kind, c, fill=SENT, **kw)
        rc, idx, dist, cnt = raw_guided(fd, kind, c, **kw)
        assert rc == 0
        assert_same((idx, dist, cnt), exp)


@pytest.mark.parametrize("kw", G.BRIEF_CASES, ids=G.case_id)
def test_brief_sizes_positions_and_radii(fd, kw):
    run_case(fd, "brief", G.brief_case(**kw))


@pytest.mark.parametrize("kw", G.NN_CASES, ids=G.case_id)
def test_nn_sizes_positions_and_radii(fd, kw):
    run_case(fd, "nn", G.nn_case(**kw))


def raw_nn_guided_dev(fd, torch, c, q_off, t_off, **kw):
    """fd_nn_match_guided through ctypes on device pointers, the descriptor sets as views q_off / t_off floats
    into their allocations (unaligned.offset_view), the outputs between guards. Returns (idx, dist, counts)."""
    from feature_detector_amd import _lib
    from unaligned import guarded, offset_view, unguard

    L, ctx = fd.load(), fd.default_context()
    ctx.set_stream(torch.cuda.current_stream(ctx.device).cuda_stream)
    B, Sq, St = c["q"].shape[0], c["q"].shape[1], c["t"].shape[1]
    (dq, keep_q), (dt, keep_t) = offset_view(torch, c["q"], q_off), offset_view(torch, c["t"], t_off)
    assert (dq.data_ptr() % 16 != 0) == (q_off != 0) and (dt.data_ptr() % 16 != 0) == (t_off != 0)
    d = {k: None if c[k] is None else torch.from_numpy(np.ascontiguousarray(c[k])).cuda() for k in ("qv", "qc", "q_xy", "tv", "tc", "t_xy")}
    p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())  # noqa: E731
    shapes = ((B, Sq), (B, Sq, 2), (B,))
    bufs = [guarded(torch, s, SENT, ty) for s, ty in zip(shapes, (torch.int32, torch.float32, torch.int32))]
    rx, ry = G.radii(c["radius"])
    gate = _lib.fd_match_gate(rx, ry)
    opts = _lib.fd_nn_match_opts(c["q"].shape[2], kw.get("max_distance", -1.0), kw.get("max_ratio", 0.0), int(kw.get("cross_check", 0)))
    rc = L.fd_nn_match_guided(ctx.ptr, B, ctypes.byref(opts), ctypes.byref(gate), p(dq), p(d["qv"]), p(d["qc"]), Sq, p(d["q_xy"]),
                              p(dt), p(d["tv"]), p(d["tc"]), St, p(d["t_xy"]), *(ctypes.c_void_p(ptr) for _, ptr in bufs), 1)
    assert rc == 0, L.fd_last_error(ctx.ptr)
    torch.cuda.synchronize()
    del keep_q, keep_t
    return tuple(unguard(buf, s, SENT) for (buf, _), s in zip(bufs, shapes))


@pytest.mark.parametrize("dim,regime", [(128, "round"), (256, "int"), (4, "round")])
def test_nn_unaligned_device_descriptors(fd, dim, regime):
    """The gated instances on descriptor bases that are float-aligned but not 16-byte aligned: k_nn_norms and
    the tile fill take their scalar loads. Train counts leave the last tile of either instance partial; with
    the cross-check the reverse pass searches the (offset) query set. Equal to the restatement and to the same
    call on aligned copies."""
    torch = pytest.importorskip("torch")
    c = G.nn_case(70, 130, B=2, qc=[70, 41], tc=[130, 77], flags=True, dim=dim, regime=regime, variant="tenth", radius=(12.0, 20.0))
    for kw in ({}, dict(cross_check=True), every_test_on("nn", c)):
        exp = ref("nn", c, fill=SENT, **kw)
        assert exp[2].sum() > 0
        for q_off, t_off in ((1, 0), (0, 3), (2, 2)):
            assert_same(raw_nn_guided_dev(fd, torch, c, q_off, t_off, **kw), exp)
        assert_same(raw_nn_guided_dev(fd, torch, c, 0, 0, **kw), exp)


@pytest.mark.parametrize("kind", KINDS)
def test_binding_host_and_device(fd, kind):
    """fd.brief_match / fd.nn_match with q_xy, t_xy, radius: numpy in, numpy out (-1 past the counts); torch
    device tensors in, torch out; [S, 2] positions for batch 1; out= keeps the sentinel."""
    torch = pytest.importorskip("torch")
    make = G.brief_case if kind == "brief" else G.nn_case
    c = make(70, 130, B=3, qc=[70, 41, 66], tc=[130, 99, 17], flags=True, radius=(3.0, 11.0), variant="tenth")
    kw = every_test_on(kind, c)
    m = bound(fd, kind, c, **kw)
    assert isinstance(m.idx, np.ndarray)
    assert_same((m.idx, m.dist, m.counts), ref(kind, c, **kw))
    d = {k: (torch.from_numpy(v.view(np.int32) if v.dtype == np.uint32 else v).cuda() if isinstance(v, np.ndarray) else v)
         for k, v in c.items()}
    m = bound(fd, kind, d, **kw)
    torch.cuda.synchronize()
    assert_same((m.idx, m.dist, m.counts), ref(kind, c, **kw))
    out = (torch.full((3, 70), SENT, dtype=torch.int32, device="cuda"),
           torch.full((3, 70, 2), SENT, dtype=torch.int32 if kind == "brief" else torch.float32, device="cuda"),
           torch.full((3,), SENT, dtype=torch.int32, device="cuda"))
    bound(fd, kind, d, out=out, **kw)
    torch.cuda.synchronize()
    assert_same(out, ref(kind, c, fill=SENT, **kw))
    one = make(20, 30)
    flat = dict(one, q=one["q"][0], t=one["t"][0], q_xy=one["q_xy"][0], t_xy=one["t_xy"][0])
    m = bound(fd, kind, flat)
    assert_same((m.idx, m.dist, m.counts), ref(kind, one))
    # positions on the other side than the descriptors, of another type or shape
    with pytest.raises(ValueError):
        bound(fd, kind, dict(c, q_xy=d["q_xy"]))
    with pytest.raises(TypeError):
        bound(fd, kind, dict(c, t_xy=c["t_xy"].astype(np.float64)))
    with pytest.raises(ValueError):
        bound(fd, kind, dict(c, t_xy=c["t_xy"][:, :-1]))


def hand_case(kind):
    """Queries at (10, 10), (30, 30), (50, 50), (70, 70), (90, 90) with radius 8.
    0: trains 0, 2, 4 tie for the best; 0, the lowest index, is outside the window: 2 wins, 4 is the second.
    1: its exact copy (train 1) is outside; the best inside is train 3, the second train 5.
    2: the window holds exactly one candidate (train 6): no second.  3: an empty window.
    4: trains 7 and 8 tie inside the window, a closer train 9 is outside."""
    q_xy = np.array([(10, 10), (30, 30), (50, 50), (70, 70), (90, 90)], F32)[None]
    t_xy = np.array([(20, 10), (30, 39), (12, 10), (31, 30), (10, 13), (28, 30), (50, 58), (91, 90), (90, 91), (99, 90)],
                    F32)[None]
    if kind == "brief":
        rng = np.random.default_rng(3)
        P = G.rand_words(rng, 5, 8)  # prototypes ~128 bits apart

        def f(w, *bits):
            w = w.copy()
            for b in bits:
                w[b // 32] ^= np.uint32(1 << (b % 32))
            return w

        q = P[None].copy()
        t = np.stack([f(P[0], 0), P[1], f(P[0], 40), f(P[1], 5), f(P[0], 255), f(P[1], 1, 2, 3), f(P[2], 7, 8), f(P[4], 9, 10),
                      f(P[4], 200, 201), f(P[4], 3)])[None]
        d = [[1, 1], [1, 3], [2, -1], [-1, -1], [2, 2]]
        plain = [0, 1, 6, None, 9]
        return dict(q=q, t=t, length=256), q_xy, t_xy, d, plain
    e = np.eye(8, dtype=F32)
    P = (F32(10) * e[:5])
    q = P[None].copy()
    t = np.stack([P[0] + e[5], P[1], P[0] + e[6], P[1] + e[5], P[0] - e[7], P[1] + e[5] + e[6] + e[7], P[2] + e[5] + e[6],
                  P[4] + e[5] - e[6], P[4] + e[6] + e[7], P[4] + e[5]])[None]
    d = [[1, 1], [1, 3], [2, -1], [-1, -1], [2, 2]]
    return dict(q=q, t=t), q_xy, t_xy, d, [0, 1, 6, None, 9]


@pytest.mark.parametrize("kind", KINDS)
def test_ties_best_outside_single_and_empty_windows(fd, kind):
    c, q_xy, t_xy, d, plain = hand_case(kind)
    c = dict(c, q_xy=q_xy, t_xy=t_xy, radius=8.0, qc=None, tc=None, qv=None, tv=None)
    un = (fd.brief_match(c["q"], c["t"]) if kind == "brief" else fd.nn_match(c["q"], c["t"]))
    for i, p in enumerate(plain):  # what the unguided matcher picks: the partner outside the window
        assert p is None or un.idx[0, i] == p
    m = bound(fd, kind, c, max_ratio=0.9)
    assert m.idx[0].tolist() == [-1, 3, 6, -1, -1]  # ties fail the ratio test; one candidate skips it
    m = bound(fd, kind, c)
    assert m.idx[0].tolist() == [2, 3, 6, -1, 7] and m.dist[0].tolist() == d and m.counts.tolist() == [4]
    assert_same((m.idx, m.dist, m.counts), ref(kind, c))
    # the same queries seen through a window that is wide along y only: query 1 reaches its copy again
    m = bound(fd, kind, c, radius=(1.0, 9.0))
    assert m.idx[0].tolist() == [4, 1, 6, -1, 7]
    assert_same((m.idx, m.dist, m.counts), ref(kind, c, radius=(1.0, 9.0)))


@pytest.mark.parametrize("kind", KINDS)
def test_cross_check_on_planted_mutual_pairs(fd, kind):
    """Query i and train perm[i] are copies at (almost) the same place for i < 40: mutual pairs, accepted under
    the cross-check. Queries 40..59 are copies of a train entry that already has a closer partner in its own
    window, so the cross-check rejects them; the rest is noise."""
    rng = np.random.default_rng(21)
    nq, nt = 90, 140
    make = G.brief_case if kind == "brief" else G.nn_case
    c = make(nq, nt, radius=4.0, seed=9) if kind == "brief" else make(nq, nt, dim=128, regime="round", radius=4.0, seed=9)
    perm = rng.permutation(nt)
    c["q_xy"][0] = (rng.permutation(45 * 45)[:nq, None] // np.array([45, 1]) % 45 * 20).astype(F32)  # a 20 px grid: windows apart
    c["t_xy"][0] = F32(5000) + rng.integers(0, 999, (nt, 2)).astype(F32)  # noise trains far away
    for i in range(40):
        c["t"][0, perm[i]] = c["q"][0, i]
        c["t_xy"][0, perm[i]] = c["q_xy"][0, i] + rng.integers(-4, 5, 2).astype(F32)
    for i in range(40, 60):
        c["q"][0, i] = c["q"][0, i - 40]
        if kind == "brief":
            c["q"][0, i, 0] ^= np.uint32(6)  # two bits from the copy
        else:
            c["q"][0, i, :2] += F32(0.01)
        c["q_xy"][0, i] = c["q_xy"][0, i - 40]  # the same window as the closer partner
    on, off = ref(kind, c, cross_check=True), ref(kind, c)
    assert on[0][0, :40].tolist() == perm[:40].tolist() and (on[0][0, 40:60] == -1).all()
    assert off[0][0, 40:60].tolist() == perm[:20].tolist()
    for kw, exp in ((dict(cross_check=True), on), ({}, off)):
        m = bound(fd, kind, c, **kw)
        assert_same((m.idx, m.dist, m.counts), exp)


@pytest.mark.parametrize("kind", KINDS)
def test_huge_radius_equals_the_unguided_entry(fd, kind):
    """With finite positions and both radii 3.0e38f every output has the unguided entry's bits, with every
    acceptance test on and off, across several tiles and a batch with counts and flags."""
    if kind == "brief":
        cases = [G.brief_case(70, 600, B=3, qc=[70, 0, 65], tc=[600, 5, 257], flags=True, variant="far", length=length)
                 for length in (256, 100)]
    else:
        cases = [G.nn_case(70, 130, B=3, qc=[70, 41, 66], tc=[130, 99, 17], flags=True, variant="far", dim=dim, regime=reg)
                 for dim, reg in ((128, "round"), (256, "round"), (256, "int"))]
    for c in cases:
        for kw in ({}, every_test_on(kind, c)):
            if kind == "brief":
                un = fd.brief_match(c["q"], c["t"], c["qc"], c["tc"], c["qv"], c["tv"], length=c["length"], **kw)
                plain = match_ref(c["q"], c["t"], c["qc"], c["tc"], c["qv"], c["tv"], length=c["length"], **kw)
            else:
                un = fd.nn_match(c["q"], c["t"], c["qc"], c["tc"], c["qv"], c["tv"], **kw)
                plain = nn_match_ref(c["q"], c["t"], c["qc"], c["tc"], c["qv"], c["tv"], **kw)
            m = bound(fd, kind, c, radius=HUGE, **kw)
            assert_same((m.idx, m.dist, m.counts), (un.idx, un.dist, un.counts))
            assert_same((m.idx, m.dist, m.counts), plain)


@pytest.mark.parametrize("kind", KINDS)
def test_nan_positions_never_match_and_are_never_a_second(fd, kind):
    """Position layout: NaN planted in x or in y of entries on both sides. With a huge radius every finite
    pair passes, so what differs from the unguided call is exactly the NaN entries: such a query is absent,
    such a train entry is neither a best nor a second (as if it were flagged invalid)."""
    make = G.brief_case if kind == "brief" else G.nn_case
    c = make(65, 300, variant="tenth") if kind == "brief" else make(65, 129, dim=128, regime="int", variant="tenth")
    rng = np.random.default_rng(5)
    qn, tn = rng.random(65) < 0.2, rng.random(c["t"].shape[1]) < 0.3
    c["q_xy"][0, qn, rng.integers(0, 2, qn.sum())] = np.nan
    c["t_xy"][0, tn, rng.integers(0, 2, tn.sum())] = np.nan
    flagged = dict(c, qv=(~qn).astype(np.uint8)[None], tv=(~tn).astype(np.uint8)[None])
    for kw in ({}, dict(cross_check=True)):
        if kind == "brief":
            exp = match_ref(c["q"], c["t"], None, None, flagged["qv"], flagged["tv"], **kw)
        else:
            exp = nn_match_ref(c["q"], c["t"], None, None, flagged["qv"], flagged["tv"], **kw)
        m = bound(fd, kind, c, radius=HUGE, **kw)
        assert_same((m.idx, m.dist, m.counts), exp)
        assert (m.idx[0, qn] == -1).all() and (m.dist[0, qn] == -1).all() and not np.isin(m.idx[0], np.flatnonzero(tn)).any()
        m = bound(fd, kind, c, **kw)  # and under a real window
        assert_same((m.idx, m.dist, m.counts), ref(kind, c, **kw))


def test_device_chain_brief(fd, image_png):
    """detect_points -> brief_compute -> guided brief_match on device tensors, frame i against frame i + 1 of
    one batch (the train pointers advanced by one frame), on the positions detect_points left on the device."""
    torch = pytest.importorskip("torch")
    host = np.stack([image_png, np.roll(image_png, (3, 5), (0, 1)), np.roll(image_png, (-2, 9), (0, 1))])
    dev = torch.from_numpy(host).cuda()
    res = fd.detect_points("harris", dev, 200, 15, 30.0)
    bits, valid = fd.brief_compute(dev, res.xy, res.counts, with_valid=True)
    kw = dict(cross_check=True, max_distance=64)
    m = fd.brief_match(bits[:-1], bits[1:], res.counts[:-1], res.counts[1:], valid[:-1], valid[1:], q_xy=res.xy[:-1],
                       t_xy=res.xy[1:], radius=(12.0, 6.0), **kw)
    torch.cuda.synchronize()
    b, v, c, p = bits.cpu().numpy(), valid.cpu().numpy(), res.counts.cpu().numpy(), res.xy.cpu().numpy()
    exp = match_guided_ref(b[:-1], b[1:], p[:-1], p[1:], (12.0, 6.0), c[:-1], c[1:], v[:-1], v[1:], **kw)
    assert_same((m.idx, m.dist, m.counts), exp)
    assert int(m.counts.min()) >= 1


def test_device_chain_nn(fd):
    """nn_select -> nn_descriptors -> guided nn_match on device tensors, the same frame-to-frame chain."""
    torch = pytest.importorskip("torch")
    from feature_detector_amd.superpoint import Options, nn_descriptors, nn_select

    g = torch.Generator().manual_seed(11)
    B, C, h, w = 3, 256, 12, 16
    heat = torch.rand((1, 8 * h, 8 * w), generator=g)
    heat = torch.stack([torch.roll(heat[0], (2 * b, 3 * b), (0, 1)) for b in range(B)]).cuda()
    dmap = torch.nn.functional.normalize(torch.randn((B, C, h, w), generator=g), dim=1).cuda()
    xy, counts = nn_select(heat, Options(kMinFeatureDistance=6, kMaxNumberOfDetectedFeatures=60, kMinResponse=0.5))
    desc = nn_descriptors(dmap, xy, counts)
    kw = dict(cross_check=True, max_ratio=0.99)
    m = fd.nn_match(desc[:-1], desc[1:], counts[:-1], counts[1:], q_xy=xy[:-1], t_xy=xy[1:], radius=20.0, **kw)
    torch.cuda.synchronize()
    d, c, p = desc.cpu().numpy(), counts.cpu().numpy(), xy.cpu().numpy()
    exp = nn_match_guided_ref(d[:-1], d[1:], p[:-1], p[1:], 20.0, c[:-1], c[1:], **kw)
    assert_same((m.idx, m.dist, m.counts), exp)
    assert int(c.min()) >= 10 and int(m.counts.min()) >= 1


@pytest.mark.parametrize("cross_check", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_graph_capture(fd, kind, cross_check):
    """The guided call is kernels only on device pointers: captured after one warm call of the shape, replayed
    on new contents of the same tensors, equal to the eager call and to the reference."""
    torch = pytest.importorskip("torch")
    make = G.brief_case if kind == "brief" else G.nn_case
    B, Sq, St = 2, 90, 140
    cases = [make(Sq, St, B=B, qc=[90, 77], flags=True, seed=s, variant=v) for s, v in ((1, "tenth"), (2, "far"))]
    names = ("q", "t", "q_xy", "t_xy", "qc", "qv", "tv")
    as_t = lambda v: torch.from_numpy(v.view(np.int32) if v.dtype == np.uint32 else v)  # noqa: E731
    d = dict(cases[0], **{k: torch.zeros_like(as_t(cases[0][k])).cuda() for k in names})
    d["qc"].copy_(as_t(cases[0]["qc"]))
    out = (torch.empty((B, Sq), dtype=torch.int32, device="cuda"),
           torch.empty((B, Sq, 2), dtype=torch.int32 if kind == "brief" else torch.float32, device="cuda"),
           torch.empty((B,), dtype=torch.int32, device="cuda"))
    kw = dict(every_test_on(kind, cases[0]), cross_check=cross_check)
    bound(fd, kind, d, out=out, **kw)  # sizes the workspace
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        bound(fd, kind, d, out=out, **kw)
    for c in cases:
        for k in names:
            d[k].copy_(as_t(c[k]))
        for o in out:
            o.fill_(SENT)
        g.replay()
        torch.cuda.synchronize()
        replayed = [o.cpu().numpy().copy() for o in out]
        assert_same(replayed, ref(kind, c, fill=SENT, **kw))
        for o in out:
            o.fill_(SENT)
        bound(fd, kind, d, out=out, **kw)
        torch.cuda.synchronize()
        assert_same(out, replayed)
    del g


@pytest.mark.parametrize("kind", KINDS)
def test_bad_arguments(fd, kind):
    from feature_detector_amd import _lib

    c = (G.brief_case if kind == "brief" else G.nn_case)(4, 4)
    assert raw_guided(fd, kind, c)[0] == 0
    # gate, q_xy or t_xy NULL; what the unguided entry rejects: descriptors / out_idx / opts NULL, batch, strides
    for name in ("gate", "q_xy", "t_xy", "q", "t", "idx", "opts"):
        assert raw_guided(fd, kind, c, **{name: None})[0] == _lib.FD_ERR_INVALID, name
    for over in (dict(batch=0), dict(sq=-1), dict(st=-1)):
        assert raw_guided(fd, kind, c, **over)[0] == _lib.FD_ERR_INVALID, over
    for bad in (-1.0, -0.5, float("nan"), float("inf"), float("-inf")):
        for radius in ((bad, 1.0), (1.0, bad)):
            assert raw_guided(fd, kind, c, radius=radius)[0] == _lib.FD_ERR_INVALID, radius
            with pytest.raises(fd.FdError):
                bound(fd, kind, c, radius=radius)
    assert raw_guided(fd, kind, c, max_ratio=float("nan"))[0] == _lib.FD_ERR_INVALID
    if kind == "brief":
        for length in (0, 257):
            assert raw_guided(fd, kind, dict(c, length=length))[0] == _lib.FD_ERR_INVALID
    else:
        assert raw_guided(fd, kind, c, max_distance=float("inf"))[0] == _lib.FD_ERR_INVALID
        bad = G.nn_case(4, 4, dim=8)
        bad["q"], bad["t"] = bad["q"][..., :6].copy(), bad["t"][..., :6].copy()
        assert raw_guided(fd, kind, bad)[0] == _lib.FD_ERR_INVALID
    # radius -0.0 is radius 0; the zero-stride cases are the unguided entry's
    assert raw_guided(fd, kind, c, radius=-0.0)[0] == 0
    e = dict(c, q=c["q"][:, :0], q_xy=c["q_xy"][:, :0])
    rc, idx, dist, cnt = raw_guided(fd, kind, e)
    assert rc == 0 and cnt.tolist() == [0]
    e = dict(c, t=c["t"][:, :0], t_xy=c["t_xy"][:, :0])
    rc, idx, dist, cnt = raw_guided(fd, kind, e)
    assert rc == 0 and (idx == -1).all() and (dist == -1).all() and cnt.tolist() == [0]
