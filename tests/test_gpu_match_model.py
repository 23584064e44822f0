"""GPU: model-gated matching, fd_brief_match_model and fd_nn_match_model, against tests/match_model_ref.py.

Bar: every output array equal to the numpy restatement (np.array_equal): accepted indices, both raw
distances (the float ones as bit patterns), the per-frame counts, and the sentinel in every slot that must
not be written. The random fixtures are match_model_ref.BRIEF_CASES / NN_CASES;
tests/test_match_model_host.py proves that the gate changes most answers on each of them.
"""
import ctypes

import numpy as np
import pytest

import match_guided_ref as G
import match_model_ref as MM
from match_model_ref import FUNDAMENTAL, HOMOGRAPHY, OPEN

pytestmark = pytest.mark.gpu

F32 = np.float32
SENT = -77  # prefill of the output slots that must not be written
WHICH = ("brief", "nn")
NAMES = {FUNDAMENTAL: "fundamental", HOMOGRAPHY: "homography"}


@pytest.fixture(scope="module")
def fd():
    import feature_detector_amd as fd

    fd.load()
    return fd


def raw_model(fd, which, c, max_distance=-1, max_ratio=0.0, cross_check=False, fill=SENT, **over):
    """The model entry through ctypes on host pointers, the outputs prefilled with `fill`. `over` replaces
    arguments by name (gate, model, q, q_xy, t, t_xy, idx, batch, sq, st, opts, kind, threshold, radius)."""
    from feature_detector_amd import _lib

    L = fd.load()
    ctx = fd.default_context()
    ctx.set_stream(None)
    q, t = c["q"], c["t"]
    B, Sq, St = q.shape[0], q.shape[1], t.shape[1]
    idx = np.full((B, Sq), fill, np.int32)
    dist = np.full((B, Sq, 2), fill, np.int32 if which == "brief" else F32)
    cnt = np.full((B,), fill, np.int32)
    p = lambda x: None if x is None else ctypes.c_void_p(x.ctypes.data)  # noqa: E731
    rx, ry = G.radii(over.pop("radius", c["radius"]))
    gate = _lib.fd_match_model_gate(over.pop("kind", c["kind"]), over.pop("threshold", c["threshold"]), rx, ry)
    if which == "brief":
        opts, fn = _lib.fd_match_opts(c["length"], int(max_distance), max_ratio, int(cross_check)), L.fd_brief_match_model
    else:
        opts, fn = _lib.fd_nn_match_opts(q.shape[2], max_distance, max_ratio, int(cross_check)), L.fd_nn_match_model
    a = dict(gate=ctypes.byref(gate), model=p(c["model"]), q=p(q), q_xy=p(c["q_xy"]), t=p(t), t_xy=p(c["t_xy"]), idx=p(idx),
             batch=B, sq=Sq, st=St, opts=ctypes.byref(opts))
    a.update(over)
    rc = fn(ctx.ptr, a["batch"], a["opts"], a["gate"], a["model"], a["q"], p(c["qv"]), p(c["qc"]), a["sq"], a["q_xy"], a["t"],
            p(c["tv"]), p(c["tc"]), a["st"], a["t_xy"], a["idx"], p(dist), p(cnt), 0)
    return rc, idx, dist, cnt


def bound(fd, which, c, **kw):
    """fd.brief_match / fd.nn_match with the model keywords, on the case's arrays (or tensors)."""
    radius = None if isinstance(c["radius"], float) and c["radius"] == OPEN else c["radius"]
    mk = dict(q_xy=c["q_xy"], t_xy=c["t_xy"], radius=radius, model=c["model"], model_kind=NAMES[c["kind"]],
              threshold=c["threshold"])
    if which == "brief":
        return fd.brief_match(c["q"], c["t"], c["qc"], c["tc"], c["qv"], c["tv"], length=c["length"], **mk, **kw)
    return fd.nn_match(c["q"], c["t"], c["qc"], c["tc"], c["qv"], c["tv"], **mk, **kw)


def assert_same(got, exp):
    for g, e, name in zip(got, exp, ("idx", "dist", "counts")):
        g = g.cpu().numpy() if hasattr(g, "cpu") else g
        assert g.dtype == e.dtype, name
        if g.dtype == F32:
            g, e = g.view(np.uint32), e.view(np.uint32)
        assert np.array_equal(g, e), name


def every_test_on(which, c):
    """Every acceptance test enabled, at bounds that reject some and keep some."""
    if which == "brief":
        return dict(max_distance=int(0.45 * c["length"]), max_ratio=0.97, cross_check=True)
    integer = bool((c["q"] == np.rint(c["q"])).all())  # the integer regime: random rows are ~37 dim apart, unit rows ~2
    return dict(max_distance=36.0 * c["q"].shape[2] if integer else 1.9, max_ratio=0.97, cross_check=True)


def run_case(fd, which, c):
    for kw in ({}, every_test_on(which, c)):
        exp = MM.ref(which, c, fill=SENT, **kw)
        rc, idx, dist, cnt = raw_model(fd, which, c, **kw)
        assert rc == 0
        assert_same((idx, dist, cnt), exp)


@pytest.mark.parametrize("kw", MM.BRIEF_CASES, ids=MM.case_id)
def test_brief_sizes_kinds_and_thresholds(fd, kw):
    run_case(fd, "brief", MM.brief_case(**kw))


@pytest.mark.parametrize("kw", MM.NN_CASES, ids=MM.case_id)
def test_nn_sizes_kinds_and_thresholds(fd, kw):
    run_case(fd, "nn", MM.nn_case(**kw))


def _batch_case(which, kind, models="mixed", radius=8.0):
    make = MM.brief_case if which == "brief" else MM.nn_case
    return make(70, 130, B=3, qc=[70, 41, 66], tc=[130, 99, 17], flags=True, kind=kind, threshold=2.5, models=models, radius=radius)


def _to_device(torch, c):
    return {k: (torch.from_numpy(v.view(np.int32) if v.dtype == np.uint32 else v).cuda() if isinstance(v, np.ndarray) else v)
            for k, v in c.items()}


@pytest.mark.parametrize("kind", [FUNDAMENTAL, HOMOGRAPHY])
@pytest.mark.parametrize("which", WHICH)
def test_binding_host_and_device(fd, which, kind):
    """fd.brief_match / fd.nn_match with model=: numpy in, numpy out (-1 past the counts); torch device tensors in,
    torch out, equal to the host-pointer call; a GeometryResult as the model; [9] for batch 1; out= keeps the
    sentinel; a batch with a zero-model and a NaN-model frame under a finite window."""
    torch = pytest.importorskip("torch")
    c = _batch_case(which, kind)
    kw = every_test_on(which, c)
    exp = MM.ref(which, c, **kw)
    assert exp[2][0] >= 1 and exp[2][1] >= 1 and exp[2][2] == 0  # the NaN-model frame matches nothing
    m = bound(fd, which, c, **kw)
    assert isinstance(m.idx, np.ndarray)
    assert_same((m.idx, m.dist, m.counts), exp)
    d = _to_device(torch, c)
    m = bound(fd, which, d, **kw)
    torch.cuda.synchronize()
    assert_same((m.idx, m.dist, m.counts), exp)
    res = fd.GeometryResult(d["model"], None, None, None)
    m = bound(fd, which, dict(d, model=res), **kw)
    torch.cuda.synchronize()
    assert_same((m.idx, m.dist, m.counts), exp)
    out = (torch.full((3, 70), SENT, dtype=torch.int32, device="cuda"),
           torch.full((3, 70, 2), SENT, dtype=torch.int32 if which == "brief" else torch.float32, device="cuda"),
           torch.full((3,), SENT, dtype=torch.int32, device="cuda"))
    bound(fd, which, d, out=out, **kw)
    torch.cuda.synchronize()
    assert_same(out, MM.ref(which, c, fill=SENT, **kw))
    one = (MM.brief_case if which == "brief" else MM.nn_case)(20, 30, kind=kind, threshold=4.0)
    flat = dict(one, q=one["q"][0], t=one["t"][0], q_xy=one["q_xy"][0], t_xy=one["t_xy"][0], model=one["model"][0])
    m = bound(fd, which, flat)
    assert_same((m.idx, m.dist, m.counts), MM.ref(which, one))
    # the model on the other side than the descriptors, of another type or shape
    with pytest.raises(ValueError):
        bound(fd, which, dict(c, model=d["model"]))
    with pytest.raises(TypeError):
        bound(fd, which, dict(c, model=c["model"].astype(F32)))
    with pytest.raises(ValueError):
        bound(fd, which, dict(c, model=c["model"][:2]))


@pytest.mark.parametrize("kind", [FUNDAMENTAL, HOMOGRAPHY])
@pytest.mark.parametrize("which", WHICH)
def test_zero_model_is_the_guided_and_the_unguided_call(fd, which, kind):
    """Nine zeros pass every pair: with a window the outputs are the guided entry's, with the open radius the
    unguided entry's, bit for bit, with every acceptance test on."""
    c = _batch_case(which, kind, models="real")
    c["model"][:] = 0.0
    kw = every_test_on(which, c)
    pos = dict(q_xy=c["q_xy"], t_xy=c["t_xy"])
    args = (c["q"], c["t"], c["qc"], c["tc"], c["qv"], c["tv"])
    fn, ext = (fd.brief_match, dict(length=c["length"])) if which == "brief" else (fd.nn_match, {})
    m = bound(fd, which, c, **kw)
    g = fn(*args, radius=8.0, **pos, **ext, **kw)
    assert_same((m.idx, m.dist, m.counts), (g.idx, g.dist, g.counts))
    m = bound(fd, which, dict(c, radius=OPEN), **kw)
    u = fn(*args, **ext, **kw)
    assert_same((m.idx, m.dist, m.counts), (u.idx, u.dist, u.counts))
    assert int(u.counts.sum()) >= 1


def test_hand_cases_on_the_device(fd):
    """tests/test_match_model_host.py's band case (a tie inside with the copy outside, one candidate, an empty
    band) and its directional homography case, through the binding."""
    q_xy = np.array([(10, 10), (10, 30), (10, 50), (10, 70)], F32)[None]
    t_xy = np.array([(40, 20), (50, 10), (60, 11), (20, 30), (30, 51), (40, 49), (50, 50.5)], F32)[None]
    q = np.array([0x0, 0x0, 0xFF00, 0x0], np.uint32).reshape(1, -1, 1)
    t = np.array([0x0, 0x1, 0x2, 0xFF, 0xFF01, 0xFF03, 0xFF00FF], np.uint32).reshape(1, -1, 1)
    F = np.array([[0, 0, 0, 0, 0, -1, 0, 1, 0]], np.float64)
    kw = dict(length=32, q_xy=q_xy, t_xy=t_xy, model=F, model_kind="fundamental", threshold=1.0)
    m = fd.brief_match(q, t, **kw)
    assert m.idx.tolist() == [[1, 3, 4, -1]] and m.dist.tolist() == [[[1, 1], [8, -1], [1, 2], [-1, -1]]] and m.counts.tolist() == [3]
    m = fd.brief_match(q, t, max_ratio=0.6, **kw)
    assert m.idx.tolist() == [[-1, 3, 4, -1]] and m.counts.tolist() == [2]
    H = np.array([[1, 0, 3, 0, 1, -2, 0, 0, 1]], np.float64)
    q, t = np.array([0x3, 0x1], np.uint32).reshape(1, 2, 1), np.array([0x1], np.uint32).reshape(1, 1, 1)
    q_xy, t_xy = np.array([(5, 7), (8, 5)], F32)[None], np.array([(8, 5)], F32)[None]
    m = fd.brief_match(q, t, length=32, cross_check=True, q_xy=q_xy, t_xy=t_xy, model=H, model_kind="homography", threshold=0.5)
    assert m.idx.tolist() == [[0, -1]] and m.dist.tolist() == [[[1, -1], [-1, -1]]] and m.counts.tolist() == [1]
    # the inclusive bound and the next threshold down (train (11, 9) is 5 px from where H sends (5, 7))
    t_xy = np.array([(11, 9)], F32)[None]
    for thr, hit in ((5.0, 0), (float(np.nextafter(F32(5.0), F32(0))), -1)):
        m = fd.brief_match(q[:, :1], t, length=32, q_xy=q_xy[:, :1], t_xy=t_xy, model=H, model_kind="homography", threshold=thr)
        assert m.idx.tolist() == [[hit]]


def test_device_chain(fd):
    """brief_match -> verify_geometry -> refit_geometry -> brief_match(model=result), all on device tensors: the
    second pass equals the restatement fed the same model bytes and accepts strictly more than the first."""
    torch = pytest.importorskip("torch")
    s = MM.two_view_scene()
    d = {k: torch.from_numpy(v.view(np.int32) if v.dtype == np.uint32 else v).cuda() for k, v in s.items()
         if isinstance(v, np.ndarray) and k in ("q", "t", "q_xy", "t_xy")}
    kw = dict(max_ratio=0.8, cross_check=True)
    first = fd.brief_match(d["q"], d["t"], **kw)
    geo = dict(matches=first.idx, model="homography", threshold=2.0, image_size=(480, 640))
    res = fd.verify_geometry(d["q_xy"], d["t_xy"], hypotheses=256, seed=1, **geo)
    res = fd.refit_geometry(d["q_xy"], d["t_xy"], res, **geo)
    second = fd.brief_match(d["q"], d["t"], q_xy=d["q_xy"], t_xy=d["t_xy"], model=res, model_kind="homography", threshold=2.0, **kw)
    torch.cuda.synchronize()
    model = res.model.cpu().numpy()
    assert np.isfinite(model).all() and model.any()
    exp = MM.match_model_ref(s["q"], s["t"], s["q_xy"], s["t_xy"], model, HOMOGRAPHY, 2.0, **kw)
    assert_same((second.idx, second.dist, second.counts), exp)
    assert int(second.counts[0]) > int(first.counts[0]) >= 8


@pytest.mark.parametrize("kind,cross_check", [(FUNDAMENTAL, True), (HOMOGRAPHY, True), (HOMOGRAPHY, False)])
@pytest.mark.parametrize("which", WHICH)
def test_graph_capture(fd, which, kind, cross_check):
    """The model call is kernels only on device pointers: captured after one warm call of the shape, replayed on
    new contents of the same tensors (the model among them), equal to the eager call and to the reference."""
    torch = pytest.importorskip("torch")
    make = MM.brief_case if which == "brief" else MM.nn_case
    B, Sq, St = 2, 90, 140
    cases = [make(Sq, St, B=B, qc=[90, 77], flags=True, seed=s, kind=kind, threshold=2.5) for s in (1, 2)]
    names = ("q", "t", "q_xy", "t_xy", "qc", "qv", "tv", "model")
    as_t = lambda v: torch.from_numpy(v.view(np.int32) if v.dtype == np.uint32 else v)  # noqa: E731
    d = dict(cases[0], **{k: torch.zeros_like(as_t(cases[0][k])).cuda() for k in names})
    d["qc"].copy_(as_t(cases[0]["qc"]))
    out = (torch.empty((B, Sq), dtype=torch.int32, device="cuda"),
           torch.empty((B, Sq, 2), dtype=torch.int32 if which == "brief" else torch.float32, device="cuda"),
           torch.empty((B,), dtype=torch.int32, device="cuda"))
    kw = dict(every_test_on(which, cases[0]), cross_check=cross_check)
    bound(fd, which, d, out=out, **kw)  # sizes the workspace
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        bound(fd, which, d, out=out, **kw)
    for c in cases:
        for k in names:
            d[k].copy_(as_t(c[k]))
        for o in out:
            o.fill_(SENT)
        g.replay()
        torch.cuda.synchronize()
        replayed = [o.cpu().numpy().copy() for o in out]
        assert_same(replayed, MM.ref(which, c, fill=SENT, **kw))
        for o in out:
            o.fill_(SENT)
        bound(fd, which, d, out=out, **kw)
        torch.cuda.synchronize()
        assert_same(out, replayed)
    del g


@pytest.mark.parametrize("which", WHICH)
def test_bad_arguments(fd, which):
    from feature_detector_amd import _lib

    c = (MM.brief_case if which == "brief" else MM.nn_case)(4, 4)
    assert raw_model(fd, which, c)[0] == 0
    # gate, model, q_xy or t_xy NULL; what the guided entry rejects: descriptors / out_idx / opts NULL, batch, strides
    for name in ("gate", "model", "q_xy", "t_xy", "q", "t", "idx", "opts"):
        assert raw_model(fd, which, c, **{name: None})[0] == _lib.FD_ERR_INVALID, name
    for over in (dict(batch=0), dict(sq=-1), dict(st=-1), dict(kind=2), dict(kind=-1)):
        assert raw_model(fd, which, c, **over)[0] == _lib.FD_ERR_INVALID, over
    for bad in (0.0, -1.0, float("nan"), float("inf"), float("-inf")):
        assert raw_model(fd, which, c, threshold=bad)[0] == _lib.FD_ERR_INVALID, bad
        with pytest.raises(fd.FdError):
            bound(fd, which, dict(c, threshold=bad))
    for bad in (-1.0, float("nan"), float("inf")):
        for radius in ((bad, 1.0), (1.0, bad)):
            assert raw_model(fd, which, c, radius=radius)[0] == _lib.FD_ERR_INVALID, radius
    assert raw_model(fd, which, c, max_ratio=float("nan"))[0] == _lib.FD_ERR_INVALID
    # the zero-stride cases are the unguided entry's
    e = dict(c, q=c["q"][:, :0], q_xy=c["q_xy"][:, :0])
    rc, idx, dist, cnt = raw_model(fd, which, e)
    assert rc == 0 and cnt.tolist() == [0]
    e = dict(c, t=c["t"][:, :0], t_xy=c["t_xy"][:, :0])
    rc, idx, dist, cnt = raw_model(fd, which, e)
    assert rc == 0 and (idx == -1).all() and (dist == -1).all() and cnt.tolist() == [0]
