"""fd_pyr_build / fd_flow_lk on the GPU against tests/flow_ref.py: every output exactly, positions and
errors as bit patterns. Small frames (96 x 128) keep the numpy restatement at a few milliseconds a feature."""
import ctypes

import numpy as np
import pytest

import flow_ref as R

pytestmark = pytest.mark.gpu

ROWS, COLS, PAD = 96, 128, 16
SENT_XY, SENT_ST, SENT_ERR, SENT_CNT = -77.0, 99, -55.0, -7


@pytest.fixture(scope="module")
def fd():
    import feature_detector_amd as fd

    fd.load()
    return fd


def _box(a, k):
    """k x k box mean (edge-replicated) of a float array."""
    p = np.pad(a, k // 2, mode="edge")
    c = np.cumsum(np.cumsum(np.pad(p, ((1, 0), (1, 0))), 0), 1)
    return (c[k:, k:] - c[:-k, k:] - c[k:, :-k] + c[:-k, :-k]) / (k * k)


@pytest.fixture(scope="module")
def canvas(oracle):
    """Two noise-plus-blobs canvases (one per frame of the batch), PAD pixels larger than a frame all round."""
    out = []
    for seed in (5, 6):
        r, c = ROWS + 2 * PAD, COLS + 2 * PAD
        coarse = oracle.make_frame("noise", seed, r // 8 + 1, c // 8 + 1).astype(np.float64)
        blobs = _box(np.kron(coarse, np.ones((8, 8)))[:r, :c], 7)
        fine = oracle.make_frame("noise", seed + 100, r, c).astype(np.float64)
        out.append(np.clip(np.rint(0.85 * blobs + 0.15 * fine), 0, 255).astype(np.uint8))
    return np.stack(out)


def view(canvas, sx=0, sy=0):
    """The frames whose content sits (sx, sy) pixels right / down of view(canvas)'s."""
    return np.ascontiguousarray(canvas[:, PAD - sy:PAD - sy + ROWS, PAD - sx:PAD - sx + COLS])


def half_shift(canvas, sx, sy):
    """Content moved by (sx + 0.5, sy + 0.5): the rounded mean of four integer shifts."""
    s = sum(view(canvas, sx + i, sy + j).astype(np.int32) for i in (0, 1) for j in (0, 1))
    return ((s + 2) >> 2).astype(np.uint8)


@pytest.fixture(scope="module")
def features():
    """[2, 40, 2] positions: integer and fractional ones, away from the border."""
    rng = np.random.default_rng(3)
    xy = np.stack([rng.uniform(14, COLS - 15, (2, 40)), rng.uniform(14, ROWS - 15, (2, 40))], -1).astype(np.float32)
    xy[:, :12] = np.rint(xy[:, :12])
    return xy


COUNTS = np.array([40, 17], np.int32)


def same(res, exp):
    xy, st, err, cnt = (np.asarray(t.cpu()) if hasattr(t, "cpu") else np.asarray(t) for t in (res.xy, res.status, res.err, res.counts))
    exy, est, eerr, ecnt = exp
    assert np.array_equal(st, est), (st.tolist(), est.tolist())
    assert np.array_equal(xy.view(np.uint32), exy.view(np.uint32))
    assert np.array_equal(err.view(np.uint32), eerr.view(np.uint32))
    assert np.array_equal(cnt, ecnt)


# ---- pyramid ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows,cols,levels", [(1, 1, 1), (5, 7, 2), (37, 53, 3), (64, 256, 1), (64, 256, 3), (64, 256, 6)])
@pytest.mark.parametrize("batch", [1, 3])
def test_pyramid(fd, rows, cols, levels, batch):
    torch = pytest.importorskip("torch")
    frames = np.random.default_rng(rows * cols + batch).integers(0, 256, (batch, rows, cols), dtype=np.uint8)
    exp = R.pyr_ref(frames, levels)
    off = R.pyr_layout(batch, rows, cols, levels)
    host = fd.build_pyramid(frames, levels)
    assert host.offsets == off and isinstance(host.data, np.ndarray) and host.data.size == off[-1]
    assert np.array_equal(host.data, R.pyr_pack(exp))  # (the padding stays as it was: zeros)
    dev = fd.build_pyramid(torch.from_numpy(frames).cuda(), levels)
    mixed = fd.build_pyramid(frames, levels, device_out=True)
    torch.cuda.synchronize()
    for l in range(levels):
        assert np.array_equal(host.level(l), exp[l])
        assert np.array_equal(dev.level(l).cpu().numpy(), exp[l])
        assert np.array_equal(mixed.level(l).cpu().numpy(), exp[l])


# ---- tracker ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("r", [1, 3, 7, 10])
@pytest.mark.parametrize("levels", [1, 3])
@pytest.mark.parametrize("motion", ["integer", "half"])
def test_sweep(fd, canvas, features, r, levels, motion):
    """The main case (batch 2, stride 40, counts 40 and 17) over the lane-share edges of the window (n = 9 and 49
    below one wave, 225 and 441 over 4 and 7 rounds), one and three levels, an integer shift (2, -1) and a
    half-pixel one, where the iterations run more than once."""
    prev = view(canvas)
    nxt = view(canvas, 2, -1) if motion == "integer" else half_shift(canvas, 1, -1)
    kw = dict(counts=COUNTS, levels=levels, half_window=r, max_iters=20, epsilon=0.01, min_eigen=1e-4)
    exp = R.flow_ref(prev, nxt, features, **kw)
    res = fd.track_lk(prev, nxt, features, **kw)
    same(res, exp)
    assert (exp[1] == 1).sum() >= 10
    if motion == "half":  # more than one iteration somewhere: one iteration gives another answer
        one = R.flow_ref(prev, nxt, features, **dict(kw, max_iters=1))
        assert not np.array_equal(one[0], exp[0])


def test_six_levels(fd, canvas, features):
    """The deepest pyramid the contract allows: 96 x 128 keeps a 3 x 4 top level, where every window is mostly
    clamped reads; with and without the forward-backward check."""
    prev, nxt = view(canvas), view(canvas, 3, -2)
    for extra in ({}, {"fb_max_dist": 0.5}):
        kw = dict(counts=COUNTS, levels=6, half_window=4, max_iters=10, min_eigen=1e-4, **extra)
        exp = R.flow_ref(prev, nxt, features, **kw)
        same(fd.track_lk(prev, nxt, features, **kw), exp)
        assert (exp[1] == 1).sum() >= 10


def test_edges_and_corners(fd, canvas):
    """Features on the frame edge and in the corners: the window hangs over the edge at every level, the
    reads are clamped."""
    prev, nxt = view(canvas)[:1], view(canvas, 1, 1)[:1]
    xs, ys = [0, 0.5, 3, COLS / 2, COLS - 4.25, COLS - 1], [0, 0.75, 2, ROWS / 2, ROWS - 3.5, ROWS - 1]
    xy = np.array([[x, y] for x in xs for y in ys], np.float32)[None]
    kw = dict(levels=3, half_window=7, max_iters=10, min_eigen=1e-4)
    exp = R.flow_ref(prev, nxt, xy, **kw)
    same(fd.track_lk(prev, nxt, xy, **kw), exp)
    assert set(np.unique(exp[1])) >= {1}


def test_lost_cases(fd, canvas):
    prev = view(canvas)[:1].copy()
    prev[0, 8:40, 8:40] = 90                                   # flat patch
    prev[0, 50:90, 8:28], prev[0, 50:90, 28:48] = 40, 200      # pure vertical edge at x = 28
    yy, xx = np.mgrid[0:40, 0:40]
    prev[0, 8:48, 80:120] = np.where(((yy >> 1) + (xx >> 1)) & 1, 220, 30)  # 2 x 2 blocks: flat from level 1 up
    nxt = prev.copy()
    xy = np.array([[24, 24], [28, 70], [100, 28], [60.5, 40.25], [np.nan, 5], [5, np.inf], [-0.5, 5], [COLS - 0.5, 5],
                   [5, ROWS], [70, 60]], np.float32)[None]
    guess = xy.copy()
    guess[0, 9] = (70 + 4 * COLS, 60)  # pushed out of the frame
    kw = dict(levels=3, half_window=3, max_iters=10, min_eigen=1e-3)
    exp = R.flow_ref(prev, nxt, xy, guess=guess, **kw)
    assert exp[1][0].tolist() == [3, 3, 1, 1, 2, 2, 2, 2, 2, 2]
    trace = []
    pl, nl = R._levels_i64(prev, 3)[0], R._levels_i64(nxt, 3)[0]
    R.track_one(pl, nl, xy[0, 2], None, ROWS, COLS, 3, 10, 0.01, 1e-3, -1.0, trace=trace)
    assert [(l, u) for l, u, _ in trace] == [(2, False), (1, False), (0, True)]  # skipped above, tracked at level 0
    same(fd.track_lk(prev, nxt, xy, guess=guess, **kw), exp)


def test_valid_counts_and_unwritten_slots(fd, canvas, features):
    torch = pytest.importorskip("torch")
    prev, nxt = view(canvas), view(canvas, 1, 0)
    valid = (np.random.default_rng(4).random((2, 40)) < 0.7).astype(np.uint8)
    counts = np.array([31 | (1 << 25) | (1 << 31), 17 | (1 << 28)], np.int64).astype(np.int32)  # guard bits set
    init = (np.full((2, 40, 2), SENT_XY, np.float32), np.full((2, 40), SENT_ST, np.uint8), np.full((2, 40), SENT_ERR, np.float32))
    kw = dict(levels=2, half_window=4, max_iters=10, min_eigen=1e-4)
    exp = R.flow_ref(prev, nxt, features, counts=counts, valid=valid, init=init, **kw)
    assert (exp[1] == 0).any() and (exp[2][exp[1] == 0] == SENT_ERR).all() and (exp[1][0, 31:] == SENT_ST).all()
    out = tuple(torch.from_numpy(a.copy()).cuda() for a in init) + (torch.full((2,), SENT_CNT, dtype=torch.int32, device="cuda"),)
    dev = [torch.from_numpy(a).cuda() for a in (prev, nxt, features, counts, valid)]
    res = fd.track_lk(dev[0], dev[1], dev[2], counts=dev[3], valid=dev[4], out=out, **kw)
    torch.cuda.synchronize()
    assert res.xy is out[0]
    same(res, exp)
    # host pointers: the same through the staging buffers (fresh outputs are zeros)
    same(fd.track_lk(prev, nxt, features, counts=counts, valid=valid, **kw),
         R.flow_ref(prev, nxt, features, counts=counts, valid=valid, **kw))


@pytest.mark.parametrize("kw", [dict(max_iters=1), dict(epsilon=1e6), dict(max_iters=100, epsilon=1e-6)])
def test_termination(fd, canvas, features, kw):
    prev, nxt = view(canvas), half_shift(canvas, 0, 0)
    kw = dict(dict(levels=2, half_window=6, min_eigen=1e-4, counts=COUNTS), **kw)
    exp = R.flow_ref(prev, nxt, features, **kw)
    same(fd.track_lk(prev, nxt, features, **kw), exp)
    assert (exp[1] == 1).sum() >= 10


def test_forward_backward_and_max_error(fd, canvas, features):
    """An occlusion patch planted in `next` over some features: the forward-backward check and max_error
    reject there and accept elsewhere."""
    prev, nxt = view(canvas), view(canvas, 1, 1).copy()
    occ = np.random.default_rng(8).integers(0, 256, (2, 40, 50), dtype=np.uint8)
    nxt[:, 20:60, 30:80] = occ
    kw = dict(counts=COUNTS, levels=3, half_window=7, max_iters=20, min_eigen=1e-4)
    plain = R.flow_ref(prev, nxt, features, **kw)
    for extra in (dict(fb_max_dist=0.5), dict(max_error=6.0), dict(fb_max_dist=0.25, max_error=8.0), dict(fb_max_dist=0.0)):
        exp = R.flow_ref(prev, nxt, features, **kw, **extra)
        same(fd.track_lk(prev, nxt, features, **kw, **extra), exp)
        if extra.get("fb_max_dist", 0) > 0:
            assert (exp[1] == 5).any() and ((exp[1] == 1) & (plain[1] == 1)).any()
        if "max_error" in extra:
            assert (exp[1] == 6).any()
    assert ((plain[1] == 1).sum(1) == plain[3]).all()


def test_guess_recovers_a_large_shift(fd, canvas, features):
    """A shift of (14, -12) is beyond one level's reach for most features; the guess brings it within it."""
    prev, nxt = view(canvas), view(canvas, 14, -12)
    xy = features[:, :20]
    kw = dict(levels=1, half_window=7, max_iters=20, min_eigen=1e-4)
    guess = (xy + np.array([13.0, -11.5], np.float32)).astype(np.float32)
    exp = R.flow_ref(prev, nxt, xy, guess=guess, **kw)
    same(fd.track_lk(prev, nxt, xy, guess=guess, **kw), exp)
    none = R.flow_ref(prev, nxt, xy, **kw)
    same(fd.track_lk(prev, nxt, xy, **kw), none)

    def hits(o):
        return ((o[1] == 1) & (np.abs(o[0] - xy - np.array([14, -12], np.float32)).max(-1) < 0.1)).sum()

    assert hits(exp) >= 35 and hits(none) <= 15


def test_device_chain(fd, oracle, image_png):
    """detect_points -> build_pyramid x 2 -> track_lk -> detect_points(prior = survivors) on device tensors:
    the survivors' boolean mask is already the concatenated prior layout."""
    torch = pytest.importorskip("torch")
    prev_h = np.ascontiguousarray(image_png[24:264, 24:344])
    next_h = np.ascontiguousarray(image_png[26:266, 21:341])  # content moves by (3, -2)
    prev, nxt = torch.from_numpy(prev_h[None]).cuda(), torch.from_numpy(next_h[None]).cuda()
    det = fd.detect_points("shi_tomasi", prev, 60, 15, 40.0)
    p0, p1 = fd.build_pyramid(prev, 3), fd.build_pyramid(nxt, 3)
    res = fd.track_lk(p0, p1, det.xy, counts=det.counts, levels=3, min_eigen=1e-4, fb_max_dist=0.5)
    torch.cuda.synchronize()
    n = int(det.counts[0]) & 0x01FFFFFF
    feat = det.xy[0, :n].cpu().numpy()
    exp = R.flow_ref(prev_h, next_h, feat[None], levels=3, min_eigen=1e-4, fb_max_dist=0.5)
    got = (res.xy[:, :n].cpu().numpy(), res.status[:, :n].cpu().numpy(), res.err[:, :n].cpu().numpy(), res.counts.cpu().numpy())
    for g, e in zip(got, exp):
        assert np.array_equal(g.view(np.uint8), e.view(np.uint8))
    assert exp[3][0] >= 40
    keep = res.status[0, :n] == 1
    prior = res.xy[0, :n][keep].cpu().numpy()
    top = fd.detect_points("shi_tomasi", nxt, 60, 15, 40.0, prior=[prior])
    torch.cuda.synchronize()
    want, _ = oracle.detect(1, next_h, 15, 40.0, 60, prior=exp[0][0][exp[1][0] == 1], sort_mode=0)
    assert np.array_equal(top.features(0), want)


def test_graph_capture(fd, canvas, features):
    torch = pytest.importorskip("torch")
    frames = [torch.from_numpy(view(canvas)).cuda(), torch.from_numpy(view(canvas, 1, -1)).cuda()]
    xy = torch.from_numpy(features).cuda()
    cn = torch.from_numpy(COUNTS).cuda()
    out = (torch.empty((2, 40, 2), dtype=torch.float32, device="cuda"), torch.empty((2, 40), dtype=torch.uint8, device="cuda"),
           torch.empty((2, 40), dtype=torch.float32, device="cuda"), torch.empty((2,), dtype=torch.int32, device="cuda"))
    kw = dict(levels=3, half_window=5, max_iters=10, min_eigen=1e-4, fb_max_dist=1.0)

    def chain():
        p0, p1 = fd.build_pyramid(frames[0], 3), fd.build_pyramid(frames[1], 3)
        fd.track_lk(p0, p1, xy, counts=cn, out=out, **kw)
        return p0, p1

    chain()  # sizes the workspace
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        keep = chain()
    for shift in ((2, 0), (0, -2)):  # new contents in the same tensors
        host = view(canvas, *shift)
        frames[1].copy_(torch.from_numpy(host))
        for o, v in zip(out, (SENT_XY, SENT_ST, SENT_ERR, SENT_CNT)):
            o.fill_(v)
        g.replay()
        torch.cuda.synchronize()
        init = (np.full((2, 40, 2), SENT_XY, np.float32), np.full((2, 40), SENT_ST, np.uint8), np.full((2, 40), SENT_ERR, np.float32))
        exp = R.flow_ref(view(canvas), host, features, counts=COUNTS, init=init, **kw)
        same(fd.FlowResult(*out), exp)
    del g, keep


def test_bad_arguments(fd, canvas, features):
    from feature_detector_amd import _lib
    from feature_detector_amd._lib import fd_flow_opts

    prev, nxt = view(canvas), view(canvas, 1, 0)
    for kw in ({"levels": 0}, {"levels": 7}, {"half_window": 0}, {"half_window": 11}, {"max_iters": 0}, {"max_iters": 101},
               {"epsilon": 0.0}, {"epsilon": float("nan")}, {"min_eigen": -1.0}, {"min_eigen": float("inf")},
               {"fb_max_dist": float("nan")}, {"max_error": float("inf")}):
        with pytest.raises(fd.FdError) as e:
            fd.track_lk(prev, nxt, features, **kw)
        assert str(e.value).strip()
    with pytest.raises(fd.FdError):
        fd.build_pyramid(np.zeros((1, 8, 40), np.uint8), 5)  # the top level would have no row
    with pytest.raises(fd.FdError):
        fd.build_pyramid(prev, 0)
    # through the C ABI: NULL arrays, a negative stride (each with a message); stride 0 only zeroes the counts
    L, ctx = fd.load(), fd.default_context()
    ctx.set_stream(None)
    pyr = fd.build_pyramid(prev, 2, device_out=True)
    opts = fd_flow_opts(3, 5, 0.01, 1e-4, -1.0, -1.0)
    xy = np.ascontiguousarray(features)
    oxy, ost, cnt = np.zeros((2, 40, 2), np.float32), np.zeros((2, 40), np.uint8), np.full((2,), SENT_CNT, np.int32)
    p = lambda a: None if a is None else ctypes.c_void_p(a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data)  # noqa: E731

    def call(prev_p, xy_a, stride, oxy_a, ost_a):
        return L.fd_flow_lk(ctx.ptr, 2, ROWS, COLS, 2, ctypes.byref(opts), p(prev_p), p(pyr.data), p(xy_a), None, None, stride,
                            None, p(oxy_a), p(ost_a), None, p(cnt), 0)

    for args in ((None, xy, 40, oxy, ost), (pyr.data, None, 40, oxy, ost), (pyr.data, xy, 40, None, ost),
                 (pyr.data, xy, 40, oxy, None), (pyr.data, xy, -1, oxy, ost)):
        with pytest.raises(fd.FdError) as e:
            _lib.check(ctx.ptr, call(*args))
        assert str(e.value).strip()
    assert call(pyr.data, xy, 0, oxy, ost) == 0 and cnt.tolist() == [0, 0] and not ost.any()
    assert L.fd_flow_lk(None, 2, ROWS, COLS, 2, ctypes.byref(opts), p(pyr.data), p(pyr.data), p(xy), None, None, 40, None,
                        p(oxy), p(ost), None, None, 0) == _lib.FD_ERR_INVALID
