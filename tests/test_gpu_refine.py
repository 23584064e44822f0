"""fd_points_refine on the GPU against tests/refine_ref.py: every output exactly, positions as bit patterns.
Small frames (96 x 128, batch 2, stride 40, counts 40 and 17) keep the numpy restatement at milliseconds a feature."""
import ctypes
import functools

import numpy as np
import pytest

import refine_cases as C
import refine_ref as R

pytestmark = pytest.mark.gpu

ROWS, COLS, COUNTS = C.ROWS, C.COLS, C.COUNTS
SENT_XY, SENT_ST, SENT_CNT = -77.0, 99, -7


@pytest.fixture(scope="module")
def fd():
    import feature_detector_amd as fd

    fd.load()
    return fd


@functools.lru_cache(maxsize=None)
def main_case():
    """(frames, xy, valid, expected with sentinels in the unwritten slots, expected with zeros there)."""
    frames, corners = C.main_frames()
    xy = C.main_features(corners)
    valid = (np.random.default_rng(4).random((2, 40)) < 0.8).astype(np.uint8)
    init = (np.full((2, 40, 2), SENT_XY, np.float32), np.full((2, 40), SENT_ST, np.uint8))
    kw = dict(counts=COUNTS, valid=valid)
    return frames, xy, valid, R.refine_ref(frames, xy, init=init, **kw), R.refine_ref(frames, xy, **kw)


def same(res, exp):
    xy, st, cnt = (np.asarray(t.cpu()) if hasattr(t, "cpu") else np.asarray(t) for t in (res.xy, res.status, res.counts))
    exy, est, ecnt = exp
    assert np.array_equal(st, est), (st.tolist(), est.tolist())
    assert np.array_equal(xy.view(np.uint32), exy.view(np.uint32))
    assert np.array_equal(cnt, ecnt)


def test_expected_main_case_is_not_trivial():
    _, xy, valid, exp_sent, exp_zero = main_case()
    st = exp_sent[1]
    assert (st == 0).sum() == (valid[0] == 0).sum() + (valid[1, :17] == 0).sum() > 0
    assert (st[0] == 1).sum() >= 25 and (st[1, :17] == 1).sum() >= 3 and (st[1, 17:] == SENT_ST).all()
    moved = np.abs(exp_zero[0] - xy).max(-1)[exp_zero[1] == 1]
    assert (moved > 0.2).sum() >= 20  # a sub-pixel step really happened


def test_host_io_host_and_device_frames(fd):
    torch = pytest.importorskip("torch")
    frames, xy, valid, _, exp = main_case()
    same(fd.refine_points(frames, xy, counts=COUNTS, valid=valid), exp)
    same(fd.refine_points(torch.from_numpy(frames).cuda(), xy, counts=COUNTS, valid=valid), exp)


def test_device_io_out_sentinels_and_in_place(fd):
    torch = pytest.importorskip("torch")
    frames, xy, valid, exp_sent, exp_zero = main_case()
    dev = [torch.from_numpy(a).cuda() for a in (frames, xy, COUNTS, valid)]
    out = (torch.full((2, 40, 2), SENT_XY, dtype=torch.float32, device="cuda"),
           torch.full((2, 40), SENT_ST, dtype=torch.uint8, device="cuda"), torch.full((2,), SENT_CNT, dtype=torch.int32, device="cuda"))
    res = fd.refine_points(dev[0], dev[1], counts=dev[2], valid=dev[3], out=out)
    torch.cuda.synchronize()
    assert res.xy is out[0]
    same(res, exp_sent)
    assert np.array_equal(dev[1].cpu().numpy(), xy)  # the inputs are not touched
    # fresh outputs: zeros in the unwritten slots; host frames with device feature arrays
    same(fd.refine_points(dev[0], dev[1], counts=dev[2], valid=dev[3]), exp_zero)
    same(fd.refine_points(frames, dev[1], counts=dev[2], valid=dev[3]), exp_zero)
    # in place: out_xy is xy; the unwritten slots keep their positions
    pos = dev[1].clone()
    st = torch.full((2, 40), SENT_ST, dtype=torch.uint8, device="cuda")
    res = fd.refine_points(dev[0], pos, counts=dev[2], valid=dev[3], out=(pos, st, out[2]))
    torch.cuda.synchronize()
    assert res.xy is pos
    exy = exp_sent[0].copy()
    exy[1, 17:] = xy[1, 17:]
    same(res, (exy, exp_sent[1], exp_sent[2]))


def test_pyramid_as_frames_and_none_arguments(fd):
    torch = pytest.importorskip("torch")
    frames, xy, valid, _, exp = main_case()
    pyr = fd.build_pyramid(torch.from_numpy(frames).cuda(), 3)
    dxy = torch.from_numpy(xy).cuda()
    same(fd.refine_points(pyr, dxy, counts=torch.from_numpy(COUNTS).cuda(), valid=torch.from_numpy(valid).cuda()), exp)
    same(fd.refine_points(fd.build_pyramid(frames, 2), xy, counts=COUNTS, valid=valid), exp)  # a host pyramid
    # counts / valid None: every slot, on both io paths; a single frame without the batch axis
    full = R.refine_ref(frames, xy[:, :24])
    assert (full[1] != 0).all()
    same(fd.refine_points(frames, xy[:, :24]), full)
    same(fd.refine_points(pyr, dxy[:, :24]), full)
    one = R.refine_ref(frames[0], xy[0, :8])
    same(fd.refine_points(frames[0], xy[0, :8]), one)


def test_stride_zero(fd):
    from feature_detector_amd._lib import fd_refine_opts

    frames = main_case()[0]
    res = fd.refine_points(frames, np.zeros((2, 0, 2), np.float32))
    assert res.xy.shape == (2, 0, 2) and res.status.shape == (2, 0) and res.counts.tolist() == [0, 0]
    L, ctx = fd.load(), fd.default_context()
    ctx.set_stream(None)
    opts = fd_refine_opts(5, 20, 0.01, 1e-3, 5.0)
    oxy, ost, cnt = np.full((4,), SENT_XY, np.float32), np.full((4,), SENT_ST, np.uint8), np.full((2,), SENT_CNT, np.int32)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    rc = L.fd_points_refine(ctx.ptr, p(frames), 0, 2, ROWS, COLS, ctypes.byref(opts), p(oxy), None, None, 0, p(oxy), p(ost), p(cnt), 0)
    assert rc == 0 and cnt.tolist() == [0, 0] and (ost == SENT_ST).all() and (oxy == SENT_XY).all()


@pytest.mark.parametrize("r", range(1, 11))
def test_every_half_window(fd, r):
    """r = 1..10: ROUNDS = 1, 1, 1, 2, 2, 3, 4, 5, 6, 7, every instantiation of k_refine; 8 features each."""
    frames, xy, _, _, _ = main_case()
    sel = np.ascontiguousarray(xy[:, [0, 5, 13, 18, 24, 27, 33, 38]])
    kw = dict(half_window=r, max_iters=10, min_eigen=1e-4)
    exp = R.refine_ref(frames, sel, **kw)
    same(fd.refine_points(frames, sel, **kw), exp)
    assert (exp[1] == 1).any()


@functools.lru_cache(maxsize=None)
def status_case():
    """Frame 0: corners that lie just outside the frame (the iteration follows them out) and a constant block;
    frame 1: a long straight edge with a little noise. Features for every status."""
    outside = [(-1.5, 40.0, 0.3), (129.0, 60.3, 0.7), (60.0, -1.2, 0.4), (90.2, 97.0, 0.5), (40.3, 30.6, 0.2)]
    f0 = C.render_corners(ROWS, COLS, outside, seed=4)
    f0[60:96, 0:40] = 90
    f1 = np.full((ROWS, COLS), 60.0)
    f1[:, 64:] = 200.0
    f1 = np.clip(np.rint(f1 + np.random.default_rng(5).normal(0, 1.5, f1.shape)), 0, 255).astype(np.uint8)
    nan, inf = np.nan, np.inf
    xy0 = [(1, 40), (2, 41), (126, 60), (127, 61), (60, 1), (61, 2), (90, 94), (91, 95), (20, 78), (12.5, 80.25), (40, 31), (41.5, 30),
           (nan, 5), (5, inf), (-0.5, 5), (COLS - 0.5, 5), (5, ROWS - 0.5), (5, -inf), (40, 30), (40.25, 30.5)]
    xy1 = [(64, 48), (64.2, 70), (63.5, 30.2), (63, 12), (65, 85.5), (64, 20)] + [(30, 30 + i) for i in range(14)]
    xy = np.array([xy0, xy1], np.float32)
    valid = np.ones((2, 20), np.uint8)
    valid[0, 18] = valid[1, 7] = 0
    return np.stack([f0, f1]), xy, valid


def test_status_coverage(fd):
    frames, xy, valid = status_case()
    seen = set()
    for kw in (dict(min_eigen=1e-3), dict(min_eigen=0.0), dict(max_shift=0.25), dict(max_iters=1)):
        exp = R.refine_ref(frames, xy, valid=valid, **kw)
        same(fd.refine_points(frames, xy, valid=valid, **kw), exp)
        seen |= set(np.unique(exp[1]).tolist())
        if kw == dict(min_eigen=1e-3):
            assert exp[1][0, :8].tolist() == [2] * 8    # stepped out of the frame: caught by the next iteration's test
            assert exp[1][0, 8:10].tolist() == [3, 3] and exp[1][0, 12:18].tolist() == [2] * 6
        if kw == dict(min_eigen=0.0):
            assert (exp[1][1, :6] == 4).any()           # slides along the edge until it is max_shift away
        if kw == dict(max_shift=0.25):
            assert exp[1][0, 11] == 4 and exp[1][0, 19] == 1  # 1.2 px and 0.1 px off the corner
        if kw == dict(max_iters=1):                     # no test follows the last update: refined, outside the frame
            assert exp[1][0, 0] == 1 and exp[0][0, 0, 0] < 0
    assert seen == {0, 1, 2, 3, 4}


def test_frame_edges(fd):
    """Features in the frame's corners and within r of each edge (clamped reads), a 5 x 7 and a 1 x 1 frame with r = 10."""
    frames = main_case()[0]
    xs, ys = [0, 0.5, 3, 9.75, COLS - 10.5, COLS - 4.25, COLS - 1], [0, 0.75, 2, 10, ROWS - 9.5, ROWS - 3.5, ROWS - 1]
    xy = np.array([[x, y] for x in xs for y in ys], np.float32)
    xy = np.stack([xy, xy])
    for r in (5, 10):
        kw = dict(half_window=r, max_iters=8, min_eigen=1e-4)
        exp = R.refine_ref(frames, xy, **kw)
        same(fd.refine_points(frames, xy, **kw), exp)
        assert (exp[1] == 1).any()
    small = np.random.default_rng(9).integers(0, 256, (1, 5, 7), dtype=np.uint8)
    sxy = np.array([[[0, 0], [6, 4], [3, 2], [2.5, 1.25], [5.75, 3.5], [0.25, 3.9]]], np.float32)
    for r in (1, 10):
        exp = R.refine_ref(small, sxy, half_window=r, min_eigen=0.0)
        same(fd.refine_points(small, sxy, half_window=r, min_eigen=0.0), exp)
    dot = np.array([[[200]]], np.uint8)
    dxy = np.array([[[0, 0], [0.5, 0]]], np.float32)
    exp = R.refine_ref(dot, dxy, half_window=10, min_eigen=0.0)
    assert exp[1].tolist() == [[3, 2]]
    same(fd.refine_points(dot, dxy, half_window=10, min_eigen=0.0), exp)


def test_wide_sums(fd):
    """Random {0, 255} pixels with r = 10: single terms pass 2^31 and totals pass 2^32, so the int64 accumulation
    and the three-limb wave total are exercised."""
    img = (np.random.default_rng(0).integers(0, 2, (1, ROWS, COLS)) * 255).astype(np.uint8)
    xy = np.array([[[60.3, 40.7], [20, 20], [100.5, 70.25], [64, 48], [11, 84.5], [117.75, 11], [40.1, 60.9], [80, 30]]], np.float32)
    kw = dict(half_window=10, max_iters=4, min_eigen=0.0, max_shift=10.0)
    big_term = big_total = negative = False
    for p in xy[0]:
        trace = []
        R.refine_one(img[0].astype(np.int64), p, 10, 4, 0.01, 0.0, 10.0, trace=trace)
        for totals, term in trace:
            big_term |= term >= 2 ** 31
            big_total |= max(abs(t) for t in totals) >= 2 ** 32
            negative |= min(totals) <= -2 ** 32
    assert big_term and big_total and negative
    exp = R.refine_ref(img, xy, **kw)
    same(fd.refine_points(img, xy, **kw), exp)
    assert (exp[1] == 1).any()


def test_graph_capture(fd):
    torch = pytest.importorskip("torch")
    frames, xy, valid, _, _ = main_case()
    dfr, dxy = torch.from_numpy(frames).cuda(), torch.from_numpy(xy).cuda()
    cn, dv = torch.from_numpy(COUNTS).cuda(), torch.from_numpy(valid).cuda()
    out = (torch.empty((2, 40, 2), dtype=torch.float32, device="cuda"), torch.empty((2, 40), dtype=torch.uint8, device="cuda"),
           torch.empty((2,), dtype=torch.int32, device="cuda"))
    kw = dict(half_window=4, max_iters=10)
    fd.refine_points(dfr, dxy, counts=cn, valid=dv, out=out, **kw)  # one warm call of the shape
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        fd.refine_points(dfr, dxy, counts=cn, valid=dv, out=out, **kw)
    for step in (1, 2):  # new contents in the same tensors
        host_frames = np.ascontiguousarray(frames[::-1]) if step == 1 else frames
        host_xy = (xy + np.float32(0.25 * step)).astype(np.float32)
        dfr.copy_(torch.from_numpy(host_frames))
        dxy.copy_(torch.from_numpy(host_xy))
        for o, v in zip(out, (SENT_XY, SENT_ST, SENT_CNT)):
            o.fill_(v)
        g.replay()
        torch.cuda.synchronize()
        init = (np.full((2, 40, 2), SENT_XY, np.float32), np.full((2, 40), SENT_ST, np.uint8))
        same(fd.RefineResult(*out), R.refine_ref(host_frames, host_xy, counts=COUNTS, valid=valid, init=init, **kw))
    del g


def test_chain_detect_refine_track(fd, image_png):
    """detect_points -> refine_points on the detector's device xy and counts as they are -> track_lk on the result."""
    torch = pytest.importorskip("torch")
    import flow_ref

    prev_h = np.ascontiguousarray(image_png[24:264, 24:344])
    next_h = np.ascontiguousarray(image_png[26:266, 21:341])  # content moves by (3, -2)
    prev, nxt = torch.from_numpy(prev_h[None]).cuda(), torch.from_numpy(next_h[None]).cuda()
    det = fd.detect_points("shi_tomasi", prev, 60, 15, 40.0)
    ref = fd.refine_points(prev, det.xy, counts=det.counts)
    trk = fd.track_lk(prev, nxt, ref.xy, counts=det.counts, levels=3, min_eigen=1e-4)
    torch.cuda.synchronize()
    n = int(det.counts[0]) & 0x01FFFFFF
    feat = det.xy[0, :n].cpu().numpy()
    exp = R.refine_ref(prev_h, feat[None])
    assert n >= 40 and exp[2][0] >= 20 and np.array_equal(feat, np.rint(feat))
    assert np.array_equal(ref.xy[:, :n].cpu().numpy().view(np.uint32), exp[0].view(np.uint32))
    assert np.array_equal(ref.status[:, :n].cpu().numpy(), exp[1]) and ref.counts.cpu().numpy().tolist() == exp[2].tolist()
    assert not np.array_equal(exp[0][exp[1] == 1], feat[None][exp[1] == 1])
    texp = flow_ref.flow_ref(prev_h, next_h, exp[0], levels=3, min_eigen=1e-4)
    assert np.array_equal(trk.xy[:, :n].cpu().numpy().view(np.uint32), texp[0].view(np.uint32))
    assert np.array_equal(trk.status[:, :n].cpu().numpy(), texp[1]) and texp[3][0] >= 30


def test_bad_arguments(fd):
    frames, xy, _, _, _ = main_case()
    for kw in ({"half_window": 0}, {"half_window": 11}, {"max_iters": 0}, {"max_iters": 101}, {"epsilon": 0.0},
               {"epsilon": float("nan")}, {"min_eigen": -1.0}, {"min_eigen": float("inf")}, {"max_shift": 0.0},
               {"max_shift": float("inf")}, {"max_shift": float("nan")}):
        with pytest.raises(fd.FdError) as e:
            fd.refine_points(frames, xy, **kw)
        assert str(e.value).strip()
    from feature_detector_amd import _lib
    from feature_detector_amd._lib import fd_refine_opts

    L, ctx = fd.load(), fd.default_context()
    ctx.set_stream(None)
    opts = fd_refine_opts(5, 20, 0.01, 1e-3, 5.0)
    oxy, ost = np.zeros((2, 40, 2), np.float32), np.zeros((2, 40), np.uint8)
    p = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    for fr, o, x, ox, os_, stride, rows in ((None, opts, xy, oxy, ost, 40, ROWS), (frames, None, xy, oxy, ost, 40, ROWS),
                                            (frames, opts, None, oxy, ost, 40, ROWS), (frames, opts, xy, None, ost, 40, ROWS),
                                            (frames, opts, xy, oxy, None, 40, ROWS), (frames, opts, xy, oxy, ost, -1, ROWS),
                                            (frames, opts, xy, oxy, ost, 40, 0)):
        with pytest.raises(fd.FdError) as e:
            _lib.check(ctx.ptr, L.fd_points_refine(ctx.ptr, p(fr), 0, 2, rows, COLS, None if o is None else ctypes.byref(o), p(x), None,
                                                   None, stride, p(ox), p(os_), None, 0))
        assert str(e.value).strip()
