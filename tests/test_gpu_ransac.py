"""fd_ransac on the GPU against tests/ransac_ref.py: every output exactly (the model as uint64 bit patterns,
the mask, counts and best index), through the C ABI into sentinel-guarded buffers, with host and with device
pointers; then the property tests on planted scenes, which do not use the restatement."""
import ctypes

import numpy as np
import pytest

import ransac_ref as R

pytestmark = pytest.mark.gpu

GUARD = 32
SENT_MODEL, SENT_INL, SENT_CNT, SENT_BEST = -123.25, 0xAB, -7, -9
CENTER, SCALE = R.conditioning((R.ROWS, R.COLS))


@pytest.fixture(scope="module")
def fd():
    import feature_detector_amd as fd

    fd.load()
    return fd


@pytest.fixture(scope="module")
def ctx(fd):
    return fd.default_context()


def scenes(model, stride, batch, seed=0):
    """[batch, stride, 2] query and train positions of planted scenes (a quarter of each frame outliers)."""
    q, t = zip(*(R.planted_scene(model, 50 * seed + b, n=stride, outliers=stride // 4)[:2] for b in range(batch)))
    return np.stack(q), np.stack(t)


def call(fd, ctx, q, t, counts=None, idx=None, valid=None, device=False, skip=(), **opt):
    """fd_ransac through the C ABI. Outputs sit in the middle of sentinel-filled buffers (GUARD elements on
    either side, checked here); returns (model, inlier, counts, best) as numpy, unwritten slots sentinel."""
    from feature_detector_amd._lib import fd_ransac_opts

    B, S, T = q.shape[0], q.shape[1], t.shape[1]
    o = dict(model=R.FUNDAMENTAL, hypotheses=256, seed=0, threshold=1.0, center=CENTER, scale=SCALE)
    o.update(opt)
    opts = fd_ransac_opts(o["model"], o["hypotheses"], o["seed"], o["threshold"], o["center"][0], o["center"][1], o["scale"])
    outs = [np.full(B * 9 + 2 * GUARD, SENT_MODEL, np.float64), np.full(B * S + 2 * GUARD, SENT_INL, np.uint8),
            np.full(B + 2 * GUARD, SENT_CNT, np.int32), np.full(B + 2 * GUARD, SENT_BEST, np.int32)]
    ins = [np.ascontiguousarray(q, np.float32) if q.size else np.zeros(2, np.float32),  # (an empty tensor has no pointer)
           None if counts is None else np.ascontiguousarray(counts, np.int32),
           np.ascontiguousarray(t, np.float32), None if idx is None else np.ascontiguousarray(idx, np.int32),
           None if valid is None else np.ascontiguousarray(valid, np.uint8)]
    if device:
        import torch

        ins = [None if a is None else torch.from_numpy(a).cuda() for a in ins]
        outs = [torch.from_numpy(a).cuda() for a in outs]
        ctx.set_stream(torch.cuda.current_stream(ctx.device).cuda_stream)
        base = lambda a: a.data_ptr()
    else:
        ctx.set_stream(None)
        base = lambda a: a.ctypes.data
    ip = [None if a is None else ctypes.c_void_p(base(a)) for a in ins]
    size = (lambda a: a.element_size()) if device else (lambda a: a.itemsize)
    op = [None if k in skip else ctypes.c_void_p(base(a) + GUARD * size(a)) for k, a in enumerate(outs)]
    rc = fd.load().fd_ransac(ctx.ptr, B, ctypes.byref(opts), ip[0], ip[1], S, ip[2], T, ip[3], ip[4], op[0], op[1], op[2], op[3],
                             1 if device else 0)
    assert rc == 0, fd.load().fd_last_error(ctx.ptr)
    if device:
        torch.cuda.synchronize()
        outs = [a.cpu().numpy() for a in outs]
    for a, s in zip(outs, (SENT_MODEL, SENT_INL, SENT_CNT, SENT_BEST)):
        assert np.all(a[:GUARD] == s) and np.all(a[-GUARD:] == s), "a write outside the output"
    return (outs[0][GUARD:-GUARD].reshape(B, 9), outs[1][GUARD:-GUARD].reshape(B, S), outs[2][GUARD:-GUARD], outs[3][GUARD:-GUARD])


def check(fd, ctx, q, t, counts=None, idx=None, valid=None, sides=(False, True), **opt):
    """Host-pointer and device-pointer calls equal the restatement, bit for bit. Returns the restatement's outputs."""
    o = dict(model=R.FUNDAMENTAL, hypotheses=256, seed=0, threshold=1.0, center=CENTER, scale=SCALE)
    o.update(opt)
    exp = R.ransac_ref(q, t, counts, idx, valid, fill=SENT_INL, **o)
    for device in sides:
        got = call(fd, ctx, q, t, counts, idx, valid, device=device, **opt)
        assert np.array_equal(got[3], exp[3]), (device, got[3], exp[3])
        assert np.array_equal(got[2], exp[2]), (device, got[2], exp[2])
        assert np.array_equal(got[1], exp[1]), device
        assert np.array_equal(got[0].view(np.uint64), exp[0].view(np.uint64)), (device, got[0], exp[0])
    return exp


MODELS = [R.FUNDAMENTAL, R.HOMOGRAPHY]


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("n", [0, 3, 4, 7, 8, 9, 63, 64, 65, 257])
def test_correspondence_counts(fd, ctx, model, n):
    """n on both sides of the sample size (4, 8), of a wave and of the 256-entry LDS tile; batch 1."""
    q, t = scenes(model, max(n, 1) + 3, 1, seed=n)
    exp = check(fd, ctx, q, t, counts=[n], model=model, hypotheses=65, seed=n)
    assert (exp[3][0] >= 0) == (n >= R.SAMPLE[model])


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("hypotheses", [1, 63, 64, 65, 256, 1000])
def test_hypothesis_counts(fd, ctx, model, hypotheses):
    """Hypothesis counts around the 64-lane workgroup; batch 3 with a different count per frame."""
    q, t = scenes(model, 70, 3, seed=hypotheses)
    exp = check(fd, ctx, q, t, counts=[65, 9, 70], model=model, hypotheses=hypotheses, seed=hypotheses + 1)
    assert np.all(exp[3] >= 0)


@pytest.mark.parametrize("model", MODELS)
def test_ties_go_to_the_lowest_hypothesis(fd, ctx, model):
    q, t, _ = R.planted_scene(model, 0)
    detail = []
    exp = R.ransac_ref(q[None], t[None], model=model, center=CENTER, scale=SCALE, detail=detail)
    score, valid = detail[0]
    tied = np.flatnonzero(valid & (score == score[valid].max()))
    assert len(tied) >= 2 and exp[3][0] == tied[0]
    check(fd, ctx, q[None], t[None], model=model)


@pytest.mark.parametrize("model", MODELS)
def test_match_index_valid_bytes_and_non_finite(fd, ctx, model):
    """match_idx with -1, out-of-range and repeated train indices; pair_valid with every byte 0..6; a NaN
    and an inf coordinate; flag bits above bit 24 of a count; batch 3."""
    rng = np.random.default_rng(11)
    S, T = 90, 75
    q, t = scenes(model, S, 3, seed=3)
    t = np.ascontiguousarray(t[:, :T])
    idx = np.tile(np.arange(S, dtype=np.int32) % T, (3, 1))  # slots T.. repeat the train indices 0..
    idx[:, 5], idx[:, 6], idx[:, 7], idx[:, 8] = -1, T, -2 ** 31, 2 ** 31 - 1
    idx[1, 20:30] = 3
    valid = np.ones((3, S), np.uint8)
    valid[0, 10:24] = np.arange(14) % 7
    valid[2] = rng.integers(0, 7, S)
    q[0, 30, 0], q[0, 31, 1], t[0, 32, 0], t[0, 33, 1] = np.nan, np.inf, -np.inf, np.nan
    counts = np.array([S, 60 | (1 << 25) | (1 << 31), 77], np.uint32).view(np.int32)
    exp = check(fd, ctx, q, t, counts=counts, idx=idx, valid=valid, model=model, hypotheses=128, seed=5)
    assert exp[1][0, 5:9].sum() == 0 and exp[1][0, 30:32].sum() == 0 and np.all(exp[3] >= 0)
    check(fd, ctx, q, t, counts=counts, idx=idx, model=model, hypotheses=128, seed=5)
    check(fd, ctx, q, q.copy() + np.float32(1.5), counts=counts, valid=valid, model=model, hypotheses=128, seed=5)


def test_degenerate_inputs_have_no_model(fd, ctx):
    """All points identical (both models), q_xy == t_xy with F (rank below 8), collinear points with H."""
    rng = np.random.default_rng(2)
    same = np.tile(np.array([100.5, 200.25], np.float32), (1, 40, 1))
    pts = np.stack([rng.uniform(0, 639, 40), rng.uniform(0, 479, 40)], -1).astype(np.float32)[None]
    x = rng.integers(0, 300, 40).astype(np.float32)
    line = np.stack([x, 2 * x + 1], -1)[None]
    for model, q, t in ((R.FUNDAMENTAL, same, same), (R.HOMOGRAPHY, same, same), (R.FUNDAMENTAL, pts, pts.copy()),
                        (R.HOMOGRAPHY, line, pts)):
        exp = check(fd, ctx, q, t, model=model, hypotheses=64)
        assert exp[3][0] == -1 and exp[2][0] == 0 and not exp[1].any() and not exp[0].any()


@pytest.mark.parametrize("model", MODELS)
def test_slots_past_the_count_do_not_matter(fd, ctx, model):
    q, t = scenes(model, 80, 2, seed=7)
    counts = [50, 33]
    a = check(fd, ctx, q, t, counts=counts, model=model, hypotheses=64)
    q2, t2 = q.copy(), t.copy()
    for b, c in enumerate(counts):
        p = np.random.default_rng(b).permutation(80 - c) + c
        q2[b, c:], t2[b, c:] = q[b, p], t[b, p[::-1]]
    b2 = check(fd, ctx, q2, t2, counts=counts, model=model, hypotheses=64)
    for x, y in zip(a, b2):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))


def test_empty_stride_and_skipped_outputs(fd, ctx):
    q, t = np.zeros((2, 0, 2), np.float32), np.zeros((2, 5, 2), np.float32)
    for device in (False, True):
        m, inl, cnt, best = call(fd, ctx, q, t, device=device)
        assert not m.any() and cnt.tolist() == [0, 0] and best.tolist() == [-1, -1]
    q, t = scenes(R.HOMOGRAPHY, 40, 2)
    exp = R.ransac_ref(q, t, model=R.HOMOGRAPHY, hypotheses=64, center=CENTER, scale=SCALE)
    for device in (False, True):
        m, inl, cnt, best = call(fd, ctx, q, t, device=device, skip=(1, 2, 3), model=R.HOMOGRAPHY, hypotheses=64)
        assert np.array_equal(m.view(np.uint64), exp[0].view(np.uint64))
        assert np.all(inl == SENT_INL) and np.all(cnt == SENT_CNT) and np.all(best == SENT_BEST)


def test_rejected_arguments(fd, ctx):
    from feature_detector_amd._lib import FD_ERR_INVALID, fd_ransac_opts

    L = fd.load()
    q = np.zeros((1, 8, 2), np.float32)
    m = np.zeros(9)
    pq, pm = ctypes.c_void_p(q.ctypes.data), ctypes.c_void_p(m.ctypes.data)
    good = dict(model=0, hypotheses=16, seed=0, threshold=1.0, center_x=0.0, center_y=0.0, scale=1.0)

    def rc(batch=1, qs=8, ts=8, q=pq, t=pq, out=pm, idx=None, opts=True, **kw):
        o = fd_ransac_opts(**{**good, **kw})
        return L.fd_ransac(ctx.ptr, batch, ctypes.byref(o) if opts else None, q, None, qs, t, ts, idx, None, out, None, None, None, 0)

    ctx.set_stream(None)
    assert rc() == 0
    for bad in (dict(model=2), dict(model=-1), dict(hypotheses=0), dict(hypotheses=4097), dict(threshold=0.0),
                dict(threshold=-1.0), dict(threshold=float("nan")), dict(threshold=float("inf")), dict(center_x=float("nan")),
                dict(center_y=float("inf")), dict(scale=0.0), dict(scale=-1.0), dict(scale=float("inf")), dict(scale=float("nan")),
                dict(batch=0), dict(qs=-1), dict(ts=-1), dict(ts=7), dict(q=None), dict(t=None), dict(out=None), dict(opts=False)):
        assert rc(**bad) == FD_ERR_INVALID, bad
    idx = np.zeros((1, 8), np.int32)
    assert rc(ts=7, idx=ctypes.c_void_p(idx.ctypes.data)) == 0  # a shorter train set is fine with match_idx


def test_python_wrapper_host_and_device(fd):
    torch = pytest.importorskip("torch")
    q, t = scenes(R.FUNDAMENTAL, 64, 2, seed=1)
    exp = R.ransac_ref(q, t, model=R.FUNDAMENTAL, hypotheses=128, seed=9, threshold=1.5, center=CENTER, scale=SCALE)
    host = fd.verify_geometry(q, t, hypotheses=128, seed=9, threshold=1.5, image_size=(R.ROWS, R.COLS))
    dev = fd.verify_geometry(torch.from_numpy(q).cuda(), torch.from_numpy(t).cuda(), hypotheses=128, seed=9, threshold=1.5,
                             image_size=(R.ROWS, R.COLS))
    torch.cuda.synchronize()
    for res in (host, dev):
        got = [np.asarray(x.cpu()) if hasattr(x, "cpu") else x for x in (res.model, res.inliers, res.counts, res.best)]
        for g, e in zip(got, exp):
            assert g.dtype == e.dtype and np.array_equal(g.view(np.uint8), e.view(np.uint8))
    # the default conditioning: centre (0, 0), scale 1 / 256
    exp = R.ransac_ref(q[:1], t[:1], model=R.HOMOGRAPHY, hypotheses=64)
    res = fd.verify_geometry(q[0], t[0], model="homography", hypotheses=64)
    assert np.array_equal(res.model.view(np.uint64), exp[0].view(np.uint64)) and np.array_equal(res.inliers, exp[1])


def test_graph_capture(fd):
    torch = pytest.importorskip("torch")
    q, t = scenes(R.FUNDAMENTAL, 64, 2, seed=2)
    dq, dt = torch.from_numpy(q).cuda(), torch.from_numpy(t).cuda()
    cn = torch.tensor([64, 40], dtype=torch.int32, device="cuda")
    out = (torch.empty((2, 9), dtype=torch.float64, device="cuda"), torch.empty((2, 64), dtype=torch.uint8, device="cuda"),
           torch.empty((2,), dtype=torch.int32, device="cuda"), torch.empty((2,), dtype=torch.int32, device="cuda"))
    kw = dict(hypotheses=128, seed=4, image_size=(R.ROWS, R.COLS))
    fd.verify_geometry(dq, dt, counts=cn, out=out, **kw)  # sizes the workspace
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        fd.verify_geometry(dq, dt, counts=cn, out=out, **kw)
    q2, t2 = scenes(R.FUNDAMENTAL, 64, 2, seed=3)  # new contents in the same tensors
    dq.copy_(torch.from_numpy(q2))
    dt.copy_(torch.from_numpy(t2))
    for o, v in zip(out, (SENT_MODEL, SENT_INL, SENT_CNT, SENT_BEST)):
        o.fill_(v)
    g.replay()
    torch.cuda.synchronize()
    exp = R.ransac_ref(q2, t2, [64, 40], model=R.FUNDAMENTAL, hypotheses=128, seed=4, center=CENTER, scale=SCALE, fill=SENT_INL)
    for o, e in zip(out, exp):
        assert np.array_equal(o.cpu().numpy().view(np.uint8), e.view(np.uint8))
    del g


# ---- property tests, independent of the restatement ------------------------------------------------------
# The seeds are those tests/test_ransac_host.py confirms on the restatement (PROPERTY_SEEDS there).

@pytest.mark.parametrize("model,name", [(R.FUNDAMENTAL, "fundamental"), (R.HOMOGRAPHY, "homography")])
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_planted_scene(fd, model, name, seed):
    """n = 64, a quarter of the train positions random, 256 hypotheses, threshold 1.0: every planted inlier is
    flagged and lies within 1e-3 px of the returned pixel-coordinate model (for F one random outlier may
    lie within a pixel of its epipolar line, so false inliers are not asserted to be none)."""
    q, t, planted = R.planted_scene(model, seed)
    res = fd.verify_geometry(q, t, model=name, hypotheses=256, seed=seed, threshold=1.0, image_size=(R.ROWS, R.COLS))
    assert planted.sum() == 48 and np.all(res.inliers[0][planted] == 1)
    assert res.counts[0] == res.inliers[0].sum() and res.best[0] >= 0
    resid = R.pixel_residual(model, res.model[0], q, t)
    print("largest planted-inlier residual [px]:", resid[planted].max())
    assert resid[planted].max() < 1e-3
    if model == R.HOMOGRAPHY:
        assert not res.inliers[0][~planted].any()
