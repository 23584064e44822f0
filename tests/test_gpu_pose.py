"""fd_pose_recover and fd_triangulate on the GPU against tests/pose_ref.py: every output exactly (the pose as
uint64 bit patterns, the points as uint32, the bytes, counts and choice), through the C ABI into
sentinel-guarded buffers, with host and with device pointers; then the Python wrappers, graph capture and the
verify -> refit -> recover chain."""
import ctypes

import numpy as np
import pytest

import pose_ref as P
import ransac_ref as R
import refit_ref as F

pytestmark = pytest.mark.gpu

GUARD = 32
SENT_POSE, SENT_CH, SENT_PT, SENT_VAL, SENT_CNT = -123.25, -9, -77.5, 0xAB, -7
SENTS = (SENT_POSE, SENT_CH, SENT_PT, SENT_VAL, SENT_CNT)
FILL = (SENT_PT, SENT_VAL)
CASES = dict(P.all_cases())


@pytest.fixture(scope="module")
def fd():
    import feature_detector_amd as fd

    fd.load()
    return fd


@pytest.fixture(scope="module")
def ctx(fd):
    return fd.default_context()


def call(fd, ctx, case, pose=None, device=False, skip=(), use_inlier=True):
    """fd_pose_recover (pose None) or fd_triangulate (pose [B, 12]) through the C ABI. Outputs sit in the middle
    of sentinel-filled buffers (GUARD elements on either side, checked here); returns (pose, choice, points,
    valid, counts) as numpy, unwritten slots sentinel (fd_triangulate leaves pose and choice alone)."""
    from feature_detector_amd._lib import fd_pose_opts

    q, t = case["q"], case["t"]
    B, S, T = q.shape[0], q.shape[1], t.shape[1]
    opts = fd_pose_opts(*case["cam_q"], *case["cam_t"], case["max_depth"], case["min_parallax"])
    outs = [np.full(B * 12 + 2 * GUARD, SENT_POSE, np.float64), np.full(B + 2 * GUARD, SENT_CH, np.int32),
            np.full(B * S * 3 + 2 * GUARD, SENT_PT, np.float32), np.full(B * S + 2 * GUARD, SENT_VAL, np.uint8),
            np.full(B + 2 * GUARD, SENT_CNT, np.int32)]
    opt = lambda a, dt: None if a is None else np.ascontiguousarray(a, dt)
    given = case["in_model"] if pose is None else pose
    ins = [np.ascontiguousarray(q, np.float32) if q.size else np.zeros(2, np.float32), opt(case["counts"], np.int32),
           np.ascontiguousarray(t, np.float32) if t.size else np.zeros(2, np.float32), opt(case["idx"], np.int32),
           opt(case["valid"], np.uint8), np.ascontiguousarray(given, np.float64),
           (np.ascontiguousarray(case["in_inlier"], np.uint8) if S else np.zeros(1, np.uint8)) if use_inlier else None]
    if device:
        import torch

        ins = [None if a is None else torch.from_numpy(a).cuda() for a in ins]
        outs = [torch.from_numpy(a).cuda() for a in outs]
        ctx.set_stream(torch.cuda.current_stream(ctx.device).cuda_stream)
        base, size = (lambda a: a.data_ptr()), (lambda a: a.element_size())
    else:
        ctx.set_stream(None)
        base, size = (lambda a: a.ctypes.data), (lambda a: a.itemsize)
    ip = [None if a is None else ctypes.c_void_p(base(a)) for a in ins]
    op = [None if k in skip else ctypes.c_void_p(base(a) + GUARD * size(a)) for k, a in enumerate(outs)]
    L = fd.load()
    if pose is None:
        rc = L.fd_pose_recover(ctx.ptr, B, ctypes.byref(opts), ip[0], ip[1], S, ip[2], T, ip[3], ip[4], ip[5], ip[6],
                               op[0], op[1], op[2], op[3], op[4], 1 if device else 0)
    else:
        rc = L.fd_triangulate(ctx.ptr, B, ctypes.byref(opts), ip[0], ip[1], S, ip[2], T, ip[3], ip[4], ip[5], ip[6],
                              op[2], op[3], op[4], 1 if device else 0)
    assert rc == 0, L.fd_last_error(ctx.ptr)
    if device:
        torch.cuda.synchronize()
        outs = [a.cpu().numpy() for a in outs]
    for a, s in zip(outs, SENTS):
        assert np.all(a[:GUARD] == s) and np.all(a[-GUARD:] == s), "a write outside the output"
    return (outs[0][GUARD:-GUARD].reshape(B, 12), outs[1][GUARD:-GUARD], outs[2][GUARD:-GUARD].reshape(B, S, 3),
            outs[3][GUARD:-GUARD].reshape(B, S), outs[4][GUARD:-GUARD])


def same(got, exp, what):
    for k, (g, e) in enumerate(zip(got, exp)):
        assert g.dtype == e.dtype and g.shape == e.shape, (what, k)
        assert np.array_equal(g.view(np.uint8), e.view(np.uint8)), (what, k, g, e)


def check(fd, ctx, case, sides=(False, True)):
    """fd_pose_recover with host and with device pointers equals the restatement bit for bit, and fd_triangulate
    with the restatement's pose gives the same points. Returns the restatement's outputs."""
    exp = P.run_pose(case, fill=FILL)
    tri = P.run_triangulate(case, exp[0], fill=FILL)
    for device in sides:
        same(call(fd, ctx, case, device=device), exp, ("pose", device))
        same(call(fd, ctx, case, pose=exp[0], device=device)[2:], tri, ("triangulate", device))
    if np.all(exp[1] >= 0):
        same(tri, exp[2:], "the winner's points are the triangulation of its pose")
    return exp


@pytest.mark.parametrize("stride", [8, 255, 256, 257, 513])
def test_strides(fd, ctx, stride):
    """n = 8 at stride 8, and strides on both sides of one, two and three trips of the 256-thread walk (a ragged
    last chunk of fd_triangulate's grid); two different cameras, a quarter outliers."""
    exp = check(fd, ctx, CASES[f"stride-{stride}"])
    assert exp[1][0] >= 0 and exp[4][0] == stride - stride // 4


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_each_choice(fd, ctx, k):
    assert check(fd, ctx, CASES[f"choice-{k}"])[1][0] == k


def test_batch_zero_model_short_count_full(fd, ctx):
    exp = check(fd, ctx, CASES["batch"])
    assert exp[1][0] == -1 and not exp[0][0].any() and exp[4][0] == 0 and exp[1][1] >= 0 and exp[1][2] >= 0
    assert np.all(exp[3][0] == 0) and np.all(exp[3][1, 60:] == SENT_VAL) and np.all(exp[2][1, 60:] == SENT_PT)


def test_match_index_valid_inlier_bytes_and_non_finite(fd, ctx):
    """match_idx with -1, out-of-range and repeated entries, pair_valid bytes 0..6, in_inlier bytes 0, 2, 0xFF,
    NaN and inf coordinates; batch 3 with counts. Then without pair_valid, and without match_idx."""
    case = CASES["holes"]
    exp = check(fd, ctx, case)
    assert exp[4].min() >= 20 and not exp[3][:, 5:9].any() and not exp[3][0, 30:34].any()
    check(fd, ctx, dict(case, valid=None))
    check(fd, ctx, dict(case, idx=None, t=np.ascontiguousarray(np.concatenate([case["t"], case["t"][:, :15]], 1))))


def test_tie_no_pose_and_pure_rotation(fd, ctx):
    det = []
    exp = P.run_pose(CASES["tie"], detail=det)
    top = sorted(det[0])[-2:]
    assert top[0] == top[1] == 32 and exp[1][0] == det[0].index(32)
    check(fd, ctx, CASES["tie"])
    for name in ("count0", "rotation", "nonfinite-model"):
        exp = check(fd, ctx, CASES[name])
        assert exp[1][0] == -1 and exp[4][0] == 0 and not exp[0].any() and not exp[3].any() and not exp[2].any(), name


@pytest.mark.parametrize("name", ["depth", "parallax"])
def test_depth_and_parallax_limits(fd, ctx, name):
    """max_depth and min_parallax each exclude some, not all, of the planted inliers."""
    case = CASES[name]
    exp = check(fd, ctx, case)
    free = P.run_pose(dict(case, max_depth=P.MAX_DEPTH, min_parallax=0.0))
    assert 0 < exp[4][0] < free[4][0] == case["in_inlier"].sum()


def test_triangulate_all_pairs_and_scaled_translation(fd, ctx):
    """in_inlier NULL (every correspondence, outliers included), and a pose whose t has length 2.5: the points
    scale with it."""
    case = CASES["stride-257"]
    pose = P.run_pose(case)[0]
    big = pose.copy()
    big[:, 9:] *= 2.5
    for device in (False, True):
        for p in (pose, big):
            exp = P.triangulate_ref(case["q"], case["t"], p, None, fill=FILL, **P._opts(case))
            same(call(fd, ctx, case, pose=p, device=device, use_inlier=False)[2:], exp, device)
    a = P.run_triangulate(case, pose)
    b = P.run_triangulate(case, big)
    assert np.array_equal(a[1], b[1]) and np.allclose(b[0], 2.5 * a[0], rtol=1e-6)
    assert P.triangulate_ref(case["q"], case["t"], pose, None, **P._opts(case))[2][0] > a[2][0]


def test_empty_stride_and_skipped_outputs(fd, ctx):
    empty = dict(CASES["stride-8"], q=np.zeros((2, 0, 2), np.float32), t=np.zeros((2, 5, 2), np.float32),
                 in_model=np.ones((2, 9)), in_inlier=np.zeros((2, 0), np.uint8))
    for device in (False, True):
        pose, ch, pts, val, cnt = call(fd, ctx, empty, device=device)
        assert not pose.any() and ch.tolist() == [-1, -1] and cnt.tolist() == [0, 0]
        out = call(fd, ctx, empty, pose=np.ones((2, 12)), device=device)
        assert out[4].tolist() == [0, 0] and np.all(out[0] == SENT_POSE)
    case = CASES["batch"]
    exp = P.run_pose(case, fill=FILL)
    for device in (False, True):
        for skip in ((0, 1, 2, 3), (2, 3, 4), (0, 1, 2, 3, 4), (3,)):
            got = call(fd, ctx, case, device=device, skip=skip)
            for k in range(5):
                if k in skip:
                    assert np.all(got[k] == SENTS[k]), (skip, k)
                else:
                    same(got[k:k + 1], exp[k:k + 1], (skip, k))
        got = call(fd, ctx, case, pose=exp[0], device=device, skip=(2, 4))
        assert np.array_equal(got[3], P.run_triangulate(case, exp[0], fill=FILL)[1]) and np.all(got[2] == SENT_PT)


def test_rejected_arguments(fd, ctx):
    from feature_detector_amd._lib import FD_ERR_INVALID, fd_pose_opts

    L = fd.load()
    q = np.zeros((1, 8, 2), np.float32)
    m, inl = np.zeros(12), np.zeros(8, np.uint8)
    pq, pm, pi = (ctypes.c_void_p(a.ctypes.data) for a in (q, m, inl))
    good = dict(fx_q=500.0, fy_q=500.0, cx_q=320.0, cy_q=240.0, fx_t=-500.0, fy_t=500.0, cx_t=0.0, cy_t=0.0, max_depth=float("inf"),
                min_parallax=0.0)

    def rc(fn="fd_pose_recover", batch=1, qs=8, ts=8, q=pq, t=pq, im=pm, ii=pi, idx=None, opts=True, **kw):
        o = fd_pose_opts(**{**good, **kw})
        po = ctypes.byref(o) if opts else None
        if fn == "fd_pose_recover":
            return L.fd_pose_recover(ctx.ptr, batch, po, q, None, qs, t, ts, idx, None, im, ii, None, None, None, None, None, 0)
        return L.fd_triangulate(ctx.ptr, batch, po, q, None, qs, t, ts, idx, None, im, ii, None, None, None, 0)

    ctx.set_stream(None)
    for fn in ("fd_pose_recover", "fd_triangulate"):
        assert rc(fn) == 0 and rc(fn, max_depth=1e-3, min_parallax=1.0) == 0
        bads = [dict(batch=0), dict(qs=-1), dict(ts=-1), dict(ts=7), dict(q=None), dict(t=None), dict(im=None), dict(opts=False),
                dict(max_depth=0.0), dict(max_depth=-1.0), dict(max_depth=float("nan")), dict(min_parallax=-0.5),
                dict(min_parallax=1.5), dict(min_parallax=float("nan"))]
        for name in ("fx_q", "fy_q", "cx_q", "cy_q", "fx_t", "fy_t", "cx_t", "cy_t"):
            bads += [{name: float("nan")}, {name: float("inf")}] + ([{name: 0.0}] if name[0] == "f" else [])
        for bad in bads:
            assert rc(fn, **bad) == FD_ERR_INVALID, (fn, bad)
        idx = np.zeros((1, 8), np.int32)
        assert rc(fn, ts=7, idx=ctypes.c_void_p(idx.ctypes.data)) == 0
    assert rc("fd_pose_recover", ii=None) == FD_ERR_INVALID and rc("fd_triangulate", ii=None) == 0


def test_python_wrappers_host_device_and_out(fd):
    torch = pytest.importorskip("torch")
    case = CASES["stride-257"]
    q, t = case["q"], case["t"]
    K = np.array([[case["cam_q"][0], 0, case["cam_q"][2]], [0, case["cam_q"][1], case["cam_q"][3]], [0, 0, 1]])
    given = fd.GeometryResult(case["in_model"], case["in_inlier"], None, None)
    exp = P.run_pose(case)
    tri = P.triangulate_ref(q, t, exp[0], None, **P._opts(case))
    host = fd.recover_pose(q, t, given, K, case["cam_t"])
    same((host.pose, host.choice, host.points, host.valid, host.counts), exp, "host")
    ht = fd.triangulate(q, t, host.pose, K, case["cam_t"])
    same((ht.points, ht.valid, ht.counts), tri, "host triangulate")
    dq, dt = torch.from_numpy(q).cuda(), torch.from_numpy(t).cuda()
    dgiven = fd.GeometryResult(torch.from_numpy(case["in_model"]).cuda(), torch.from_numpy(case["in_inlier"]).cuda(), None, None)
    dev = fd.recover_pose(dq, dt, dgiven, K, case["cam_t"])
    dtri = fd.triangulate(dq, dt, dev.pose, K, case["cam_t"], inliers=dgiven.inliers)
    out = (torch.full((1, 12), 5.0, dtype=torch.float64, device="cuda"), torch.full((1,), 5, dtype=torch.int32, device="cuda"),
           torch.full((1, 257, 3), 5.0, dtype=torch.float32, device="cuda"), torch.full((1, 257), 5, dtype=torch.uint8, device="cuda"),
           torch.full((1,), 5, dtype=torch.int32, device="cuda"))
    again = fd.recover_pose(dq, dt, dgiven, K, case["cam_t"], out=out)
    torch.cuda.synchronize()
    assert again.pose is out[0] and again.points is out[2]
    for res in (dev, again):
        same([x.cpu().numpy() for x in (res.pose, res.choice, res.points, res.valid, res.counts)], exp, "device")
    same([x.cpu().numpy() for x in (dtri.points, dtri.valid, dtri.counts)], exp[2:], "device triangulate")
    assert np.array_equal(host.rotation(0), exp[0][0, :9].reshape(3, 3)) and np.array_equal(host.translation(0), exp[0][0, 9:])
    with pytest.raises(ValueError):
        fd.recover_pose(q, t, given, np.array([[500.0, 0.1, 320], [0, 500, 240], [0, 0, 1]]))
    with pytest.raises(ValueError):
        fd.triangulate(q, t, host.pose, (500.0, 0.0, 1.0, 1.0))


def test_graph_capture(fd):
    torch = pytest.importorskip("torch")
    a, b = CASES["choice-1"], CASES["choice-2"]
    dq, dt = torch.from_numpy(a["q"]).cuda(), torch.from_numpy(a["t"]).cuda()
    given = fd.GeometryResult(torch.from_numpy(a["in_model"]).cuda(), torch.from_numpy(a["in_inlier"]).cuda(), None, None)
    S = a["q"].shape[1]
    out = (torch.empty((1, 12), dtype=torch.float64, device="cuda"), torch.empty((1,), dtype=torch.int32, device="cuda"),
           torch.empty((1, S, 3), dtype=torch.float32, device="cuda"), torch.empty((1, S), dtype=torch.uint8, device="cuda"),
           torch.empty((1,), dtype=torch.int32, device="cuda"))
    tout = tuple(torch.empty_like(o) for o in out[2:])
    fd.recover_pose(dq, dt, given, P.CAM, out=out)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        res = fd.recover_pose(dq, dt, given, P.CAM, out=out)
        fd.triangulate(dq, dt, res.pose, P.CAM, inliers=given.inliers, out=tout)
    dq.copy_(torch.from_numpy(b["q"]))
    dt.copy_(torch.from_numpy(b["t"]))
    given.model.copy_(torch.from_numpy(b["in_model"]))
    given.inliers.copy_(torch.from_numpy(b["in_inlier"]))
    exp = P.run_pose(b)
    for _ in range(2):
        for o, v in zip(out + tout, SENTS + SENTS[2:]):
            o.fill_(v)
        g.replay()
        torch.cuda.synchronize()
        same([o.cpu().numpy() for o in out], exp, "replay")
        same([o.cpu().numpy() for o in tout], exp[2:], "replay triangulate")
    assert exp[1][0] == 2
    del g


def test_verify_refit_recover_chain(fd):
    """verify_geometry -> refit_geometry -> recover_pose on device tensors against the three restatements
    composed (a scene of tests/test_pose_host.py's accuracy list); the pose is close to the planted one."""
    torch = pytest.importorskip("torch")
    sc = P.scene(5, n=96, outliers=24)
    q, t = sc["q"][None], sc["t"][None]
    kw = dict(model="fundamental", image_size=(R.ROWS, R.COLS))
    dq, dt = torch.from_numpy(q).cuda(), torch.from_numpy(t).cuda()
    ver = fd.verify_geometry(dq, dt, hypotheses=F.HYP, seed=5, **kw)
    ref = fd.refit_geometry(dq, dt, ver, rounds=2, **kw)
    pose = fd.recover_pose(dq, dt, ref, P.CAM)
    torch.cuda.synchronize()
    ran = R.ransac_ref(q, t, model=R.FUNDAMENTAL, hypotheses=F.HYP, seed=5, center=F.CENTER, scale=F.SCALE)
    fit = F.refit_ref(q, t, ran[0], ran[1], model=R.FUNDAMENTAL, rounds=2, center=F.CENTER, scale=F.SCALE)
    exp = P.pose_ref(q, t, fit[0], fit[1])
    assert np.array_equal(ref.model.cpu().numpy().view(np.uint64), fit[0].view(np.uint64)) and fit[3][0] >= 1
    same([x.cpu().numpy() for x in (pose.pose, pose.choice, pose.points, pose.valid, pose.counts)], exp, "chain")
    assert exp[1][0] >= 0 and exp[4][0] >= 60
    assert P.rotation_angle(exp[0][0, :9], sc["R"]) < 1e-3 and P.direction_angle(exp[0][0, 9:], sc["t_vec"]) < 1e-2
