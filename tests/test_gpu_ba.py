"""fd_bundle_adjust on the GPU against tests/ba_ref.py: every output exactly (the poses as uint64 bit patterns, the
points as uint32, the inlier bytes, counts, cost bits and rounds), through the C ABI into sentinel-guarded buffers,
with host and with device pointers; then the Python wrapper, graph capture and the verify -> refit -> recover -> PnP
-> bundle adjustment chain."""
import ctypes
import functools

import numpy as np
import pytest

import ba_ref as B
import pnp_ref as P
import pose_ref as PO
import ransac_ref as R
import refit_ref as F

pytestmark = pytest.mark.gpu

GUARD = 32
SENTS = (-123.25, -77.5, 0xAB, -7, -5.5, -9)  # poses, points, inlier, counts, cost, rounds
DTYPES = (np.float64, np.float32, np.uint8, np.int32, np.float64, np.int32)
CASES = dict(B.all_cases())


@pytest.fixture(scope="module")
def fd():
    import feature_detector_amd as fd

    fd.load()
    return fd


@pytest.fixture(scope="module")
def ctx(fd):
    return fd.default_context()


@functools.lru_cache(maxsize=None)
def expected(name):
    """The restatement's outputs of a case, computed once (unwritten slots hold the sentinels)."""
    return B.run(CASES[name], fill_points=SENTS[1], fill_inlier=SENTS[2])


def call(fd, ctx, case, device=False, skip=(), alias=False):
    """fd_bundle_adjust through the C ABI. Outputs sit in the middle of sentinel-filled buffers (GUARD elements on
    either side, checked here); alias: out_poses and out_points are the in_poses and p_xyz arrays themselves.
    Returns the six outputs as numpy."""
    from feature_detector_amd._lib import fd_ba_opts

    poses, p, obs = case["poses"], case["p"], case["obs"]
    Bn, C, S, O = poses.shape[0], poses.shape[1], p.shape[1], obs.shape[2]
    opts = fd_ba_opts(case["rounds"], case["threshold"], *case["cam"], case["lam"], case["up"], case["down"])
    shapes = ((Bn, C, 12), (Bn, S, 3), (Bn, C, O), (Bn,), (Bn, 2), (Bn,))
    outs = [np.full(int(np.prod(s)) + 2 * GUARD, v, dt) for s, v, dt in zip(shapes, SENTS, DTYPES)]
    opt = lambda a, dt: None if a is None else np.ascontiguousarray(a, dt)  # noqa: E731
    some = lambda a, dt, k: np.ascontiguousarray(a, dt) if a.size else np.zeros(k, dt)  # noqa: E731
    ins = [np.ascontiguousarray(poses, np.float64), opt(case["fixed"], np.uint8), some(p, np.float32, 3), opt(case["p_valid"], np.uint8),
           opt(case["counts"], np.int32), some(obs, np.float32, 2), opt(case["obs_valid"], np.uint8)]
    if alias:  # the inputs live inside the output buffers
        outs[0][GUARD:GUARD + poses.size] = poses.reshape(-1)
        outs[1][GUARD:GUARD + p.size] = p.reshape(-1)
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
    if alias:
        ip[0], ip[2] = op[0], op[1]
    L = fd.load()
    rc = L.fd_bundle_adjust(ctx.ptr, Bn, C, ctypes.byref(opts), ip[0], ip[1], ip[2], ip[3], ip[4], S, ip[5], ip[6], O,
                            op[0], op[1], op[2], op[3], op[4], op[5], 1 if device else 0)
    assert rc == 0, L.fd_last_error(ctx.ptr)
    if device:
        torch.cuda.synchronize()
        outs = [a.cpu().numpy() for a in outs]
    for a, s in zip(outs, SENTS):
        assert np.all(a[:GUARD] == s) and np.all(a[-GUARD:] == s), "a write outside the output"
    return tuple(a[GUARD:-GUARD].reshape(s) for a, s in zip(outs, shapes))


def same(got, exp, what):
    for k, (g, e) in enumerate(zip(got, exp)):
        assert g.dtype == e.dtype and g.shape == e.shape, (what, k)
        assert np.array_equal(g.view(np.uint8), e.view(np.uint8)), (what, k, g, e)


def check(fd, ctx, name, sides=(False, True)):
    """Host and device pointers equal the restatement bit for bit. Returns the restatement's outputs."""
    exp = expected(name)
    for device in sides:
        same(call(fd, ctx, CASES[name], device=device), exp, (name, device))
    return exp


@pytest.mark.parametrize("n", [0, 1, 2, 255, 256, 257, 600])
def test_counts(fd, ctx, n):
    """n on both sides of one and two trips of the slot walk and of the 256 partials, three cameras."""
    exp = check(fd, ctx, f"n-{n}")
    if n >= 2:
        assert exp[5][0] >= 1 and exp[4][0, 1] < exp[4][0, 0]
    else:
        assert exp[5][0] == 0


@pytest.mark.parametrize("kind", ["1-held", "2", "7-free", "8-free", "8-held", "8-null"])
def test_cameras(fd, ctx, kind):
    """One held camera (nothing moves: its points have one observation each), two, R = 42, R = 48 (eight free cameras:
    49 columns in the pivot search, 48 lanes in the back substitution), structure-only with eight held cameras, and
    cam_fixed NULL (camera 0 alone is held)."""
    exp = check(fd, ctx, f"cams-{kind}")
    case = CASES[f"cams-{kind}"]
    if kind == "1-held":
        assert exp[5][0] == 0 and np.array_equal(exp[1].view(np.uint32), case["p"].view(np.uint32))
    else:
        assert exp[5][0] >= 1
    if kind in ("1-held", "8-held"):
        assert np.array_equal(exp[0].view(np.uint64), case["poses"].view(np.uint64))
    if kind == "8-free":
        assert all(not np.array_equal(exp[0][0, c], case["poses"][0, c]) for c in range(8))
    if kind == "8-null":
        assert np.array_equal(exp[0][0, 0], case["poses"][0, 0]) and not np.array_equal(exp[0][0, 1], case["poses"][0, 1])


@pytest.mark.parametrize("rounds", [1, 16])
def test_rounds(fd, ctx, rounds):
    exp = check(fd, ctx, f"rounds-{rounds}")
    assert 1 <= exp[5][0] <= rounds


def test_forced_rejection_then_accept(fd, ctx):
    """A damping far too small for the start: a trial is rejected, lambda grows by `up`, a later trial is accepted."""
    trace = []
    B.run(CASES["reject"], trace=trace)
    acc = [t[1] for t in trace[0]]
    assert not acc[0] and any(acc[1:])
    check(fd, ctx, "reject")


def test_singular_schur_system_keeps_the_state(fd, ctx):
    """One held camera, down = 1 and lambda = 1e-300 (1.0 + lambda == 1.0): the scale gauge is undamped, the Schur
    system fails the pivot test, every trial is invalid and the state is the given one bit for bit."""
    trace = []
    B.run(CASES["gauge"], trace=trace)
    assert all(not t[0] for t in trace[0])
    exp = check(fd, ctx, "gauge")
    case = CASES["gauge"]
    assert exp[5][0] == 0 and np.array_equal(exp[0].view(np.uint64), case["poses"].view(np.uint64))
    assert np.array_equal(exp[1].view(np.uint32), case["p"].view(np.uint32)) and exp[4][0, 0] == exp[4][0, 1]


def test_held_point_paths(fd, ctx):
    """A point seen once, one behind every camera, one whose two rays are parallel: none moves. Then every point held."""
    exp = check(fd, ctx, "held-points")
    case = CASES["held-points"]
    assert exp[5][0] >= 1
    assert np.array_equal(exp[1][0, :3].view(np.uint32), case["p"][0, :3].view(np.uint32))
    assert not np.array_equal(exp[1][0, 3:], case["p"][0, 3:]) and not exp[2][0, :, 1].any()
    exp = check(fd, ctx, "all-held")
    case = CASES["all-held"]
    assert exp[5][0] >= 1 and np.array_equal(exp[1].view(np.uint32), case["p"].view(np.uint32))
    assert not np.array_equal(exp[0][0, 1:], case["poses"][0, 1:])


def test_masks_non_finite_and_layout(fd, ctx):
    """p_valid and obs_valid with bytes other than 1, a NaN / inf in each coordinate place, counts below the stride
    with flag bits, o_stride > p_stride; then each mask absent."""
    exp = check(fd, ctx, "masks")
    case = CASES["masks"]
    assert not exp[2][0, :, 30:33].any() and not exp[2][0, 1, 33] and not exp[2][0, 2, 34]
    assert np.all(exp[2][0, :, 77:] == SENTS[2]) and np.all(exp[1][0, 77:] == np.float32(SENTS[1]))
    assert np.array_equal(exp[1][0, 30:33].view(np.uint32), case["p"][0, 30:33].view(np.uint32))
    for drop in (dict(p_valid=None), dict(obs_valid=None), dict(counts=None)):
        c = dict(case, **drop)
        ref = B.run(c, fill_points=SENTS[1], fill_inlier=SENTS[2])
        for device in (False, True):
            same(call(fd, ctx, c, device=device), ref, (drop, device))


def test_batch_of_mixed_problems(fd, ctx):
    exp = check(fd, ctx, "batch")
    assert exp[5].tolist()[1] == 0 and exp[5][0] >= 1 and exp[5][2] >= 1 and exp[3][1] == 0
    assert np.array_equal(exp[0][2].view(np.uint64), CASES["batch"]["poses"][2].view(np.uint64))


def test_aliasing_skipped_outputs_and_empty_stride(fd, ctx):
    case, exp = CASES["batch"], expected("batch")
    written = np.arange(70)[None, :] < np.array([70, 0, 70, 70, 9])[:, None]
    ali = list(exp)
    ali[1] = np.where(written[:, :, None], exp[1], case["p"])  # slots past counts keep what the buffer held: the input
    for device in (False, True):
        same(call(fd, ctx, case, device=device, alias=True), ali, ("aliased", device))
        for skip in ((1,), (2,), (3,), (4,), (5,), (1, 2, 3, 4, 5)):
            got = call(fd, ctx, case, device=device, skip=skip)
            for k in range(6):
                if k in skip:
                    assert np.all(got[k] == DTYPES[k](SENTS[k])), (skip, k)
                else:
                    same(got[k:k + 1], exp[k:k + 1], (skip, k))
    empty = dict(CASES["n-2"], p=np.zeros((1, 0, 3), np.float32), obs=np.zeros((1, 3, 4, 2), np.float32), counts=None)
    for device in (False, True):
        for alias in (False, True):
            out = call(fd, ctx, empty, device=device, alias=alias)
            assert np.array_equal(out[0].view(np.uint64), empty["poses"].view(np.uint64))
            assert out[3].tolist() == [0] and out[5].tolist() == [0] and out[4].tolist() == [[0.0, 0.0]]
            assert np.all(out[2] == SENTS[2])


def test_rejected_arguments(fd, ctx):
    from feature_detector_amd._lib import FD_ERR_INVALID, fd_ba_opts

    L = fd.load()
    poses, p, obs = np.tile(B.IDENTITY, (1, 2, 1)), np.zeros((1, 8, 3), np.float32), np.zeros((1, 2, 8, 2), np.float32)
    pposes, pp, pobs = (ctypes.c_void_p(a.ctypes.data) for a in (poses, p, obs))
    good = dict(rounds=2, threshold=2.0, fx=500.0, fy=-500.0, cx=320.0, cy=240.0, lambda_=1e-3, up=10.0, down=0.1)

    def rc(batch=1, cams=2, ps=8, os_=8, ip=pposes, p=pp, o=pobs, op=pposes, opts=True, **kw):
        ob = fd_ba_opts(**{**good, **kw})
        return L.fd_bundle_adjust(ctx.ptr, batch, cams, ctypes.byref(ob) if opts else None, ip, None, p, None, None, ps, o, None, os_,
                                  op, None, None, None, None, None, 0)

    ctx.set_stream(None)
    nan, inf = float("nan"), float("inf")
    assert rc() == 0 and rc(rounds=16) == 0 and rc(down=1.0) == 0 and rc(cams=1) == 0
    bads = [dict(batch=0), dict(cams=0), dict(cams=9), dict(ps=-1), dict(os_=-1), dict(os_=7), dict(ip=None), dict(p=None), dict(o=None),
            dict(op=None), dict(opts=False), dict(rounds=0), dict(rounds=17), dict(threshold=0.0), dict(threshold=-1.0),
            dict(threshold=nan), dict(threshold=inf), dict(lambda_=0.0), dict(lambda_=-1.0), dict(lambda_=nan), dict(lambda_=inf),
            dict(up=1.0), dict(up=0.5), dict(up=nan), dict(up=inf), dict(down=0.0), dict(down=1.5), dict(down=-0.1), dict(down=nan)]
    for name in ("fx", "fy", "cx", "cy"):
        bads += [{name: nan}, {name: inf}] + ([{name: 0.0}] if name[0] == "f" else [])
    for bad in bads:
        assert rc(**bad) == FD_ERR_INVALID, bad


def test_python_wrapper_host_device_and_out(fd):
    torch = pytest.importorskip("torch")
    case = CASES["masks"]
    exp = B.run(case)
    cam = case["cam"]
    K = np.array([[cam[0], 0, cam[2]], [0, cam[1], cam[3]], [0, 0, 1]])
    kw = dict(obs_valid=case["obs_valid"], point_valid=case["p_valid"], counts=case["counts"], fixed=case["fixed"], rounds=case["rounds"],
              threshold=case["threshold"], lam=case["lam"], up=case["up"], down=case["down"])
    host = fd.bundle_adjust(case["poses"], case["p"], case["obs"], K, **kw)
    got = (host.poses, host.points, host.inliers, host.counts, host.cost, host.rounds)
    same(got, exp, "host")
    assert np.array_equal(host.rotation(0, 2), exp[0][0, 2, :9].reshape(3, 3)) and np.array_equal(host.translation(0, 2), exp[0][0, 2, 9:])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    dkw = dict(kw, obs_valid=dev(case["obs_valid"]), point_valid=dev(case["p_valid"]), counts=dev(case["counts"]), fixed=dev(case["fixed"]))
    out = tuple(torch.full(e.shape, 5, dtype=getattr(torch, str(e.dtype)), device="cuda") for e in exp)
    res = fd.bundle_adjust(dev(case["poses"]), dev(case["p"]), dev(case["obs"]), cam, out=out, **dkw)
    torch.cuda.synchronize()
    assert res.poses is out[0]
    n = 77
    got = [x.cpu().numpy() for x in (res.poses, res.points, res.inliers, res.counts, res.cost, res.rounds)]
    same([got[0], got[1][:, :n], got[2][:, :, :n], got[3], got[4], got[5]],
         [exp[0], exp[1][:, :n], exp[2][:, :, :n], exp[3], exp[4], exp[5]], "device")
    assert np.all(got[1][:, n:] == 5) and np.all(got[2][:, :, n:] == 5)
    # a PointsResult passes as it is (its valid bytes are the point mask), and a list of poses stacks
    plain = dict(kw, point_valid=None)
    lst = [case["poses"][:, c] for c in range(4)]
    res = fd.bundle_adjust(lst, fd.PointsResult(case["p"], case["p_valid"], None), case["obs"], K, **plain)
    same((res.poses, res.points, res.inliers, res.counts, res.cost, res.rounds), exp, "PointsResult")
    with pytest.raises(ValueError):
        fd.bundle_adjust(case["poses"], case["p"], case["obs"][:, :, :50], K)
    with pytest.raises(ValueError):
        fd.bundle_adjust(case["poses"][:, :3], case["p"], case["obs"], K)


def test_graph_capture(fd):
    torch = pytest.importorskip("torch")
    a, b = CASES["rounds-1"], B.case(B.scene(501, cams=3, n=50), rounds=3)
    a = dict(a, rounds=3)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
    dposes, dp, dobs, dfix = dev(a["poses"]), dev(a["p"]), dev(a["obs"]), dev(a["fixed"])
    exp = B.run(b)
    out = tuple(torch.empty(e.shape, dtype=getattr(torch, str(e.dtype)), device="cuda") for e in exp)
    kw = dict(fixed=dfix, rounds=3, threshold=a["threshold"], lam=a["lam"], up=a["up"], down=a["down"], out=out)
    fd.bundle_adjust(dposes, dp, dobs, a["cam"], **kw)  # the sizing call
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        fd.bundle_adjust(dposes, dp, dobs, a["cam"], **kw)
    dposes.copy_(dev(b["poses"]))
    dp.copy_(dev(b["p"]))
    dobs.copy_(dev(b["obs"]))
    for _ in range(2):
        for o, v in zip(out, SENTS):
            o.fill_(v)
        g.replay()
        torch.cuda.synchronize()
        same([o.cpu().numpy() for o in out], exp, "replay")
    assert exp[5][0] >= 1
    del g


def test_two_view_pnp_bundle_chain(fd):
    """verify_geometry -> refit_geometry -> recover_pose on two views, solve_pnp -> refine_pnp of a third view, then
    bundle_adjust over the three with the first two held: device tensors against the restatements composed, and the
    final cost below the initial one."""
    torch = pytest.importorskip("torch")
    sc = PO.scene(5, n=96, outliers=24)
    q, t = sc["q"][None], sc["t"][None]
    R3, t3 = PO.planted_pose(77)
    rng = np.random.default_rng(7)
    y = sc["X"] @ R3.T + t3
    K = np.array(PO.kmat(PO.CAM), np.float64)
    uv = (y @ K.T)[:, :2] / y[:, 2:3] + rng.normal(0.0, 0.3, (96, 2))
    uv[~sc["planted"]] = rng.uniform(0, 400, (24, 2))
    t_xy3 = uv.astype(np.float32)[None]
    kw = dict(model="fundamental", image_size=(R.ROWS, R.COLS))
    dq, dt, d3 = (torch.from_numpy(x).cuda() for x in (q, t, t_xy3))
    ver = fd.verify_geometry(dq, dt, hypotheses=F.HYP, seed=5, **kw)
    ref = fd.refit_geometry(dq, dt, ver, rounds=2, **kw)
    two = fd.recover_pose(dq, dt, ref, PO.CAM)
    pnp = fd.solve_pnp(two, d3, PO.CAM, hypotheses=128, seed=9, threshold=2.0)
    fin = fd.refine_pnp(two, d3, pnp, PO.CAM, rounds=4, threshold=2.0)
    ident = torch.from_numpy(B.IDENTITY[None].copy()).cuda()
    fixed = torch.tensor([[1, 1, 0]], dtype=torch.uint8, device="cuda")
    obs = torch.stack([dq, dt, d3], 1)
    ov = torch.stack([ref.inliers, ref.inliers, fin.inliers], 1)
    ba = fd.bundle_adjust([ident, two, fin], two, obs, PO.CAM, obs_valid=ov, fixed=fixed, rounds=6, threshold=2.0)
    torch.cuda.synchronize()
    ran = R.ransac_ref(q, t, model=R.FUNDAMENTAL, hypotheses=F.HYP, seed=5, center=F.CENTER, scale=F.SCALE)
    fit = F.refit_ref(q, t, ran[0], ran[1], model=R.FUNDAMENTAL, rounds=2, center=F.CENTER, scale=F.SCALE)
    pose = PO.pose_ref(q, t, fit[0], fit[1])
    e1 = P.pnp_ransac_ref(pose[2], t_xy3, p_valid=pose[3], cam=PO.CAM, hypotheses=128, seed=9, threshold=2.0)
    e2 = P.pnp_refit_ref(pose[2], t_xy3, e1[0], e1[1], p_valid=pose[3], cam=PO.CAM, rounds=4, threshold=2.0)
    poses = np.stack([B.IDENTITY[None], pose[0], e2[0]], 1)
    exp = B.bundle_adjust_ref(poses, pose[2], np.stack([q, t, t_xy3], 1), fixed=np.array([[1, 1, 0]], np.uint8), p_valid=pose[3],
                              obs_valid=np.stack([fit[1], fit[1], e2[1]], 1), cam=PO.CAM, rounds=6, threshold=2.0)
    same([x.cpu().numpy() for x in (ba.poses, ba.points, ba.inliers, ba.counts, ba.cost, ba.rounds)], exp, "bundle_adjust")
    assert exp[5][0] >= 1 and exp[4][0, 1] < exp[4][0, 0] and exp[3][0] >= 150
