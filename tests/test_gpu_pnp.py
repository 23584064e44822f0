"""fd_pnp_ransac and fd_pnp_refit on the GPU against tests/pnp_ref.py: every output exactly (the pose as uint64 bit
patterns, the bytes, counts, best and rounds), through the C ABI into sentinel-guarded buffers, with host and with
device pointers; then the Python wrappers, graph capture and the verify -> refit -> recover -> PnP chain."""
import ctypes
import functools

import numpy as np
import pytest

import pnp_ref as P
import pose_ref as PO
import ransac_ref as R
import refit_ref as F

pytestmark = pytest.mark.gpu

GUARD = 32
SENT_POSE, SENT_INL, SENT_CNT, SENT_LAST = -123.25, 0xAB, -7, -9
SENTS = (SENT_POSE, SENT_INL, SENT_CNT, SENT_LAST)
CASES = dict(P.all_cases())
STOPPED_SEED = 1015  # of the seeds 1000..1119 of scene(seed, n=64, outliers=0.3, noise=0.7) one whose refit stops at round 3 of 8


@pytest.fixture(scope="module")
def fd():
    import feature_detector_amd as fd

    fd.load()
    return fd


@pytest.fixture(scope="module")
def ctx(fd):
    return fd.default_context()


@functools.lru_cache(maxsize=None)
def ransac_of(name):
    """The restatement's fd_pnp_ransac outputs of a case, computed once (unwritten slots hold the sentinel)."""
    return P.run_ransac(CASES[name], fill=SENT_INL)


def call(fd, ctx, case, refit=None, device=False, skip=(), alias=False):
    """fd_pnp_ransac (refit None) or fd_pnp_refit (refit = (in_pose, in_inlier, rounds)) through the C ABI. Outputs sit
    in the middle of sentinel-filled buffers (GUARD elements on either side, checked here); alias: out_pose and
    out_inlier are the in_pose and in_inlier arrays themselves. Returns the four outputs as numpy."""
    from feature_detector_amd._lib import fd_pnp_opts

    p, t = case["p"], case["t"]
    B, S, T = p.shape[0], p.shape[1], t.shape[1]
    rounds = 1 if refit is None else refit[2]
    opts = fd_pnp_opts(case["hypotheses"], case["seed"], rounds, case["threshold"], *case["cam"],
                       (ctypes.c_double * 3)(*case["center"]), case["scale"])
    outs = [np.full(B * 12 + 2 * GUARD, SENT_POSE, np.float64), np.full(B * S + 2 * GUARD, SENT_INL, np.uint8),
            np.full(B + 2 * GUARD, SENT_CNT, np.int32), np.full(B + 2 * GUARD, SENT_LAST, np.int32)]
    opt = lambda a, dt: None if a is None else np.ascontiguousarray(a, dt)  # noqa: E731
    ins = [np.ascontiguousarray(p, np.float32) if p.size else np.zeros(3, np.float32), opt(case["p_valid"], np.uint8),
           opt(case["counts"], np.int32), np.ascontiguousarray(t, np.float32) if t.size else np.zeros(2, np.float32),
           opt(case["idx"], np.int32), opt(case["valid"], np.uint8)]
    if refit is not None:
        if alias:  # the inputs live inside the output buffers
            outs[0][GUARD:GUARD + B * 12] = np.asarray(refit[0], np.float64).reshape(-1)
            outs[1][GUARD:GUARD + B * S] = np.asarray(refit[1], np.uint8).reshape(-1)
        else:
            ins += [np.ascontiguousarray(refit[0], np.float64), np.ascontiguousarray(refit[1], np.uint8) if S else np.zeros(1, np.uint8)]
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
    if refit is None:
        rc = L.fd_pnp_ransac(ctx.ptr, B, ctypes.byref(opts), ip[0], ip[1], ip[2], S, ip[3], T, ip[4], ip[5],
                             op[0], op[1], op[2], op[3], 1 if device else 0)
    else:
        given = (op[0], op[1]) if alias else (ip[6], ip[7])
        rc = L.fd_pnp_refit(ctx.ptr, B, ctypes.byref(opts), ip[0], ip[1], ip[2], S, ip[3], T, ip[4], ip[5], given[0], given[1],
                            op[0], op[1], op[2], op[3], 1 if device else 0)
    assert rc == 0, L.fd_last_error(ctx.ptr)
    if device:
        torch.cuda.synchronize()
        outs = [a.cpu().numpy() for a in outs]
    for a, s in zip(outs, SENTS):
        assert np.all(a[:GUARD] == s) and np.all(a[-GUARD:] == s), "a write outside the output"
    return (outs[0][GUARD:-GUARD].reshape(B, 12), outs[1][GUARD:-GUARD].reshape(B, S), outs[2][GUARD:-GUARD], outs[3][GUARD:-GUARD])


def same(got, exp, what):
    for k, (g, e) in enumerate(zip(got, exp)):
        assert g.dtype == e.dtype and g.shape == e.shape, (what, k)
        assert np.array_equal(g.view(np.uint8), e.view(np.uint8)), (what, k, g, e)


def check(fd, ctx, name, rounds=(4,), sides=(False, True)):
    """fd_pnp_ransac with host and with device pointers equals the restatement bit for bit, and fd_pnp_refit on its
    outputs does for every `rounds`. Returns the restatement's (ransac, refit of the last rounds)."""
    case, exp = CASES[name], ransac_of(name)
    for device in sides:
        same(call(fd, ctx, case, device=device), exp, (name, "ransac", device))
    given = (exp[0], np.where(exp[1] == SENT_INL, 0, exp[1]).astype(np.uint8))
    fit = None
    for r in rounds:
        fit = P.run_refit(case, *given, r, fill=SENT_INL)
        for device in sides:
            same(call(fd, ctx, case, refit=(*given, r), device=device), fit, (name, "refit", r, device))
    return exp, fit


@pytest.mark.parametrize("n", [0, 5, 6, 7, 255, 256, 257, 600])
def test_counts(fd, ctx, n):
    """n on both sides of the sample size, of one and two trips of the 256 partials and of the hypothesis kernel's
    tile; refit rounds 1 and 8."""
    exp, fit = check(fd, ctx, f"n-{n}", rounds=(1, 8))
    if n < 6:
        assert exp[3][0] == -1 and not exp[0].any() and exp[2][0] == 0 and fit[3][0] == 0
    else:
        assert exp[3][0] >= 0 and fit[3][0] >= 1 and fit[2][0] >= 0.7 * n * (1.0 if n < 40 else 0.75)


@pytest.mark.parametrize("h", [1, 63, 64, 65, 4096])
def test_hypothesis_counts(fd, ctx, h):
    """One wave per workgroup: a partial wave, exactly one, one more, and 64 workgroups racing on the atomicMax."""
    exp, _ = check(fd, ctx, f"hyp-{h}", rounds=())
    assert exp[3][0] >= 0
    if h == 4096:  # several hypotheses tie at the top: the lowest index wins
        detail = []
        P.run_ransac(CASES["hyp-4096"], detail=detail)
        score, valid, _ = detail[0]
        top = np.flatnonzero(valid & (score == score[valid].max()))
        assert exp[3][0] == top[0]


def test_batch_counts_with_flag_bits(fd, ctx):
    exp, fit = check(fd, ctx, "batch", rounds=(2,))
    assert exp[3][0] >= 0 and exp[3][1] >= 0 and np.all(exp[1][1, 60:] == SENT_INL) and np.all(exp[1][2, 7:] == SENT_INL)
    assert len({int(b) for b in exp[3]}) > 1 or exp[3][0] == -1


def test_masks_index_and_non_finite(fd, ctx):
    """p_valid and pair_valid with bytes other than 1, match_idx with -1, out-of-range and repeated entries,
    t_stride != q_stride, a NaN / inf in each of the five coordinate places; then each mask absent."""
    exp, _ = check(fd, ctx, "holes", rounds=(2,))
    assert not (exp[1][:, 5:9] == 1).any() and not (exp[1][0, 30:35] == 1).any() and exp[2].min() >= 10
    case = CASES["holes"]
    for drop in (dict(valid=None), dict(p_valid=None), dict(valid=None, p_valid=None)):
        c = dict(case, **drop)
        ref = P.run_ransac(c, fill=SENT_INL)
        for device in (False, True):
            same(call(fd, ctx, c, device=device), ref, (drop, device))
    c = dict(case, idx=None, t=np.ascontiguousarray(np.concatenate([case["t"], case["t"][:, :15]], 1)))
    same(call(fd, ctx, c, device=True), P.run_ransac(c, fill=SENT_INL), "no match_idx")


def test_degenerate_scenes(fd, ctx):
    """Coplanar and duplicate points: no pose (twelve zeros, best -1, bytes 0). A nearly coplanar scene, a sampler
    that gives up, points behind the camera: whatever the restatement says."""
    for name in ("coplanar", "duplicate"):
        exp, fit = check(fd, ctx, name, rounds=(2,))
        assert exp[3][0] == -1 and not exp[0].any() and not exp[1].any() and exp[2][0] == 0 and fit[3][0] == 0
    check(fd, ctx, "near-coplanar", rounds=(2,))
    exp, _ = check(fd, ctx, "few-distinct", rounds=(1,))
    assert exp[3][0] >= 0
    exp, _ = check(fd, ctx, "behind", rounds=(1,))
    assert exp[3][0] >= 0 and exp[2][0] == 0 and not exp[1].any()


def test_conditioning(fd, ctx):
    a, _ = check(fd, ctx, "unconditioned")
    b, _ = check(fd, ctx, "conditioned")
    assert a[3][0] >= 0 and b[3][0] >= 0 and not np.array_equal(a[0], b[0])


def _stopped():
    c = P.case(P.scene(STOPPED_SEED, n=64, outliers=0.3, noise=0.7))
    return c, P.run_ransac(c)


def test_refit_guard_singular_and_aliasing(fd, ctx):
    c, ran = _stopped()
    given = (ran[0], ran[1])
    eight = P.run_refit(c, *given, 8, fill=SENT_INL)
    assert 1 <= eight[3][0] < 8
    # the stopped frame's pose is the last accepted round's, bit for bit
    same(P.run_refit(c, *given, int(eight[3][0]), fill=SENT_INL)[:3], eight[:3], "restatement")
    two = np.zeros_like(ran[1])
    two[0, np.flatnonzero(ran[1][0])[:2]] = 1            # fewer than 3 points: a singular 6 x 6 system
    none = np.zeros_like(ran[1])                         # an empty set: a zero system
    mixed = np.zeros_like(ran[1])                        # members that pull the pose off: round 1 loses inliers
    sc = P.scene(STOPPED_SEED, n=64, outliers=0.3, noise=0.7)
    mixed[0, np.flatnonzero(sc["planted"])[:4]] = 1
    mixed[0, np.flatnonzero(~sc["planted"])[:6]] = 1
    for inl in (two, none, mixed):
        exp = P.run_refit(c, eight[0], inl, 8, fill=SENT_INL)
        assert exp[3][0] == 0 and np.array_equal(exp[0].view(np.uint64), eight[0].view(np.uint64)) and exp[2][0] == inl.sum()
    for device in (False, True):
        same(call(fd, ctx, c, refit=(*given, 8), device=device), eight, ("stopped", device))
        same(call(fd, ctx, c, refit=(*given, 8), device=device, alias=True), eight, ("aliased", device))
        for inl in (two, none, mixed):
            exp = P.run_refit(c, eight[0], inl, 8, fill=SENT_INL)
            same(call(fd, ctx, c, refit=(eight[0], inl, 8), device=device), exp, ("rejected", device))
            same(call(fd, ctx, c, refit=(eight[0], inl, 8), device=device, alias=True), exp, ("rejected, aliased", device))


def test_empty_stride_and_skipped_outputs(fd, ctx):
    empty = dict(CASES["n-6"], p=np.zeros((2, 0, 3), np.float32), t=np.zeros((2, 5, 2), np.float32), counts=None)
    pose = np.arange(24, dtype=np.float64).reshape(2, 12)
    for device in (False, True):
        out = call(fd, ctx, empty, device=device)
        assert not out[0].any() and out[2].tolist() == [0, 0] and out[3].tolist() == [-1, -1]
        out = call(fd, ctx, empty, refit=(pose, np.zeros((2, 0), np.uint8), 3), device=device)
        assert np.array_equal(out[0], pose) and out[2].tolist() == [0, 0] and out[3].tolist() == [0, 0]
    case, exp = CASES["batch"], ransac_of("batch")
    given = (exp[0], np.where(exp[1] == SENT_INL, 0, exp[1]).astype(np.uint8))
    fit = P.run_refit(case, *given, 2, fill=SENT_INL)
    for device in (False, True):
        for skip in ((1,), (2, 3), (1, 2, 3)):
            for refit, ref in ((None, exp), ((*given, 2), fit)):
                got = call(fd, ctx, case, refit=refit, device=device, skip=skip)
                for k in range(4):
                    if k in skip:
                        assert np.all(got[k] == SENTS[k]), (skip, k)
                    else:
                        same(got[k:k + 1], ref[k:k + 1], (skip, k))


def test_rejected_arguments(fd, ctx):
    from feature_detector_amd._lib import FD_ERR_INVALID, fd_pnp_opts

    L = fd.load()
    p, t = np.zeros((1, 8, 3), np.float32), np.zeros((1, 8, 2), np.float32)
    pose, inl = np.zeros(12), np.zeros(8, np.uint8)
    pp, pt, ppose, pinl = (ctypes.c_void_p(a.ctypes.data) for a in (p, t, pose, inl))
    good = dict(hypotheses=4, seed=0, rounds=2, threshold=2.0, fx=500.0, fy=-500.0, cx=320.0, cy=240.0, scale=1.0)

    def rc(fn, batch=1, qs=8, ts=8, p=pp, t=pt, ip=ppose, ii=pinl, op=ppose, idx=None, opts=True, center=(0.0, 0.0, 0.0), **kw):
        o = fd_pnp_opts(**{**good, **kw}, center=(ctypes.c_double * 3)(*center))
        po = ctypes.byref(o) if opts else None
        if fn == "fd_pnp_ransac":
            return L.fd_pnp_ransac(ctx.ptr, batch, po, p, None, None, qs, t, ts, idx, None, op, None, None, None, 0)
        return L.fd_pnp_refit(ctx.ptr, batch, po, p, None, None, qs, t, ts, idx, None, ip, ii, op, None, None, None, 0)

    ctx.set_stream(None)
    nan, inf = float("nan"), float("inf")
    for fn in ("fd_pnp_ransac", "fd_pnp_refit"):
        assert rc(fn) == 0
        bads = [dict(batch=0), dict(qs=-1), dict(ts=-1), dict(ts=7), dict(p=None), dict(t=None), dict(op=None), dict(opts=False),
                dict(threshold=0.0), dict(threshold=-1.0), dict(threshold=nan), dict(threshold=inf)]
        for name in ("fx", "fy", "cx", "cy"):
            bads += [{name: nan}, {name: inf}] + ([{name: 0.0}] if name[0] == "f" else [])
        for bad in bads:
            assert rc(fn, **bad) == FD_ERR_INVALID, (fn, bad)
        idx = np.zeros((1, 8), np.int32)
        assert rc(fn, ts=7, idx=ctypes.c_void_p(idx.ctypes.data)) == 0
    for bad in (dict(hypotheses=0), dict(hypotheses=4097), dict(scale=0.0), dict(scale=-1.0), dict(scale=nan), dict(scale=inf),
                dict(center=(nan, 0.0, 0.0)), dict(center=(0.0, inf, 0.0)), dict(center=(0.0, 0.0, -inf))):
        assert rc("fd_pnp_ransac", **bad) == FD_ERR_INVALID, bad
    assert rc("fd_pnp_ransac", rounds=0) == 0 and rc("fd_pnp_refit", hypotheses=0, scale=nan, center=(nan, nan, nan)) == 0
    for bad in (dict(rounds=0), dict(rounds=9), dict(ip=None), dict(ii=None)):
        assert rc("fd_pnp_refit", **bad) == FD_ERR_INVALID, bad
    assert rc("fd_pnp_refit", rounds=8) == 0


def test_python_wrappers_host_device_and_out(fd):
    torch = pytest.importorskip("torch")
    name = "conditioned"
    case, exp = CASES[name], P.run_ransac(CASES[name])
    fit = P.run_refit(case, exp[0], exp[1], 4)
    p, t, cam = case["p"], case["t"], case["cam"]
    K = np.array([[cam[0], 0, cam[2]], [0, cam[1], cam[3]], [0, 0, 1]])
    kw = dict(hypotheses=case["hypotheses"], seed=case["seed"], threshold=case["threshold"])
    host = fd.solve_pnp(p, t, K, center=case["center"], scale=case["scale"], **kw)
    same((host.pose, host.inliers, host.counts, host.best), exp, "host")
    hfit = fd.refine_pnp(p, t, host, K, rounds=4, threshold=case["threshold"])
    same((hfit.pose, hfit.inliers, hfit.counts, hfit.rounds), fit, "host refine")
    assert hfit.best is host.best and np.array_equal(hfit.rotation(0), fit[0][0, :9].reshape(3, 3))
    dp, dt = torch.from_numpy(p).cuda(), torch.from_numpy(t).cuda()
    dev = fd.solve_pnp(dp, dt, cam, center=case["center"], scale=case["scale"], **kw)
    out = (torch.full((1, 12), 5.0, dtype=torch.float64, device="cuda"), torch.full((1, 80), 5, dtype=torch.uint8, device="cuda"),
           torch.full((1,), 5, dtype=torch.int32, device="cuda"), torch.full((1,), 5, dtype=torch.int32, device="cuda"))
    dfit = fd.refine_pnp(dp, dt, dev, cam, rounds=4, threshold=case["threshold"], out=out)
    torch.cuda.synchronize()
    assert dfit.pose is out[0]
    same([x.cpu().numpy() for x in (dev.pose, dev.inliers, dev.counts, dev.best)], exp, "device")
    same([x.cpu().numpy() for x in (dfit.pose, dfit.inliers, dfit.counts, dfit.rounds)], fit, "device refine")
    # a PointsResult passes as it is: its valid bytes are the point mask
    pv = np.ones((1, 80), np.uint8)
    pv[0, ::7] = 0
    masked = P.run_ransac(dict(case, p_valid=pv))
    res = fd.solve_pnp(fd.PointsResult(p, pv, None), t, K, center=case["center"], scale=case["scale"], **kw)
    same((res.pose, res.inliers, res.counts, res.best), masked, "PointsResult")
    with pytest.raises(ValueError):
        fd.solve_pnp(p, t, np.array([[500.0, 0.1, 320], [0, 500, 240], [0, 0, 1]]))
    with pytest.raises(ValueError):
        fd.solve_pnp(p[:, :, :2], t, K)


def test_graph_capture(fd):
    torch = pytest.importorskip("torch")
    a, b = CASES["unconditioned"], P.case(P.scene(902, n=80), center=(0.0, 0.0, 0.0), scale=1.0)
    dp, dt = torch.from_numpy(a["p"]).cuda(), torch.from_numpy(a["t"]).cuda()
    spec = ((1, 12), torch.float64), ((1, 80), torch.uint8), ((1,), torch.int32), ((1,), torch.int32)
    out = tuple(torch.empty(s, dtype=d, device="cuda") for s, d in spec)
    fout = tuple(torch.empty(s, dtype=d, device="cuda") for s, d in spec)
    kw = dict(hypotheses=a["hypotheses"], seed=a["seed"], threshold=a["threshold"])
    first = fd.solve_pnp(dp, dt, a["cam"], out=out, **kw)
    fd.refine_pnp(dp, dt, first, a["cam"], rounds=3, threshold=a["threshold"], out=fout)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        res = fd.solve_pnp(dp, dt, a["cam"], out=out, **kw)
        fd.refine_pnp(dp, dt, res, a["cam"], rounds=3, threshold=a["threshold"], out=fout)
    dp.copy_(torch.from_numpy(b["p"]))
    dt.copy_(torch.from_numpy(b["t"]))
    exp = P.run_ransac(b)
    fit = P.run_refit(b, exp[0], exp[1], 3)
    for _ in range(2):
        for o, v in zip(out + fout, SENTS + SENTS):
            o.fill_(v)
        g.replay()
        torch.cuda.synchronize()
        same([o.cpu().numpy() for o in out], exp, "replay")
        same([o.cpu().numpy() for o in fout], fit, "replay refine")
    assert exp[3][0] >= 0 and fit[3][0] >= 1
    del g


def test_two_view_to_pnp_chain(fd):
    """verify_geometry -> refit_geometry -> recover_pose on two views, then solve_pnp -> refine_pnp of a third view
    against the recovered points, the PointsResult passed as it is: device tensors against the restatements
    composed, and the third pose close to the planted one at the two-view scale."""
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
    torch.cuda.synchronize()
    ran = R.ransac_ref(q, t, model=R.FUNDAMENTAL, hypotheses=F.HYP, seed=5, center=F.CENTER, scale=F.SCALE)
    fit = F.refit_ref(q, t, ran[0], ran[1], model=R.FUNDAMENTAL, rounds=2, center=F.CENTER, scale=F.SCALE)
    pose = PO.pose_ref(q, t, fit[0], fit[1])
    e1 = P.pnp_ransac_ref(pose[2], t_xy3, p_valid=pose[3], cam=PO.CAM, hypotheses=128, seed=9, threshold=2.0)
    e2 = P.pnp_refit_ref(pose[2], t_xy3, e1[0], e1[1], p_valid=pose[3], cam=PO.CAM, rounds=4, threshold=2.0)
    same([x.cpu().numpy() for x in (pnp.pose, pnp.inliers, pnp.counts, pnp.best)], e1, "solve_pnp")
    same([x.cpu().numpy() for x in (fin.pose, fin.inliers, fin.counts, fin.rounds)], e2, "refine_pnp")
    assert e1[3][0] >= 0 and e2[3][0] >= 1 and e2[2][0] >= 55
    # the recovered points are in units of the two-view baseline: the third pose's translation scales with it
    scale = np.linalg.norm(sc["t_vec"])
    assert PO.rotation_angle(e2[0][0, :9], R3) < 1e-2 and np.linalg.norm(e2[0][0, 9:] * scale - t3) < 5e-2
