"""fd_align_ransac, fd_align_refit and fd_align_apply on the GPU against tests/align_ref.py: every output exactly (the
model as uint64 bit patterns, the bytes, counts, best and rounds, the applied points as uint32), through the C ABI into
sentinel-guarded buffers, with host and with device pointers; then the Python wrappers, graph capture and the
recover_pose -> align_points chain."""
import ctypes
import functools

import numpy as np
import pytest

import align_ref as A
import pose_ref as PO

pytestmark = pytest.mark.gpu

GUARD = 32
SENT_MODEL, SENT_INL, SENT_CNT, SENT_LAST = -123.25, 0xAB, -7, -9
SENTS = (SENT_MODEL, SENT_INL, SENT_CNT, SENT_LAST)
CASES = dict(A.all_cases())
CASES["stopped"] = A.stopped_case()


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
    """The restatement's fd_align_ransac outputs of a case, computed once (unwritten slots hold the sentinel)."""
    return A.run_ransac(CASES[name], fill=SENT_INL)


def _sides(ctx, ins, outs, device):
    """The arrays on the side of the call, and how to take their addresses."""
    if device:
        import torch

        ins = [None if a is None else torch.from_numpy(a).cuda() for a in ins]
        outs = [torch.from_numpy(a).cuda() for a in outs]
        ctx.set_stream(torch.cuda.current_stream(ctx.device).cuda_stream)
        return ins, outs, (lambda a: a.data_ptr()), (lambda a: a.element_size())
    ctx.set_stream(None)
    return ins, outs, (lambda a: a.ctypes.data), (lambda a: a.itemsize)


def call(fd, ctx, case, refit=None, device=False, skip=(), alias=False):
    """fd_align_ransac (refit None) or fd_align_refit (refit = (in_model, in_inlier, rounds)) through the C ABI. Outputs
    sit in the middle of sentinel-filled buffers (GUARD elements on either side, checked here); alias: out_model and
    out_inlier are the in_model and in_inlier arrays themselves. Returns the four outputs as numpy."""
    from feature_detector_amd._lib import fd_align_opts

    q, t = case["q"], case["t"]
    B, S, T = q.shape[0], q.shape[1], t.shape[1]
    rounds = 1 if refit is None else refit[2]
    opts = fd_align_opts(case["kind"], case["hypotheses"], case["seed"], rounds, case["threshold"])
    outs = [np.full(B * 13 + 2 * GUARD, SENT_MODEL, np.float64), np.full(B * S + 2 * GUARD, SENT_INL, np.uint8),
            np.full(B + 2 * GUARD, SENT_CNT, np.int32), np.full(B + 2 * GUARD, SENT_LAST, np.int32)]
    opt = lambda a, dt: None if a is None else np.ascontiguousarray(a, dt)  # noqa: E731
    ins = [np.ascontiguousarray(q, np.float32) if q.size else np.zeros(3, np.float32), opt(case["q_valid"], np.uint8),
           opt(case["counts"], np.int32), np.ascontiguousarray(t, np.float32) if t.size else np.zeros(3, np.float32),
           opt(case["t_valid"], np.uint8), opt(case["idx"], np.int32), opt(case["valid"], np.uint8)]
    if refit is not None:
        if alias:  # the inputs live inside the output buffers
            outs[0][GUARD:GUARD + B * 13] = np.asarray(refit[0], np.float64).reshape(-1)
            outs[1][GUARD:GUARD + B * S] = np.asarray(refit[1], np.uint8).reshape(-1)
        else:
            ins += [np.ascontiguousarray(refit[0], np.float64), np.ascontiguousarray(refit[1], np.uint8) if S else np.zeros(1, np.uint8)]
    ins, outs, base, size = _sides(ctx, ins, outs, device)
    ip = [None if a is None else ctypes.c_void_p(base(a)) for a in ins]
    op = [None if k in skip else ctypes.c_void_p(base(a) + GUARD * size(a)) for k, a in enumerate(outs)]
    L = fd.load()
    if refit is None:
        rc = L.fd_align_ransac(ctx.ptr, B, ctypes.byref(opts), ip[0], ip[1], ip[2], S, ip[3], ip[4], T, ip[5], ip[6],
                               op[0], op[1], op[2], op[3], 1 if device else 0)
    else:
        given = (op[0], op[1]) if alias else (ip[7], ip[8])
        rc = L.fd_align_refit(ctx.ptr, B, ctypes.byref(opts), ip[0], ip[1], ip[2], S, ip[3], ip[4], T, ip[5], ip[6], given[0],
                              given[1], op[0], op[1], op[2], op[3], 1 if device else 0)
    assert rc == 0, L.fd_last_error(ctx.ptr)
    if device:
        import torch

        torch.cuda.synchronize()
        outs = [a.cpu().numpy() for a in outs]
    for a, s in zip(outs, SENTS):
        assert np.all(a[:GUARD] == s) and np.all(a[-GUARD:] == s), "a write outside the output"
    return (outs[0][GUARD:-GUARD].reshape(B, 13), outs[1][GUARD:-GUARD].reshape(B, S), outs[2][GUARD:-GUARD], outs[3][GUARD:-GUARD])


def apply_call(fd, ctx, model, xyz, valid, counts, device, in_place):
    """fd_align_apply through the C ABI into a sentinel-filled buffer (in_place: into the input itself, whose guards
    hold the sentinel too). Returns float32 [B, S, 3]."""
    B, S = xyz.shape[0], xyz.shape[1]
    sent = np.float32(SENT_MODEL)
    buf = np.full(B * S * 3 + 2 * GUARD, sent, np.float32)
    src = np.full(B * S * 3 + 2 * GUARD, sent, np.float32)
    src[GUARD:-GUARD] = xyz.reshape(-1)
    opt = lambda a, dt: None if a is None else np.ascontiguousarray(a, dt)  # noqa: E731
    ins, outs, base, size = _sides(ctx, [np.ascontiguousarray(model, np.float64), src, opt(valid, np.uint8), opt(counts, np.int32)],
                                   [buf], device)
    pin = ctypes.c_void_p(base(ins[1]) + GUARD * 4)
    pout = pin if in_place else ctypes.c_void_p(base(outs[0]) + GUARD * 4)
    ip = [None if a is None else ctypes.c_void_p(base(a)) for a in ins]
    L = fd.load()
    rc = L.fd_align_apply(ctx.ptr, B, ip[0], pin, ip[2], ip[3], S, pout, 1 if device else 0)
    assert rc == 0, L.fd_last_error(ctx.ptr)
    res = ins[1] if in_place else outs[0]
    if device:
        import torch

        torch.cuda.synchronize()
        res = res.cpu().numpy()
    assert np.all(res[:GUARD] == sent) and np.all(res[-GUARD:] == sent), "a write outside the output"
    return res[GUARD:-GUARD].reshape(B, S, 3)


def same(got, exp, what):
    for k, (g, e) in enumerate(zip(got, exp)):
        assert g.dtype == e.dtype and g.shape == e.shape, (what, k)
        assert np.array_equal(g.view(np.uint8), e.view(np.uint8)), (what, k, g, e)


def check(fd, ctx, name, rounds=(4,), sides=(False, True)):
    """fd_align_ransac with host and with device pointers equals the restatement bit for bit, and fd_align_refit on its
    outputs does for every `rounds`. Returns the restatement's (ransac, refit of the last rounds)."""
    case, exp = CASES[name], ransac_of(name)
    for device in sides:
        same(call(fd, ctx, case, device=device), exp, (name, "ransac", device))
    given = (exp[0], np.where(exp[1] == SENT_INL, 0, exp[1]).astype(np.uint8))
    fit = None
    for r in rounds:
        fit = A.run_refit(case, *given, r, fill=SENT_INL)
        for device in sides:
            same(call(fd, ctx, case, refit=(*given, r), device=device), fit, (name, "refit", r, device))
    return exp, fit


@pytest.mark.parametrize("n", [0, 2, 3, 4, 255, 256, 257, 513])
def test_counts(fd, ctx, n):
    """n on both sides of the sample size, of one, two and three trips of the 256 partials and of the hypothesis
    kernel's tile; refit rounds 1, 4 and 8."""
    exp, fit = check(fd, ctx, f"n-{n}", rounds=(1, 4, 8))
    if n < 3:
        assert exp[3][0] == -1 and not exp[0].any() and exp[2][0] == 0 and fit[3][0] == 0
    else:
        assert exp[3][0] >= 0 and fit[3][0] >= 1 and fit[2][0] >= 0.95 * n * (1.0 if n < 40 else 0.75)


@pytest.mark.parametrize("h", [1, 64, 65, 4096])
def test_hypothesis_counts(fd, ctx, h):
    """One wave per workgroup: a single lane, exactly one wave, one more, and 64 workgroups racing on the atomicMax."""
    exp, _ = check(fd, ctx, f"hyp-{h}", rounds=())
    assert exp[3][0] >= 0
    if h == 4096:  # several hypotheses may tie at the top: the lowest index wins
        detail = []
        A.run_ransac(CASES["hyp-4096"], detail=detail)
        score, valid, _ = detail[0]
        assert exp[3][0] == np.flatnonzero(valid & (score == score[valid].max()))[0]


def test_batch_unequal_counts_with_flag_bits_and_an_empty_frame(fd, ctx):
    exp, fit = check(fd, ctx, "batch", rounds=(2,))
    assert exp[3][0] >= 0 and exp[3][1] == -1 and exp[3][2] >= 0 and not exp[0][1].any() and fit[3].tolist()[1] == 0
    assert np.all(exp[1][1] == SENT_INL) and np.all(exp[1][2, 37:] == SENT_INL)


def test_masks_index_and_non_finite(fd, ctx):
    """q_valid, t_valid and pair_valid with bytes other than 1, match_idx with -1, out-of-range and repeated entries,
    t_stride != q_stride, a NaN / inf in each of the six coordinate places; then each mask absent."""
    exp, _ = check(fd, ctx, "holes", rounds=(2,))
    assert not (exp[1][:, 5:9] == 1).any() and not (exp[1][0, 30:36] == 1).any() and not (exp[1][0, 50:57][[0, 2, 3, 4, 5, 6]] == 1).any()
    assert exp[2].min() >= 10
    case = CASES["holes"]
    for drop in (dict(valid=None), dict(q_valid=None), dict(t_valid=None), dict(valid=None, q_valid=None, t_valid=None)):
        c = dict(case, **drop)
        ref = A.run_ransac(c, fill=SENT_INL)
        for device in (False, True):
            same(call(fd, ctx, c, device=device), ref, (drop, device))
    grown = np.ascontiguousarray(np.concatenate([case["t"], case["t"][:, :15]], 1))
    c = dict(case, idx=None, t=grown, t_valid=np.ascontiguousarray(np.concatenate([case["t_valid"], case["t_valid"][:, :15]], 1)))
    same(call(fd, ctx, c, device=True), A.run_ransac(c, fill=SENT_INL), "no match_idx")


def test_degenerate_and_special_frames(fd, ctx):
    """Collinear and duplicate points: no valid hypothesis (thirteen zeros, best -1, bytes 0). An exactly planar frame
    and the rigid kind on a scaled target: models, as the restatement has them."""
    for name in ("collinear", "duplicate"):
        exp, fit = check(fd, ctx, name, rounds=(2,))
        assert exp[3][0] == -1 and not exp[0].any() and not exp[1].any() and exp[2][0] == 0 and fit[3][0] == 0
    exp, fit = check(fd, ctx, "planar", rounds=(1, 4))
    assert exp[3][0] >= 0 and fit[3][0] >= 1 and fit[2][0] >= 60 and abs(fit[0][0, 12] - 2.0) < 1e-2
    exp, fit = check(fd, ctx, "rigid-scaled", rounds=(2,))
    assert exp[3][0] >= 0 and exp[0][0, 12] == 1.0 and exp[2][0] < 20 and (fit[3][0] == 0 or fit[0][0, 12] == 1.0)
    a, fa = check(fd, ctx, "rigid")
    b, fb = check(fd, ctx, "similarity")
    assert a[0][0, 12] == 1.0 and fa[0][0, 12] == 1.0 and b[0][0, 12] != 1.0 and fb[3][0] >= 1


def test_refit_guard_and_aliasing(fd, ctx):
    c, ran = CASES["stopped"], ransac_of("stopped")
    given = (ran[0], ran[1])
    eight = A.run_refit(c, *given, 8, fill=SENT_INL)
    assert eight[3][0] == 3
    two = np.zeros_like(ran[1])
    two[0, np.flatnonzero(ran[1][0])[:2]] = 1            # fewer than 3 members: an invalid round
    none = np.zeros_like(ran[1])                         # an empty set
    sc = A.scene(A.STOPPED_SEED, n=64, outliers=0.3, noise=0.02)
    mixed = np.zeros_like(ran[1])                        # members that pull the model off: round 1 loses inliers
    mixed[0, np.flatnonzero(sc["planted"])[:3]] = 1
    mixed[0, np.flatnonzero(~sc["planted"])[:8]] = 1
    for inl in (two, none, mixed):
        exp = A.run_refit(c, eight[0], inl, 8, fill=SENT_INL)
        assert exp[3][0] == 0 and np.array_equal(exp[0].view(np.uint64), eight[0].view(np.uint64)) and exp[2][0] == inl.sum()
    for device in (False, True):
        same(call(fd, ctx, c, refit=(*given, 8), device=device), eight, ("stopped", device))
        same(call(fd, ctx, c, refit=(*given, 8), device=device, alias=True), eight, ("aliased", device))
        for inl in (two, none, mixed):
            exp = A.run_refit(c, eight[0], inl, 8, fill=SENT_INL)
            same(call(fd, ctx, c, refit=(eight[0], inl, 8), device=device), exp, ("rejected", device))
            same(call(fd, ctx, c, refit=(eight[0], inl, 8), device=device, alias=True), exp, ("rejected, aliased", device))


def test_apply_in_place_and_apart(fd, ctx):
    """Three frames of 300 slots (two trips of a workgroup's 256), valid bytes 0..3, unequal counts: the transformed
    slots bit for bit, every other slot's bits (the sentinel, or in place the input) untouched."""
    rng = np.random.default_rng(5)
    B, S = 3, 300
    xyz = rng.uniform(-5, 5, (B, S, 3)).astype(np.float32)
    xyz[0, 7, 1], xyz[1, 9, 2] = np.nan, np.inf
    model = np.stack([np.concatenate([A.planted(k)[0].reshape(9), A.planted(k)[1], [A.planted(k)[2]]]) for k in range(B)])
    model[2] = 0.0  # a frame without a model maps every point to the origin
    valid = rng.integers(0, 4, (B, S)).astype(np.uint8)
    counts = np.array([S, 0, 257], np.int32)
    sent = np.full((B, S, 3), np.float32(SENT_MODEL), np.float32)
    for v, cn in ((valid, counts), (None, counts), (valid, None), (None, None)):
        apart, inpl = A.align_apply_ref(model, xyz, v, cn, out=sent), A.align_apply_ref(model, xyz, v, cn)
        for device in (False, True):
            got = apply_call(fd, ctx, model, xyz, v, cn, device, False)
            assert np.array_equal(got.view(np.uint32), apart.view(np.uint32)), ("apart", device, v is None, cn is None)
            got = apply_call(fd, ctx, model, xyz, v, cn, device, True)
            assert np.array_equal(got.view(np.uint32), inpl.view(np.uint32)), ("in place", device, v is None, cn is None)
    apart = A.align_apply_ref(model, xyz, valid, counts, out=sent)
    assert (apart[0][valid[0] != 1] == np.float32(SENT_MODEL)).all() and (apart[1] == np.float32(SENT_MODEL)).all()
    assert not apart[2, :257][valid[2, :257] == 1].any() and (apart[2, 257:] == np.float32(SENT_MODEL)).all()


def test_empty_stride_and_skipped_outputs(fd, ctx):
    empty = dict(CASES["n-3"], q=np.zeros((2, 0, 3), np.float32), t=np.zeros((2, 5, 3), np.float32), counts=None)
    model = np.arange(26, dtype=np.float64).reshape(2, 13)
    for device in (False, True):
        out = call(fd, ctx, empty, device=device)
        assert not out[0].any() and out[2].tolist() == [0, 0] and out[3].tolist() == [-1, -1]
        out = call(fd, ctx, empty, refit=(model, np.zeros((2, 0), np.uint8), 3), device=device)
        assert np.array_equal(out[0], model) and out[2].tolist() == [0, 0] and out[3].tolist() == [0, 0]
    case, exp = CASES["batch"], ransac_of("batch")
    given = (exp[0], np.where(exp[1] == SENT_INL, 0, exp[1]).astype(np.uint8))
    fit = A.run_refit(case, *given, 2, fill=SENT_INL)
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
    from feature_detector_amd._lib import FD_ERR_INVALID, fd_align_opts

    L = fd.load()
    q, t = np.zeros((1, 8, 3), np.float32), np.zeros((1, 8, 3), np.float32)
    model, inl = np.zeros(13), np.zeros(8, np.uint8)
    pq, pt, pm, pi = (ctypes.c_void_p(a.ctypes.data) for a in (q, t, model, inl))
    good = dict(kind=0, hypotheses=4, seed=0, rounds=2, threshold=0.5)

    def rc(fn, batch=1, qs=8, ts=8, q=pq, t=pt, im=pm, ii=pi, om=pm, idx=None, opts=True, **kw):
        o = fd_align_opts(**{**good, **kw})
        po = ctypes.byref(o) if opts else None
        if fn == "fd_align_ransac":
            return L.fd_align_ransac(ctx.ptr, batch, po, q, None, None, qs, t, None, ts, idx, None, om, None, None, None, 0)
        return L.fd_align_refit(ctx.ptr, batch, po, q, None, None, qs, t, None, ts, idx, None, im, ii, om, None, None, None, 0)

    ctx.set_stream(None)
    nan, inf = float("nan"), float("inf")
    for fn in ("fd_align_ransac", "fd_align_refit"):
        assert rc(fn) == 0 and rc(fn, kind=1) == 0
        for bad in (dict(batch=0), dict(qs=-1), dict(ts=-1), dict(ts=7), dict(q=None), dict(t=None), dict(om=None), dict(opts=False),
                    dict(threshold=0.0), dict(threshold=-1.0), dict(threshold=nan), dict(threshold=inf), dict(kind=-1), dict(kind=2)):
            assert rc(fn, **bad) == FD_ERR_INVALID, (fn, bad)
        idx = np.zeros((1, 8), np.int32)
        assert rc(fn, ts=7, idx=ctypes.c_void_p(idx.ctypes.data)) == 0
    for bad in (dict(hypotheses=0), dict(hypotheses=4097)):
        assert rc("fd_align_ransac", **bad) == FD_ERR_INVALID, bad
    assert rc("fd_align_ransac", rounds=0) == 0 and rc("fd_align_refit", hypotheses=0) == 0
    for bad in (dict(rounds=0), dict(rounds=9), dict(im=None), dict(ii=None)):
        assert rc("fd_align_refit", **bad) == FD_ERR_INVALID, bad
    assert rc("fd_align_refit", rounds=8) == 0

    def ap(batch=1, m=pm, xin=pq, s=8, xout=pq):
        return L.fd_align_apply(ctx.ptr, batch, m, xin, None, None, s, xout, 0)

    assert ap() == 0 and ap(s=0) == 0
    for bad in (dict(batch=0), dict(m=None), dict(xin=None), dict(xout=None), dict(s=-1)):
        assert ap(**bad) == FD_ERR_INVALID, bad


def test_python_wrappers_host_device_and_out(fd):
    torch = pytest.importorskip("torch")
    for name in ("similarity", "rigid"):
        case, exp = CASES[name], A.run_ransac(CASES[name])
        fit = A.run_refit(case, exp[0], exp[1], 4)
        q, t = case["q"], case["t"]
        kw = dict(kind=name, threshold=case["threshold"])
        rkw = dict(hypotheses=case["hypotheses"], seed=case["seed"], **kw)
        host = fd.align_points(q, t, **rkw)
        same((host.model, host.inliers, host.counts, host.best), exp, "host")
        hfit = fd.refine_alignment(q, t, host, rounds=4, **kw)
        same((hfit.model, hfit.inliers, hfit.counts, hfit.rounds), fit, "host refine")
        assert hfit.best is host.best and np.array_equal(hfit.rotation(0), fit[0][0, :9].reshape(3, 3))
        assert np.array_equal(hfit.translation(0), fit[0][0, 9:12]) and hfit.scale(0) == fit[0][0, 12]
        moved = A.align_apply_ref(fit[0], q, exp[1])
        assert np.array_equal(fd.transform_points(hfit, q, valid=host.inliers).view(np.uint32), moved.view(np.uint32))
        dq, dt = torch.from_numpy(q).cuda(), torch.from_numpy(t).cuda()
        dev = fd.align_points(dq, dt, **rkw)
        out = (torch.full((1, 13), 5.0, dtype=torch.float64, device="cuda"), torch.full((1, 80), 5, dtype=torch.uint8, device="cuda"),
               torch.full((1,), 5, dtype=torch.int32, device="cuda"), torch.full((1,), 5, dtype=torch.int32, device="cuda"))
        dfit = fd.refine_alignment(dq, dt, dev, rounds=4, out=out, **kw)
        dmoved = fd.transform_points(dfit, dq, valid=dev.inliers)
        inpl = dq.clone()
        assert fd.transform_points(dfit.model, inpl, valid=dev.inliers, out=inpl) is inpl
        torch.cuda.synchronize()
        assert dfit.model is out[0]
        same([x.cpu().numpy() for x in (dev.model, dev.inliers, dev.counts, dev.best)], exp, "device")
        same([x.cpu().numpy() for x in (dfit.model, dfit.inliers, dfit.counts, dfit.rounds)], fit, "device refine")
        assert np.array_equal(dmoved.cpu().numpy().view(np.uint32), moved.view(np.uint32))
        assert np.array_equal(inpl.cpu().numpy().view(np.uint32), moved.view(np.uint32))
    # a PointsResult passes on either side as it is: its valid bytes are the point masks
    case = CASES["similarity"]
    qv, tv = np.ones((1, 80), np.uint8), np.ones((1, 80), np.uint8)
    qv[0, ::7], tv[0, ::5] = 0, 2
    masked = A.run_ransac(dict(case, q_valid=qv, t_valid=tv))
    res = fd.align_points(fd.PointsResult(case["q"], qv, None), fd.PointsResult(case["t"], tv, None), hypotheses=case["hypotheses"],
                          seed=case["seed"], threshold=case["threshold"])
    same((res.model, res.inliers, res.counts, res.best), masked, "PointsResult")
    with pytest.raises(ValueError):
        fd.align_points(case["q"], case["t"], kind="affine")
    with pytest.raises(ValueError):
        fd.align_points(case["q"][:, :, :2], case["t"])
    with pytest.raises(ValueError):
        fd.align_points(case["q"], case["t"][:, :70])


def test_graph_capture(fd):
    torch = pytest.importorskip("torch")
    a, b = CASES["similarity"], A.case(A.scene(902, n=80))
    dq, dt = torch.from_numpy(a["q"]).cuda(), torch.from_numpy(a["t"]).cuda()
    spec = ((1, 13), torch.float64), ((1, 80), torch.uint8), ((1,), torch.int32), ((1,), torch.int32)
    out = tuple(torch.empty(s, dtype=d, device="cuda") for s, d in spec)
    fout = tuple(torch.empty(s, dtype=d, device="cuda") for s, d in spec)
    moved = torch.empty((1, 80, 3), dtype=torch.float32, device="cuda")
    kw = dict(threshold=a["threshold"])
    rkw = dict(hypotheses=a["hypotheses"], seed=a["seed"], **kw)
    first = fd.align_points(dq, dt, out=out, **rkw)
    fd.transform_points(fd.refine_alignment(dq, dt, first, rounds=3, out=fout, **kw), dq, out=moved)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        res = fd.align_points(dq, dt, out=out, **rkw)
        fit = fd.refine_alignment(dq, dt, res, rounds=3, out=fout, **kw)
        fd.transform_points(fit, dq, valid=fit.inliers, out=moved)
    dq.copy_(torch.from_numpy(b["q"]))
    dt.copy_(torch.from_numpy(b["t"]))
    exp = A.run_ransac(b)
    efit = A.run_refit(b, exp[0], exp[1], 3)
    sent = np.full((1, 80, 3), np.float32(SENT_MODEL), np.float32)
    emoved = A.align_apply_ref(efit[0], b["q"], efit[1], out=sent)
    for _ in range(2):
        for o, v in zip(out + fout, SENTS + SENTS):
            o.fill_(v)
        moved.fill_(SENT_MODEL)
        g.replay()
        torch.cuda.synchronize()
        same([o.cpu().numpy() for o in out], exp, "replay")
        same([o.cpu().numpy() for o in fout], efit, "replay refine")
        assert np.array_equal(moved.cpu().numpy().view(np.uint32), emoved.view(np.uint32))
    assert exp[3][0] >= 0 and efit[3][0] >= 1
    del g


def test_two_baselines_chain(fd):
    """recover_pose of one scene against two second views that differ in their baseline only, then align_points
    (similarity) of the two point sets, each passed as it is: device tensors against the restatements composed, and the
    scale close to the planted ratio of the baselines (both point sets are in the first camera's frame: R = I, t = 0)."""
    torch = pytest.importorskip("torch")
    sc = PO.scene(5, n=96, outliers=0)
    R2, ta = sc["R"], sc["t_vec"]
    tb = 2.5 * ta
    K = np.array(PO.kmat(PO.CAM), np.float64)
    rng = np.random.default_rng(17)
    views = []
    for tv in (ta, tb):
        y = (sc["X"] @ R2.T + tv) @ K.T
        views.append((y[:, :2] / y[:, 2:3] + rng.normal(0.0, 0.05, (96, 2))).astype(np.float32)[None])
    q = sc["q"][None]
    ones = np.ones((1, 96), np.uint8)
    models = [PO.model_of(R2, tv)[None] for tv in (ta, tb)]
    poses = [PO.pose_ref(q, t, m, ones) for t, m in zip(views, models)]
    th = 0.25  # in units of the second baseline: the triangulated depths are 2.5 to 6 of them
    e1 = A.align_ransac_ref(poses[0][2], poses[1][2], q_valid=poses[0][3], t_valid=poses[1][3], hypotheses=128, seed=9, threshold=th)
    e2 = A.align_refit_ref(poses[0][2], poses[1][2], e1[0], e1[1], q_valid=poses[0][3], t_valid=poses[1][3], rounds=4, threshold=th)
    dq = torch.from_numpy(q).cuda()
    two = [fd.recover_pose(dq, torch.from_numpy(t).cuda(), fd.GeometryResult(torch.from_numpy(m).cuda(), torch.from_numpy(ones).cuda(), None, None),
                           PO.CAM) for t, m in zip(views, models)]
    ali = fd.align_points(two[0], two[1], kind="similarity", hypotheses=128, seed=9, threshold=th)
    fin = fd.refine_alignment(two[0], two[1], ali, rounds=4, threshold=th)
    torch.cuda.synchronize()
    same([x.cpu().numpy() for x in (ali.model, ali.inliers, ali.counts, ali.best)], e1, "align_points")
    same([x.cpu().numpy() for x in (fin.model, fin.inliers, fin.counts, fin.rounds)], e2, "refine_alignment")
    assert e1[3][0] >= 0 and e2[3][0] >= 1 and e2[2][0] >= 80
    # the host test's margin after RANSAC: the relative scale within 2 * th / rho of the planted ratio
    src = poses[0][2][0][poses[0][3][0] == 1].astype(np.float64)
    rho = np.sqrt(np.mean(np.sum((src - src.mean(0)) ** 2, axis=1)))
    ratio = np.linalg.norm(ta) / np.linalg.norm(tb)
    for model in (e1[0][0], e2[0][0]):
        assert abs(model[12] / ratio - 1.0) <= 2 * th / rho
    assert PO.rotation_angle(e2[0][0, :9], np.eye(3)) <= 2 * th / rho
