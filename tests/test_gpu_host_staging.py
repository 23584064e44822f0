"""Host-pointer calls of the keypoint stages share one pool of staging buffers (fdrt::HostIo, fd_ctx.h), taken in
call order. GPU: every stage's host-pointer call, interleaved on one context with the stride going 8 -> 40 -> 8 and
then the whole sequence backwards, equals the same call on device tensors on a fresh context bit for bit, and the
numpy restatement where tests/ has one; then the cases a shared pool could break (in-place refinement, the
tracker's preloaded out_err, zero strides, a captured graph surviving the pool's growth). CPU: the binding's shared
argument helpers (feature_detector_amd/_slots.py) keep the exception types and messages of the five modules."""
import ctypes
import functools

import numpy as np
import pytest

import flow_ref
import match_guided_ref as G
import ransac_ref
import refine_ref
from match_ref import match_ref

gpu = pytest.mark.gpu

B, ROWS, COLS, LEVELS = 2, 48, 64, 2
STRIDES = (8, 40, 8)
STAGES = ("brief", "brief_match", "nn_guided", "track", "refine", "ransac_f", "ransac_h")
SENT = -77.0
FLOW = dict(levels=LEVELS, half_window=4, max_iters=10, min_eigen=1e-4, fb_max_dist=1.0)
REFINE = dict(half_window=3, max_iters=10, min_eigen=1e-4)
CENTER, SCALE = ransac_ref.conditioning((ransac_ref.ROWS, ransac_ref.COLS))


@pytest.fixture(scope="module")
def fd():
    import feature_detector_amd as fd

    fd.load()
    return fd


@pytest.fixture(scope="module")
def ctx(fd):
    c = fd.Context(fd.default_context().device)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def frames():
    """(prev, next) uint8 [B, ROWS, COLS]: a smooth random texture, next = prev moved by (2, -1) pixels."""
    rng = np.random.default_rng(7)
    coarse = rng.uniform(0, 255, (B, ROWS // 4 + 4, COLS // 4 + 4))
    canvas = np.kron(coarse, np.ones((4, 4)))
    for _ in range(3):  # a 3 x 3 box blur, three times
        canvas = sum(np.roll(canvas, (dy, dx), (1, 2)) for dy in (-1, 0, 1) for dx in (-1, 0, 1)) / 9
    canvas = np.clip(np.rint(canvas + rng.normal(0, 2, canvas.shape)), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(canvas[:, 8:8 + ROWS, 8:8 + COLS]), np.ascontiguousarray(canvas[:, 9:9 + ROWS, 6:6 + COLS])


@functools.lru_cache(maxsize=None)
def inputs(s):
    """The arrays of every stage at stride s, uneven counts (s, 3)."""
    rng = np.random.default_rng(100 + s)
    xy = (rng.integers(32, 4 * np.array([COLS - 8, ROWS - 8]), (B, s, 2)) / 4).astype(np.float32)
    valid = (rng.random((B, s)) < 0.8).astype(np.uint8)
    valid[:, 0], valid[:, 1] = 1, 0
    scenes = {m: [ransac_ref.planted_scene(m, 10 * s + b, n=s, outliers=s // 4)[:2] for b in range(B)]
              for m in (ransac_ref.FUNDAMENTAL, ransac_ref.HOMOGRAPHY)}
    t = s + 5
    return dict(xy=xy, valid=valid, counts=np.array([s, 3], np.int32), guess=(xy + np.float32(1.5)).astype(np.float32),
                brief=G.brief_case(s, t, B=B, qc=[s, 3], tc=[t, 4], flags=True, seed=s),
                nn=G.nn_case(s, t, dim=128, regime="round", variant="tenth", radius=20.0, B=B, qc=[s, 3], tc=[t, 4], flags=True, seed=s),
                scenes={m: (np.stack([q for q, _ in v]), np.stack([p for _, p in v])) for m, v in scenes.items()},
                matches=np.stack([rng.permutation(s).astype(np.int32) for _ in range(B)]))


def to_side(x, device):
    if not device or not isinstance(x, np.ndarray):
        return x
    import torch

    return torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else x).cuda()


def host(x):
    return np.ascontiguousarray(x.cpu().numpy() if hasattr(x, "cpu") else x)


def run(fd, ctx, stage, s, device):
    """One stage's call at stride s on host arrays or device tensors; its outputs as numpy arrays."""
    i = inputs(s)
    d = lambda x: to_side(x, device)  # noqa: E731
    prev, nxt = frames()
    if stage == "brief":
        res = fd.brief_compute(d(prev), d(i["xy"]), d(i["counts"]), length=100, half_patch_size=4, with_valid=True, ctx=ctx)
    elif stage == "brief_match":
        c = i["brief"]
        m = fd.brief_match(d(c["q"]), d(c["t"]), d(c["qc"]), d(c["tc"]), d(c["qv"]), d(c["tv"]), length=c["length"],
                           max_ratio=0.97, cross_check=True, ctx=ctx)
        res = (m.idx, m.dist, m.counts)
    elif stage == "nn_guided":
        c = i["nn"]
        m = fd.nn_match(d(c["q"]), d(c["t"]), d(c["qc"]), d(c["tc"]), d(c["qv"]), d(c["tv"]), cross_check=True, q_xy=d(c["q_xy"]),
                        t_xy=d(c["t_xy"]), radius=c["radius"], ctx=ctx)
        res = (m.idx, m.dist, m.counts)
    elif stage == "track":
        pp, pn = fd.build_pyramid(d(prev), LEVELS, ctx=ctx), fd.build_pyramid(d(nxt), LEVELS, ctx=ctx)
        f = fd.track_lk(pp, pn, d(i["xy"]), counts=d(i["counts"]), valid=d(i["valid"]), guess=d(i["guess"]), ctx=ctx, **FLOW)
        res = tuple(q.level(l) for q in (pp, pn) for l in range(LEVELS)) + (f.xy, f.status, f.err, f.counts)
    elif stage == "refine":
        r = fd.refine_points(d(prev), d(i["xy"]), counts=d(i["counts"]), valid=d(i["valid"]), ctx=ctx, **REFINE)
        res = (r.xy, r.status, r.counts)
    else:
        model = ransac_ref.FUNDAMENTAL if stage == "ransac_f" else ransac_ref.HOMOGRAPHY
        q, t = i["scenes"][model]
        # matches pair slot j with train slot matches[j]: the planted pairs, found through a permuted train set
        tp = np.empty_like(t)
        for b in range(B):
            tp[b, i["matches"][b]] = t[b]
        g = fd.verify_geometry(d(q), d(tp), matches=d(i["matches"]), valid=d(i["valid"]), counts=d(i["counts"]),
                               model="fundamental" if model == ransac_ref.FUNDAMENTAL else "homography", hypotheses=32, seed=s,
                               image_size=(ransac_ref.ROWS, ransac_ref.COLS), ctx=ctx)
        res = (g.model, g.inliers, g.counts, g.best)
    if device:
        import torch

        torch.cuda.synchronize()
    return tuple(host(x) for x in res)


@functools.lru_cache(maxsize=None)
def restated(stage, s):
    """The numpy restatement's outputs (zeros / -1 in the unwritten slots, as the binding's fresh outputs), or None."""
    i = inputs(s)
    prev, nxt = frames()
    if stage == "brief_match":
        c = i["brief"]
        return match_ref(c["q"], c["t"], c["qc"], c["tc"], c["qv"], c["tv"], length=c["length"], max_ratio=0.97, cross_check=True)
    if stage == "nn_guided":
        c = i["nn"]
        return G.nn_match_guided_ref(c["q"], c["t"], c["q_xy"], c["t_xy"], c["radius"], c["qc"], c["tc"], c["qv"], c["tv"],
                                     cross_check=True)
    if stage == "track":
        pyr = tuple(level for f in (prev, nxt) for level in flow_ref.pyr_ref(f, LEVELS))
        return pyr + tuple(flow_ref.flow_ref(prev, nxt, i["xy"], i["counts"], i["valid"], i["guess"], **FLOW))
    if stage == "refine":
        return refine_ref.refine_ref(prev, i["xy"], counts=i["counts"], valid=i["valid"], **REFINE)
    if stage in ("ransac_f", "ransac_h"):
        model = ransac_ref.FUNDAMENTAL if stage == "ransac_f" else ransac_ref.HOMOGRAPHY
        q, t = i["scenes"][model]
        tp = np.empty_like(t)
        for b in range(B):
            tp[b, i["matches"][b]] = t[b]
        return ransac_ref.ransac_ref(q, tp, i["counts"], i["matches"], i["valid"], model=model, hypotheses=32, seed=s,
                                     center=CENTER, scale=SCALE)
    return None


def same_bits(got, exp, what):
    assert len(got) == len(exp), what
    for k, (g, e) in enumerate(zip(got, exp)):
        g, e = np.ascontiguousarray(g), np.ascontiguousarray(e)
        assert g.shape == e.shape and g.itemsize == e.itemsize, (what, k)
        assert np.array_equal(g.view(np.uint8), e.view(np.uint8)), (what, k)


@pytest.fixture(scope="module")
def expected(fd):
    """(stage, stride) -> the call on device tensors, each on a fresh context; computed once."""
    out = {}
    for s in sorted(set(STRIDES)):
        for stage in STAGES:
            fresh = fd.Context(fd.default_context().device)
            out[stage, s] = run(fd, fresh, stage, s, device=True)
            fresh.close()
    return out


@gpu
def test_device_results_equal_the_restatements_and_are_not_trivial(expected):
    for (stage, s), got in expected.items():
        exp = restated(stage, s)
        if exp is not None:
            same_bits(got, exp, (stage, s))
    assert expected["brief", 40][1][0].sum() >= 5 and expected["brief", 40][0][0].any() and not expected["brief", 40][0][1, 3:].any()
    assert expected["brief_match", 40][2][0] >= 1 and expected["nn_guided", 40][2][0] >= 1
    assert expected["track", 40][-1][0] >= 10 and (expected["track", 40][-3] == 0).any()
    assert expected["refine", 40][2][0] >= 5
    assert expected["ransac_f", 40][3][0] >= 0 and expected["ransac_h", 40][3][0] >= 0 and expected["ransac_h", 8][3][1] == -1


@gpu
def test_interleaved_host_calls_on_one_context(fd, ctx, expected):
    order = [(stage, s) for s in STRIDES for stage in STAGES]
    for stage, s in order + order[::-1]:
        same_bits(run(fd, ctx, stage, s, device=False), expected[stage, s], (stage, s))


def p(a):
    if a is None:
        return None
    return ctypes.c_void_p(a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data)


@gpu
def test_in_place_host_refinement(fd, ctx):
    """out_xy == xy through the C ABI: the staged input and output do not share a buffer. Unwritten slots keep the
    caller's contents: the input positions in place, the sentinel out of place."""
    from feature_detector_amd._lib import fd_refine_opts

    i, (prev, _) = inputs(40), frames()
    opts = fd_refine_opts(3, 10, 0.01, 1e-4, 3.0)
    ctx.set_stream(None)
    res = []
    for in_place in (False, True):
        xy = i["xy"].copy()
        oxy = xy if in_place else np.full((B, 40, 2), SENT, np.float32)
        ost, cnt = np.full((B, 40), 99, np.uint8), np.full((B,), -7, np.int32)
        rc = fd.load().fd_points_refine(ctx.ptr, p(prev), 0, B, ROWS, COLS, ctypes.byref(opts), p(xy), p(i["valid"]), p(i["counts"]),
                                        40, p(oxy), p(ost), p(cnt), 0)
        assert rc == 0
        res.append((oxy, ost, cnt))
    (oxy, ost, cnt), (ixy, ist, icnt) = res
    exp = refine_ref.refine_ref(prev, i["xy"], counts=i["counts"], valid=i["valid"],
                                init=(np.full((B, 40, 2), SENT, np.float32), np.full((B, 40), 99, np.uint8)), **REFINE)
    same_bits((oxy, ost, cnt), exp, "out of place")
    assert np.array_equal(ist, ost) and np.array_equal(icnt, cnt) and (cnt > 0).any()
    assert np.array_equal(ixy[0].view(np.uint32), oxy[0].view(np.uint32))
    assert np.array_equal(ixy[1, :3].view(np.uint32), oxy[1, :3].view(np.uint32)) and np.array_equal(ixy[1, 3:], i["xy"][1, 3:])


@gpu
def test_flow_keeps_the_callers_out_err_in_invalid_slots(fd, ctx):
    from feature_detector_amd._lib import fd_flow_opts

    i, (prev, nxt) = inputs(40), frames()
    pp = fd.build_pyramid(prev, LEVELS, ctx=ctx, device_out=True)
    pn = fd.build_pyramid(nxt, LEVELS, ctx=ctx, device_out=True)
    ctx.synchronize()
    opts = fd_flow_opts(4, 10, 0.01, 1e-4, 1.0, -1.0)
    oxy, ost = np.full((B, 40, 2), SENT, np.float32), np.full((B, 40), 99, np.uint8)
    oerr, cnt = np.full((B, 40), SENT, np.float32), np.full((B,), -7, np.int32)
    ctx.set_stream(None)
    rc = fd.load().fd_flow_lk(ctx.ptr, B, ROWS, COLS, LEVELS, ctypes.byref(opts), p(pp.data), p(pn.data), p(i["xy"]), p(i["valid"]),
                              p(i["counts"]), 40, p(i["guess"]), p(oxy), p(ost), p(oerr), p(cnt), 0)
    assert rc == 0
    init = (np.full((B, 40, 2), SENT, np.float32), np.full((B, 40), 99, np.uint8), np.full((B, 40), SENT, np.float32))
    same_bits((oxy, ost, oerr, cnt), flow_ref.flow_ref(prev, nxt, i["xy"], i["counts"], i["valid"], i["guess"], init=init, **FLOW),
              "flow")
    dead = i["valid"][0] == 0
    assert dead.any() and (oerr[0][dead] == SENT).all() and (oerr[1, 3:] == SENT).all()


@gpu
def test_zero_strides(fd, ctx):
    prev, nxt = frames()
    none, some = np.zeros((B, 0, 2), np.float32), inputs(8)["xy"]
    bits = fd.brief_compute(prev, none, ctx=ctx)
    assert bits.shape == (B, 0, 8)
    f = fd.track_lk(prev, nxt, none, ctx=ctx, **FLOW)
    assert f.xy.shape == (B, 0, 2) and f.counts.tolist() == [0, 0]
    r = fd.refine_points(prev, none, ctx=ctx)
    assert r.xy.shape == (B, 0, 2) and r.counts.tolist() == [0, 0]
    cb, cn = inputs(8)["brief"], inputs(8)["nn"]
    for c, call, kw in ((cb, fd.brief_match, dict(length=cb["length"])), (cn, fd.nn_match, {})):
        for gate in (False, True):
            for side in ("q", "t"):
                e = dict(c, **{side: c[side][:, :0], side + "_xy": c[side + "_xy"][:, :0]})
                g = dict(q_xy=e["q_xy"], t_xy=e["t_xy"], radius=4.0) if gate else {}
                m = call(e["q"], e["t"], cross_check=True, ctx=ctx, **kw, **g)
                assert m.counts.tolist() == [0, 0] and m.idx.shape == (B, e["q"].shape[1]) and (m.idx == -1).all() and (m.dist == -1).all()
    for model in ("fundamental", "homography"):
        g = fd.verify_geometry(none, some, model=model, ctx=ctx)
        assert not g.model.any() and g.counts.tolist() == [0, 0] and g.best.tolist() == [-1, -1] and g.inliers.shape == (B, 0)
        g = fd.verify_geometry(some, none, matches=np.zeros((B, 8), np.int32), model=model, hypotheses=16, ctx=ctx)
        assert not g.model.any() and g.counts.tolist() == [0, 0] and g.best.tolist() == [-1, -1] and not g.inliers.any()


@gpu
@pytest.mark.parametrize("stage", ["track", "refine"])
def test_captured_graph_survives_staging_growth(fd, stage):
    """A device-path call holds no staging buffer, so a later, larger host-path call on the same context, which
    frees and reallocates the pool, leaves the captured graph's addresses alone."""
    torch = pytest.importorskip("torch")
    own = fd.Context(fd.default_context().device)
    i, (prev, nxt) = inputs(8), frames()
    dev = {k: torch.from_numpy(i[k]).cuda() for k in ("xy", "valid", "counts", "guess")}
    dprev = torch.from_numpy(prev).cuda()
    if stage == "track":
        pp, pn = fd.build_pyramid(dprev, LEVELS, ctx=own), fd.build_pyramid(torch.from_numpy(nxt).cuda(), LEVELS, ctx=own)
        out = tuple(torch.zeros(sh, dtype=dt, device="cuda") for sh, dt in (((B, 8, 2), torch.float32), ((B, 8), torch.uint8),
                                                                           ((B, 8), torch.float32), ((B,), torch.int32)))
        call = lambda: fd.track_lk(pp, pn, dev["xy"], counts=dev["counts"], valid=dev["valid"], guess=dev["guess"], out=out,  # noqa: E731
                                   ctx=own, **FLOW)
        exp = restated("track", 8)[2 * LEVELS:]
    else:
        out = tuple(torch.zeros(sh, dtype=dt, device="cuda") for sh, dt in (((B, 8, 2), torch.float32), ((B, 8), torch.uint8),
                                                                           ((B,), torch.int32)))
        call = lambda: fd.refine_points(dprev, dev["xy"], counts=dev["counts"], valid=dev["valid"], out=out, ctx=own, **REFINE)  # noqa: E731
        exp = restated("refine", 8)
    call()  # sizes the scratch
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call()
    for host_stage in ("brief", "nn_guided", "refine", "ransac_h"):  # larger host-path calls, none of the tracker's scratch: the pool grows
        run(fd, own, host_stage, 40, device=False)
    for o in out:
        o.zero_()
    g.replay()
    torch.cuda.synchronize()
    same_bits(tuple(host(o) for o in out), exp, stage)
    del g
    own.close()


# ---- CPU: the binding's argument helpers -------------------------------------------------------------------

def test_positions_rules():
    from feature_detector_amd import _slots as S

    xy = np.zeros((3, 5, 2), np.float32)
    assert S.positions(xy, "xy", False) is not None and S.positions(xy[0], "xy", False).shape == (1, 5, 2)
    assert S.positions(xy[:, ::2], "xy", False).flags.c_contiguous  # a non-contiguous view is copied
    assert S.positions(xy.tolist(), "uv", False, convert=True).dtype == np.float32  # brief_compute converts
    with pytest.raises(TypeError, match="^q_xy must be float32$"):
        S.positions(xy.astype(np.float64), "q_xy", False)
    for bad in (np.zeros((5,), np.float32), np.zeros((5, 3), np.float32), np.zeros((1, 5, 3), np.float32), np.zeros((1, 1, 5, 2), np.float32)):
        with pytest.raises(ValueError, match=r"^xy must be \[batch, S, 2\] or \[S, 2\]$"):
            S.positions(bad, "xy", False)
    with pytest.raises(ValueError, match="^uv must be \\[batch, S, 2\\] matching frames$"):
        S.positions(np.zeros((2, 5, 3)), "uv", False, convert=True, msg="uv must be [batch, S, 2] matching frames")
    with pytest.raises(TypeError, match="^guess must be float32$"):
        S.f32(np.zeros((5, 2), np.int32), "guess", False)
    torch = pytest.importorskip("torch")
    t = torch.zeros((3, 6, 2))
    assert S.positions(t[0], "xy", True).shape == (1, 6, 2) and S.positions(t[:, ::2], "xy", True).is_contiguous()
    with pytest.raises(TypeError, match="^t_xy must be float32$"):
        S.positions(t.double(), "t_xy", True)
    with pytest.raises(ValueError, match=r"^t_xy must be \[batch, S, 2\] or \[S, 2\]$"):
        S.positions(t[..., :1], "t_xy", True)


def test_gate_positions_rules():
    from feature_detector_amd import match as M

    q, t = np.zeros((1, 4, 2), np.float32), np.zeros((1, 6, 2), np.float32)
    gate, gq, gt = M._gate(q[0], t, (2, 3), False, 1, 4, 6)  # [S, 2] with batch 1
    assert (gate.radius_x, gate.radius_y) == (2.0, 3.0) and gq.shape == (1, 4, 2) and gt.shape == (1, 6, 2)
    assert M._gate(None, None, None, False, 1, 4, 6) is None
    with pytest.raises(ValueError, match="^guided matching needs q_xy, t_xy and radius together$"):
        M._gate(q, None, 1.0, False, 1, 4, 6)
    with pytest.raises(ValueError, match=r"^t_xy must be \[1, 6, 2\] or \[6, 2\]$"):
        M._gate(q, t[:, :5], 1.0, False, 1, 4, 6)
    with pytest.raises(ValueError, match=r"^q_xy must be \[2, 4, 2\]$"):
        M._gate(q[0], np.zeros((2, 6, 2), np.float32), 1.0, False, 2, 4, 6)  # [S, 2] needs batch 1
    with pytest.raises(TypeError, match="^q_xy must be float32$"):
        M._gate(q.astype(np.float64), t, 1.0, False, 1, 4, 6)
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError, match=r"^q_xy must be on the side \(host / device\) of the descriptors$"):
        M._gate(torch.zeros((1, 4, 2)), t, 1.0, True, 1, 4, 6)  # (a CPU tensor is not a device tensor)


def test_slot_arg_rules():
    from feature_detector_amd import _slots as S

    assert S.slot_arg(None, "uint8", (2, 3), False) is None
    v = S.slot_arg(np.ones((2, 3), bool), "uint8", (2, 3), False)
    assert v.dtype == np.uint8 and v.shape == (2, 3) and v.flags.c_contiguous
    c = S.slot_arg(np.array([[5], [7]], np.int64), "int32", (2,), False)
    assert c.dtype == np.int32 and c.tolist() == [5, 7]
    flagged = S.slot_arg(np.array([5 | 1 << 31], np.uint32), "int32", (1,), False)  # detect_points' count words pass as they are
    assert flagged.view(np.uint32)[0] == 5 | 1 << 31
    m = S.slot_arg(np.arange(12, dtype=np.int64).reshape(3, 4)[:, ::2], "int32", (3, 2), False)
    assert m.dtype == np.int32 and m.flags.c_contiguous and m[2].tolist() == [8, 10]
    with pytest.raises(ValueError):
        S.slot_arg(np.ones((2, 4), np.uint8), "uint8", (2, 3), False)
    torch = pytest.importorskip("torch")
    tv = S.slot_arg(torch.ones((2, 6), dtype=torch.bool)[:, ::2], "uint8", (2, 3), True)
    assert tv.dtype == torch.uint8 and tuple(tv.shape) == (2, 3) and tv.is_contiguous()
    with pytest.raises(RuntimeError):
        S.slot_arg(torch.ones((2, 4)), "uint8", (2, 3), True)


def test_outputs_rules():
    from feature_detector_amd import _slots as S

    specs = (((2, 3), "int32", -1), ((2, 3, 2), "float32", -1), ((2,), "int32", 0))
    idx, dist, cnt = S.outputs(specs, None, False)
    assert idx.dtype == np.int32 and (idx == -1).all() and dist.dtype == np.float32 and dist.shape == (2, 3, 2) and cnt.tolist() == [0, 0]
    with pytest.raises(ValueError, match="^out= is for device tensors$"):
        S.outputs(specs, (idx, dist, cnt), False)
    torch = pytest.importorskip("torch")
    fresh = S.outputs(specs, None, True, "cpu")
    assert fresh[1].dtype == torch.float32 and (fresh[0] == -1).all() and tuple(fresh[2].shape) == (2,)
    assert S.outputs(specs, fresh, True)[0] is fresh[0]  # the caller's tensors are used as they are
    msg = r"^out must be contiguous tensors: int32 \(2, 3\), float32 \(2, 3, 2\), int32 \(2,\)$"
    for bad in ((fresh[0], fresh[1].int(), fresh[2]), (fresh[0][:, :2], fresh[1], fresh[2]), (fresh[0], fresh[1], torch.zeros(4).int()[::2]),
                fresh[:2]):
        with pytest.raises(ValueError, match=msg):
            S.outputs(specs, bad, True)
    with pytest.raises(ValueError, match=r"^out must be contiguous int32 tensors of shapes \(2, 3\)$"):
        S.outputs(specs[:1], (fresh[1],), True, msg="out must be contiguous int32 tensors of shapes (2, 3)")
