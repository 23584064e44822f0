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


# ---- the sampler's "no new index in 32 draws" exit ---------------------------------------------------------
EXHAUSTING = R.EXHAUSTING  # (model, seed, hypotheses) with n equal to the sample size whose frame 0 has exhausted hypotheses


def minimal_frame(model, seed=0, pad=3):
    """One frame whose count is the sample size (no outliers), in a stride `pad` slots longer."""
    m = R.SAMPLE[model]
    q, t, _ = R.planted_scene(model, seed, n=m + pad, outliers=0)
    return q[None], t[None], [m]


@pytest.mark.parametrize("model,seed,hypotheses", EXHAUSTING)
def test_sampler_exhaustion(fd, ctx, model, seed, hypotheses):
    """n = sample size: the last pick has one free index, so some hypotheses give up. Such a lane goes on
    through the solver, the scoring loop and the wave reduction with ok = false: it must not win."""
    m = R.SAMPLE[model]
    dead = R.exhausted(seed, 0, m, m, hypotheses)
    assert len(dead) >= 1, "these inputs do not reach the sampler's exit"
    q, t, counts = minimal_frame(model)
    detail = []
    exp = R.ransac_ref(q, t, counts, model=model, hypotheses=hypotheses, seed=seed, center=CENTER, scale=SCALE, detail=detail)
    score, valid = detail[0]
    assert not valid[dead].any() and valid.any() and exp[3][0] >= 0 and exp[3][0] not in dead
    check(fd, ctx, q, t, counts=counts, model=model, hypotheses=hypotheses, seed=seed)


@pytest.mark.parametrize("model,seed,hypotheses", EXHAUSTING)
def test_sampler_exhaustion_beside_a_normal_frame(fd, ctx, model, seed, hypotheses):
    """Batch 2: frame 0 has n equal to the sample size (dead lanes among its hypotheses), then n below it
    (every lane dead); frame 1 is a normal scene whose outputs must be those it has alone."""
    m = R.SAMPLE[model]
    assert len(R.exhausted(seed, 0, m, m, hypotheses)) >= 1
    q, t = scenes(model, 40, 2, seed=6)
    opt = dict(model=model, hypotheses=hypotheses, seed=seed)
    exp = check(fd, ctx, q, t, counts=[m, 40], **opt)
    none = check(fd, ctx, q, t, counts=[m - 1, 40], **opt)
    assert exp[3][0] >= 0 and none[3][0] == -1 and exp[3][1] >= 0 and exp[2][1] >= 20
    # frame 1's hypotheses depend on its frame index, so "alone" is the same batch with frame 0 emptied
    alone = R.ransac_ref(q, t, [0, 40], fill=SENT_INL, center=CENTER, scale=SCALE, **opt)
    for with_dead, all_dead, one in zip(exp, none, alone):
        assert np.array_equal(with_dead[1:].view(np.uint8), one[1:].view(np.uint8))
        assert np.array_equal(all_dead[1:].view(np.uint8), one[1:].view(np.uint8))


EDGE_SEEDS = R.EDGE_SEEDS  # (model, seed, what hypothesis 0 does): see tests/ransac_ref.py


@pytest.mark.parametrize("model,seed,what", EDGE_SEEDS)
def test_sampler_edge_decides_the_winner(fd, ctx, model, seed, what):
    m = R.SAMPLE[model]
    picks, tries = R.sample_trace(seed, 0, 0, m, m)
    if what == "last draw":
        assert len(picks) == m and max(tries) == 32
    else:
        assert len(picks) < m and 0 not in picks
    q, t, counts = minimal_frame(model)
    detail = []
    exp = check(fd, ctx, q, t, counts=counts, model=model, hypotheses=64, seed=seed, detail=detail)
    score, valid = detail[0]
    assert valid.sum() >= 2 and np.all(score[valid] == m)
    assert (exp[3][0] == 0) == (what == "last draw") and valid[0] == (what == "last draw")


# ---- k_ransac_compact across its 256-slot chunks ----------------------------------------------------------
SEAM_S = 600  # chunks 0..255, 256..511, 512..599


def _punch(q, t, idx, valid, slots):
    """Make every slot of `slots` a hole, cycling through the six ways a slot is not taken."""
    T = t.shape[0]
    for i, s in enumerate(slots):
        kind = i % 6
        if kind == 0:
            valid[s] = 0
        elif kind == 1:
            valid[s] = 2 + i % 250
        elif kind == 2:
            idx[s] = -1
        elif kind == 3:
            idx[s] = T + i % 3
        elif kind == 4:
            q[s, i % 2] = np.nan
        else:
            t[s, i % 2] = np.inf if i % 4 else -np.inf  # (match_idx is the identity: only slot s reads t[s])


def seam_holes(pattern):
    """(hole slots, count word) of one frame of SEAM_S slots."""
    rng = np.random.default_rng(pattern)
    S = SEAM_S
    if pattern == 0:
        return [255, 256], S
    if pattern == 1:
        return [511, 512], S
    if pattern == 2:  # the whole first chunk untaken
        return list(range(256)), S
    if pattern == 3:  # a whole chunk taken between two sparse ones
        return sorted(rng.choice(256, 200, replace=False).tolist() + (512 + rng.choice(88, 60, replace=False)).tolist()), S
    if pattern in (4, 5):  # exactly 256 / 257 survivors
        return sorted(rng.choice(S, S - (256 if pattern == 4 else 257), replace=False).tolist()), S
    # a count word of 520 with flag bits: the last chunk is 512..519 (kept whole), the slots past it stay as they were
    word = int(np.array([520 | (1 << 25) | (1 << 28) | (1 << 31)], np.uint32).view(np.int32)[0])
    return list(range(3, 512, 7)) + [255, 256], word


SEAM_FRAMES = [(0, 1, 2), (3, 4, 5), (6, 2, 4)]


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("patterns", SEAM_FRAMES)
def test_compaction_across_chunk_seams(fd, ctx, model, patterns):
    """q_stride 600, batch 3, a different hole pattern per frame: the running base of k_ransac_compact over
    three chunks with holes on, before and after the seams. A wrong carry shifts cidx, hence the inlier mask,
    of the slots at or past 256; the mask has ones in every chunk that has a survivor."""
    S = SEAM_S
    q, t, idx, valid, counts = [], [], [], [], []
    for b, p in enumerate(patterns):
        qb, tb, _ = R.planted_scene(model, 100 + 10 * p + b, n=S, outliers=150)
        ib, vb = np.arange(S, dtype=np.int32), np.ones(S, np.uint8)
        holes, word = seam_holes(p)
        _punch(qb, tb, ib, vb, holes)
        n = min(word & R.COUNT_MASK, S)
        survivors = np.setdiff1d(np.arange(n), holes)
        assert len(R.correspondences(qb, tb, word, ib, vb, 0.0, 0.0, 1.0)[1]) == len(survivors)
        if p in (4, 5):
            assert len(survivors) == 252 + p
        q.append(qb), t.append(tb), idx.append(ib), valid.append(vb), counts.append(word)
    q, t, idx, valid = np.stack(q), np.stack(t), np.stack(idx), np.stack(valid)
    counts = np.array(counts, np.int32)
    exp = check(fd, ctx, q, t, counts=counts, idx=idx, valid=valid, model=model, hypotheses=128, seed=3)
    for b, p in enumerate(patterns):
        holes, word = seam_holes(p)
        n = min(word & R.COUNT_MASK, S)
        assert exp[3][b] >= 0 and not exp[1][b, holes].any() and np.all(exp[1][b, n:] == SENT_INL)
        for lo in range(0, n, 256):
            chunk = np.arange(lo, min(lo + 256, n))
            if len(np.setdiff1d(chunk, holes)):
                assert exp[1][b, chunk].sum() >= 1, (p, lo)
        assert exp[1][b, 256:n].sum() >= 2 and exp[1][b, 512:n].sum() >= 1  # the slots a wrong carry moves


# ---- the documented maximum of 4096 hypotheses: 64 wave-groups per frame ----------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_hypothesis_cap(fd, ctx, model):
    """Batch 2 with different counts: blockIdx.x / groups at its widest, and the tie rule across workgroups:
    the tied best hypotheses lie in at least two groups of 64 and the lowest index wins."""
    q, t = scenes(model, 40, 2, seed=1)
    detail = []
    exp = check(fd, ctx, q, t, counts=[40, 33], model=model, hypotheses=4096, seed=2, detail=detail)
    for b in range(2):
        score, valid = detail[b]
        tied = np.flatnonzero(valid & (score == score[valid].max()))
        assert len(set((tied // 64).tolist())) >= 2 and exp[3][b] == tied[0]
        assert tied[-1] // 64 > tied[0] // 64 and exp[2][b] == score[tied[0]]


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
