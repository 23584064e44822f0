"""What the six estimator entry points (fd_ransac, fd_pnp_ransac, fd_align_ransac and their refits) share on the host,
through the C ABI: the order of their argument checks, as the text of the context's last error when two things are wrong
at once, and a host-pointer call with every optional input and every output given, which takes the most staging buffers
a call of that entry point can take (fd_align_refit: all of them), bit for bit against the restatements."""
import ctypes

import numpy as np
import pytest

import align_ref as A
import pnp_ref as PN
import ransac_ref as R
import refit_ref as RF

pytestmark = pytest.mark.gpu

NAN = float("nan")
BATCH = "batch must be >= 1"
THRESHOLD = "threshold must be finite and > 0"
STRIDES = "without match_idx slot i pairs with slot i: t_stride must be >= q_stride"
MODEL = "model must be FD_RANSAC_FUNDAMENTAL or FD_RANSAC_HOMOGRAPHY"
KIND = "kind must be FD_ALIGN_SIMILARITY or FD_ALIGN_RIGID"
BAD = "bad arguments"
ENTRY_POINTS = ("fd_ransac", "fd_ransac_refit", "fd_pnp_ransac", "fd_pnp_refit", "fd_align_ransac", "fd_align_refit")


@pytest.fixture(scope="module")
def fd():
    import feature_detector_amd as fd

    fd.load()
    return fd


@pytest.fixture(scope="module")
def ctx(fd):
    c = fd.default_context()
    c.set_stream(None)
    return c


def ptr(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def options(fn, count, threshold, model=0, cam=PN.CAM, center=(0.0, 0.0, 0.0), scale=1.0, cxy=(0.0, 0.0), seed=0):
    """The entry point's option struct; count: hypotheses of a RANSAC call, rounds of a refit. model: fd_ransac's model
    or fd_align's kind; cxy and scale: the two-view conditioning, center and scale: fd_pnp_ransac's."""
    from feature_detector_amd import _lib

    refit = fn.endswith("refit")
    if fn == "fd_ransac":
        return _lib.fd_ransac_opts(model, count, seed, threshold, cxy[0], cxy[1], scale)
    if fn == "fd_ransac_refit":
        return _lib.fd_refit_opts(model, count, threshold, cxy[0], cxy[1], scale)
    if fn.startswith("fd_pnp"):
        return _lib.fd_pnp_opts(1 if refit else count, seed, count if refit else 1, threshold, *cam, (ctypes.c_double * 3)(*center),
                                scale)
    return _lib.fd_align_opts(model, 1 if refit else count, seed, count if refit else 1, threshold)


def invoke(L, ctx, fn, batch, opts, first, q_counts, qs, t, ts, idx, valid, given, outs):
    """One C ABI call with host pointers. first: the query side's own arrays (q_xy; p_xyz, p_valid; q_xyz, q_valid); t:
    the train side's (t_xy; t_xyz, t_valid); given: a refit's (in_model, in_inlier), else ()."""
    po = None if opts is None else ctypes.byref(opts)
    args = [*map(ptr, first), ptr(q_counts), qs, *map(ptr, t), ts, ptr(idx), ptr(valid), *map(ptr, given), *map(ptr, outs)]
    return getattr(L, fn)(ctx.ptr, batch, po, *args, 0)


def error_text(fd, ctx, fn, batch=1, qs=8, ts=8, opts=None):
    """The last-error text of a call that must be rejected, on zeroed arrays of 8 slots and no optional input."""
    from feature_detector_amd._lib import FD_ERR_INVALID

    L = fd.load()
    two_view, align = fn.startswith("fd_ransac"), fn.startswith("fd_align")
    q, t = np.zeros((1, 8, 2 if two_view else 3), np.float32), np.zeros((1, 8, 3 if align else 2), np.float32)
    first = (q,) if two_view else (q, None)
    train = (t, None) if align else (t,)
    model, inl = np.zeros(13), np.zeros(8, np.uint8)
    given = (model, inl) if fn.endswith("refit") else ()
    rc = invoke(L, ctx, fn, batch, opts, first, None, qs, train, ts, None, None, given, (model, None, None, None))
    assert rc == FD_ERR_INVALID, fn
    return L.fd_last_error(ctx.ptr).decode()


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_check_order(fd, ctx, fn):
    """Two faults at once: the slot checks come before the option checks, those in their order, and the range of
    hypotheses or rounds last; a null opts is caught before anything is read."""
    assert error_text(fd, ctx, fn, batch=0, opts=options(fn, 0, 1.0)) == BATCH
    assert error_text(fd, ctx, fn, opts=options(fn, 0, NAN)) == THRESHOLD
    if fn.startswith("fd_ransac"):
        assert error_text(fd, ctx, fn, opts=options(fn, 2, 0.0, model=2)) == MODEL
    elif fn.startswith("fd_align"):
        assert error_text(fd, ctx, fn, opts=options(fn, 2, 0.0, model=2)) == KIND
    else:
        assert error_text(fd, ctx, fn, opts=options(fn, 2, 0.0, cam=(0.0,) + PN.CAM[1:])) == THRESHOLD
    assert error_text(fd, ctx, fn, ts=7, opts=options(fn, 2, NAN)) == STRIDES
    assert error_text(fd, ctx, fn, batch=0, opts=None) == BAD


# ---- a call with every array given -------------------------------------------------------------------------------
B, S, T, HYP, SEED = 2, 12, 13, 64, 3
SENT_MODEL, SENT_INL, SENT_CNT, SENT_LAST = -123.25, 0xAB, -7, -9


def holes():
    """The slot arguments of the three scenes: counts (frame 1 one short), match_idx with a -1, an index past the end, a
    repeated one and the train side's extra slot, pair_valid with a 0 and a 2."""
    idx = np.tile(np.arange(S, dtype=np.int32), (B, 1))
    idx[0, 2], idx[0, 5], idx[1, 7], idx[1, 3] = -1, T - 1, 6, T
    valid = np.ones((B, S), np.uint8)
    valid[0, 9], valid[1, 1] = 0, 2
    return np.array([S, S - 1], np.int32), idx, valid


def side_mask(n, frame, slot, byte):
    m = np.ones((B, n), np.uint8)
    m[frame, slot] = byte
    return m


def pair_scene(model):
    q, t = zip(*(R.planted_scene(model, 40 + b, n=T, outliers=1)[:2] for b in range(B)))
    return np.ascontiguousarray(np.stack(q)[:, :S]), np.stack(t)


def pnp_scene():
    sc = [PN.scene(40 + b, n=T, outliers=1 / T) for b in range(B)]
    counts, idx, valid = holes()
    center, scale = PN.conditioning(np.stack([s["p"][:S] for s in sc]))
    return dict(p=np.ascontiguousarray(np.stack([s["p"][:S] for s in sc])), t=np.stack([s["t"] for s in sc]),
                p_valid=side_mask(S, 0, 11, 3), counts=counts, idx=idx, valid=valid, cam=PN.CAM, hypotheses=HYP, seed=SEED,
                threshold=PN.THRESHOLD, center=center, scale=scale)


def align_scene():
    sc = [A.scene(40 + b, n=T, outliers=1 / T) for b in range(B)]
    counts, idx, valid = holes()
    return dict(q=np.ascontiguousarray(np.stack([s["q"][:S] for s in sc])), t=np.stack([s["t"] for s in sc]),
                q_valid=side_mask(S, 0, 11, 3), t_valid=side_mask(T, 1, 4, 0), counts=counts, idx=idx, valid=valid,
                kind=A.SIMILARITY, hypotheses=HYP, seed=SEED, threshold=A.THRESHOLD)


def full_call(fd, ctx, fn, opts, width, first, t, given=()):
    """The call on host pointers with the slot arguments of holes() and all four outputs, into sentinel-filled arrays."""
    counts, idx, valid = holes()
    outs = (np.full((B, width), SENT_MODEL, np.float64), np.full((B, S), SENT_INL, np.uint8), np.full(B, SENT_CNT, np.int32),
            np.full(B, SENT_LAST, np.int32))
    L = fd.load()
    rc = invoke(L, ctx, fn, B, opts, first, counts, S, t, T, idx, valid, given, outs)
    assert rc == 0, L.fd_last_error(ctx.ptr)
    return outs


def same(got, exp, what):
    for k, (g, e) in enumerate(zip(got, exp)):
        assert g.dtype == e.dtype and g.shape == e.shape, (what, k)
        assert np.array_equal(g.view(np.uint8), e.view(np.uint8)), (what, k, g, e)


def given_of(exp):
    """A RANSAC restatement's model and inliers as a refit takes them (unwritten slots 0)."""
    return exp[0], np.where(exp[1] == SENT_INL, 0, exp[1]).astype(np.uint8)


@pytest.mark.parametrize("model", [R.FUNDAMENTAL, R.HOMOGRAPHY])
def test_two_view_with_every_array(fd, ctx, model):
    """fd_ransac: 5 inputs and 4 outputs; fd_ransac_refit: 7 and 4."""
    q, t = pair_scene(model)
    counts, idx, valid = holes()
    center, scale = R.conditioning((R.ROWS, R.COLS))
    exp = R.ransac_ref(q, t, counts, idx, valid, model=model, hypotheses=HYP, seed=SEED, center=center, scale=scale, fill=SENT_INL)
    assert (exp[3] >= 0).all()
    opts = options("fd_ransac", HYP, 1.0, model=model, cxy=center, scale=scale, seed=SEED)
    same(full_call(fd, ctx, "fd_ransac", opts, 9, (q,), (t,)), exp, "fd_ransac")
    given = given_of(exp)
    fit = RF.refit_ref(q, t, *given, counts, idx, valid, model=model, rounds=2, center=center, scale=scale, fill=SENT_INL)
    opts = options("fd_ransac_refit", 2, 1.0, model=model, cxy=center, scale=scale)
    same(full_call(fd, ctx, "fd_ransac_refit", opts, 9, (q,), (t,), given), fit, "fd_ransac_refit")


def test_pnp_with_every_array(fd, ctx):
    """fd_pnp_ransac: 6 inputs and 4 outputs; fd_pnp_refit: 8 and 4."""
    c = pnp_scene()
    exp = PN.run_ransac(c, fill=SENT_INL)
    assert (exp[3] >= 0).all()
    opts = options("fd_pnp_ransac", HYP, c["threshold"], center=c["center"], scale=c["scale"], seed=SEED)
    first = (c["p"], c["p_valid"])
    same(full_call(fd, ctx, "fd_pnp_ransac", opts, 12, first, (c["t"],)), exp, "fd_pnp_ransac")
    given = given_of(exp)
    fit = PN.run_refit(c, *given, 4, fill=SENT_INL)
    opts = options("fd_pnp_refit", 4, c["threshold"])
    same(full_call(fd, ctx, "fd_pnp_refit", opts, 12, first, (c["t"],), given), fit, "fd_pnp_refit")


def test_align_with_every_array(fd, ctx):
    """fd_align_ransac: 7 inputs and 4 outputs; fd_align_refit: 9 and 4, every staging buffer of the context."""
    c = align_scene()
    exp = A.run_ransac(c, fill=SENT_INL)
    assert (exp[3] >= 0).all()
    first, train = (c["q"], c["q_valid"]), (c["t"], c["t_valid"])
    opts = options("fd_align_ransac", HYP, c["threshold"], model=c["kind"], seed=SEED)
    same(full_call(fd, ctx, "fd_align_ransac", opts, 13, first, train), exp, "fd_align_ransac")
    given = given_of(exp)
    fit = A.run_refit(c, *given, 4, fill=SENT_INL)
    opts = options("fd_align_refit", 4, c["threshold"], model=c["kind"])
    same(full_call(fd, ctx, "fd_align_refit", opts, 13, first, train, given), fit, "fd_align_refit")
