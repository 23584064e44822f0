"""CPU: tests/refine_ref.py (the yardstick of the GPU refinement tests) against a rendered scene and cases
worked by hand, and fd_points_refine's entry checks that need no GPU."""
import ctypes

import numpy as np

import refine_cases as C
import refine_ref as R


def test_restatement_finds_rendered_corners():
    """Guards the yardstick: 12 rotated two-tone corners with known sub-pixel positions, each started from the
    rounded truth and from that plus (1, -1) and (-2, 1). Not a measurement."""
    img, corners = C.corner_scene()
    i64 = img.astype(np.int64)
    errs, iters = [], []
    for cx, cy, _ in corners:
        for ox, oy in ((0, 0), (1, -1), (-2, 1)):
            trace = []
            out, st = R.refine_one(i64, (np.rint(cx) + ox, np.rint(cy) + oy), 5, 20, 0.01, 1e-3, 5.0, trace=trace)
            errs.append(float(np.hypot(float(out[0]) - cx, float(out[1]) - cy)) if st == R.ST_REFINED else np.inf)
            iters.append(len(trace))
    errs = np.array(errs)
    print(f"median {np.median(errs):.4f} px, max {errs.max():.4f} px, iterations <= {max(iters)}")
    assert len(errs) == 36 and (errs <= 0.1).sum() >= 30


def test_constant_frame_is_flat():
    img = np.full((40, 50), 123, np.int64)
    out, st = R.refine_one(img, (20.25, 17.5), 5, 20, 0.01, 1e-3, 5.0)
    assert st == R.ST_FLAT and out.tolist() == [20.25, 17.5]
    out, st = R.refine_one(img, (20.25, 17.5), 5, 20, 0.01, 0.0, 5.0)  # det = 0 fails without a threshold too
    assert st == R.ST_FLAT


def test_symmetric_corner_stays_in_one_iteration():
    """An axis-aligned noise-free corner, symmetric about the pixel (30, 25): G's terms are even in (u, v), B's odd,
    so B = 0 and the first step is exactly zero."""
    img = np.full((50, 60), 60, np.int64)
    yy, xx = np.mgrid[0:50, 0:60]
    img[((xx > 30) & (yy > 25)) | ((xx < 30) & (yy < 25))] = 200
    img[(xx == 30) | (yy == 25)] = 130
    trace = []
    out, st = R.refine_one(img, (30.0, 25.0), 5, 20, 0.01, 1e-3, 5.0, trace=trace)
    assert st == R.ST_REFINED and out.tolist() == [30.0, 25.0] and len(trace) == 1
    (g11, g12, g22, b1, b2), _ = trace[0]
    assert b1 == 0 and b2 == 0 and g11 > 0 and g22 > 0
    # started one pixel off it comes back
    out, st = R.refine_one(img, (31.0, 24.0), 5, 20, 0.01, 1e-3, 5.0)
    assert st == R.ST_REFINED and np.abs(out - np.array([30, 25], np.float32)).max() < 0.05


def test_positions_outside_the_frame():
    img, _ = C.corner_scene()
    rows, cols = img.shape
    for xy in ((np.nan, 5), (5, np.inf), (-np.inf, 5), (-0.5, 5), (cols - 0.5, 5), (5, -0.5), (5, rows - 0.5)):
        out, st = R.refine_one(img.astype(np.int64), xy, 5, 20, 0.01, 1e-3, 5.0)
        assert st == R.ST_OUTSIDE
        assert np.array_equal(out.view(np.uint32), np.array(xy, np.float32).view(np.uint32))


def test_batch_form_counts_valid_and_unwritten_slots():
    frames, corners = C.main_frames()
    xy = C.main_features(corners)
    valid = np.ones((2, 40), np.uint8)
    valid[0, 3] = valid[1, 5] = 0
    init = (np.full((2, 40, 2), -77.0, np.float32), np.full((2, 40), 99, np.uint8))
    oxy, st, cnt = R.refine_ref(frames, xy, counts=C.COUNTS, valid=valid, init=init)
    assert st[0, 3] == 0 and st[1, 5] == 0 and np.array_equal(oxy[0, 3], xy[0, 3])
    assert (st[1, 17:] == 99).all() and (oxy[1, 17:] == -77.0).all()
    assert cnt.tolist() == [(st[0] == 1).sum(), (st[1, :17] == 1).sum()] and cnt[0] >= 30
    lost = (st != 1) & (st != 99)
    assert np.array_equal(oxy[lost], xy[lost])


def test_null_context_is_rejected():
    import feature_detector_amd as fd
    from feature_detector_amd._lib import fd_refine_opts

    L = fd.load()
    opts = fd_refine_opts(5, 20, 0.01, 1e-3, 5.0)
    buf = np.zeros(64, np.float32)
    p = ctypes.c_void_p(buf.ctypes.data)
    assert L.fd_points_refine(None, p, 0, 1, 8, 8, ctypes.byref(opts), p, None, None, 1, p, p, None, 0) == fd._lib.FD_ERR_INVALID
