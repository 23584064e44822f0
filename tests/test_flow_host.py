"""CPU checks of the tracker's yardstick tests/flow_ref.py (the numpy restatement of fd_pyr_build /
fd_flow_lk in include/fd_hip.h) and of the entry points that need no GPU."""
import ctypes

import numpy as np

import flow_cases as C
import flow_ref as R


def test_restatement_tracks_the_golden_image(oracle, image_png):
    """Guards against a broken restatement (not a measurement): the golden image's crop displaced by
    (3, -2), 60 Shi-Tomasi corners, 3 levels, r 7, 30 iterations, epsilon 0.01, min_eigen 1e-4. At least 80 %
    must be tracked to within 0.1 px (a prototype of the contract gave 54 of 60, 3 lost, median 0.0007 px)."""
    assert image_png.shape == (480, 752)
    prev = np.ascontiguousarray(image_png[24:264, 24:344])
    nxt = np.ascontiguousarray(image_png[26:266, 21:341])  # content moves by (+3, -2)
    assert np.array_equal(nxt[10:100, 13:100], prev[12:102, 10:97])
    feat, _ = oracle.detect(1, prev, 15, 40.0, 60, sort_mode=0)
    assert len(feat) == 60
    xy, st, err, cnt = R.flow_ref(prev, nxt, feat[None], levels=3, half_window=7, max_iters=30, epsilon=0.01, min_eigen=1e-4)
    e = np.hypot(xy[0, :, 0] - feat[:, 0] - 3, xy[0, :, 1] - feat[:, 1] + 2)
    good = (st[0] == 1) & (e < 0.1)
    print("within 0.1 px:", good.sum(), "lost:", (st[0] != 1).sum(), "median error:", np.median(e[st[0] == 1]))
    assert good.sum() >= 48
    assert cnt[0] == (st[0] == 1).sum()


def test_zero_shift_returns_xy_in_one_iteration_per_level(oracle):
    img = oracle.make_frame("checker", 9, 64, 80)
    levels = R._levels_i64(img[None], 3)[0]
    for xy in ([40, 32], [17.25, 20.5], [33.125, 40.75]):
        xy = np.array(xy, np.float32)
        trace = []
        out, st, err = R.track_one(levels, levels, xy, None, 64, 80, 7, 30, 0.01, 1e-4, -1.0, trace=trace)
        assert st == 1 and np.array_equal(out, xy) and err == 0
        assert [(l, n) for l, u, n in trace if u] and all(n == 1 for l, u, n in trace if u)
        assert trace[-1] == (0, True, 1)


def test_pyramid_restatement_by_hand():
    f = np.array([[0, 1, 2, 3, 4, 5, 6],
                  [10, 11, 12, 13, 14, 15, 16],
                  [255, 255, 0, 0, 7, 8, 200],
                  [255, 254, 0, 1, 9, 9, 200],
                  [50, 60, 70, 80, 90, 100, 110]], np.uint8)
    p = R.pyr_ref(f, 2)
    assert p[0].shape == (1, 5, 7) and np.array_equal(p[0][0], f)
    # (0+1+10+11+2)>>2 = 6, (2+3+12+13+2)>>2 = 8, (4+5+14+15+2)>>2 = 10; the odd row and column are dropped
    assert p[1].tolist() == [[[6, 8, 10], [255, 0, 8]]]
    assert R.pyr_ref(f, 3)[2].tolist() == [[[(6 + 8 + 255 + 0 + 2) >> 2]]]


def test_pyr_layout_offsets():
    import feature_detector_amd as fd

    assert R.pyr_layout(1, 1, 1, 1) == [0, 256]
    assert R.pyr_layout(3, 37, 53, 3) == [0, 5888, 7424, 7936]  # 5883 -> 5888; + 3*18*26 = 7292 -> 7424; + 3*9*13 = 7775
    for shape in ((1, 1, 1, 1), (3, 37, 53, 3), (2, 64, 256, 6), (64, 720, 1280, 3), (1, 480, 752, 4)):
        assert fd.pyramid_layout(*shape) == R.pyr_layout(*shape)
    L = fd.load()
    off = (ctypes.c_int64 * 8)()
    for bad in ((0, 8, 8, 1), (1, 8, 8, 0), (1, 8, 8, 7), (1, 8, 40, 5), (1, 40, 8, 5), (1, 0, 8, 1)):
        assert L.fd_pyr_layout(*bad, off) == fd._lib.FD_ERR_INVALID
    assert L.fd_pyr_layout(1, 8, 8, 1, None) == fd._lib.FD_ERR_INVALID


def test_half_windows_reach_every_round_count():
    """k_flow_lk is instantiated per ROUNDS = ceil((2r + 1)^2 / 64): half_window 1..10 reach all seven, and 8
    and 9 are the only ones that reach 5 and 6 (tests/test_gpu_flow_edges.py launches all ten)."""
    got = {r: C.rounds(r) for r in range(1, 11)}
    assert got == {1: 1, 2: 1, 3: 1, 4: 2, 5: 2, 6: 3, 7: 4, 8: 5, 9: 6, 10: 7}
    assert set(got.values()) == set(range(1, 8))


def test_saturated_frames_pass_the_32_bit_sums():
    """The inputs of test_gpu_flow_edges.py::test_saturated_contrast have what they were built for: level-0
    window sums that a 32-bit total would get wrong. sum gx*gx reaches 2^31 at half_window 8, 9 and 10 and
    2^32 at 10; with the content moving by (-1, -1) the first iteration's b1 or b2 is below -2^31 (the
    arithmetic shift of negative lane values and the signed recombination in wave_sum_i32)."""
    prev, nxt = C.sat_frames()
    assert set(np.unique(prev)) == {0, 255} and np.array_equal(nxt[0, :-1, :-1], prev[0, 1:, 1:])
    xy = C.sat_features()[0]
    assert xy.shape == (24, 2) and (xy == np.rint(xy)).all(1).sum() == 8
    for r in (8, 9, 10):
        sums = [C.level0_sums(prev[0], nxt[0], p, r) for p in xy]
        a11, b = max(s[0] for s in sums), min(min(s[1], s[2]) for s in sums)
        print(f"half_window {r}: largest sum gx*gx {a11:.4g}, most negative b {b:.4g}")
        assert a11 >= 2 ** 31
        assert b < 0 and -b >= 2 ** 31
        if r == 10:
            assert a11 >= 2 ** 32
    # the sums are the tracker's own: at an integral feature d = 0 gives the first iteration of track_one
    p = xy[0]
    st = R.track_one([prev[0].astype(np.int64)], [nxt[0].astype(np.int64)], p, None, C.ROWS, C.COLS, 10, 1, 0.01, 1e-4, -1.0)
    assert st[1] == 1 and not np.array_equal(st[0], p)


def test_odd_frame_features_pass_the_coarse_levels_last_column():
    """97 x 131 loses a column at every level (65, 32, 16 columns): a feature on the last column of level 0
    lies beyond the last column of a coarser level, where the template patch is all clamped reads, and
    level 0 of frame 1 starts at an odd byte offset."""
    xy = C.odd_features()
    assert xy.shape == (3, 20, 2)
    rows, cols = C.ODD_ROWS, C.ODD_COLS
    for p in ((cols - 1, rows - 1), (cols - 1, 40), (50, rows - 1), (cols - 1.25, rows - 1.5), (0, 0), (cols - 1, 0), (0, rows - 1)):
        assert (xy[0] == np.array(p, np.float32)).all(1).any(), p
    beyond = C.beyond_last_column(xy[0], cols, 4)
    assert beyond and {l for _, l in beyond} >= {1, 2, 3} and all(l > 0 for _, l in beyond)
    assert any(np.float32(p[1]) * np.float32(0.5) > (rows >> 1) - 1 for p in xy[0])
    assert (rows * cols) % 2 == 1  # frame 1's level 0 starts at an odd byte
    assert (rows >> 3, cols >> 3) == (12, 16)


def test_null_context_is_rejected():
    import feature_detector_amd as fd
    from feature_detector_amd._lib import fd_flow_opts

    L = fd.load()
    buf = np.zeros(4096, np.uint8)
    p = ctypes.c_void_p(buf.ctypes.data)
    assert L.fd_pyr_build(None, p, 0, 1, 8, 8, 1, p, 0) == fd._lib.FD_ERR_INVALID
    opts = fd_flow_opts(7, 30, 0.01, 1e-3, -1.0, -1.0)
    assert L.fd_flow_lk(None, 1, 8, 8, 1, ctypes.byref(opts), p, p, p, None, None, 1, None, p, p, None, None, 0) == fd._lib.FD_ERR_INVALID
