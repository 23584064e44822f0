"""The shared candidate-list writer (csrc/fd_emit.h) on both branches of the sorted-segment flush, for each of
its three callers: k_corner (FD_PX=0), k_corner_lp (FD_PX=4) and k_fast.

Every case runs a batch in sorted-segment mode whose tiles are tall enough to overflow a wave's staging:
frame A carries a dense lattice in its top rows only, so its first workgroups overflow (plain flush, frame
marked unsorted) while its other workgroups write sorted segments; frame B overflows nowhere. The test asserts
those facts itself from the oracle's candidate positions and tests/point_geometry.py before it looks at the
GPU, then compares fd_points_response's full lists (bit for bit) and detect in both tie orders with the oracle.

Shapes (the smallest found that overflow: a taller tile needs batch * tiles_x * out_rows >= 7 * 10240 for the
corner kernels, 8 * 10240 for FAST; CPU oracle, candidates of frame A / B, overflowing workgroups of A):
  harris      px 0: 72 x 504 x 498, tile_h 12, 21 workgroups / frame: 6319 / 626, A overflows {0, 1} (max tile 625 > 508)
  shi_tomasi  px 4: 72 x 504 x 498, tile_h 12, 21 workgroups / frame: 9068 / 622, A overflows {0, 1, 2}
  fast            : 80 x 518 x 498, tile_h 14, 19 workgroups / frame: 9559 / 1441, A overflows {0, 1, 2} (max tile 992 > 640)
FD_PX=2 is left out: a lane of 2 columns needs 10 entries, i.e. tile_h >= 18 and twice the batch.
"""
import numpy as np
import pytest

import point_geometry as PG

pytestmark = pytest.mark.gpu

CASES = {  # name: kind, px, thr, batch, rows, cols, rows of frame A that carry the lattice
    "harris": (0, 0, 30.0, 72, 504, 498, 60),
    "shi_tomasi": (1, 4, 40.0, 72, 504, 498, 60),
    "fast": (2, 0, 10.0, 80, 518, 498, 70),
}


@pytest.fixture(scope="module")
def fd():
    import feature_detector_amd as fd

    fd.load()
    return fd


def make_frames(kind, rows, cols, band):
    """A: a dense lattice of random bright pixels in rows [0, band) of a black frame (corner detectors: the
    lattice pixels are strict 4-neighbour maxima at a density above 1/6; FAST: 3x3 bright blocks, period 6,
    every block pixel a FAST-12 corner) plus B's patch; B: a small noise patch on black."""
    rng = np.random.default_rng(7 + kind)
    rr, cc = np.mgrid[0:rows, 0:cols]
    a = np.zeros((rows, cols), np.uint8)
    if kind == 0:
        m = (rr + cc) % 2 == 0
        a[m] = rng.integers(0, 256, m.sum())
    elif kind == 1:
        m = (rr % 2 == 0) & (cc % 2 == 0)
        a[m] = rng.integers(128, 256, m.sum())
    else:
        m = (rr % 6 < 3) & (cc % 6 < 3)
        a[m] = rng.integers(200, 256, m.sum())
    a[band:] = 0
    b = np.zeros((rows, cols), np.uint8)
    b[rows // 2:rows // 2 + 40, 20:200] = rng.integers(0, 256, (40, 180))
    a[rows // 2:rows // 2 + 40, 20:200] = b[rows // 2:rows // 2 + 40, 20:200]  # (A's sorted segments are not all empty)
    return a, b


def oracle_candidates(oracle, kind, img, thr):
    if kind == 2:
        return oracle.fast_candidates(img, thr, None)
    return oracle.nms(oracle.response_map(img, kind, thr, None), thr)


@pytest.mark.parametrize("name", list(CASES))
def test_segment_flush_both_branches(fd, oracle, monkeypatch, name):
    torch = pytest.importorskip("torch")
    kind, px, thr, batch, rows, cols, band = CASES[name]
    monkeypatch.setenv("FD_DEBUG_AB", "1")  # (the library reads A/B switches only with it)
    monkeypatch.setenv("FD_PX", str(px))
    templ = make_frames(kind, rows, cols, band)
    which = np.array([0 if b % 8 == 0 else 1 for b in range(batch)])  # frame b is template which[b]
    cand = [oracle_candidates(oracle, kind, t, thr) for t in templ]

    # the launch this test is about, from the geometry and the oracle's candidates alone
    assert PG.corner_px(kind, batch, rows, cols, thr, forced=px) == px
    g = PG.point_geom(kind, batch, rows, cols, px)
    assert PG.use_seg_lists(g, rows, cols)
    over = [PG.overflowing_workgroups(g, c[1], c[2], kind, px) for c in cand]
    print(name, g, "candidates", [len(c[0]) for c in cand], "overflowing workgroups", over)
    assert over[0] and len(over[0]) < g["blocks_per_frame"]  # A: some workgroups overflow, others do not
    wg_a = set((PG.tile_of(g, cand[0][1], cand[0][2]) // 4).tolist())
    assert wg_a - over[0]  # ... and one that does not still has candidates (a sorted segment in a marked frame)
    assert not over[1] and len(cand[1][0]) > 0  # B: a frame that overflows nowhere

    frames = np.stack([templ[w] for w in which])
    dev = torch.from_numpy(frames).cuda()
    resp, idx, cnt = fd.point_response(("harris", "shi_tomasi", "fast")[kind], dev, thr)
    torch.cuda.synchronize()
    cnt = cnt.cpu().numpy()
    for b in range(batch):
        er, ex, ey = cand[which[b]]
        assert cnt[b] == len(er), (b, cnt[b], len(er))
        gi = idx[b, :cnt[b]].cpu().numpy().astype(np.int64)
        gr = resp[b, :cnt[b]].cpu().numpy()
        o = np.argsort(gi, kind="stable")
        assert np.array_equal(gi[o], ey.astype(np.int64) * cols + ex)
        assert np.array_equal(gr[o].view(np.uint32), er.view(np.uint32))
    for ties, mode in (("reference", 0), ("raster", 1)):
        exp = [oracle.detect(kind, t, 20, thr, 200, sort_mode=mode)[0] for t in templ]
        res = fd.detect_points(("harris", "shi_tomasi", "fast")[kind], dev, 200, 20, thr, ties=ties)
        flags = res.frame_flags()
        assert not (flags & np.uint32(fd.points.FRAME_GUARD | fd.points.FRAME_UNRESOLVED)).any(), flags
        for b in range(batch):
            assert np.array_equal(res.features(b), exp[which[b]]), (ties, b)
