"""GPU: k_select where a per-shape constant (grid geometry, the scan / grid regimes, the reciprocals of
udiv16q, the threads per sorted segment) or a barrier removed from the first chunk's path could go wrong,
against the oracle exactly as tests/test_gpu_select.py does, in both tie orders.

The grid thresholds are read from fd_kernels.h (the pipelined scan's state, fd_greedy.h ScanLds, takes
8 + 4 + 4 bytes per 64-batch of a chunk and 4 control words from the LDS grid's tail). At 120x160 no distance >= 1 reaches them (d = 1 gives
82 x 62 = 5084 cells, the most any distance can), so the threshold cases keep 120 rows and d = 1 and take
the widths whose cell counts fall in each regime: pipelined scan, LDS grid without room for the scan's
state, and the global grid."""
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

THR = {"harris": 30.0, "shi_tomasi": 40.0, "fast": 10.0}
KIND = {"harris": 0, "shi_tomasi": 1, "fast": 2}
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "feature_detector_amd", "csrc",
                      "fd_kernels.h")


def _const(name):
    src = open(HEADER).read()
    m = re.search(r"constexpr int %s = ([^;]+);" % name, src)
    assert m, name
    expr = re.sub(r"\bk[A-Z]\w+", lambda k: str(_const(k.group(0))), m.group(1))
    return int(eval(expr.replace("/", "//"), {"__builtins__": {}}))


def _scan_words():
    return (_const("kSelectChunk") // 64) * 4 + 4


def _cells(rows, cols, d):
    return ((cols + d) // (d + 1) + 2) * ((rows + d) // (d + 1) + 2)


def _threshold_widths(rows=120, d=1):
    """Widths at which the bordered grid of a rows-high frame lies just inside the pipelined scan's limit,
    between it and the LDS limit, at the LDS limit's side and past it."""
    lds = _const("kGridLdsCells")
    fast = lds - _scan_words()
    assert _cells(120, 160, 1) < fast  # (why 120x160 alone cannot straddle them)
    pick = {}
    for cols in range(16, 4096):
        c = _cells(rows, cols, d)
        regime = "scan" if c <= fast else ("lds" if c <= lds else "global")
        if regime == "scan":
            pick["scan"] = cols  # the widest below the scan's limit
        else:
            pick.setdefault(regime, cols)  # the narrowest of each later regime
        if regime == "global":
            break
    assert set(pick) == {"scan", "lds", "global"}, pick
    return [pick["scan"], pick["lds"], pick["global"]]


@pytest.fixture(scope="module")
def fd():
    import feature_detector_amd as fd

    fd.load()
    return fd


def _check(fd, oracle, name, frames, need, dist, min_accept=1, min_cands=0):
    if min_cands:  # the case is non-trivial: more candidates than one scan batch in some frame
        n_cand = max(len(oracle.detect(KIND[name], f, dist, THR[name], need, sort_mode=1)[1][0]) for f in frames)
        assert n_cand > min_cands, n_cand
    for ties, mode in (("raster", 1), ("reference", 0)):
        res = fd.detect_points(name, frames, need, dist, THR[name], ties=ties)
        total = 0
        for i in range(frames.shape[0]):
            exp = oracle.detect(KIND[name], frames[i], dist, THR[name], need, sort_mode=mode)[0]
            total += len(exp)
            np.testing.assert_array_equal(res.features(i), exp, err_msg=f"{name} frame {i} ties={ties}")
        assert total >= min_accept, "the case is trivial: nothing accepted"


@pytest.mark.parametrize("dist", [1, 2, 6, 20])
@pytest.mark.parametrize("rows,cols", [(97, 131), (61, 259)])
@pytest.mark.parametrize("name", ["harris", "fast"])
def test_odd_sizes_decode_and_partial_cells(fd, oracle, name, rows, cols, dist):
    # cols and d + 1 divide neither the frame nor each other: udiv16q's correction, the grid's partial last cell
    img = oracle.make_frame("noise", 1000 + rows + dist, rows, cols)
    _check(fd, oracle, name, img[None], 50, dist, min_cands=64)


def test_grid_flags_at_120x160(fd, oracle):
    # distance 0 (no grid) and 1 (the largest grid this frame can have: far below both thresholds)
    img = oracle.make_frame("noise", 2001, 120, 160)
    for dist in (0, 1):
        for name in ("harris", "fast"):
            _check(fd, oracle, name, img[None], 50, dist, min_cands=64)


@pytest.mark.parametrize("which", [0, 1, 2])
def test_grid_flags_across_thresholds(fd, oracle, which):
    # cells on both sides of kGridLdsCells - kScanLdsWords and of kGridLdsCells (the global-grid path)
    cols = _threshold_widths()[which]
    lds = _const("kGridLdsCells")
    c = _cells(120, cols, 1)
    assert [c <= lds - _scan_words(), lds - _scan_words() < c <= lds, c > lds][which]
    img = oracle.make_frame("noise", 2100 + which, 120, cols)
    for name in ("harris", "fast"):
        _check(fd, oracle, name, img[None], 300, 1, min_cands=64)


def test_partial_batches(fd, oracle):
    # the 64x64 checker frame (280 Harris candidates: the last scan batch is partial), and a 32x32 one
    # with fewer than 64 candidates: batch 0 is the only scan batch, and partial
    img = oracle.make_frame("checker", 3001, 64, 64)
    _check(fd, oracle, "harris", img[None], 200, 20)
    small = oracle.make_frame("checker", 3001, 32, 32)
    n_cand = len(oracle.detect(0, small, 3, THR["harris"], 200, sort_mode=1)[1][0])
    assert 0 < n_cand < 64, n_cand
    for dist in (3, 20):
        _check(fd, oracle, "harris", small[None], 200, dist)


@pytest.mark.parametrize("rows,cols", [(48, 64), (96, 128)])
@pytest.mark.parametrize("name", ["harris", "fast"])
def test_need_never_reached(fd, oracle, name, rows, cols):
    # every candidate is visited; at 96x128 (1018 Harris, 1981 FAST candidates) over several chunks: the
    # sorted segments' later prefixes, gathered behind their own barrier
    img = oracle.make_frame("noise", 3002 if rows == 48 else 3003, rows, cols)
    _check(fd, oracle, name, img[None], 100000, 3, min_cands=64)


@pytest.mark.parametrize("need", [1, 64, 65])
def test_need_cutoff_around_batch_0(fd, oracle, need):
    img = oracle.make_frame("noise", 4001, 120, 160)
    for dist in (0, 1, 5):
        _check(fd, oracle, "harris", img[None], need, dist, min_cands=64)


def test_mixed_batch_with_empty_frame(fd, oracle):
    frames = np.stack([np.zeros((120, 160), np.uint8), oracle.make_frame("noise", 5001, 120, 160),
                       oracle.make_frame("checker", 5002, 120, 160)])
    assert len(oracle.detect(0, frames[0], 5, THR["harris"], 60, sort_mode=1)[1][0]) == 0
    for name in ("harris", "fast"):
        _check(fd, oracle, name, frames, 60, 5, min_cands=64)


def test_constants_follow_the_call(fd, oracle):
    # the same context: 200x300 Harris, 97x131 FAST, 200x300 Harris again
    a = oracle.make_frame("noise", 6001, 200, 300)
    b = oracle.make_frame("noise", 6002, 97, 131)
    for name, img in (("harris", a), ("fast", b), ("harris", a)):
        _check(fd, oracle, name, img[None], 150, 7, min_cands=64)
