"""GPU: the point path on the adversarial frames of tests/adversarial_frames.py, bit-exact against the oracle.

tests/test_adversarial_frames.py proves on the CPU that the frames meet their conditions. Here:

* saturated frames: response maps, candidates and features with tensor sums at the ends of the domain of
  corner_response2's biased integer sums, at every lane width of the per-pixel kernels and with a threshold
  below every response (the G1 = false branch, negative responses stored);
* saturated noise through the selection: hundreds of equal responses in the top level-0 key bins, both tie
  orders, every distance / need regime;
* stamp frames: 511 ... 4,100 bit-identical detector-produced candidates, i.e. exact ties on both sides of
  k_select's sub-chunk (512) and chunk (2048) and above two chunks, where the histogram cut cannot split the
  tie and the radix descent runs down to the index bits; reference and raster order, host and device frames,
  every prelude setting of k_select_reference;
* FAST: all 65,536 (centre, sample) value pairs and all 65,536 ring patterns in bright, dark and mixed form,
  each centre in every byte position of its dword, plain and masked.
"""
import numpy as np
import pytest

import adversarial_frames as af
from test_adversarial_frames import STAMP_COUNTS
from test_gpu_points import KIND, THR, assert_same_candidates, build_mask, check_detect, oracle_candidates

pytestmark = pytest.mark.gpu

GUARD_BIT = 0x04000000  # k_select's consistency guard (part of FD_FRAME_GUARD)
SIZES = [(61, 253), (120, 160)]  # cols % 4 != 0 (unaligned dword loads), and aligned


@pytest.fixture(scope="module")
def fd():
    import feature_detector_amd as fd

    fd.load()
    return fd


def saturated_frames(rows, cols):
    return np.stack([af.stripes(rows, cols, "v"), af.stripes(rows, cols, "h"), af.stripes(rows, cols, "diag"),
                     af.stripes(rows, cols, "anti"), af.blocks(rows, cols, 4), af.blocks(rows, cols, 5),
                     af.two_level(rows, cols, 3), af.n_level(rows, cols, 4, 4)])


_memo = {}


def memo(key, fn):
    """Oracle results shared between the parametrised cases (never modified by a test)."""
    if key not in _memo:
        _memo[key] = fn()
    return _memo[key]


def low_threshold(oracle, frames, name):
    """A threshold below every response of every frame, from the oracle's unthresholded maps."""
    lo = min(float(oracle.response_map(f, KIND[name], -np.inf).min()) for f in frames)
    return float(np.float32(min(2.0 * lo, -1.0)))


def assert_same_list(got_resp, got_idx, exp, cols):
    er, ex, ey = exp
    assert len(got_idx) == len(er)
    o = np.argsort(got_idx, kind="stable")
    assert np.array_equal(got_idx[o], ey.astype(np.int64) * cols + ex)
    assert np.array_equal(got_resp[o].view(np.uint32), er.view(np.uint32))


# ------------------------------------------------------------------ response maps on saturated frames

@pytest.mark.parametrize("px", ["0", "2", "4", "8"])
@pytest.mark.parametrize("size", SIZES)
def test_saturated_maps_and_lists(fd, oracle, monkeypatch, size, px):
    """Map and raster-ordered candidates (k_corner), and the unordered list of the lane-wide kernels
    (FD_PX: k_corner / k_corner_lp with 2, 4, 8 columns per lane), at the default threshold, 0.0 and a
    threshold below every response."""
    torch = pytest.importorskip("torch")
    monkeypatch.setenv("FD_DEBUG_AB", "1")  # (the library reads A/B switches only with it)
    monkeypatch.setenv("FD_PX", px)
    rows, cols = size
    frames = saturated_frames(rows, cols)
    dev = torch.from_numpy(frames).cuda()
    for name in ("harris", "shi_tomasi"):
        low = memo(("low", size, name), lambda: low_threshold(oracle, frames, name))
        assert low < 0
        for thr in (THR[name], 0.0, low):
            exp = memo(("map", size, name, thr), lambda: [
                (m, oracle.nms(m, thr)) for m in (oracle.response_map(f, KIND[name], thr) for f in frames)])
            got, rmap = fd.point_candidates(name, frames, 15, thr, response_map=True)
            resp, idx, cnt = fd.point_response(name, dev, thr)
            torch.cuda.synchronize()
            cnt = cnt.cpu().numpy()
            for b, (emap, ecand) in enumerate(exp):
                assert np.array_equal(rmap[b].view(np.uint32), emap.view(np.uint32)), (name, thr, b)
                assert_same_candidates(got[b], ecand)
                assert_same_list(resp[b, :cnt[b]].cpu().numpy(), idx[b, :cnt[b]].cpu().numpy().astype(np.int64), ecand, cols)
            if thr == low and name == "harris":  # (Shi-Tomasi's larger eigenvalue is never negative)
                assert min(float(e[0].min()) for e in exp) < -1e8  # the negative responses are in the maps


@pytest.mark.parametrize("px", ["0", "2", "4", "8"])
def test_saturated_detect_lane_widths(fd, oracle, monkeypatch, px):
    """Features through detect (sorted-segment lists written by each per-pixel variant), both tie orders."""
    monkeypatch.setenv("FD_DEBUG_AB", "1")
    monkeypatch.setenv("FD_PX", px)
    for size in SIZES:
        frames = saturated_frames(*size)
        for name in ("harris", "shi_tomasi"):
            for b in range(len(frames)):
                check_detect(fd, oracle, name, frames[b], 5, THR[name], 100)
            check_detect(fd, oracle, name, frames[6], 5, 0.0, 100)
            check_detect(fd, oracle, name, frames[7], 5, low_threshold(oracle, frames, name), 100)


# ------------------------------------------------------------------ selection on saturated frames

NOISE_FRAMES = {"two_level_120x160": lambda: af.two_level(120, 160, 1),
                "two_level_240x320": lambda: af.two_level(240, 320, 2),
                "four_level_240x320": lambda: af.n_level(240, 320, 5, 4)}


@pytest.mark.parametrize("name", ["harris", "shi_tomasi", "fast"])
@pytest.mark.parametrize("frame", sorted(NOISE_FRAMES))
def test_saturated_selection(fd, oracle, frame, name):
    img = NOISE_FRAMES[frame]()
    for dist in (0, 1, 5, 20):
        for need in (64, 300, 100000):
            check_detect(fd, oracle, name, img, dist, THR[name], need)


def test_saturated_selection_with_priors(fd, oracle):
    img = NOISE_FRAMES["two_level_240x320"]()
    prior = np.array([(x, y) for x in range(17, 320, 41) for y in range(13, 240, 37)], np.float32)
    for name in ("harris", "shi_tomasi", "fast"):
        check_detect(fd, oracle, name, img, 5, THR[name], len(prior) + 300, prior)


# ------------------------------------------------------------------ mass ties through the detector

@pytest.fixture(params=["auto", "wide", "narrow"])
def ref_wide(request, monkeypatch):
    """k_select_reference's multi-workgroup prelude: by frame size, forced on, forced off (FD_REF_WIDE)."""
    if request.param != "auto":
        monkeypatch.setenv("FD_DEBUG_AB", "1")
        monkeypatch.setenv("FD_REF_WIDE", "1" if request.param == "wide" else "0")
    return request.param


def both_orders(fd, oracle, name, frames, need, dist, key):
    """Host frames in both tie orders and device frames in the reference order (no host fallback behind
    the device path: check() raises on FRAME_UNRESOLVED) against the oracle; no guard bit anywhere."""
    import torch

    ref = fd.detect_points(name, frames, need, dist, THR[name])
    ras = fd.detect_points(name, frames, need, dist, THR[name], ties="raster")
    dev = fd.detect_points(name, torch.from_numpy(np.ascontiguousarray(frames)).cuda(), need, dist, THR[name],
                           ties="reference")
    torch.cuda.synchronize()
    dev.check()
    for res in (ref, ras, dev):
        assert not (res.frame_flags() & GUARD_BIT).any()
        assert not (res.frame_flags() & (fd.points.FRAME_GUARD | fd.points.FRAME_UNRESOLVED)).any()
    for b in range(frames.shape[0]):
        e0, e1 = memo((key, name, b, need, dist), lambda: tuple(
            oracle.detect(KIND[name], frames[b], dist, THR[name], need, sort_mode=m)[0] for m in (0, 1)))
        np.testing.assert_array_equal(ref.features(b), e0, err_msg=f"{name} frame {b} reference order")
        np.testing.assert_array_equal(ras.features(b), e1, err_msg=f"{name} frame {b} raster order")
        np.testing.assert_array_equal(dev.features(b), e0, err_msg=f"{name} frame {b} device path")
        if not np.array_equal(e0, e1):
            assert ref.frame_flags()[b] & fd.points.FRAME_TIES and ref.frame_flags()[b] & fd.points.FRAME_RESOLVED
            assert dev.frame_flags()[b] & fd.points.FRAME_RESOLVED
            assert ras.frame_flags()[b] & fd.points.FRAME_TIES


@pytest.mark.parametrize("name", ["harris", "shi_tomasi"])
@pytest.mark.parametrize("n", STAMP_COUNTS)
def test_stamp_ties(fd, oracle, ref_wide, n, name):
    """n bit-identical candidates (2n in two values for Shi-Tomasi): a need that stops inside the tie run,
    one never reached, a distance at which every stamp is accepted, and one at which neighbours suppress
    each other, so that the features depend on the whole order."""
    img, _ = af.stamp_frame(*af.stamp_shape(n), n)
    for dist, need in ((0, n // 2), (0, 100000), (5, 100000), (20, 100000)):
        both_orders(fd, oracle, name, img[None], need, dist, ("stamps", n))


@pytest.mark.parametrize("name", ["harris", "shi_tomasi"])
def test_stamp_ties_mixed_batch(fd, oracle, ref_wide, name):
    rows, cols = af.stamp_shape(2049)
    frames = np.stack([af.stamp_frame(rows, cols, 513)[0], af.stamp_frame(rows, cols, 2049)[0],
                       np.full((rows, cols), 100, np.uint8), oracle.make_frame("noise", 9, rows, cols)])
    for dist, need in ((0, 300), (20, 100000)):
        both_orders(fd, oracle, name, frames, need, dist, "stamp_batch")


# ------------------------------------------------------------------ FAST, exhaustive

def fast_batches():
    yield "pairs", lambda: np.stack([af.fast_pairs(p, p + 64) for p in range(0, 256, 64)])
    for mode in ("bright", "dark", "mixed"):
        yield mode, lambda mode=mode: np.stack([af.fast_rings(lo, lo + 16384, mode) for lo in range(0, 65536, 16384)])


def as_map(cand, shape):
    resp, x, y = cand
    m = np.zeros(shape, np.float32)
    m[y, x] = resp
    return m


@pytest.mark.parametrize("batch", ["pairs", "bright", "dark", "mixed"])
def test_fast_exhaustive(fd, oracle, batch):
    """k_fast's byte-parallel compare (clamps at p < 15 and p > 240, the non-strict edge v == p +- 15, the
    127/128 split) on every (p, v) pair, and its ring bit order and run table on every 16-bit pattern:
    the whole candidate list against the oracle, the patch centres against the rule."""
    frames = dict(fast_batches())[batch]()
    assert frames.shape == (4, 448, 1792)
    got = fd.point_candidates("fast", frames, 15, THR["fast"])
    for b in range(4):
        exp = memo(("fast", batch, b), lambda: oracle.fast_candidates(frames[b], THR["fast"]))
        assert_same_candidates(got[b], exp)
        cy, cx, _, want = af.fast_expected_at_centres(frames[b], THR["fast"])
        assert np.array_equal(as_map(got[b], frames[b].shape)[cy, cx].view(np.uint32), want.view(np.uint32))
    check_detect(fd, oracle, "fast", frames[1], 5, THR["fast"], 300)


def test_fast_exhaustive_masked(fd, oracle):
    """The MASKED variant of k_fast on the (p, v) pairs: a prior lattice whose boxes cover a part of the
    patches, so that the candidate numbering (the running offset) skips the masked pixels."""
    frames = np.stack([af.fast_pairs(p, p + 64) for p in range(0, 256, 64)])
    prior = [np.array([(x + 5 * b, y + 3 * b) for x in range(9, 1792, 53) for y in range(11, 448, 47)], np.float32)
             for b in range(4)]
    got = fd.point_candidates("fast", frames, 10, THR["fast"], prior=prior)
    for b in range(4):
        mask = build_mask(448, 1792, 10, prior[b])
        assert 0.1 < 1.0 - mask.mean() < 0.9
        assert_same_candidates(got[b], oracle.fast_candidates(frames[b], THR["fast"], mask))
