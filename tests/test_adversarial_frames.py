"""CPU: the adversarial frames (tests/adversarial_frames.py) meet the conditions that
tests/test_gpu_adversarial.py relies on, measured on the oracle, so that no GPU test there passes by being
trivial: tensor sums at the ends of their domain, exact counts of tied candidates on both sides of the
selection's sub-chunk (512) and chunk (2048) and above two chunks, tie orders that select different
features, and the FAST rule at every patch centre (which also checks the oracle against a restatement that
is not the oracle).
"""
import numpy as np
import pytest

import adversarial_frames as af

HARRIS, SHI_TOMASI = 0, 1
THR = {HARRIS: 30.0, SHI_TOMASI: 40.0}
S_MAX = 9 * 255 * 255

# Tied-candidate counts around kSubChunk = 512 and kSelectChunk = 2048 (fd_kernels.h), and one above two
# chunks: 4,100 stamps, on the smallest near-square frame that holds them (773 x 785; 640 x 640 holds 2,704).
STAMP_COUNTS = [511, 512, 513, 2047, 2048, 2049, 4100]


def tensor_sums_i64(img):
    """Sxx, Syy, Sxy of the interior [2, R-2) x [2, C-2): central differences, 3x3 box sums
    (feature_point_harris_detector.cpp:35-41, :66-116), in int64."""
    i = img.astype(np.int64)
    ix = np.zeros_like(i)
    iy = np.zeros_like(i)
    ix[:, 1:-1] = i[:, 2:] - i[:, :-2]
    iy[1:-1, :] = i[2:, :] - i[:-2, :]
    R, C = i.shape

    def box(a):
        return sum(a[1 + dr:R - 3 + dr, 1 + dc:C - 3 + dc] for dr in range(3) for dc in range(3))

    return box(ix * ix), box(iy * iy), box(ix * iy)


@pytest.mark.parametrize("shape", [(61, 253), (120, 160)])
def test_stripes_reach_the_extreme_sums(oracle, shape):
    want = {"v": (S_MAX, 0, 0), "h": (0, S_MAX, 0), "diag": (S_MAX, S_MAX, S_MAX), "anti": (S_MAX, S_MAX, -S_MAX)}
    for kind, (exx, eyy, exy) in want.items():
        img = af.stripes(*shape, kind)
        sxx, syy, sxy = tensor_sums_i64(img)
        assert (sxx == exx).all() and (syy == eyy).all() and (sxy == exy).all(), kind
        # the oracle's int32 sums are these sums
        oxx, oyy, oxy = oracle.tensor_sums(img)
        for o, s in ((oxx, sxx), (oyy, syy), (oxy, sxy)):
            assert np.array_equal(o[2:-2, 2:-2], s)
    assert S_MAX < 2 ** 22  # the domain fd_corner_common.h states for its biased sums


def test_blocks_and_stripes_have_no_candidate_but_extreme_maps(oracle):
    frames = [af.stripes(120, 160, k) for k in ("v", "h", "diag", "anti")] + [af.blocks(120, 160, 4), af.blocks(120, 160, 5)]
    for i, img in enumerate(frames):
        for kind in (HARRIS, SHI_TOMASI):
            # flat maxima of equal responses: the strict 4-neighbour NMS lets none through
            assert len(oracle.nms(oracle.response_map(img, kind, THR[kind]), THR[kind])[0]) == 0
        full = oracle.response_map(img, HARRIS, -np.inf)
        if i < 4:
            assert full.max() == 0 and full.min() < -1e8  # stripes: only large negative responses
        else:
            assert full.max() > 1e9  # blocks: plateaus of equal responses in the top key bins


def _tie_groups(resp):
    _, counts = np.unique(resp.view(np.uint32), return_counts=True)
    return counts


@pytest.mark.parametrize("kind", [HARRIS, SHI_TOMASI])
def test_two_level_noise_ties(oracle, kind):
    img = af.two_level(120, 160, 1)
    f0, (resp, _, _) = oracle.detect(kind, img, 5, THR[kind], 300, sort_mode=0)
    f1, _ = oracle.detect(kind, img, 5, THR[kind], 300, sort_mode=1)
    assert len(resp) > 64
    assert _tie_groups(resp).max() > 64
    assert not np.array_equal(f0, f1)
    if kind == HARRIS:
        assert resp.max() > 2e9  # top level-0 bins of the selection key


@pytest.mark.parametrize("n", STAMP_COUNTS)
def test_stamp_frames_tie_counts(oracle, n):
    rows, cols = af.stamp_shape(n)
    ny, nx = af.stamp_grid(rows, cols)
    assert ny * nx >= n and min(af.stamp_grid(rows - 1, cols)[0] * nx, ny * af.stamp_grid(rows, cols - 1)[1]) < n
    img, origins = af.stamp_frame(rows, cols, n)
    assert len(origins) == n
    resp, x, y = oracle.nms(oracle.response_map(img, HARRIS, THR[HARRIS]), THR[HARRIS])
    assert len(resp) == n and len(np.unique(resp.view(np.uint32))) == 1
    # one candidate per stamp, at one place inside it
    assert len({(int(a), int(b)) for a, b in zip(x - origins[:, 0], y - origins[:, 1])}) == 1
    sresp = oracle.nms(oracle.response_map(img, SHI_TOMASI, THR[SHI_TOMASI]), THR[SHI_TOMASI])[0]
    assert len(sresp) == 2 * n and sorted(_tie_groups(sresp)) == [n, n]
    for kind in (HARRIS, SHI_TOMASI):
        for dist in (0, 20):
            f0, _ = oracle.detect(kind, img, dist, THR[kind], 100000, sort_mode=0)
            f1, _ = oracle.detect(kind, img, dist, THR[kind], 100000, sort_mode=1)
            assert not np.array_equal(f0, f1), (kind, dist)


def test_stamp_frame_shapes():
    # the counts the stamp geometry was laid out for
    assert af.stamp_grid(240, 320) == (19, 26) and af.stamp_grid(480, 640) == (39, 52) and af.stamp_grid(640, 640) == (52, 52)
    with pytest.raises(AssertionError):
        af.stamp_frame(240, 320, 495)


def check_fast_centres(oracle, img, n_rows, thr=10.0):
    """The oracle's FAST candidates at the patch centres of `img` equal the rule: present exactly when
    score + offset > thr, with response fl(score + offset). Returns the scores."""
    rows, cols = img.shape
    assert rows == n_rows * af.PATCH
    cy, cx, score, want = af.fast_expected_at_centres(img, thr)
    resp, x, y = oracle.fast_candidates(img, thr)
    got = np.zeros((rows, cols), np.float32)
    got[y, x] = resp
    assert (resp > 0).all()
    assert np.array_equal(got[cy, cx].view(np.uint32), want.view(np.uint32))
    early = (want > 0) & (af.fast_offsets(rows, cols, cy, cx) < 0.5)  # (later offsets reach 8)
    assert np.array_equal(got[cy, cx][early].astype(np.int32), score[early])
    return score


def test_fast_offsets_are_the_recurrence(oracle):
    n = 442 * 1786
    assert np.array_equal(af.fast_offsets(448, 1792, np.repeat(np.arange(3, 445), 1786), np.tile(np.arange(3, 1789), 442)),
                          oracle.fast_offsets(n))
    assert oracle.fast_offsets(n)[-1] < 8.1  # a pixel of score 0 never passes threshold 10


@pytest.mark.parametrize("p_lo", [0, 64, 128, 192])
def test_fast_pairs_rule(oracle, p_lo):
    img = af.fast_pairs(p_lo, p_lo + 64)
    assert img.shape == (448, 1792)
    score = check_fast_centres(oracle, img, 64)
    p, v = np.divmod(np.arange(64 * 256), 256)
    assert np.array_equal(score, np.where(np.abs(v - (p + p_lo)) > 15, 16, 0))


@pytest.mark.parametrize("mode", ["bright", "dark", "mixed"])
def test_fast_rings_rule(oracle, mode):
    seen = set()
    for lo in range(0, 65536, 16384):
        img = af.fast_rings(lo, lo + 16384, mode)
        assert img.shape == (448, 1792)
        seen.update(np.unique(check_fast_centres(oracle, img, 64)).tolist())
    # every run length occurs; 1..11 pass the pre-check but only reach the threshold with the offset
    assert seen == set(range(17))
