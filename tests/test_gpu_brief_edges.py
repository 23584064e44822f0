"""fd_brief_compute where k_brief changes behaviour, bits and valid exactly against oracle.brief for both
samplers: the half_patch_size thresholds of the LDS staging and of the moment paths, keypoints exactly on the
border, the staged patch hanging over the frame, frames narrower than a staged row, and the largest moments.
tests/test_brief_host.py pins oracle.brief itself at the large patch sizes."""
import numpy as np
import pytest

from test_gpu_brief import fd, oracle_batch  # noqa: F401

pytestmark = pytest.mark.gpu

SAMPLERS = [0, 1]


def check(fd, oracle, frames, uv, length, half, sampler):
    """Parity of one call; frames [B, R, C] or [R, C], uv [B, S, 2] or [S, 2]. Returns the reference's valid."""
    frames3 = frames if frames.ndim == 3 else frames[None]
    uv3 = np.ascontiguousarray(uv if uv.ndim == 3 else uv[None], np.float32)
    bits, valid = fd.brief_compute(frames3, uv3, length=length, half_patch_size=half, sampler=sampler, with_valid=True)
    eb, ev = oracle_batch(oracle, frames3, uv3, None, length, half, sampler)
    assert np.array_equal(valid, ev), (valid.tolist(), ev.tolist())
    assert np.array_equal(bits, eb)
    return ev


def bound(half):
    return max(19, 2 * half)


@pytest.mark.parametrize("sampler", SAMPLERS)
@pytest.mark.parametrize("length", [256, 33])
@pytest.mark.parametrize("half", [9, 10, 19, 20, 30, 31, 32])
def test_staging_thresholds(fd, oracle, sampler, length, half):
    """half 9 | 10: the border leaves 19 for 2 * half (the last patch that can hang over the frame). 19 | 20: the
    staged reach turns from the pattern's 20 to the moments' half + 1. 30 | 31: the last staged patch (side 63)
    and the first global loads, still with integer moments. 31 | 32: the first sequential float moments."""
    mb = bound(half)
    size = 2 * mb + 24
    frame = oracle.make_frame("noise", 300 + half, size, size)
    rng = np.random.default_rng(half * 7 + length)
    uv = rng.uniform(mb - 2, size - mb + 2, (16, 2)).astype(np.float32)
    uv[:6] = np.rint(uv[:6])
    uv[6] = (mb, mb)
    uv[7] = (size - mb, size - mb)
    uv[8] = (mb + 0.5, size - mb - 0.25)
    uv[9] = (np.nan, size / 2)
    uv[10] = (size + 3.0, size / 2)
    ev = check(fd, oracle, frame, uv, length, half, sampler)
    assert ev[0, 6:9].tolist() == [1, 1, 1] and ev[0, 9:11].tolist() == [0, 0] and ev.sum() >= 8


@pytest.mark.parametrize("sampler", SAMPLERS)
@pytest.mark.parametrize("half", [8, 12])
@pytest.mark.parametrize("axis", [0, 1])
def test_exact_borders(fd, oracle, sampler, half, axis):
    """u (axis 0) or v (axis 1) at the bound, one ulp inside the border, at size - bound and one ulp beyond."""
    rows, cols = 120, 160
    frame = oracle.make_frame("noise", 41, rows, cols)
    b, size = np.float32(bound(half)), np.float32((cols, rows)[axis])
    edge = [b, np.nextafter(b, np.float32(0)), size - b, np.nextafter(size - b, np.float32(np.inf))]
    assert edge[1] < b and edge[3] > size - b and all(e.dtype == np.float32 for e in edge)
    uv = np.full((4, 2), 60.0, np.float32)
    uv[:, axis] = edge
    ev = check(fd, oracle, frame, uv, 256, half, sampler)
    assert ev[0].tolist() == [1, 0, 1, 0]


def ringed(oracle, seed, rows, cols):
    """Noise in [0, 200) with the frame's outermost rows and columns 255: a read that leaves the frame on one
    side and comes back in on the other (or in the neighbouring frame) sees 255 where 0 is due."""
    f = (oracle.make_frame("noise", seed, rows, cols).astype(np.uint16) * 200 // 256).astype(np.uint8)
    f[0], f[-1], f[:, 0], f[:, -1] = 255, 255, 255, 255
    return f


@pytest.mark.parametrize("sampler", SAMPLERS)
@pytest.mark.parametrize("half", [8, 9])
def test_overhang_and_tiny_frames(fd, oracle, sampler, half):
    """With half <= 9 the border is 19 and the staged reach 20: at floor(v) == 19 the patch stages row -1 (a
    negative linear index: 0), at floor(u) == 19 column -1 (the previous row's last byte), and the like at the
    far edges. At 38 and 40 columns one staged row of 41 bytes spans two frame rows."""
    for length in (256, 33):
        # 38 x 38: one admissible keypoint, the patch hangs over on all four sides
        ev = check(fd, oracle, ringed(oracle, 1, 38, 38), np.array([[19, 19]], np.float32), length, half, sampler)
        assert ev.tolist() == [[1]]
        # 39 rows x 40 columns in a batch behind a white frame (what frame 1 must not read at index -1)
        frames = np.stack([np.full((39, 40), 255, np.uint8), ringed(oracle, 2, 39, 40)])
        frames[0, 15:30, 17:34] = 0  # (a flat patch has no orientation)
        uv = np.array([[19, 19], [21, 19], [19, 20], [21, 20], [19.5, 19.75]], np.float32)
        ev = check(fd, oracle, frames, np.stack([uv, uv]), length, half, sampler)
        assert ev.tolist() == [[1] * 5] * 2
        # 120 x 160: floor of a coordinate 19 or size - 19
        uv = np.array([[19, 60], [19.5, 60.25], [141, 60], [80, 19], [80.25, 19.875], [80, 101], [19, 19], [141, 101],
                       [19.99, 101], [141, 19.5], [140.5, 100.5], [80, 60]], np.float32)
        ev = check(fd, oracle, ringed(oracle, 3, 120, 160), uv, length, half, sampler)
        assert ev.all()


@pytest.mark.parametrize("sampler", SAMPLERS)
@pytest.mark.parametrize("half", [31, 32])
@pytest.mark.parametrize("transpose", [False, True])
def test_largest_moments(fd, oracle, sampler, half, transpose):
    """A black / white step through the patch: |m10| (transposed: |m01|) is 255 * (2 * half + 1) * half * (half + 1)
    / 2 = 7.97e6 at half 31, the largest integer sum of the exact path, and 8.75e6 at half 32."""
    size = 2 * bound(half) + 12
    frame = np.zeros((size, size), np.uint8)
    frame[:, size // 2:] = 255
    c = size // 2
    uv = np.array([[c, c], [c - 1, c], [c + 1, c - 2], [c + 0.5, c + 0.25], [c - 0.5, c - 2.75], [c - 3, c + 3]], np.float32)
    if transpose:
        frame, uv = np.ascontiguousarray(frame.T), np.ascontiguousarray(uv[:, ::-1])
    mom = oracle.brief(frame, uv, 256, half, sampler)[2]
    big = np.abs(mom[:, 1 if transpose else 0])
    print("largest moment:", big.max())
    assert big.max() > 7e6 and big[0] == 255 * (2 * half + 1) * half * (half + 1) // 2
    ev = check(fd, oracle, frame, uv, 256, half, sampler)
    assert ev.all()
    check(fd, oracle, frame, uv, 33, half, sampler)
