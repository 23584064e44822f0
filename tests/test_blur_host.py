"""CPU: fd_blur_taps (a host function), tests/blur_ref.py (the yardstick of the GPU smoothing tests) on the
consequences include/fd_hip.h states, the entry points that need no GPU, and the value of the stage measured on the
CPU oracle alone: BRIEF descriptors of two noisy copies of a frame differ less after smoothing."""
import ctypes
import math

import numpy as np
import pytest

import blur_ref as R

# the crop, noise and keypoints of test_smoothing_steadies_brief_under_noise (and of the GPU chain test)
NOISE_CROP = (slice(240, 480), slice(48, 368))
NOISE_SIGMA = 8.0


def formula_taps(sigma, radius=0):
    """include/fd_hip.h's fd_blur_taps, restated with math.exp."""
    r = radius if 1 <= radius <= 15 else min(15, max(1, math.ceil(3 * sigma)))
    g = [math.exp(-(k * k) / (2 * sigma * sigma)) for k in range(r + 1)]
    s = g[0] + 2 * sum(g[1:])
    w = [0] + [math.floor(256 * g[k] / s + 0.5) for k in range(1, r + 1)]
    w[0] = 256 - 2 * sum(w[1:])
    return r, w


@pytest.mark.parametrize("sigma,radius", ((0.5, 2), (0.8, 3), (1.0, 3), (2.0, 6), (5.0, 15), (10, 15)))
def test_taps_of_chosen_radius(sigma, radius):
    import feature_detector_amd as fd
    from feature_detector_amd._lib import fd_blur_opts

    r, w = fd.gaussian_taps(sigma)
    assert r == radius and len(w) == r + 1
    assert w[0] + 2 * sum(w[1:]) == 256 and all(t >= 0 for t in w)
    assert all(w[k] >= w[k + 1] for k in range(r)), w
    assert (r, w) == formula_taps(sigma)
    opts = fd_blur_opts()
    for k in range(16):
        opts.taps[k] = -7
    opts.step = 9
    assert fd.load().fd_blur_taps(float(sigma), 0, ctypes.byref(opts)) == 0
    assert opts.step == 1 and opts.radius == r
    assert list(opts.taps)[:r + 1] == w and all(t == 0 for t in list(opts.taps)[r + 1:])  # unused taps zero


def test_taps_of_given_radius_and_rejections():
    import feature_detector_amd as fd
    from feature_detector_amd._lib import fd_blur_opts

    for sigma, radius in ((2.0, 3), (1.0, 2), (2.0, 15), (0.3, 1), (100.0, 7)):
        assert fd.gaussian_taps(sigma, radius) == formula_taps(sigma, radius), (sigma, radius)
    assert fd.gaussian_taps(2.0, 3) == (3, [54, 49, 34, 18])
    assert fd.gaussian_taps(2.0, 16) == fd.gaussian_taps(2.0) == fd.gaussian_taps(2.0, 0)  # outside 1..15: chosen
    assert fd.gaussian_taps(1e6)[0] == 15
    L = fd.load()
    opts = fd_blur_opts()
    for bad in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        assert L.fd_blur_taps(bad, 0, ctypes.byref(opts)) == fd._lib.FD_ERR_INVALID
        with pytest.raises(fd.FdError):
            fd.gaussian_taps(bad)
    assert L.fd_blur_taps(1.0, 0, None) == fd._lib.FD_ERR_INVALID


def test_reflect_index_equals_numpy_pad():
    for n in (2, 3, 5, 16, 17):
        for r in range(0, n):  # numpy's reflect takes any pad width, but one bounce is what n > r pins down
            want = np.pad(np.arange(n), r, mode="reflect")
            assert np.array_equal(R.reflect_index(np.arange(-r, n + r), n), want), (n, r)
    # iterated: dimension 3, indices -7 .. 9; dimension 2; dimension 1
    assert R.reflect_index(np.arange(-7, 10), 3).tolist() == [1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1]
    assert R.reflect_index(np.arange(-3, 5), 2).tolist() == [1, 0, 1, 0, 1, 0, 1, 0]
    assert R.reflect_index(np.arange(-20, 20), 1).tolist() == [0] * 40
    want = np.pad(np.arange(5), 15, mode="reflect")  # numpy iterates the same reflection
    assert np.array_equal(R.reflect_index(np.arange(-15, 20), 5), want)


@pytest.mark.parametrize("taps", ([256], [128, 64], [96, 64, 16], [0, 128], [54, 49, 34, 18]))
def test_impulse_gives_the_outer_product(taps):
    r = len(taps) - 1
    n = 4 * r + 5
    frame = np.zeros((n, n), np.uint8)
    frame[n // 2, n // 2] = 255
    full = np.array(taps[:0:-1] + taps, np.int64)
    want = np.zeros((n, n), np.int64)
    want[n // 2 - r:n // 2 + r + 1, n // 2 - r:n // 2 + r + 1] = np.outer(full, full) * 255
    assert np.array_equal(R.blur_ref(frame, taps), ((want + 32768) >> 16).astype(np.uint8))


def test_constant_frames_copy_and_bounds():
    for value in (0, 1, 77, 255):
        for shape in ((1, 1), (2, 5), (9, 4)):
            frame = np.full(shape, value, np.uint8)
            for taps in ([256], [96, 64, 16], [12, 12, 11, 11, 11, 10, 10, 9, 8, 8, 7, 6, 6, 5, 4, 4]):
                assert np.array_equal(R.blur_ref(frame, taps), frame)  # (asserts h <= 65280 and v <= 255 * 2^16)
                assert np.array_equal(R.blur_ref(frame, taps, 2), frame[::2, ::2])
    noise = np.random.default_rng(1).integers(0, 256, (3, 7, 9), dtype=np.uint8)
    assert np.array_equal(R.blur_ref(noise, [256]), noise)  # r = 0, step 1: a copy


def test_pyrdown_taps_equal_the_binomial_form():
    """{96, 64, 16} with step 2 against (sum under [1 4 6 4 1] x [1 4 6 4 1] + 128) >> 8 on an np.pad-reflected frame."""
    k = np.array([1, 4, 6, 4, 1], np.int64)
    k2 = np.outer(k, k)
    rng = np.random.default_rng(5)
    for shape in ((9, 11), (8, 11), (9, 8), (3, 30), (6, 6)):
        frame = rng.integers(0, 256, shape, dtype=np.uint8)
        pad = np.pad(frame.astype(np.int64), 2, mode="reflect")
        rows, cols = (shape[0] + 1) // 2, (shape[1] + 1) // 2
        want = np.zeros((rows, cols), np.int64)
        for y in range(rows):
            for x in range(cols):
                want[y, x] = ((pad[2 * y:2 * y + 5, 2 * x:2 * x + 5] * k2).sum() + 128) >> 8
        assert np.array_equal(R.blur_ref(frame, R.PYR_TAPS, 2), want.astype(np.uint8)), shape
    levels = R.pyr_gauss_ref(rng.integers(0, 256, (2, 33, 17), dtype=np.uint8), 4)
    assert [a.shape for a in levels] == [(2, 33, 17), (2, 16, 8), (2, 8, 4), (2, 4, 2)]
    assert np.array_equal(levels[1], R.blur_ref(levels[0], R.PYR_TAPS, 2)[:, :16, :8])


def noisy_copies(image_png):
    """Two copies of the crop with independent seeded Gaussian noise of NOISE_SIGMA gray levels."""
    clean = np.ascontiguousarray(image_png[NOISE_CROP]).astype(np.float64)
    rng = np.random.default_rng(2024)
    return [np.clip(np.rint(clean + rng.normal(0.0, NOISE_SIGMA, clean.shape)), 0, 255).astype(np.uint8) for _ in range(2)]


def brief_medians(oracle, image_png, taps):
    """Median Hamming distance between the two noisy copies' BRIEF descriptors at the clean crop's Shi-Tomasi corners:
    on the copies as they are, and after blur_ref."""
    clean = np.ascontiguousarray(image_png[NOISE_CROP])
    kps, _ = oracle.detect(1, clean, 10, 0.1, 300, sort_mode=0)
    a, b = noisy_copies(image_png)
    out = []
    for fa, fb in ((a, b), (R.blur_ref(a, taps), R.blur_ref(b, taps))):
        ba, va, _ = oracle.brief(fa, kps, 256, 8, 0)
        bb, vb, _ = oracle.brief(fb, kps, 256, 8, 0)
        ok = (va != 0) & (vb != 0)
        assert ok.sum() >= 100, int(ok.sum())
        dist = np.unpackbits((ba[ok] ^ bb[ok]).view(np.uint8), axis=1).sum(axis=1)
        out.append(float(np.median(dist)))
    return out


def test_smoothing_steadies_brief_under_noise(oracle, image_png):
    """The gap the stage fills: on rows 240..479, columns 48..367 of the example image, two copies with seeded
    Gaussian noise (sigma 8), 256-bit BRIEF at the clean crop's Shi-Tomasi corners (oracle detector, distance 10, response 0.1, at most 300;
    oracle descriptor).
    The median Hamming distance between the copies' descriptors is strictly smaller after blur_ref with
    gaussian_taps(2.0) than before (DESIGN.md records both medians)."""
    import feature_detector_amd as fd

    raw, smooth = brief_medians(oracle, image_png, fd.gaussian_taps(2.0)[1])
    print(f"median Hamming distance between the noisy copies' BRIEF: {raw} raw, {smooth} after sigma 2")
    assert smooth < raw


def test_null_arguments_are_rejected_before_the_device():
    import feature_detector_amd as fd
    from feature_detector_amd._lib import fd_blur_opts

    L = fd.load()
    assert hasattr(L, "fd_frames_blur") and hasattr(L, "fd_pyr_build_gauss")
    opts = fd_blur_opts()
    opts.radius, opts.step = 0, 1
    opts.taps[0] = 256
    buf, out = np.zeros(4096, np.uint8), np.zeros(4096, np.uint8)
    p, q = ctypes.c_void_p(buf.ctypes.data), ctypes.c_void_p(out.ctypes.data)
    assert L.fd_frames_blur(None, p, 0, 1, 8, 8, ctypes.byref(opts), q, 0) == fd._lib.FD_ERR_INVALID
    assert L.fd_pyr_build_gauss(None, p, 0, 1, 8, 8, 1, q, 0) == fd._lib.FD_ERR_INVALID


def test_python_argument_checks_need_no_gpu():
    import feature_detector_amd as fd

    frame = np.zeros((12, 20), np.uint8)
    with pytest.raises(ValueError):
        fd.blur_frames(frame)  # neither sigma nor taps
    with pytest.raises(ValueError):
        fd.blur_frames(frame, sigma=1.0, taps=[256])  # both
    with pytest.raises(ValueError):
        fd.blur_frames(frame, taps=[16] * 17)  # more than 16 taps
    with pytest.raises(ValueError):
        fd.blur_frames(frame, taps=[96, 64, 16], radius=3)
    with pytest.raises(TypeError):
        fd.blur_frames(frame.astype(np.int8), sigma=1.0)
    with pytest.raises(ValueError):
        fd.blur_frames(np.zeros((0, 20), np.uint8), sigma=1.0)
    with pytest.raises(ValueError):
        fd.blur_frames(frame, sigma=1.0, out=np.zeros((12, 21), np.uint8))
    with pytest.raises(ValueError):
        fd.blur_frames(frame, sigma=1.0, step=2, out=np.zeros((12, 20), np.uint8))  # step 2: (6, 10)
    with pytest.raises(ValueError):
        fd.build_pyramid(frame, 2, kernel="triangle")
