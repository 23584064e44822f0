"""CPU: tests/warp_ref.py (the yardstick of the GPU warp tests) on properties that follow from fd_frames_warp's
contract, a registration round trip on the test image, and the entry checks that need no GPU."""
import ctypes

import numpy as np

import warp_ref as W

RNG = np.random.default_rng(5)
FRAME = RNG.integers(0, 256, (37, 53), dtype=np.uint8)
IDENTITY = np.eye(3).reshape(9)


def test_identity_copies():
    out, mask = W.warp_ref(FRAME, IDENTITY)
    assert np.array_equal(out[0], FRAME) and (mask == 1).all()
    out, mask = W.warp_ref(FRAME, IDENTITY * -0.25)  # any scale of H, negative W included
    assert np.array_equal(out[0], FRAME) and (mask == 1).all()


def test_integer_shift_copies_the_overlap_and_fills_the_rest():
    h = np.array([1, 0, 5, 0, 1, -3, 0, 0, 1], np.float64)  # source = destination + (5, -3)
    out, mask = W.warp_ref(FRAME, h, fill=200)
    assert np.array_equal(out[0, 3:, :48], FRAME[:34, 5:]) and (mask[0, 3:, :48] == 1).all()
    rest = np.ones((37, 53), bool)
    rest[3:, :48] = False
    assert (out[0][rest] == 200).all() and (mask[0][rest] == 0).all()


def test_half_pixel_shift_averages_neighbours():
    h = np.array([1, 0, 0.5, 0, 1, 0, 0, 0, 1], np.float64)
    out, mask = W.warp_ref(FRAME, h)
    f = FRAME.astype(np.int64)
    assert np.array_equal(out[0, :, :52], ((f[:, :52] + f[:, 1:] + 1) >> 1).astype(np.uint8))
    assert (mask[0, :, :52] == 1).all() and (mask[0, :, 52] == 0).all()  # 52.5 is outside [0, 52]


def test_camera_without_distortion_is_the_identity():
    import feature_detector_amd as fd

    K = np.array([[410.5, 0, 25.25], [0, 395.0, 17.75], [0, 0, 1]])
    p = fd.camera_params(K, K, np.zeros(5))
    assert p.dtype == np.float64 and p.shape == (22,)
    assert np.array_equal(p, W.camera_params_ref(K, K, np.zeros(5)))
    out, mask = W.warp_ref(FRAME, p, model=W.CAMERA)
    sx, sy = W.source_positions(p, W.CAMERA, 37, 53)
    assert np.abs(sx - np.arange(53)[None, :]).max() < 1e-11 and np.abs(sy - np.arange(37)[:, None]).max() < 1e-11
    # a position a few ulps off an integer may truncate to the 1023/1024 weight: one intensity step at most
    assert np.abs(out[0].astype(int) - FRAME.astype(int)).max() <= 1 and mask[0, 1:-1, 1:-1].all()
    # intrinsics that are exact in binary: bit for bit
    K2 = np.array([[256.0, 0, 24.0], [0, 512.0, 16.0], [0, 0, 1]])
    out, mask = W.warp_ref(FRAME, fd.camera_params(K2, K2, np.zeros(4)), model=W.CAMERA)
    assert np.array_equal(out[0], FRAME) and (mask == 1).all()


def test_camera_params_layout_and_checks():
    import pytest

    import feature_detector_amd as fd

    nK = np.array([[1.0, 0, 3], [0, 2, 4], [0, 0, 1]])
    K = np.array([[5.0, 0, 7], [0, 6, 8], [0, 0, 1]])
    R = np.arange(9, dtype=np.float64).reshape(3, 3) + 10
    p = fd.camera_params(nK, K, [0.1, 0.2, 0.3, 0.4], R)
    assert p.tolist() == [1, 2, 3, 4, 10, 11, 12, 13, 14, 15, 16, 17, 18, 5, 6, 7, 8, 0.1, 0.2, 0.3, 0.4, 0]
    assert fd.camera_params(nK, K, [0.1, 0.2, 0.3, 0.4, 0.5])[21] == 0.5
    with pytest.raises(ValueError):
        fd.camera_params(nK, K, [0.1])
    with pytest.raises(ValueError):
        fd.camera_params(nK[:2], K, np.zeros(5))


def test_degenerate_homographies_give_fill():
    nan = IDENTITY.copy()
    nan[4] = np.nan
    for h in (np.zeros(9), np.full(9, np.nan), nan):
        out, mask = W.warp_ref(FRAME, h, fill=77)
        assert (mask == 0).all() and (out == 77).all()


def test_registration_round_trip(image_png):
    """Guards the yardstick as a registration: a 240 x 320 crop of the test image warped by a planted homography,
    then by its inverse. Measured with this restatement: mean absolute difference from the original 0.7544
    intensity units over the 68455 pixels with a source in both passes (two bilinear interpolations of a
    natural image); the bound adds one unit for platform differences in the inversion of H."""
    crop = np.ascontiguousarray(image_png[24:264, 24:344])
    c, s = np.cos(np.deg2rad(4.0)), np.sin(np.deg2rad(4.0))
    T = lambda tx, ty: np.array([[1, 0, tx], [0, 1, ty], [0, 0, 1.0]])  # noqa: E731
    H = T(159.5, 119.5) @ np.array([[1.05 * c, -1.05 * s, 0], [1.05 * s, 1.05 * c, 0], [1e-4, -5e-5, 1]]) @ T(-155.0, -123.0)
    once, m1 = W.warp_ref(crop, H.reshape(9))
    back, m2 = W.warp_ref(once[0], np.linalg.inv(H).reshape(9))
    # mask 1 in both passes, and the second pass read no filled pixel of the first (its warped mask is solid)
    solid, _ = W.warp_ref(m1[0] * 255, np.linalg.inv(H).reshape(9))
    both = (m1[0] == 1) & (m2[0] == 1) & (solid[0] == 255)
    mad = np.abs(back[0].astype(np.int64) - crop.astype(np.int64))[both].mean()
    print(f"registration round trip: mean |diff| {mad:.4f} over {int(both.sum())} pixels")
    assert both.sum() > 0.8 * crop.size
    assert mad <= 0.7544 + 1.0


def test_symbol_exists_and_null_context_is_rejected():
    import feature_detector_amd as fd
    from feature_detector_amd._lib import fd_warp_opts

    L = fd.load()
    assert hasattr(L, "fd_frames_warp")
    opts = fd_warp_opts(0, 1, 0)
    buf = np.zeros(64, np.float64)
    p = ctypes.c_void_p(buf.ctypes.data)
    assert L.fd_frames_warp(None, p, 0, 1, 8, 8, ctypes.byref(opts), p, 0, 8, 8, p, None, 0) == fd._lib.FD_ERR_INVALID


def test_python_argument_checks():
    import pytest

    import feature_detector_amd as fd

    with pytest.raises(ValueError):
        fd.warp_frames(FRAME, IDENTITY, model="affine")
