"""CPU: tests/equalize_ref.py (the yardstick of the GPU equalization tests) on the invariants that follow from
fd_frames_equalize's contract, global equalization written independently, the chain crop on the CPU oracle, and
the entry checks that need no GPU."""
import ctypes

import numpy as np
import pytest

import equalize_ref as R

SHAPES = (((37, 53), (3, 2)), ((8, 8), (8, 8)), ((61, 67), (5, 7)), ((48, 64), (8, 8)), ((33, 45), (4, 4)))


def frame_of(shape, kind):
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    if kind == "noise":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if kind == "low contrast":
        return (rng.integers(0, 256, shape, dtype=np.uint8) >> 4) + 100
    f = np.zeros(shape, np.uint8)
    f[:, shape[1] // 2:] = 255
    return f


@pytest.mark.parametrize("shape,tiles", SHAPES)
@pytest.mark.parametrize("clip_milli", (0, 1, 3000, 40000))
def test_reference_invariants(shape, tiles, clip_milli):
    for kind in ("noise", "low contrast", "halves"):
        frame = frame_of(shape, kind)
        luts, infos = R.frame_luts(frame, tiles[0], tiles[1], clip_milli)  # (asserts that every histogram keeps its sum)
        assert luts.shape == (tiles[1], tiles[0], 256)
        assert (np.diff(luts.astype(int), axis=2) >= 0).all() and (luts[:, :, 255] == 255).all()
        assert sum(t["A"] for row in infos for t in row) == frame.size
        out = R.equalize_ref(frame, tiles, clip_milli)  # (asserts the blend below 2^32 and the fractions below 1024)
        assert out.shape == frame.shape and out.dtype == np.uint8


def test_axis_tables_cover_the_axis():
    for n, tiles in ((53, 3), (8, 8), (67, 5), (7, 1), (96, 32)):
        i0, i1, f = R.axis_table(n, tiles)
        assert i0[0] == 0 and i1[-1] == tiles - 1 and (np.diff(i0) >= 0).all() and ((i1 - i0) <= 1).all()
        assert (f[i0 == i1] == 0).all() and (f >= 0).all() and (f < 1024).all()
        pos = i0 * 1024 + f  # the interpolation coordinate never steps back
        assert (np.diff(pos) >= 0).all()


def test_one_tile_without_clipping_is_global_equalization():
    for kind in ("noise", "low contrast", "halves"):
        frame = frame_of((37, 53), kind)
        cdf = np.cumsum(np.bincount(frame.reshape(-1), minlength=256))
        lut = ((cdf * 255 + frame.size // 2) // frame.size).astype(np.uint8)
        assert np.array_equal(R.equalize_ref(frame, (1, 1), 0), lut[frame])
        assert np.array_equal(R.equalize_ref(frame, 1, 0), lut[frame])


def test_redistribution_pass_by_hand():
    """512 equal pixels, lim 129: E = 383, 1 to every bin, r = 127, step 2: one more to the even bins below 254."""
    lut, info = R.tile_lut(np.full((16, 32), 77, np.uint8), 64500)
    assert (info["lim"], info["E"], info["r"]) == (129, 383, 127)
    h = np.ones(256, np.int64)
    h[0:254:2] += 1
    h[77] += 129
    assert np.array_equal(lut, ((np.cumsum(h) * 255 + 256) // 512).astype(np.uint8))


def test_chain_crop_on_the_oracle(oracle, image_png):
    """The crop tests/test_gpu_equalize.py runs the equalize -> detect chain on (rows 240..479, columns 48..367 of
    the example image, darkened by >> 2): the CPU oracle alone finds strictly more Shi-Tomasi corners on the
    reference-equalized frame at the default options (distance 15, response 0.1): 164 -> 171."""
    dark = np.ascontiguousarray(image_png[240:480, 48:368]) >> 2
    n_dark = len(oracle.detect(1, dark, 15, 0.1, 500, sort_mode=0)[0])
    n_eq = len(oracle.detect(1, R.equalize_ref(dark), 15, 0.1, 500, sort_mode=0)[0])
    print(f"oracle: {n_dark} corners darkened, {n_eq} equalized")
    assert n_eq > n_dark


def test_symbol_exists_and_null_context_is_rejected():
    import feature_detector_amd as fd
    from feature_detector_amd._lib import fd_equalize_opts

    L = fd.load()
    assert hasattr(L, "fd_frames_equalize")
    opts = fd_equalize_opts(2, 2, 3000)
    buf = np.zeros(64, np.uint8)
    p = ctypes.c_void_p(buf.ctypes.data)
    assert L.fd_frames_equalize(None, p, 0, 1, 8, 8, ctypes.byref(opts), p, 0) == fd._lib.FD_ERR_INVALID


def test_python_argument_checks():
    import feature_detector_amd as fd

    frame = np.zeros((12, 20), np.uint8)
    for bad in (frame.astype(np.float32), frame.astype(np.int8), frame.astype(np.uint16)):
        with pytest.raises(TypeError):
            fd.equalize_frames(bad)
    for bad in (np.zeros((2, 3, 12, 20), np.uint8), np.zeros(20, np.uint8), np.zeros((0, 20), np.uint8), np.zeros((2, 12, 0), np.uint8)):
        with pytest.raises(ValueError):
            fd.equalize_frames(bad, 1)
    for tiles in (0, 33, (21, 2), (2, 13), (2, 0), (-1, 2), (2, 2, 2)):
        with pytest.raises(ValueError):
            fd.equalize_frames(frame, tiles)
    for clip in (-0.5, float("nan"), float("inf"), 3.0e6):
        with pytest.raises(ValueError):
            fd.equalize_frames(frame, 2, clip)
    with pytest.raises(ValueError):
        fd.equalize_frames(frame, 2, out=np.zeros((12, 21), np.uint8))
    with pytest.raises(ValueError):
        fd.equalize_frames(frame, 2, out=np.zeros((12, 20), np.int8))
