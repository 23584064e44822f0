"""The C++ ImageSmoother (include/feature_detector/image_smoother.h, an MI355X extension) driven by the headless
demo tests/cpp/test_image_smoother.cpp (fd_demo_blur). The GPU test compares the frames the demo wrote with
tests/blur_ref.py on the options and taps the demo printed."""
import os

import numpy as np
import pytest

import blur_ref as R
import cpp_demo
from cpp_demo import LIB, build as _build

SHAPE = (203, 331)
TESTS = ("default", "orb", "pyr_down")
FALSE_CASES = ("no_image", "mismatch", "in_place", "bad_sigma", "bad_step", "bad_taps")


def _run(frame_path, prefix, env=None):
    return cpp_demo.run("fd_demo_blur", frame_path, *SHAPE, prefix, env=env)


@pytest.fixture(scope="module")
def frame(tmp_path_factory, image_png):
    _build()
    f = np.ascontiguousarray(image_png[240:240 + SHAPE[0], 48:48 + SHAPE[1]])
    d = tmp_path_factory.mktemp("blur")
    f.tofile(d / "frame.u8")
    return f, d / "frame.u8", d


def test_demo_builds_and_exports_smoother():
    _build()
    assert os.path.exists(os.path.join(LIB, "fd_demo_blur"))
    assert cpp_demo.exported("feature_detector::ImageSmoother::Smooth")


def test_without_a_gpu_the_class_fails_loudly(frame):
    """No device visible to the demo: Smooth returns false, the destination stays, last_error() says why."""
    res, stderr = _run(frame[1], frame[2] / "nogpu", cpp_demo.NO_GPU_ENV)
    for test in TESTS:
        assert res[test]["ok"] is False and res[test]["untouched"] is True and res[test]["error"].strip()
        assert res[test]["taps"] == [] and not os.path.exists(str(frame[2] / "nogpu") + f".{test}.u8")
    f = res["blur_false_cases"]
    assert not any(f[k] for k in FALSE_CASES) and f["untouched"] is True
    assert "fd_ctx_create" in stderr


@pytest.mark.gpu
def test_blur_demo_equals_ref(frame):
    import feature_detector_amd as fd

    prefix = frame[2] / "gpu"
    res, _ = _run(frame[1], prefix)
    for test, sigma, radius, step, taps in (("default", 2.0, 0, 1, fd.gaussian_taps(2.0)[1]), ("orb", 2.0, 3, 1, [54, 49, 34, 18]),
                                            ("pyr_down", 2.0, 3, 2, [96, 64, 16])):
        t = res[test]
        assert t["ok"] is True and t["error"] == "" and t["untouched"] is False
        assert np.array([t["sigma_bits"]], np.uint32).view(np.float32)[0] == np.float32(sigma)
        assert (t["radius"], t["step"], t["taps"]) == (radius, step, taps)
        exp = R.blur_ref(frame[0], t["taps"], t["step"])
        assert exp.shape == (t["rows"], t["cols"]) and not np.array_equal(exp, frame[0][::step, ::step])
        out = np.fromfile(str(prefix) + f".{test}.u8", np.uint8).reshape(exp.shape)
        assert np.array_equal(out, exp)
    f = res["blur_false_cases"]
    assert not any(f[k] for k in FALSE_CASES) and f["untouched"] is True
    assert "taps" in f["error"]
