"""The C++ ImageWarper (include/feature_detector/image_warper.h, an MI355X extension) driven by the headless
demo tests/cpp/test_image_warper.cpp (fd_demo_warp). The GPU test compares the frames the demo wrote with
tests/warp_ref.py on the parameter bits the demo printed."""
import os

import numpy as np
import pytest

import cpp_demo
import warp_ref as W
from cpp_demo import LIB, build as _build

OUT_SHAPE = (203, 331)


def _run(frame_path, prefix, env=None):
    return cpp_demo.run("fd_demo_warp", frame_path, 240, 320, *OUT_SHAPE, prefix, env=env)


@pytest.fixture(scope="module")
def frame(tmp_path_factory, image_png):
    _build()
    f = np.ascontiguousarray(image_png[24:264, 24:344])
    d = tmp_path_factory.mktemp("warp")
    f.tofile(d / "frame.u8")
    return f, d / "frame.u8", d


def test_demo_builds_and_exports_warper():
    _build()
    assert os.path.exists(os.path.join(LIB, "fd_demo_warp"))
    assert cpp_demo.exported("feature_detector::ImageWarper::Warp")


def test_without_a_gpu_the_class_fails_loudly(frame):
    """No device visible to the demo: Warp returns false, the destination stays, last_error() says why."""
    res, stderr = _run(frame[1], frame[2] / "nogpu", cpp_demo.NO_GPU_ENV)
    for test in ("homography", "camera"):
        assert res[test]["ok"] is False and res[test]["untouched"] is True and res[test]["error"].strip()
        assert not os.path.exists(str(frame[2] / "nogpu") + f".{test}.u8")
    assert "fd_ctx_create" in stderr


@pytest.mark.gpu
def test_warp_demo_equals_ref(frame):
    prefix = frame[2] / "gpu"
    res, _ = _run(frame[1], prefix)
    for test, model in (("homography", W.HOMOGRAPHY), ("camera", W.CAMERA)):
        t = res[test]
        assert t["ok"] is True and t["error"] == ""
        params = np.array(t["params_bits"], np.uint64).view(np.float64)
        exp = W.warp_ref(frame[0], params, OUT_SHAPE, model, 200)
        assert 0.5 < exp[1].mean() < 1.0  # a real warp, with filled pixels
        out = np.fromfile(str(prefix) + f".{test}.u8", np.uint8).reshape(OUT_SHAPE)
        mask = np.fromfile(str(prefix) + f".{test}.mask", np.uint8).reshape(OUT_SHAPE)
        assert np.array_equal(out, exp[0][0]) and np.array_equal(mask, exp[1][0])
    f = res["warp_false_cases"]
    assert f["no_params"] is False and f["aliased"] is False and f["bad_option"] is False and "fill" in f["error"]
