"""The C++ ImageWarper (include/feature_detector/image_warper.h, an MI355X extension) driven by the headless
demo tests/cpp/test_image_warper.cpp (fd_demo_warp). The GPU test compares the frames the demo wrote with
tests/warp_ref.py on the parameter bits the demo printed."""
import json
import os
import subprocess

import numpy as np
import pytest

import warp_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "feature_detector_amd", "lib")
OUT_SHAPE = (203, 331)


def _build():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "feature_detector_amd", "api")])


def _run(frame_path, prefix, env=None):
    out = subprocess.run([os.path.join(LIB, "fd_demo_warp"), str(frame_path), "240", "320", *map(str, OUT_SHAPE), str(prefix)],
                         capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr
    return {r["test"]: r for r in (json.loads(l) for l in out.stdout.splitlines() if l.startswith("{"))}, out.stderr


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
    nm = subprocess.run(["nm", "-DC", os.path.join(LIB, "libfeature_detector.so")], capture_output=True, text=True).stdout
    assert "feature_detector::ImageWarper::Warp" in nm


def test_without_a_gpu_the_class_fails_loudly(frame):
    """No device visible to the demo: Warp returns false, the destination stays, last_error() says why."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    res, stderr = _run(frame[1], frame[2] / "nogpu", env)
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
