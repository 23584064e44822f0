"""What the nine C++ drop-in classes do with their device context: set_device / device() / last_error() and the
"[feature_detector]" lines on stderr, driven by tests/cpp/test_device_context.cpp (fd_demo_device).

The literals of the test without a GPU were recorded from the library as it was before the classes shared
one DeviceContext (the program compiles against either, it uses the public headers only); the differences
between the classes they show are kept on purpose, not endorsed."""
import os

import pytest

import cpp_demo

NO_DEVICE = "fd_ctx_create failed (no MI355X visible?)"
# the point detector alone resolves FD_DEVICE into device(), stays silent on the failed creation and reports
# "no device context"; the line detector has no device()
CLASSES = ("harris", "lines", "brief", "brief_match", "nn_match", "flow", "refine", "verify", "warp")


def _env(base, fd_device):
    env = {k: v for k, v in base.items() if k != "FD_DEVICE"}
    if fd_device is not None:
        env["FD_DEVICE"] = fd_device
    return env


@pytest.mark.parametrize("fd_device,resolved", [(None, 0), ("2", 2)])
def test_without_a_gpu_every_class_reports_as_before(fd_device, resolved):
    cpp_demo.build()
    res, stderr = cpp_demo.run("fd_demo_device", env=_env(cpp_demo.NO_GPU_ENV, fd_device))
    assert tuple(res) == CLASSES
    assert res["harris"] == {"test": "harris", "ok": False, "error": "no device context", "device": [-1, resolved, 3]}
    assert res["lines"] == {"test": "lines", "ok": False, "error": NO_DEVICE}
    for name in CLASSES[2:]:
        assert res[name] == {"test": name, "ok": False, "error": NO_DEVICE, "device": [-1, -1, 3]}
    assert stderr.splitlines() == ["[feature_detector] no device context"] + ["[feature_detector] " + NO_DEVICE] * 8


def test_demo_builds_and_the_classes_are_still_exported():
    cpp_demo.build()
    assert os.path.exists(os.path.join(cpp_demo.LIB, "fd_demo_device"))
    for sym in ("feature_detector::DeviceContext::Acquire", "feature_detector::ImageWarper::~ImageWarper",
                "feature_detector::FeaturePointDetector::Context"):
        assert cpp_demo.exported(sym)


@pytest.mark.gpu
def test_set_device_on_a_gpu():
    """ImageWarper (identity homography, 16 x 16) and CornerRefiner (one point) across set_device: the
    resolved device again, a device fd_ctx_create rejects by its range check, the default again."""
    cpp_demo.build()
    res, stderr = cpp_demo.run("fd_demo_device", "gpu", env=_env(os.environ, None))
    first = res["first.refine"]
    assert first["ok"] is True and first["error"] == ""
    for step, device in (("first", -1), ("same_device", 0), ("default_device", -1)):
        w, r = res[step + ".warp"], res[step + ".refine"]
        assert w == {"test": step + ".warp", "ok": True, "equals_source": True, "untouched": False, "device": device,
                     "error": ""}
        assert r == dict(first, test=step + ".refine")
    w, r = res["bad_device.warp"], res["bad_device.refine"]
    assert w["ok"] is False and w["untouched"] is True and w["device"] == 1 << 20 and "fd_ctx_create" in w["error"]
    assert r["ok"] is False and r["status"] == 0 and "fd_ctx_create" in r["error"]
    assert r["xy_bits"] == [0x41000000, 0x41000000]  # (8, 8): the position stays
    assert stderr.splitlines() == ["[feature_detector] " + NO_DEVICE] * 2
