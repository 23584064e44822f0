"""The C++ CornerRefiner (include/feature_detector/corner_refiner.h, an MI355X extension) driven by the headless
demo tests/cpp/test_corner_refiner.cpp (fd_demo_refine). The GPU tests compare with tests/refine_ref.py on the
features the demo printed."""
import os

import numpy as np
import pytest

import cpp_demo
import refine_ref as R
from cpp_demo import LIB, build as _build

RUNS = ((), (3, 1.5))  # (half_window, max_shift); (): the class defaults


def _run(frame_path, extra, env=None):
    return cpp_demo.run("fd_demo_refine", frame_path, 240, 320, *extra, env=env)


@pytest.fixture(scope="module")
def frame(tmp_path_factory, image_png):
    _build()
    f = np.ascontiguousarray(image_png[24:264, 24:344])
    path = tmp_path_factory.mktemp("refine") / "frame.u8"
    f.tofile(path)
    return f, path


@pytest.fixture(scope="module")
def demo_runs(frame):
    return {extra: _run(frame[1], extra)[0] for extra in RUNS}


def test_demo_builds_and_exports_refiner():
    _build()
    assert os.path.exists(os.path.join(LIB, "fd_demo_refine"))
    assert cpp_demo.exported("feature_detector::CornerRefiner::Refine")


def test_without_a_gpu_the_class_fails_loudly(frame):
    """No device visible to the demo: Refine returns false, the position stays, last_error() says why."""
    res, stderr = _run(frame[1], (), cpp_demo.NO_GPU_ENV)
    c = res["centre"]
    assert c["ok"] is False and c["status"] == 0 and c["error"].strip()
    assert np.array_equal(np.array(c["xy_bits"], np.uint32).view(np.float32), np.array([160, 120], np.float32))
    assert res["refine"]["ok"] is False and "fd_ctx_create" in stderr


@pytest.mark.gpu
@pytest.mark.parametrize("extra", RUNS)
def test_refine_demo_equals_ref(frame, demo_runs, extra):
    res = demo_runs[extra]
    assert res["detect"]["ok"] is True
    feat = np.array(res["detect"]["features"], np.float32).reshape(-1, 2)
    assert len(feat) == 60
    kw = dict(zip(("half_window", "max_shift"), extra))
    xy, st, cnt = R.refine_ref(frame[0], feat[None], **kw)
    t = res["refine"]
    assert t["ok"] is True and t["status"] == st[0].tolist()
    assert np.array_equal(np.array(t["xy_bits"], np.uint32), xy[0].view(np.uint32))
    assert cnt[0] >= 20
    cxy, cst, _ = R.refine_ref(frame[0], np.array([[[160, 120]]], np.float32), **kw)
    c = res["centre"]
    assert c["ok"] is True and c["status"] == cst[0, 0] and c["error"] == ""
    assert np.array_equal(np.array(c["xy_bits"], np.uint32), cxy[0, 0].view(np.uint32))


@pytest.mark.gpu
def test_refine_demo_false_cases(demo_runs):
    f = demo_runs[()]["refine_false_cases"]
    assert f["empty_features"] is False and f["bad_option"] is False and "half_window" in f["error"]
