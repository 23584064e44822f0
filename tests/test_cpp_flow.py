"""The C++ OpticalFlowLK (include/feature_detector/optical_flow_lk.h, an MI355X extension) driven by the
headless demo tests/cpp/test_optical_flow.cpp (fd_demo_flow). The GPU tests compare with tests/flow_ref.py
on the features the demo printed."""
import os

import numpy as np
import pytest

import cpp_demo
import flow_ref as R
from cpp_demo import LIB, build as _build

RUNS = ((), (2, 4, 0.5))  # (levels, half_window, max_forward_backward); (): the class defaults


@pytest.fixture(scope="module")
def demo_runs(tmp_path_factory, image_png):
    """fd_demo_flow on a crop of image_png and the crop whose content has moved by (3, -2), once per option set."""
    _build()
    d = tmp_path_factory.mktemp("flow")
    frames = [np.ascontiguousarray(image_png[24:264, 24:344]), np.ascontiguousarray(image_png[26:266, 21:341])]
    for i, f in enumerate(frames):
        f.tofile(d / f"frame{i}.u8")
    runs = {extra: cpp_demo.run("fd_demo_flow", d / "frame0.u8", 240, 320, d / "frame1.u8", *extra)[0] for extra in RUNS}
    return frames, runs


def test_demo_builds_and_exports_tracker():
    _build()
    assert os.path.exists(os.path.join(LIB, "fd_demo_flow"))
    assert cpp_demo.exported("feature_detector::OpticalFlowLK::Track")


@pytest.mark.gpu
@pytest.mark.parametrize("extra", RUNS)
def test_flow_demo_equals_ref(demo_runs, extra):
    frames, runs = demo_runs
    res = runs[extra]
    assert res["detect"]["ok"] is True
    feat = np.array(res["detect"]["features"], np.float32).reshape(-1, 2)
    assert len(feat) == 60
    kw = dict(zip(("levels", "half_window", "fb_max_dist"), extra))
    xy, st, err, cnt = R.flow_ref(frames[0], frames[1], feat[None], min_eigen=1e-4, **kw)
    t = res["track"]
    assert t["ok"] is True and t["status"] == st[0].tolist()
    assert np.array_equal(np.array(t["xy_bits"], np.uint32), xy[0].view(np.uint32))
    assert np.array_equal(np.array(t["err_bits"], np.uint32), err[0].view(np.uint32))
    assert cnt[0] >= 40


@pytest.mark.gpu
def test_flow_demo_false_cases(demo_runs):
    _, runs = demo_runs
    assert runs[()]["track_false_cases"] == {"test": "track_false_cases", "empty_features": False, "mismatched_size": False}
