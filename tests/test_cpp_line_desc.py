"""The C++ LineDescriptor (include/feature_detector/line_descriptor.h, an MI355X extension) driven by the
headless demo tests/cpp/test_line_descriptor.cpp (fd_demo_line_desc). The GPU test compares what the demo wrote
with tests/line_desc_ref.py on the lines and options the demo used."""
import os

import numpy as np
import pytest

import cpp_demo
import line_desc_ref as R
from cpp_demo import LIB, build as _build

SHAPE = (240, 320)


def _run(frame_path, prefix, env=None):
    return cpp_demo.run("fd_demo_line_desc", frame_path, *SHAPE, prefix, env=env)


@pytest.fixture(scope="module")
def frame(tmp_path_factory, image_png):
    _build()
    f = np.ascontiguousarray(image_png[:SHAPE[0], :SHAPE[1]])  # (the oracle finds 12 segments in this corner)
    d = tmp_path_factory.mktemp("line_desc")
    f.tofile(d / "frame.u8")
    return f, d / "frame.u8", d


def test_demo_builds_and_exports_descriptor():
    _build()
    assert os.path.exists(os.path.join(LIB, "fd_demo_line_desc"))
    assert cpp_demo.exported("feature_detector::LineDescriptor::Compute")


def test_without_a_gpu_the_class_fails_loudly(frame):
    """No device visible to the demo: Compute returns false, descriptors stay, last_error() says why."""
    res, stderr = _run(frame[1], frame[2] / "nogpu", cpp_demo.NO_GPU_ENV)
    assert res["detect"]["ok"] is False
    for test in ("default", "narrow"):
        assert res[test]["ok"] is False and res[test]["untouched"] is True and res[test]["error"].strip()
        assert not os.path.exists(str(frame[2] / "nogpu") + f".{test}.desc")
    f = res["compute_false_cases"]
    assert not (f["no_image"] or f["bad_bands"] or f["bad_width"]) and f["untouched"] is True
    assert "fd_ctx_create" in stderr


@pytest.mark.gpu
def test_line_desc_demo_equals_ref(frame):
    prefix = frame[2] / "gpu"
    res, _ = _run(frame[1], prefix)
    assert res["detect"]["ok"] is True and res["detect"]["lines"] >= 5
    n = res["detect"]["lines"] + 1  # the demo adds a line shorter than a pixel
    for test, bands, w in (("default", 9, 7), ("narrow", 3, 5)):
        t = res[test]
        assert t["ok"] is True and t["error"] == "" and t["untouched"] is False
        assert (t["bands"], t["band_width"], t["dim"], t["lines"], t["floats"]) == (bands, w, 8 * bands, n, n * 8 * bands)
        base = str(prefix) + f".{test}"
        lines = np.fromfile(base + ".lines", np.float32).reshape(1, n, 4)
        desc, xy, valid, _ = R.describe(frame[0][None], lines, None, bands, w)
        assert valid[0, :-1].all() and valid[0, -1] == 0
        assert np.array_equal(np.fromfile(base + ".desc", np.uint32), desc.view(np.uint32).reshape(-1))
        assert np.array_equal(np.fromfile(base + ".xy", np.uint32), xy.view(np.uint32).reshape(-1))
        assert np.array_equal(np.fromfile(base + ".valid", np.uint8), valid.reshape(-1))
    f = res["compute_false_cases"]
    assert not (f["no_image"] or f["bad_bands"] or f["bad_width"]) and f["untouched"] is True
    assert "kBandWidth" in f["error"]
