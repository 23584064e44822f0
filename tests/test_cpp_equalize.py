"""The C++ ContrastEqualizer (include/feature_detector/contrast_equalizer.h, an MI355X extension) driven by the
headless demo tests/cpp/test_contrast_equalizer.cpp (fd_demo_equalize). The GPU test compares the frames the
demo wrote with tests/equalize_ref.py on the options the demo printed."""
import os

import numpy as np
import pytest

import cpp_demo
import equalize_ref as R
from cpp_demo import LIB, build as _build

SHAPE = (203, 331)


def _run(frame_path, prefix, env=None):
    return cpp_demo.run("fd_demo_equalize", frame_path, *SHAPE, prefix, env=env)


@pytest.fixture(scope="module")
def frame(tmp_path_factory, image_png):
    _build()
    f = np.ascontiguousarray(image_png[240:240 + SHAPE[0], 48:48 + SHAPE[1]])
    d = tmp_path_factory.mktemp("equalize")
    f.tofile(d / "frame.u8")
    return f, d / "frame.u8", d


def test_demo_builds_and_exports_equalizer():
    _build()
    assert os.path.exists(os.path.join(LIB, "fd_demo_equalize"))
    assert cpp_demo.exported("feature_detector::ContrastEqualizer::Equalize")


def test_without_a_gpu_the_class_fails_loudly(frame):
    """No device visible to the demo: Equalize returns false, the destination stays, last_error() says why."""
    res, stderr = _run(frame[1], frame[2] / "nogpu", cpp_demo.NO_GPU_ENV)
    for test in ("default", "in_place"):
        assert res[test]["ok"] is False and res[test]["untouched"] is True and res[test]["error"].strip()
        assert not os.path.exists(str(frame[2] / "nogpu") + f".{test}.u8")
    f = res["equalize_false_cases"]
    assert not (f["no_image"] or f["mismatch"] or f["bad_clip"] or f["bad_tiles"]) and f["untouched"] is True
    assert "fd_ctx_create" in stderr


@pytest.mark.gpu
def test_equalize_demo_equals_ref(frame):
    prefix = frame[2] / "gpu"
    res, _ = _run(frame[1], prefix)
    for test, tiles, clip in (("default", (8, 8), 3.0), ("in_place", (5, 3), 2.5)):
        t = res[test]
        assert t["ok"] is True and t["error"] == "" and t["untouched"] is False
        assert (t["tiles_x"], t["tiles_y"]) == tiles
        assert np.array([t["clip_limit_bits"]], np.uint32).view(np.float32)[0] == np.float32(clip)
        exp = R.equalize_ref(frame[0], tiles, int(round(clip * 1000)))
        assert not np.array_equal(exp, frame[0])
        out = np.fromfile(str(prefix) + f".{test}.u8", np.uint8).reshape(SHAPE)
        assert np.array_equal(out, exp)
    f = res["equalize_false_cases"]
    assert not (f["no_image"] or f["mismatch"] or f["bad_clip"] or f["bad_tiles"]) and f["untouched"] is True
    assert "tiles_x" in f["error"]
