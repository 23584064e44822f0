"""The C++ BriefMatcher (include/feature_detector/descriptor_matcher.h, an MI355X extension) driven by
the headless demo tests/cpp/test_descriptor_matcher.cpp (fd_demo_match). The GPU tests compare with
tests/match_ref.py on the oracle's BRIEF bits of the features the demo printed."""
import os

import numpy as np
import pytest

import cpp_demo
from cpp_demo import LIB, build as _build
from match_ref import match_ref


@pytest.fixture(scope="module")
def demo_runs(tmp_path_factory, image_png):
    """fd_demo_match on image_png and its copy shifted by 3 rows and 5 columns, once per option set."""
    _build()
    d = tmp_path_factory.mktemp("match")
    frames = [image_png, np.roll(image_png, (3, 5), (0, 1))]
    for i, f in enumerate(frames):
        np.ascontiguousarray(f, np.uint8).tofile(d / f"frame{i}.u8")
    runs = {extra: cpp_demo.run("fd_demo_match", d / "frame0.u8", *image_png.shape, d / "frame1.u8", *extra)[0]
            for extra in ((), (64, 0.9, 1))}
    return frames, runs


def test_demo_builds_and_exports_matcher():
    _build()
    assert os.path.exists(os.path.join(LIB, "fd_demo_match"))
    assert cpp_demo.exported("feature_detector::BriefMatcher::Match")


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [(), (64, 0.9, 1)])
def test_match_demo_equals_ref(demo_runs, oracle, extra):
    frames, runs = demo_runs
    res = runs[extra]
    bits = []
    for i in range(2):
        r = res[f"frame{i}"]
        assert r["ok"] is True
        xy = np.array(r["features"], np.float32).reshape(-1, 2)
        assert len(xy) > 0
        bits.append(oracle.brief(frames[i], xy, 256, 8, 0)[0])
    kw = dict(zip(("max_distance", "max_ratio", "cross_check"), extra))
    kw["cross_check"] = bool(kw.get("cross_check", 0))
    idx, dist, counts = match_ref(bits[0], bits[1], **kw)
    m = res["match"]
    assert m["ok"] is True and m["train_index"] == idx[0].tolist() and m["distance"] == dist[0, :, 0].tolist()
    assert counts[0] >= 1
    # the demo's second run flags the all-zero descriptors invalid
    qv, tv = bits[0].any(axis=1).astype(np.uint8)[None], bits[1].any(axis=1).astype(np.uint8)[None]
    idx, dist, _ = match_ref(bits[0], bits[1], q_valid=qv, t_valid=tv, **kw)
    m = res["match_valid"]
    assert m["ok"] is True and m["train_index"] == idx[0].tolist() and m["distance"] == dist[0, :, 0].tolist()


@pytest.mark.gpu
def test_match_demo_false_cases(demo_runs):
    _, runs = demo_runs
    assert runs[()]["match_false_cases"] == {"test": "match_false_cases", "empty_query": False, "mismatched_length": False}
