"""The C++ NNDescriptorMatcher (include/feature_detector/descriptor_matcher.h, an MI355X extension)
driven by the headless program tests/cpp/test_nn_descriptor_matcher.cpp (fd_demo_nn_match). The GPU tests
compare with tests/nn_match_ref.py on a fixture the test writes."""
import os

import numpy as np
import pytest

import cpp_demo
from nn_match_ref import nn_match_ref

F32 = np.float32


@pytest.fixture(scope="module")
def demo():
    """The program, built against the drop-in library."""
    cpp_demo.build()
    return "fd_demo_nn_match"


def test_program_builds_and_library_exports_matcher(demo):
    assert os.path.exists(os.path.join(cpp_demo.LIB, demo))
    assert cpp_demo.exported("feature_detector::NNDescriptorMatcher::Match")


def _fixture(path, dim):
    rng = np.random.default_rng(31 + dim)
    nq, nt = 70, 130
    x, y = rng.standard_normal((nq, dim)), rng.standard_normal((nt, dim))
    q = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(F32)
    t = (y / np.linalg.norm(y, axis=1, keepdims=True)).astype(F32)
    t[10:40] = (q[20:50] + F32(0.1) * t[10:40]).astype(F32)
    t[100] = t[12]  # a tie of the best
    q[3] = 0  # descriptors of keypoints outside the map: zeros, flagged below
    t[7] = 0
    qv, tv = np.ones(nq, np.uint8), np.ones(nt, np.uint8)
    qv[3] = tv[7] = 0
    qv[50:] = rng.random(nq - 50) < 0.7
    with open(path, "wb") as f:
        f.write(np.array([nq, nt, dim], np.int32).tobytes() + q.tobytes() + t.tobytes() + qv.tobytes() + tv.tobytes())
    return q, t, qv, tv


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [(), (1.5, 0.9, 1)])
@pytest.mark.parametrize("dim", [256, 128])
def test_nn_matcher_equals_ref(demo, tmp_path, dim, extra):
    q, t, qv, tv = _fixture(tmp_path / "fixture.bin", dim)
    res, _ = cpp_demo.run(demo, tmp_path / "fixture.bin", *extra)
    kw = dict(zip(("max_distance", "max_ratio", "cross_check"), extra))
    kw["cross_check"] = bool(kw.get("cross_check", 0))
    for name, valid in (("match", (None, None)), ("match_valid", (qv[None], tv[None]))):
        idx, dist, counts = nn_match_ref(q, t, q_valid=valid[0], t_valid=valid[1], **kw)
        m = res[name]
        assert m["ok"] is True and m["train_index"] == idx[0].tolist()
        assert m["distance_bits"] == dist[0, :, 0].view(np.uint32).tolist()
        assert counts[0] >= 1 and (not extra or counts[0] < len(q))
    assert res["match_false_cases"] == {"test": "match_false_cases", "empty_query": False, "bad_dim": False,
                                        "bad_flags": False}
