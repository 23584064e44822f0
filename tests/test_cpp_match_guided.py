"""The C++ BriefMatcher::MatchGuided and NNDescriptorMatcher::MatchGuided
(include/feature_detector/descriptor_matcher.h) driven by the headless program
tests/cpp/test_descriptor_matcher_guided.cpp (fd_demo_match_guided). The GPU test compares with
tests/match_guided_ref.py on a fixture the test writes."""
import os

import numpy as np
import pytest

import cpp_demo
import match_guided_ref as G
from match_guided_ref import match_guided_ref, nn_match_guided_ref

F32 = np.float32


@pytest.fixture(scope="module")
def demo():
    """The program, built against the drop-in library."""
    cpp_demo.build()
    return "fd_demo_match_guided"


def test_program_builds_against_the_headers(demo):
    assert os.path.exists(os.path.join(cpp_demo.LIB, demo))


def _fixture(path, dim, length):
    nq, nt = 70, 300
    b = G.brief_case(nq, nt, length=256, variant="tenth", flags=True, seed=3)
    n = G.nn_case(nq, nt, dim=dim, regime="round", seed=3)
    with open(path, "wb") as f:
        f.write(np.array([nq, nt, dim, length], np.int32).tobytes())
        for a in (n["q"], n["t"], b["q"], b["t"], b["q_xy"], b["t_xy"], b["qv"], b["tv"]):
            f.write(np.ascontiguousarray(a).tobytes())
    return b, n


@pytest.mark.gpu
@pytest.mark.parametrize("dim,length,rx,ry,ratio,cross", [(256, 256, 8.0, 8.0, 0.0, 0), (128, 100, 3.0, 11.0, 0.95, 1)])
def test_match_guided_equals_ref(demo, tmp_path, dim, length, rx, ry, ratio, cross):
    b, n = _fixture(tmp_path / "fixture.bin", dim, length)
    res, _ = cpp_demo.run(demo, tmp_path / "fixture.bin", rx, ry, ratio, cross)
    kw = dict(max_ratio=ratio, cross_check=bool(cross))
    for name, valid in (("", (None, None)), ("_valid", (b["qv"], b["tv"]))):
        idx, dist, counts = match_guided_ref(b["q"], b["t"], b["q_xy"], b["t_xy"], (rx, ry), q_valid=valid[0],
                                             t_valid=valid[1], length=length, **kw)
        m = res["brief" + name]
        assert m["ok"] is True and m["train_index"] == idx[0].tolist() and m["distance"] == dist[0, :, 0].tolist()
        assert counts[0] >= 1 and (not cross or counts[0] < idx.shape[1])
        idx, dist, counts = nn_match_guided_ref(n["q"], n["t"], b["q_xy"], b["t_xy"], (rx, ry), q_valid=valid[0],
                                                t_valid=valid[1], **kw)
        m = res["nn" + name]
        assert m["ok"] is True and m["train_index"] == idx[0].tolist()
        assert m["distance_bits"] == dist[0, :, 0].view(np.uint32).tolist()
        assert counts[0] >= 1 and (not cross or counts[0] < idx.shape[1])
    assert res["false_cases"] == {"test": "false_cases", "brief_short_uv": False, "brief_negative": False, "brief_nan": False,
                                  "nn_null_xy": False, "nn_inf": False, "nn_empty": False}
