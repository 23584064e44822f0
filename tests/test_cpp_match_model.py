"""The C++ BriefMatcher::MatchModel and NNDescriptorMatcher::MatchModel
(include/feature_detector/descriptor_matcher.h) driven by the headless program
tests/cpp/test_descriptor_matcher_model.cpp (fd_demo_match_model). The GPU test compares with
tests/match_model_ref.py on a fixture the test writes."""
import os

import numpy as np
import pytest

import cpp_demo
import match_model_ref as MM
from match_model_ref import match_model_ref, nn_match_model_ref

F32 = np.float32


@pytest.fixture(scope="module")
def demo():
    """The program, built against the drop-in library."""
    cpp_demo.build()
    return "fd_demo_match_model"


def test_program_builds_against_the_headers(demo):
    assert os.path.exists(os.path.join(cpp_demo.LIB, demo))
    assert cpp_demo.exported("BriefMatcher::MatchModel") and cpp_demo.exported("NNDescriptorMatcher::MatchModel")


def _fixture(path, dim, length, kind, threshold):
    nq, nt = 70, 300
    b = MM.brief_case(nq, nt, kind=kind, threshold=threshold, length=256, flags=True, seed=3)
    n = MM.nn_case(nq, nt, kind=kind, threshold=threshold, dim=dim, regime="round", seed=3)
    n["q_xy"], n["t_xy"] = b["q_xy"], b["t_xy"]  # one set of positions (and one model: the seed's) for both classes
    with open(path, "wb") as f:
        f.write(np.array([nq, nt, dim, length], np.int32).tobytes())
        for a in (b["model"][0], n["q"], n["t"], b["q"], b["t"], b["q_xy"], b["t_xy"], b["qv"], b["tv"]):
            f.write(np.ascontiguousarray(a).tobytes())
    return b, n


@pytest.mark.gpu
@pytest.mark.parametrize("dim,length,kind,threshold,radius,ratio,cross",
                         [(256, 256, MM.FUNDAMENTAL, 2.5, -1.0, 0.0, 0), (128, 100, MM.HOMOGRAPHY, 4.0, 20.0, 0.95, 1)])
def test_match_model_equals_ref(demo, tmp_path, dim, length, kind, threshold, radius, ratio, cross):
    b, n = _fixture(tmp_path / "fixture.bin", dim, length, kind, threshold)
    res, _ = cpp_demo.run(demo, tmp_path / "fixture.bin", kind, threshold, radius, ratio, cross)
    kw = dict(max_ratio=ratio, cross_check=bool(cross))
    r = MM.OPEN if radius < 0 else radius
    for name, valid in (("", (None, None)), ("_valid", (b["qv"], b["tv"]))):
        idx, dist, counts = match_model_ref(b["q"], b["t"], b["q_xy"], b["t_xy"], b["model"], kind, threshold, r,
                                            q_valid=valid[0], t_valid=valid[1], length=length, **kw)
        m = res["brief" + name]
        assert m["ok"] is True and m["train_index"] == idx[0].tolist() and m["distance"] == dist[0, :, 0].tolist()
        assert counts[0] >= 1 and (not cross or counts[0] < idx.shape[1])
        idx, dist, counts = nn_match_model_ref(n["q"], n["t"], b["q_xy"], b["t_xy"], b["model"], kind, threshold, r,
                                               q_valid=valid[0], t_valid=valid[1], **kw)
        m = res["nn" + name]
        assert m["ok"] is True and m["train_index"] == idx[0].tolist()
        assert m["distance_bits"] == dist[0, :, 0].view(np.uint32).tolist()
        assert counts[0] >= 1 and (not cross or counts[0] < idx.shape[1])
    false = {k: v for k, v in res["false_cases"].items() if k != "test"}
    assert len(false) == 10 and not any(false.values()), false
