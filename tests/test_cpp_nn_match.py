"""The C++ NNDescriptorMatcher (include/feature_detector/descriptor_matcher.h, an MI355X extension)
driven by the headless program tests/cpp/test_nn_descriptor_matcher.cpp, which this test compiles against
include/ and libfeature_detector.so. The GPU tests compare with tests/nn_match_ref.py on a fixture the
test writes."""
import json
import os
import subprocess

import numpy as np
import pytest

from nn_match_ref import nn_match_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "feature_detector_amd", "lib")
F32 = np.float32


@pytest.fixture(scope="module")
def demo(tmp_path_factory):
    """The program, built against the drop-in library (rpath: the package's lib directory)."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "feature_detector_amd", "api")])
    exe = tmp_path_factory.mktemp("nn_match") / "nn_match_demo"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra",
                           "-I" + os.path.join(ROOT, "include"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "cpp", "test_nn_descriptor_matcher.cpp"), "-L" + LIB,
                           "-lfeature_detector", "-lfdhip", "-Wl,-rpath," + LIB])
    return str(exe)


def test_program_builds_and_library_exports_matcher(demo):
    assert os.path.exists(demo)
    nm = subprocess.run(["nm", "-DC", os.path.join(LIB, "libfeature_detector.so")], capture_output=True, text=True).stdout
    assert "feature_detector::NNDescriptorMatcher::Match" in nm


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
    out = subprocess.run([demo, str(tmp_path / "fixture.bin"), *map(str, extra)], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr
    res = {r["test"]: r for r in (json.loads(l) for l in out.stdout.splitlines() if l.startswith("{"))}
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
