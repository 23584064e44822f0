"""GeometricVerifier::RecoverPose and ::Triangulate (include/feature_detector/geometric_verifier.h, MI355X
extensions) driven by the headless demo tests/cpp/test_geometric_pose.cpp (fd_demo_pose). The GPU test compares
what the demo printed with tests/pose_ref.py bit for bit."""
import os

import numpy as np
import pytest

import cpp_demo
import pose_ref as P
from cpp_demo import LIB, build as _build

RUNS = ("stride-257", "choice-3", "depth")  # cases of pose_ref.all_cases(): batch 1, no match_idx, no pair_valid


def test_demo_builds_and_exports_pose():
    _build()
    assert os.path.exists(os.path.join(LIB, "fd_demo_pose"))
    assert cpp_demo.exported("feature_detector::GeometricVerifier::RecoverPose")
    assert cpp_demo.exported("feature_detector::GeometricVerifier::Triangulate")


@pytest.mark.gpu
@pytest.mark.parametrize("name", RUNS)
def test_pose_demo_equals_ref(tmp_path, name):
    _build()
    c = dict(P.all_cases())[name]
    n = c["q"].shape[1]
    np.concatenate([c["q"][0], c["t"][0]], axis=1).astype(np.float32).tofile(tmp_path / "pairs.f32")
    c["in_model"][0].astype(np.float64).tofile(tmp_path / "model.f64")
    c["in_inlier"][0].astype(np.uint8).tofile(tmp_path / "inliers.u8")
    res = cpp_demo.run("fd_demo_pose", tmp_path / "pairs.f32", n, tmp_path / "model.f64", tmp_path / "inliers.u8",
                       *(repr(float(v)) for v in c["cam_q"] + c["cam_t"] + (c["max_depth"], c["min_parallax"])))[0]
    pose, choice, pts, val, cnt = P.run_pose(c)
    tri = P.run_triangulate(c, pose)
    rec, tr = res["recover"], res["triangulate"]
    assert rec["ok"] is True and rec["extra"] == choice[0] >= 0 and rec["valid"] == val[0].tolist()
    assert np.array_equal(np.array(rec["pose_bits"], np.uint64), pose[0].view(np.uint64))
    assert np.array_equal(np.array(rec["point_bits"], np.uint32), pts[0].view(np.uint32).ravel())
    assert tr["ok"] is True and tr["extra"] == tri[2][0] == cnt[0] and tr["valid"] == tri[1][0].tolist()
    assert np.array_equal(np.array(tr["point_bits"], np.uint32), tri[0][0].view(np.uint32).ravel())
    assert res["pose_false_cases"] == {"test": "pose_false_cases", "no_pose": False, "cleared": True, "wrong_size": False,
                                       "bad_camera": False}
