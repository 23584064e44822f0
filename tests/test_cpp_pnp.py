"""GeometricVerifier::SolvePnP and ::RefinePnP (include/feature_detector/geometric_verifier.h, MI355X extensions)
driven by the headless demo tests/cpp/test_geometric_pnp.cpp (fd_demo_pnp). The GPU test compares what the demo
printed with tests/pnp_ref.py bit for bit."""
import os

import numpy as np
import pytest

import cpp_demo
import pnp_ref as P
from cpp_demo import LIB, build as _build

RUNS = ("n-257", "conditioned", "hyp-65")  # cases of pnp_ref.all_cases(): batch 1, no match_idx, no masks
ROUNDS = 3


def test_demo_builds_and_exports_pnp():
    _build()
    assert os.path.exists(os.path.join(LIB, "fd_demo_pnp"))
    assert cpp_demo.exported("feature_detector::GeometricVerifier::SolvePnP")
    assert cpp_demo.exported("feature_detector::GeometricVerifier::RefinePnP")


@pytest.mark.gpu
@pytest.mark.parametrize("name", RUNS)
def test_pnp_demo_equals_ref(tmp_path, name):
    _build()
    c = dict(P.all_cases())[name]
    n = c["p"].shape[1]
    assert c["counts"] is None or int(c["counts"][0]) == n
    np.concatenate([c["p"][0], c["t"][0]], axis=1).astype(np.float32).tofile(tmp_path / "points.f32")
    res = cpp_demo.run("fd_demo_pnp", tmp_path / "points.f32", n, *(repr(float(v)) for v in c["cam"]), c["hypotheses"], c["seed"],
                       repr(float(c["threshold"])), *(repr(float(v)) for v in c["center"]), repr(float(c["scale"])), ROUNDS)[0]
    pose, inl, cnt, best = P.run_ransac(c)
    fit = P.run_refit(c, pose, inl, ROUNDS)
    sol, ref = res["solve"], res["refine"]
    assert sol["ok"] is True and sol["extra"] == best[0] >= 0 and sol["inlier"] == inl[0].tolist()
    assert np.array_equal(np.array(sol["pose_bits"], np.uint64), pose[0].view(np.uint64))
    assert ref["ok"] is True and ref["extra"] == fit[3][0] >= 1 and ref["inlier"] == fit[1][0].tolist()
    assert np.array_equal(np.array(ref["pose_bits"], np.uint64), fit[0][0].view(np.uint64))
    assert res["pnp_false_cases"] == {"test": "pnp_false_cases", "no_pose": False, "cleared": True, "wrong_size": False,
                                      "bad_camera": False, "bad_rounds": False, "kept": True}
