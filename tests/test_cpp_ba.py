"""GeometricVerifier::BundleAdjust (include/feature_detector/geometric_verifier.h, an MI355X extension) driven by the
headless demo tests/cpp/test_geometric_ba.cpp (fd_demo_ba). The GPU test compares what the demo printed with
tests/ba_ref.py bit for bit."""
import os

import numpy as np
import pytest

import ba_ref as B
import cpp_demo
from cpp_demo import LIB, build as _build

RUNS = ("rounds-16", "cams-2", "cams-8-null")  # cases of ba_ref.all_cases(): batch 1, no masks, no counts


def test_demo_builds_and_exports_bundle_adjust():
    _build()
    assert os.path.exists(os.path.join(LIB, "fd_demo_ba"))
    assert cpp_demo.exported("feature_detector::GeometricVerifier::BundleAdjust")


@pytest.mark.gpu
@pytest.mark.parametrize("name", RUNS)
def test_ba_demo_equals_ref(tmp_path, name):
    _build()
    c = dict(B.all_cases())[name]
    C, n = c["poses"].shape[1], c["p"].shape[1]
    assert c["counts"] is None and c["p_valid"] is None and c["obs_valid"] is None and c["obs"].shape[2] == n
    np.concatenate([c["p"][0]] + [c["obs"][0, k] for k in range(C)], axis=1).astype(np.float32).tofile(tmp_path / "points.f32")
    c["poses"][0].astype(np.float64).tofile(tmp_path / "poses.f64")
    fixed = "1" + "0" * (C - 1) if c["fixed"] is None else "".join(str(int(v != 0)) for v in c["fixed"][0])
    res = cpp_demo.run("fd_demo_ba", tmp_path / "points.f32", tmp_path / "poses.f64", n, C, *(repr(float(v)) for v in c["cam"]),
                       c["rounds"], repr(float(c["threshold"])), repr(float(c["lam"])), repr(float(c["up"])), repr(float(c["down"])),
                       fixed)[0]
    poses, points, inl, _, cost, rounds = B.run(c)
    got = res["adjust"]
    assert got["ok"] is True and got["extra"] == rounds[0] >= 1 and got["inlier"] == inl[0].reshape(-1).tolist()
    assert np.array_equal(np.array(got["pose_bits"], np.uint64), poses[0].reshape(-1).view(np.uint64))
    assert np.array_equal(np.array(got["point_bits"], np.uint32), points[0].reshape(-1).view(np.uint32))
    assert np.array_equal(np.array(got["cost_bits"], np.uint64), cost[0].view(np.uint64))
    assert res["ba_false_cases"] == {"test": "ba_false_cases", "wrong_size": False, "bad_rounds": False, "kept": True,
                                     "held_ok": True, "held_poses_kept": True}
