"""GeometricVerifier::Refit (include/feature_detector/geometric_verifier.h, an MI355X extension) driven by the
headless demo tests/cpp/test_geometric_refit.cpp (fd_demo_refit). The GPU tests compare what the demo printed
with the Python call refit_geometry and with tests/refit_ref.py."""
import os

import numpy as np
import pytest

import cpp_demo
import ransac_ref as R
import refit_ref as F
from cpp_demo import LIB, build as _build

RUNS = ((R.FUNDAMENTAL, 128, 0, 2), (R.HOMOGRAPHY, 100, 7, 3))  # (model, hypotheses, seed, rounds)
NAMES = {R.FUNDAMENTAL: "fundamental", R.HOMOGRAPHY: "homography"}


@pytest.fixture(scope="module")
def demo_runs(tmp_path_factory):
    _build()
    d = tmp_path_factory.mktemp("refit")
    runs = {}
    for model, hyp, seed, rounds in RUNS:
        q, t = F.noisy_scene(model, 1)[:2]
        path = d / f"pairs{model}.f32"
        np.concatenate([q, t], axis=1).astype(np.float32).tofile(path)
        runs[model] = (q, t, cpp_demo.run("fd_demo_refit", path, len(q), R.ROWS, R.COLS, model, hyp, seed, rounds)[0])
    return runs


def test_demo_builds_and_exports_refit():
    _build()
    assert os.path.exists(os.path.join(LIB, "fd_demo_refit"))
    assert cpp_demo.exported("feature_detector::GeometricVerifier::Refit")
    assert cpp_demo.exported("feature_detector::GeometricVerifier::Verify")


@pytest.mark.gpu
@pytest.mark.parametrize("model,hyp,seed,rounds", RUNS)
def test_refit_demo_equals_python_and_ref(demo_runs, model, hyp, seed, rounds):
    import feature_detector_amd as fd

    q, t, res = demo_runs[model]
    kw = dict(model=NAMES[model], threshold=1.0, image_size=(R.ROWS, R.COLS))
    ver = fd.verify_geometry(q, t, hypotheses=hyp, seed=seed, **kw)
    ref = fd.refit_geometry(q, t, ver, rounds=rounds, **kw)
    exp = F.refit_ref(q[None], t[None], ver.model, ver.inliers, model=model, rounds=rounds, center=F.CENTER, scale=F.SCALE)
    v, r = res["verify"], res["refit"]
    assert v["ok"] is True and v["extra"] == ver.best[0] and v["inlier"] == ver.inliers[0].tolist()
    assert np.array_equal(np.array(v["model_bits"], np.uint64), ver.model[0].view(np.uint64))
    assert r["ok"] is True and r["extra"] == ref.rounds[0] >= 1 and r["inlier"] == ref.inliers[0].tolist()
    assert np.array_equal(np.array(r["model_bits"], np.uint64), ref.model[0].view(np.uint64))
    assert np.array_equal(ref.model.view(np.uint64), exp[0].view(np.uint64)) and np.array_equal(ref.inliers, exp[1])
    assert res["refit_false_cases"] == {"test": "refit_false_cases", "wrong_size": False, "bad_rounds": False, "empty": False,
                                        "untouched": True}
