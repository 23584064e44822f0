"""The C++ GeometricVerifier (include/feature_detector/geometric_verifier.h, an MI355X extension) driven by
the headless demo tests/cpp/test_geometric_verifier.cpp (fd_demo_geometry). The GPU tests compare what the
demo printed with tests/ransac_ref.py."""
import os

import numpy as np
import pytest

import cpp_demo
import ransac_ref as R
from cpp_demo import LIB, build as _build

RUNS = ((R.FUNDAMENTAL, 256, 0), (R.HOMOGRAPHY, 100, 7))  # (model, hypotheses, seed)
CENTER, SCALE = R.conditioning((R.ROWS, R.COLS))


@pytest.fixture(scope="module")
def demo_runs(tmp_path_factory):
    _build()
    d = tmp_path_factory.mktemp("geometry")
    runs = {}
    for model, hyp, seed in RUNS:
        q, t, _ = R.planted_scene(model, 1)
        path = d / f"pairs{model}.f32"
        np.concatenate([q, t], axis=1).astype(np.float32).tofile(path)
        runs[model] = (q, t, cpp_demo.run("fd_demo_geometry", path, len(q), R.ROWS, R.COLS, model, hyp, seed)[0])
    return runs


def test_demo_builds_and_exports_verifier():
    _build()
    assert os.path.exists(os.path.join(LIB, "fd_demo_geometry"))
    assert cpp_demo.exported("feature_detector::GeometricVerifier::Verify")


@pytest.mark.gpu
@pytest.mark.parametrize("model,hyp,seed", RUNS)
def test_geometry_demo_equals_ref(demo_runs, model, hyp, seed):
    q, t, res = demo_runs[model]
    n = len(q)
    kw = dict(model=model, hypotheses=hyp, seed=seed, center=CENTER, scale=SCALE)
    m, inl, cnt, best = R.ransac_ref(q[None], t[None], **kw)
    r = res["tracks"]
    assert r["ok"] is True and r["best"] == best[0] >= 0 and r["inlier"] == inl[0].tolist() and cnt[0] >= 48
    assert np.array_equal(np.array(r["model_bits"], np.uint64), m[0].view(np.uint64))
    idx = np.arange(n - 1, -1, -1, dtype=np.int32)
    idx[0], idx[1] = -1, n
    valid = np.where(np.arange(n) % 7 == 3, 2, 1).astype(np.uint8)
    m, inl, cnt, best = R.ransac_ref(q[None], t[None, ::-1], None, idx[None], valid[None], **kw)
    r = res["matches"]
    assert r["ok"] is True and r["best"] == best[0] >= 0 and r["inlier"] == inl[0].tolist()
    assert np.array_equal(np.array(r["model_bits"], np.uint64), m[0].view(np.uint64))
    assert inl[0][0] == 0 and inl[0][1] == 0 and not inl[0][valid == 2].any()


@pytest.mark.gpu
def test_geometry_demo_false_cases(demo_runs):
    for model in (R.FUNDAMENTAL, R.HOMOGRAPHY):
        assert demo_runs[model][2]["verify_false_cases"] == {"test": "verify_false_cases", "empty": False, "wrong_size": False,
                                                             "too_few": False, "too_few_best": -1}
