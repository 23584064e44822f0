"""GeometricVerifier::AlignPoints, ::RefineAlignment and ::TransformPoints (include/feature_detector/
geometric_verifier.h, MI355X extensions) driven by the headless demo tests/cpp/test_geometric_align.cpp
(fd_demo_align). The GPU test compares what the demo printed with tests/align_ref.py bit for bit."""
import os

import numpy as np
import pytest

import align_ref as A
import cpp_demo
from cpp_demo import LIB, build as _build

RUNS = ("n-257", "similarity", "rigid", "hyp-65")  # cases of align_ref.all_cases(): batch 1, no match_idx, no masks
ROUNDS = 3


def test_demo_builds_and_exports_align():
    _build()
    assert os.path.exists(os.path.join(LIB, "fd_demo_align"))
    for name in ("AlignPoints", "RefineAlignment", "TransformPoints"):
        assert cpp_demo.exported(f"feature_detector::GeometricVerifier::{name}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", RUNS)
def test_align_demo_equals_ref(tmp_path, name):
    _build()
    c = dict(A.all_cases())[name]
    n = c["q"].shape[1]
    assert c["counts"] is None or int(c["counts"][0]) == n
    np.concatenate([c["q"][0], c["t"][0]], axis=1).astype(np.float32).tofile(tmp_path / "points.f32")
    res = cpp_demo.run("fd_demo_align", tmp_path / "points.f32", n, c["kind"], c["hypotheses"], c["seed"], repr(float(c["threshold"])),
                       ROUNDS)[0]
    model, inl, cnt, best = A.run_ransac(c)
    fit = A.run_refit(c, model, inl, ROUNDS)
    moved = A.align_apply_ref(fit[0], c["q"], fit[1])
    ali, ref, tra = res["align"], res["refine"], res["transform"]
    assert ali["ok"] is True and ali["extra"] == best[0] >= 0 and ali["inlier"] == inl[0].tolist()
    assert np.array_equal(np.array(ali["model_bits"], np.uint64), model[0].view(np.uint64))
    assert ref["ok"] is True and ref["extra"] == fit[3][0] >= 1 and ref["inlier"] == fit[1][0].tolist()
    assert np.array_equal(np.array(ref["model_bits"], np.uint64), fit[0][0].view(np.uint64))
    assert tra["ok"] is True and np.array_equal(np.array(tra["point_bits"], np.uint32), moved[0].reshape(-1).view(np.uint32))
    assert res["align_false_cases"] == {"test": "align_false_cases", "no_model": False, "cleared": True, "wrong_size": False,
                                        "wrong_target": False, "bad_kind": False, "bad_rounds": False, "bad_mask": False, "kept": True}
