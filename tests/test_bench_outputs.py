"""`bench.py --dump-outputs DIR`: the plain run's line and the arrays of its last timed step.

CPU: dump_outputs writes float32 files that do not depend on the unspecified rows past a frame's count,
and cuts an over-sized batch to a fixed sample. GPU: one plain run of the bench (3 steps) dumps exactly
what fd.detect_points returns for the frame of its last step, and its line holds no `--full` leg."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_masks_unspecified_rows(tmp_path):
    torch = pytest.importorskip("torch")
    sys.path.insert(0, ROOT)
    import bench

    rng = np.random.default_rng(3)
    cnt = np.array([0, 2, 5], np.int32)
    files = []
    for k in range(2):  # same features, different garbage past the counts
        xy = rng.uniform(1, 600, (3, 5, 2)).astype(np.float32)
        for b, n in enumerate(cnt):
            xy[b, :n] = np.arange(2 * n, dtype=np.float32).reshape(n, 2) + 10 * b
        d = tmp_path / f"run{k}"
        bench.dump_outputs(str(d), torch.from_numpy(xy), torch.from_numpy(cnt))
        files.append({f: np.load(d / f) for f in sorted(os.listdir(d))})
    assert sorted(files[0]) == ["counts.npy", "xy.npy"]
    for name, a in files[0].items():
        assert a.dtype == np.float32 and np.array_equal(a, files[1][name]), name
    assert files[0]["counts.npy"].tolist() == [0.0, 2.0, 5.0]
    got = files[0]["xy.npy"]
    assert not got[0].any() and not got[1, 2:].any()
    assert np.array_equal(got[2], np.arange(10, dtype=np.float32).reshape(5, 2) + 20)


def test_dump_outputs_samples_large_batches(tmp_path, monkeypatch):
    torch = pytest.importorskip("torch")
    sys.path.insert(0, ROOT)
    import bench

    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 10 * (4 * 2 * 4 + 8))  # room for 10 frames of stride 4
    xy = np.arange(64 * 4 * 2, dtype=np.float32).reshape(64, 4, 2)
    cnt = np.full(64, 4, np.int32)
    kept = []
    for k in range(2):
        d = tmp_path / f"run{k}"
        bench.dump_outputs(str(d), torch.from_numpy(xy), torch.from_numpy(cnt), rank=1)
        kept.append(np.load(d / "frames_rank1.npy"))
        got = np.load(d / "xy_rank1.npy")
        assert got.shape == (10, 4, 2) and np.array_equal(got, xy[kept[-1].astype(int)])
        assert sum(os.path.getsize(d / f) - 128 for f in os.listdir(d)) <= bench.DUMP_LIMIT_BYTES
    assert np.array_equal(kept[0], kept[1]) and len(set(kept[0].tolist())) == 10


@pytest.mark.gpu
def test_plain_run_dumps_last_step(tmp_path):
    torch = pytest.importorskip("torch")
    sys.path.insert(0, ROOT)
    import bench
    import feature_detector_amd as fd

    steps, warmup = 3, 1
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", str(warmup), "--dump-outputs", str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["steps"] == steps and out["warmup"] == warmup and out["ms_per_step"] > 0
    assert out["unit"] == "Mpix/s" and out["higher_is_better"] is True and out["dtype"] == "u8->i32/f32"
    assert abs(out["value"] - 640 * 480 / (out["ms_per_step"] * 1e-3) / 1e6) <= 0.01 * out["value"]
    for leg in ("roofline", "north_star", "config3_fast_brief", "config4_lsd_map", "config5_superpoint",
                "cpu_baseline", "device_copy", "end_to_end_ingest", "headline_pipelined", "ties"):
        assert leg not in out, leg
    xy, cnt = np.load(tmp_path / "out" / "xy.npy"), np.load(tmp_path / "out" / "counts.npy")
    assert xy.dtype == np.float32 and cnt.dtype == np.float32 and xy.shape == (1, 201, 2) and cnt.shape == (1,)
    # the last timed step ran on pool frame (steps - 1) % 16 of rank 0's seeded pool
    frame = bench.make_frames(torch, "noise", 1, 480, 640, 1234 + 7919 * ((steps - 1) % 16), torch.device("cuda", 0))
    res = fd.detect_points("harris", frame, 200, 20, bench.THR["harris"], ties="raster")
    torch.cuda.synchronize()
    exp = res.features(0)
    assert int(cnt[0]) == len(exp) > 0
    assert np.array_equal(xy[0, :len(exp)], exp) and not xy[0, len(exp):].any()
