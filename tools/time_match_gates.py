"""Times the descriptor matchers under each gate on the GPU: unguided, window-guided and model-gated (F and H),
with the cross-check on, at 2048 x 2048 entries per frame and batch 8 (the defaults):
Hamming at length 256, float at dim 128 and dim 256.

Every variant is captured into a graph after a warm call; the graphs are replayed interleaved (one replay of
each per repetition, hipEvent pairs around every replay), so drift of the machine falls on all variants alike.
Prints one JSON line: per workload the median and the 10th / 90th percentile in microseconds per call, and the
ratio of every gate's median to the window-guided one. Needs a GPU; there is no CPU path.

    python tools/time_match_gates.py [--entries 2048] [--batch 8] [--reps 40]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def scene(rng, batch, n, side=640.0):
    """Positions of a homography-related pair of views with noise, the true H, and an F of the same motion class."""
    H = np.array([0.98, -0.03, 14.0, 0.025, 1.01, -9.0, 2e-5, -1e-5, 1.0])
    F = np.array([1.2e-6, -3.1e-5, 9.0e-3, 2.9e-5, 2.0e-6, -2.3e-2, -9.6e-3, 2.1e-2, 1.0])
    q = rng.uniform(0, side, (batch, n, 2))
    p = np.concatenate([q, np.ones((batch, n, 1))], 2) @ H.reshape(3, 3).T
    t = p[..., :2] / p[..., 2:] + rng.normal(0, 0.5, (batch, n, 2))
    for b in range(batch):
        t[b] = t[b][rng.permutation(n)]
    return q.astype(np.float32), t.astype(np.float32), np.tile(H / np.abs(H).max(), (batch, 1)), np.tile(F / np.abs(F).max(), (batch, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, default=2048)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=40)
    a = ap.parse_args()
    import torch

    import feature_detector_amd as fd

    assert torch.cuda.is_available(), "needs a GPU"
    rng = np.random.default_rng(0)
    B, n = a.batch, a.entries
    q_xy, t_xy, H, F = (torch.from_numpy(x).cuda() for x in scene(rng, B, n))
    gates = {
        "unguided": {},
        "window": dict(q_xy=q_xy, t_xy=t_xy, radius=24.0),
        "model_F": dict(q_xy=q_xy, t_xy=t_xy, model=F, model_kind="fundamental", threshold=1.5),
        "model_H": dict(q_xy=q_xy, t_xy=t_xy, model=H, model_kind="homography", threshold=2.0),
    }
    bits = [torch.from_numpy(rng.integers(-2**31, 2**31, (B, n, 8), dtype=np.int64).astype(np.int32)).cuda() for _ in range(2)]
    work = {"hamming_256": (fd.brief_match, bits, torch.int32)}
    for dim in (128, 256):
        d = [torch.nn.functional.normalize(torch.randn((B, n, dim), device="cuda"), dim=2) for _ in range(2)]
        work[f"float_{dim}"] = (fd.nn_match, d, torch.float32)
    result = {"entries": n, "batch": B, "reps": a.reps, "cross_check": True, "unit": "us per call"}
    stream = torch.cuda.Stream()
    for name, (fn, (qd, td), dt) in work.items():
        out = (torch.empty((B, n), dtype=torch.int32, device="cuda"), torch.empty((B, n, 2), dtype=dt, device="cuda"),
               torch.empty((B,), dtype=torch.int32, device="cuda"))
        graphs = {}
        for gname, kw in gates.items():
            fn(qd, td, cross_check=True, out=out, **kw)  # sizes the workspace, loads the code
            torch.cuda.synchronize()
            stream.wait_stream(torch.cuda.current_stream())
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=stream):
                fn(qd, td, cross_check=True, out=out, **kw)
            graphs[gname] = g
        for g in graphs.values():  # warm replays
            g.replay()
        torch.cuda.synchronize()
        times = {k: [] for k in graphs}
        for _ in range(a.reps):
            for gname, g in graphs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                g.replay()
                e1.record()
                e1.synchronize()
                times[gname].append(e0.elapsed_time(e1) * 1000.0)
        row = {k: dict(median=float(np.median(v)), p10=float(np.percentile(v, 10)), p90=float(np.percentile(v, 90)))
               for k, v in times.items()}
        for k in row:
            row[k]["vs_window"] = row[k]["median"] / row["window"]["median"]
        result[name] = row
        del graphs
    print(json.dumps(result))


if __name__ == "__main__":
    main()
