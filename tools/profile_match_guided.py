"""Kernel-time A/B of the guided matchers against the unguided ones, for rocprofv3 --kernel-trace --stats:
the gated and the ungated instance run alternately in one process, on the same tensors.

  --shape brief   FAST (need 500, dist 15) + BRIEF-256 on 64 frames of 1280x720 noise, then frame i against
                  frame i + 1 (63 pairs of ~500 x 500), on the positions detect_points left on the device
  --shape nn      64 frames x 240 x 240 L2-normalised float descriptors (--dim 256 / 128), keypoints uniform
                  on a 752 x 480 frame, the train keypoints the query ones moved by up to 6 px
  --radius R      the window: 3.0e38 passes every pair (the pure cost of the gate), 16 is a tracker's window
Both calls use max_ratio 0.9 and the cross-check (two launches per call), out= preallocated.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import feature_detector_amd as fd  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--shape", default="brief", choices=["brief", "nn"])
p.add_argument("--dim", type=int, default=256)
p.add_argument("--radius", type=float, default=3.0e38)
p.add_argument("--calls", type=int, default=20)
a = p.parse_args()
g = torch.Generator(device="cuda").manual_seed(1)

if a.shape == "brief":
    frames = torch.randint(0, 256, (64, 720, 1280), dtype=torch.uint8, device="cuda", generator=g)
    res = fd.detect_points("fast", frames, 500, 15, 10.0)
    bits, valid = fd.brief_compute(frames, res.xy, res.counts, length=256, half_patch_size=8, with_valid=True)
    B, S = 63, bits.shape[1]
    args = (bits[:-1], bits[1:], res.counts[:-1], res.counts[1:], valid[:-1], valid[1:])
    kw = dict(max_distance=64, max_ratio=0.9, cross_check=True)
    q_xy, t_xy = res.xy[:-1], res.xy[1:]
    dist_type, call = torch.int32, fd.brief_match
else:
    B, S = 64, 240
    q = torch.nn.functional.normalize(torch.randn((B, S, a.dim), generator=g, device="cuda"), dim=2)
    t = torch.nn.functional.normalize(q.roll(17, 1) + 0.3 * torch.randn((B, S, a.dim), generator=g, device="cuda"), dim=2)
    q_xy = torch.rand((B, S, 2), generator=g, device="cuda") * torch.tensor([751.0, 479.0], device="cuda")
    t_xy = (q_xy.roll(17, 1) + 12.0 * torch.rand((B, S, 2), generator=g, device="cuda") - 6.0).contiguous()
    args = (q, t)
    kw = dict(max_ratio=0.9, cross_check=True)
    dist_type, call = torch.float32, fd.nn_match
outs = [(torch.empty((B, S), dtype=torch.int32, device="cuda"), torch.empty((B, S, 2), dtype=dist_type, device="cuda"),
         torch.empty((B,), dtype=torch.int32, device="cuda")) for _ in range(2)]
for _ in range(a.calls):
    call(*args, out=outs[0], **kw)
    call(*args, out=outs[1], q_xy=q_xy, t_xy=t_xy, radius=a.radius, **kw)
torch.cuda.synchronize()
print(f"{a.shape} dim {a.dim} radius {a.radius:g}: matches per frame unguided {float(outs[0][2].float().mean()):.1f}, "
      f"guided {float(outs[1][2].float().mean()):.1f}; outputs equal: {all(bool((x == y).all()) for x, y in zip(*outs))}")
