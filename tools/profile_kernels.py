"""Profiling driver (run under rocprofv3 --kernel-trace --stats): the bench shapes' kernels only, a
fixed number of times, on seeded uniform-noise frames generated on the GPU.

  --shape bench      fd_points_detect, Harris, 640x480, batch 1 (BASELINE configs[1]), 200 calls
  --shape northstar  fd_points_response (per-pixel kernel alone), 1920x1080 batch 256, 10 calls
                     (--kind shi_tomasi by default: the north-star kernel)
  --shape fast720    fd_points_detect, FAST, 1280x720 batch 64 (BASELINE configs[2]), 10 calls
  --shape fastbrief  the same + BRIEF-256 on the detected keypoints (fd_brief_compute), 10 calls
  --shape fastmatch  FAST (need 500, dist 15) + BRIEF-256 + fd_brief_match of frame i against frame i + 1 of
                     the batch (63 frame pairs, detect's device counts and BRIEF's valid flags in place), 10
                     calls (--cross-check: with the cross-check, two k_brief_match launches per call)
  --shape fastflow   FAST (need 500, dist 15) on 64 frames of one blurred-noise scene, each moved by (-2, -1) px
                     against the one before, fd_pyr_build (3 levels) of frames 0..62 and 1..63, and fd_flow_lk
                     (r 7, the defaults) of frame i's keypoints into frame i + 1, 10 calls (--fb: with the
                     forward-backward check, two k_flow_lk launches per call)
  --shape strefine   Shi-Tomasi (need 500, dist 15) on the 64 frames of fastflow's moving scene, fd_points_refine (r 5, 20
                     iterations) of every frame's corners in place, fd_pyr_build (3 levels) and fd_flow_lk (r 7) of
                     frame i's refined corners into frame i + 1, 10 calls
  --shape fastverify FAST (need 500, dist 15) + BRIEF-256 on the 64 frames of fastflow's moving scene, fd_brief_match of
                     frame i against frame i + 1 and fd_ransac (256 hypotheses, threshold 1 px) on the matches, the
                     fundamental matrix and then the homography, 10 calls (--refit: fd_ransac_refit, rounds 2, after each;
                     --pose: fd_pose_recover and fd_triangulate on the fundamental matrix; --pnp: with --pose, fd_pnp_ransac
                     (256 hypotheses, threshold 2 px) and fd_pnp_refit (rounds 4) of frame i + 1 against the points
                     fd_pose_recover left; --align: with --pose, fd_align_ransac (256 hypotheses), fd_align_refit (rounds 4)
                     and fd_align_apply of fd_pose_recover's points against fd_triangulate's of the same slots; --ba: with --pnp, fd_bundle_adjust (rounds 8, threshold 2 px) of every pair as a
                     two-camera window: the first frame held at the identity, the second at fd_pnp_refit's pose, the
                     matched positions gathered into slot order, the points fd_pose_recover's)
  --shape warp       fd_frames_warp with a mask, on device tensors: a rotation by 3 degrees with scale 1.02 and a mild
                     perspective (homography), then a barrel-distortion camera model, at 1920x1080 batch 64 (10
                     calls each) and at 640x480 batch 1 (200 calls each), destination shape = source shape
                     (--warp-size hd / vga: one of the two, so that a trace's statistics are one shape's)
  --shape equalize   fd_frames_equalize on device tensors, tiles (8, 8), clip limit 3.0, out preallocated: k_eq_tab,
                     k_eq_lut and k_eq_apply per call, on natural-statistics frames (blurred noise, darkened) at
                     --eq-size vga1 (640x480 batch 1, 200 calls), vga64 (640x480 batch 64, 20 calls) or hd
                     (1920x1080 batch 64, 10 calls); all: the three in turn (a trace per shape keeps its statistics
                     one shape's)
  --shape blur       fd_frames_blur on device tensors, out preallocated, one k_blur per call: r = 2 {96, 64, 16} at step 1
                     and at step 2, r = 3 gaussian_taps(2.0, 3) and r = 15 gaussian_taps(5.0) at step 1 (--blur-case
                     blur); fd_pyr_build_gauss against fd_pyr_build, 3 levels (--blur-case pyramid); on blurred-noise
                     frames at --blur-size vga1 (640x480 batch 1, 200 calls), vga64 (640x480 batch 64, 20 calls) or
                     hd (1920x1080 batch 64, 10 calls); all: everything in turn (a trace per size and case keeps a
                     kernel instance's statistics one shape's). Every call is also timed here with events
  --shape linedesc   fd_lines_describe on device tensors, default options (9 bands of 7 rows, dim 72), 512 seeded
                     segments per frame with lengths 20..300 px at any angle on 640x480 frames of blurred noise:
                     batch 64 (20 calls), then batch 1 (200 calls); one k_line_desc per call, also timed here with
                     events
  --shape nnmatch    fd_nn_match on 64 frames x 240 x 240 L2-normalised float descriptors (--dim 256 SuperPoint /
                     128 DISK; --cross-check: two k_nn_match launches per call), 20 calls; then a torch
                     baseline on the same tensors (q @ t.T, norms, topk(2)), 20 calls; both also timed here with
                     events (the whole call: k_nn_norms + k_nn_match launches + the counts memset)
  --shape lsd        fd_lsd_map (dense) and fd_lsd_lines (compact map + host stage), 1920x1080 batch 256,
                     64-px checker + noise (BASELINE configs[3]), 3 calls each (--kind dense / compact: one;
                     dense_unpitched: dense maps with unpadded rows)
  --shape ties       fd_points_detect with ties="reference" on the bench tie-report frames: Harris 640x480,
                     16 seeds x 10 calls (the seeds whose frames meet a tie run k_select_reference)
  --shape nsties     the same on the north-star batch (Shi-Tomasi 1920x1080 x256), 4 calls
"""
import argparse
import os
import sys

sys.path.insert(0, os.environ.get("GRAFT_REPO_ROOT", os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

import feature_detector_amd as fd  # noqa: E402

THR = {"harris": 30.0, "shi_tomasi": 40.0, "fast": 10.0}
p = argparse.ArgumentParser()
p.add_argument("--shape", default="bench", choices=["bench", "northstar", "nsdetect", "fast720", "fast720r", "fastbrief", "fastmatch", "fastflow", "strefine", "fastverify", "warp", "equalize", "blur", "linedesc", "nnmatch", "lsd",
                                                   "ties", "nsties"])
p.add_argument("--kind", default=None, choices=[None, "harris", "shi_tomasi", "fast", "dense", "compact", "dense_unpitched"])
p.add_argument("--calls", type=int, default=0)
p.add_argument("--cross-check", action="store_true", help="fastmatch: match with the cross-check")
p.add_argument("--fb", action="store_true", help="fastflow: track with the forward-backward check")
p.add_argument("--refit", action="store_true", help="fastverify: fd_ransac_refit (rounds 2) on each model after fd_ransac")
p.add_argument("--pnp", action="store_true",
               help="fastverify: implies --pose; fd_pnp_ransac and fd_pnp_refit of the pair's second frame against fd_pose_recover's points")
p.add_argument("--align", action="store_true",
               help="fastverify: implies --pose; fd_align_ransac, fd_align_refit and fd_align_apply of fd_pose_recover's points against fd_triangulate's")
p.add_argument("--ba", action="store_true", help="fastverify: implies --pnp; fd_bundle_adjust of each pair's two cameras and its points")
p.add_argument("--pose", action="store_true",
               help="fastverify: fd_pose_recover on the fundamental matrix (the refit one with --refit), then fd_triangulate with its pose")
p.add_argument("--dim", type=int, default=256, help="nnmatch: floats per descriptor")
p.add_argument("--warp-size", default="both", choices=["both", "hd", "vga"], help="warp: one of the two shapes (a trace per shape)")
p.add_argument("--eq-size", default="all", choices=["all", "vga1", "vga64", "hd"], help="equalize: one of the three shapes (a trace per shape)")
p.add_argument("--blur-size", default="all", choices=["all", "vga1", "vga64", "hd"], help="blur: one of the three shapes (a trace per shape)")
p.add_argument("--blur-case", default="all", choices=["all", "blur", "pyramid"], help="blur: the smoothing calls or the pyramids")
p.add_argument("--thr", type=float, default=None, help="response threshold override (e.g. 1e30: no candidates)")
a = p.parse_args()
g = torch.Generator(device="cuda")
g.manual_seed(7)


def noise(b, r, c):
    return torch.randint(0, 256, (b, r, c), generator=g, device="cuda", dtype=torch.int32).to(torch.uint8)


if a.shape == "bench":
    kind = a.kind or "harris"
    frames = noise(1, 480, 640)
    for _ in range(a.calls or 200):
        fd.detect_points(kind, frames, 200, 20, THR[kind] if a.thr is None else a.thr)
elif a.shape == "northstar":
    kind = a.kind or "shi_tomasi"
    frames = noise(256, 1080, 1920)
    cap = 1080 * 1920 if kind == "fast" else 1080 * 1920 // 2 + 64
    out = (torch.empty((256, cap), dtype=torch.float32, device="cuda"),
           torch.empty((256, cap), dtype=torch.int32, device="cuda"), torch.empty((256,), dtype=torch.int32, device="cuda"))
    for _ in range(a.calls or 10):
        fd.point_response(kind, frames, THR[kind] if a.thr is None else a.thr, out=out)
elif a.shape == "lsd":
    kind = "lsd"
    rows, cols, n = 1080, 1920, 256
    r = torch.arange(rows, device="cuda").view(1, rows, 1) // 64
    c = torch.arange(cols, device="cuda").view(1, 1, cols) // 64
    base = torch.where(((r + c) % 2) == 1, 180, 60)
    frames = (base + torch.randint(-10, 11, (n, rows, cols), generator=g, device="cuda", dtype=torch.int32)).clamp(0, 255).to(torch.uint8)
    flat = None
    if a.kind == "dense_unpitched":  # the dense maps without row padding (misaligned row stores)
        mr, mc = rows - 1, cols - 1
        flat = (torch.empty((n, mr, mc), device="cuda"), torch.empty((n, mr, mc), device="cuda"),
                torch.empty((n, mr, mc), dtype=torch.uint8, device="cuda"),
                torch.empty((n, mr * mc), dtype=torch.int32, device="cuda"), torch.empty((n,), dtype=torch.int64, device="cuda"))
    for _ in range(a.calls or 3):  # --kind dense / compact: one of the two only
        if a.kind == "dense_unpitched":
            fd.lsd_map(frames, out=flat)
            continue
        if a.kind != "compact":
            fd.lsd_map(frames)
        if a.kind != "dense":
            fd.lsd_lines(frames, max_lines=2048)
elif a.shape == "nsdetect":  # north-star shape through fd_points_detect (K1 with the selection histogram)
    kind = a.kind or "shi_tomasi"
    frames = noise(256, 1080, 1920)
    for _ in range(a.calls or 10):
        try:
            fd.detect_points(kind, frames, 200, 20, THR[kind], ties="raster")
        except Exception as e:  # (diagnostic builds that break the selection still time the kernels)
            print("detect:", e)
elif a.shape in ("ties", "nsties"):  # bench.tie_report's frames (bench.make_frames)
    import bench  # noqa: E402
    if a.shape == "ties":
        kind = a.kind or "harris"
        pool = [bench.make_frames(torch, "noise", 1, 480, 640, 1234 + 7919 * i, "cuda") for i in range(16)]
        for f in pool:
            for _ in range(a.calls or 10):
                fd.detect_points(kind, f, 200, 20, THR[kind], ties="reference")
    else:
        kind = a.kind or "shi_tomasi"
        f = bench.make_frames(torch, "noise", 256, 1080, 1920, 99, "cuda")
        for _ in range(a.calls or 4):
            fd.detect_points(kind, f, 200, 20, THR[kind], ties="reference")
elif a.shape == "fast720r":  # the FAST kernel alone (fd_points_response: no selection histogram)
    kind = "fast"
    frames = noise(64, 720, 1280)
    cap = 720 * 1280
    out = (torch.empty((64, cap), dtype=torch.float32, device="cuda"),
           torch.empty((64, cap), dtype=torch.int32, device="cuda"), torch.empty((64,), dtype=torch.int32, device="cuda"))
    for _ in range(a.calls or 10):
        fd.point_response(kind, frames, THR[kind], out=out)
elif a.shape == "fastbrief":  # BASELINE configs[2]: FAST detect + BRIEF-256 on the device output
    kind = "fast"
    frames = noise(64, 720, 1280)
    for _ in range(a.calls or 10):
        res = fd.detect_points(kind, frames, 200, 20, THR[kind])
        fd.brief_compute(frames, res.xy, res.counts, length=256, half_patch_size=8)
elif a.shape == "fastmatch":  # configs[2]'s shape with need 500, then the matcher on consecutive frames
    kind = "fast"
    frames = noise(64, 720, 1280)
    out = (torch.empty((63, 501), dtype=torch.int32, device="cuda"), torch.empty((63, 501, 2), dtype=torch.int32, device="cuda"),
           torch.empty((63,), dtype=torch.int32, device="cuda"))
    for _ in range(a.calls or 10):
        res = fd.detect_points(kind, frames, 500, 15, THR[kind])
        bits, valid = fd.brief_compute(frames, res.xy, res.counts, length=256, half_patch_size=8, with_valid=True)
        fd.brief_match(bits[:-1], bits[1:], res.counts[:-1], res.counts[1:], valid[:-1], valid[1:], max_distance=64,
                       max_ratio=0.9, cross_check=a.cross_check, out=out)
    print("matches per frame pair (mean):", float(out[2].float().mean()), "keypoints:", float((res.counts & 0x1FFFFFF).float().mean()))
elif a.shape == "fastflow":  # detect -> pyramids -> track on consecutive frames of one moving scene
    kind = "fast" + (" fb" if a.fb else "")
    base = torch.nn.functional.avg_pool2d(noise(1, 720 + 64, 1280 + 128).float()[None], 3, 1, 1)[0, 0]
    base = ((base - base.mean()) * 2.5 + 128.0).clamp(0, 255).to(torch.uint8)  # (the blur's contrast restored)
    frames = torch.stack([base[i:i + 720, 2 * i:2 * i + 1280] for i in range(64)]).contiguous()
    out = None
    for _ in range(a.calls or 10):
        res = fd.detect_points("fast", frames, 500, 15, THR["fast"])
        if out is None:
            s = res.xy.shape[1]
            out = (torch.empty((63, s, 2), dtype=torch.float32, device="cuda"), torch.empty((63, s), dtype=torch.uint8, device="cuda"),
                   torch.empty((63, s), dtype=torch.float32, device="cuda"), torch.empty((63,), dtype=torch.int32, device="cuda"))
        p0, p1 = fd.build_pyramid(frames[:-1], 3), fd.build_pyramid(frames[1:], 3)
        fd.track_lk(p0, p1, res.xy[:-1], counts=res.counts[:-1], levels=3, half_window=7, fb_max_dist=1.0 if a.fb else -1.0,
                    out=out)
    n = (res.counts[:-1] & 0x1FFFFFF).float()
    moved = (out[0] - res.xy[:-1])[out[1] == 1]
    print("keypoints per frame (mean):", float(n.mean()), "tracked (mean):", float(out[3].float().mean()),
          "median displacement of the tracked:", moved.median(0).values.tolist())
elif a.shape == "strefine":  # detect -> refine -> pyramids -> track on consecutive frames of one moving scene
    kind = "shi_tomasi"
    base = torch.nn.functional.avg_pool2d(noise(1, 720 + 64, 1280 + 128).float()[None], 3, 1, 1)[0, 0]
    base = ((base - base.mean()) * 2.5 + 128.0).clamp(0, 255).to(torch.uint8)
    frames = torch.stack([base[i:i + 720, 2 * i:2 * i + 1280] for i in range(64)]).contiguous()
    out = None
    for _ in range(a.calls or 10):
        res = fd.detect_points(kind, frames, 500, 15, THR[kind])
        if out is None:
            s = res.xy.shape[1]
            rst, rcnt = torch.empty((64, s), dtype=torch.uint8, device="cuda"), torch.empty((64,), dtype=torch.int32, device="cuda")
            out = (torch.empty((63, s, 2), dtype=torch.float32, device="cuda"), torch.empty((63, s), dtype=torch.uint8, device="cuda"),
                   torch.empty((63, s), dtype=torch.float32, device="cuda"), torch.empty((63,), dtype=torch.int32, device="cuda"))
        start = res.xy.clone()
        fd.refine_points(frames, res.xy, counts=res.counts, half_window=5, max_iters=20, out=(res.xy, rst, rcnt))
        p0, p1 = fd.build_pyramid(frames[:-1], 3), fd.build_pyramid(frames[1:], 3)
        fd.track_lk(p0, p1, res.xy[:-1], counts=res.counts[:-1], levels=3, half_window=7, out=out)
    n = (res.counts & 0x1FFFFFF).float()
    step = (res.xy - start)[rst == 1].abs()
    moved = (out[0] - res.xy[:-1])[out[1] == 1]
    print("corners per frame (mean):", float(n.mean()), "refined (mean):", float(rcnt.float().mean()),
          "median |refinement| per axis:", step.median(0).values.tolist(), "tracked (mean):", float(out[3].float().mean()),
          "median displacement of the tracked:", moved.median(0).values.tolist())
elif a.shape == "fastverify":  # detect -> describe -> match -> verify on consecutive frames of one moving scene
    kind = "fast"
    base = torch.nn.functional.avg_pool2d(noise(1, 720 + 64, 1280 + 128).float()[None], 3, 1, 1)[0, 0]
    base = ((base - base.mean()) * 2.5 + 128.0).clamp(0, 255).to(torch.uint8)
    frames = torch.stack([base[i:i + 720, 2 * i:2 * i + 1280] for i in range(64)]).contiguous()
    out, refit, pose, tri, pnp, ba, ali = None, {}, None, None, None, None, None
    a.pnp = a.pnp or a.ba
    a.pose = a.pose or a.pnp or a.align
    cam = (1000.0, 1000.0, 639.5, 359.5)
    for _ in range(a.calls or 10):
        res = fd.detect_points(kind, frames, 500, 15, THR[kind])
        if out is None:
            s = res.xy.shape[1]
            out = (torch.empty((63, s), dtype=torch.int32, device="cuda"), torch.empty((63, s, 2), dtype=torch.int32, device="cuda"),
                   torch.empty((63,), dtype=torch.int32, device="cuda"))
            geo = [(torch.empty((63, 9), dtype=torch.float64, device="cuda"), torch.empty((63, s), dtype=torch.uint8, device="cuda"),
                    torch.empty((63,), dtype=torch.int32, device="cuda"), torch.empty((63,), dtype=torch.int32, device="cuda"))
                   for _ in range(2)]
        bits, valid = fd.brief_compute(frames, res.xy, res.counts, length=256, half_patch_size=8, with_valid=True)
        fd.brief_match(bits[:-1], bits[1:], res.counts[:-1], res.counts[1:], valid[:-1], valid[1:], max_distance=64,
                       max_ratio=0.9, out=out)
        for model, o in zip(("fundamental", "homography"), geo):
            fd.verify_geometry(res.xy[:-1], res.xy[1:], matches=out[0], counts=res.counts[:-1], model=model, hypotheses=256,
                               threshold=1.0, image_size=(720, 1280), out=o)
            if a.refit:
                fd.refit_geometry(res.xy[:-1], res.xy[1:], fd.GeometryResult(*o), matches=out[0], counts=res.counts[:-1],
                                  model=model, rounds=2, threshold=1.0, image_size=(720, 1280),
                                  out=refit.setdefault(model, tuple(torch.empty_like(x) for x in o)))
            if a.pose and model == "fundamental":
                given = fd.GeometryResult(*(refit[model] if a.refit else o))
                if pose is None:
                    pose = (torch.empty((63, 12), dtype=torch.float64, device="cuda"), torch.empty((63,), dtype=torch.int32, device="cuda"),
                            torch.empty((63, s, 3), dtype=torch.float32, device="cuda"), torch.empty((63, s), dtype=torch.uint8, device="cuda"),
                            torch.empty((63,), dtype=torch.int32, device="cuda"))
                    tri = tuple(torch.empty_like(x) for x in pose[2:])
                fd.recover_pose(res.xy[:-1], res.xy[1:], given, cam, matches=out[0], counts=res.counts[:-1], out=pose)
                fd.triangulate(res.xy[:-1], res.xy[1:], pose[0], cam, matches=out[0], counts=res.counts[:-1], inliers=given.inliers,
                               out=tri)
                if a.pnp:
                    if pnp is None:
                        pnp = [tuple(torch.empty_like(x) for x in (pose[0], pose[3], pose[4], pose[1])) for _ in range(2)]
                    pts = fd.PointsResult(pose[2], pose[3], pose[4])
                    # the points are in units of the pair's baseline, a few of them deep: no conditioning
                    solved = fd.solve_pnp(pts, res.xy[1:], cam, matches=out[0], counts=res.counts[:-1], hypotheses=256,
                                          threshold=2.0, out=pnp[0])
                    fd.refine_pnp(pts, res.xy[1:], solved, cam, matches=out[0], counts=res.counts[:-1], rounds=4, threshold=2.0,
                                  out=pnp[1])
                if a.align:
                    if ali is None:
                        ali = [(torch.empty((63, 13), dtype=torch.float64, device="cuda"), torch.empty_like(pose[3]),
                                torch.empty_like(pose[4]), torch.empty_like(pose[1])) for _ in range(2)]
                        moved = torch.empty_like(pose[2])
                    # the same slots triangulated twice: the list is fd_pnp_ransac's (the points in front), the model the identity
                    src, dst = fd.PointsResult(pose[2], pose[3], pose[4]), fd.PointsResult(*tri)
                    joined = fd.align_points(src, dst, counts=res.counts[:-1], hypotheses=256, threshold=0.05, out=ali[0])
                    fitted = fd.refine_alignment(src, dst, joined, counts=res.counts[:-1], rounds=4, threshold=0.05, out=ali[1])
                    fd.transform_points(fitted, src, counts=res.counts[:-1], out=moved)
                if a.ba:
                    if ba is None:
                        ident = torch.tensor([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0, 0, 0, 0], dtype=torch.float64, device="cuda").repeat(63, 1)
                        ba = (torch.empty((63, 2, 12), dtype=torch.float64, device="cuda"), torch.empty_like(pose[2]),
                              torch.empty((63, 2, s), dtype=torch.uint8, device="cuda"), torch.empty((63,), dtype=torch.int32, device="cuda"),
                              torch.empty((63, 2), dtype=torch.float64, device="cuda"), torch.empty((63,), dtype=torch.int32, device="cuda"))
                    # tracks are slot-aligned in this call: the matched train positions gathered into the query's slots
                    idx = out[0].clamp(min=0).long()[..., None].expand(-1, -1, 2)
                    obs = torch.stack([res.xy[:-1], torch.gather(res.xy[1:], 1, idx)], 1).contiguous()
                    seen = torch.stack([pnp[1][1], pnp[1][1]], 1).contiguous()
                    fd.bundle_adjust([ident, pnp[1][0]], pts, obs, cam, obs_valid=seen, counts=res.counts[:-1], rounds=8, threshold=2.0,
                                     out=ba)
    if a.ba:
        print("bundle adjustment: accepted trials (mean):", float(ba[5].float().mean()), "inlier observations (mean):",
              float(ba[3].float().mean()), "cost before / after (mean):", float(ba[4][:, 0].mean()), float(ba[4][:, 1].mean()))
    if a.align:
        print("frames with an alignment:", int((ali[0][3] >= 0).sum()), "alignment inliers (mean):", float(ali[0][2].float().mean()),
              "refined (mean):", float(ali[1][2].float().mean()), "accepted rounds (mean):", float(ali[1][3].float().mean()))
    if a.pnp:
        print("frames with a PnP pose:", int((pnp[0][3] >= 0).sum()), "PnP inliers (mean):", float(pnp[0][2].float().mean()),
              "refined (mean):", float(pnp[1][2].float().mean()), "accepted rounds (mean):", float(pnp[1][3].float().mean()))
    if a.pose:
        print("frames with a pose:", int((pose[1] >= 0).sum()), "points in front per pair (mean):", float(pose[4].float().mean()),
              "triangulated (mean):", float(tri[2].float().mean()))
    if a.refit:
        print("refit inliers F / H (mean):", *(float(refit[m][2].float().mean()) for m in ("fundamental", "homography")),
              "accepted rounds F / H (mean):", *(float(refit[m][3].float().mean()) for m in ("fundamental", "homography")))
    print("matches per frame pair (mean):", float(out[2].float().mean()), "inliers F / H (mean):",
          float(geo[0][2].float().mean()), float(geo[1][2].float().mean()), "frames without a model:",
          int((geo[0][3] < 0).sum()), int((geo[1][3] < 0).sum()))
elif a.shape == "warp":
    import math

    import numpy as np

    kind = "homography, camera"
    sizes = {"hd": (64, 1080, 1920, a.calls or 10), "vga": (1, 480, 640, a.calls or 200)}
    for b, rows, cols, calls in (sizes.values() if a.warp_size == "both" else (sizes[a.warp_size],)):
        frames = noise(b, rows, cols)
        c, s_ = 1.02 * math.cos(math.radians(3.0)), 1.02 * math.sin(math.radians(3.0))
        cx, cy = (cols - 1) / 2, (rows - 1) / 2
        h = np.array([c, -s_, cx - (c * cx - s_ * cy), s_, c, cy - (s_ * cx + c * cy), 2e-5, -1e-5, 1.0])
        K = np.array([[0.8 * cols, 0, cx], [0, 0.8 * cols, cy], [0, 0, 1.0]])
        cam = fd.camera_params(K, K, [-0.25, 0.08, 0.001, -0.001, 0.0])
        out = (torch.empty((b, rows, cols), dtype=torch.uint8, device="cuda"), torch.empty((b, rows, cols), dtype=torch.uint8, device="cuda"))
        for model, prm in (("homography", h), ("camera", cam)):
            dp = torch.from_numpy(prm).cuda()
            for _ in range(calls):
                fd.warp_frames(frames, dp, model=model, return_mask=True, out=out)
            print(f"{model} {cols}x{rows}x{b}: pixels with a source {float(out[1].float().mean()):.4f}")
elif a.shape == "equalize":
    kind = "tiles 8x8, clip 3.0"
    sizes = {"vga1": (1, 480, 640, a.calls or 200), "vga64": (64, 480, 640, a.calls or 20), "hd": (64, 1080, 1920, a.calls or 10)}
    for b, rows, cols, calls in (sizes.values() if a.eq_size == "all" else (sizes[a.eq_size],)):
        # blurred noise, darkened: neighbouring pixels are close (a camera frame's statistics; uniform noise has none)
        frames = (torch.nn.functional.avg_pool2d(noise(b, rows + 4, cols + 4).float()[:, None], 5, 1)[:, 0] / 3.0).clamp(0, 255).to(torch.uint8).contiguous()
        out = torch.empty_like(frames)
        for _ in range(calls):
            fd.equalize_frames(frames, (8, 8), 3.0, out=out)
        print(f"equalize {cols}x{rows}x{b}: mean in {float(frames.float().mean()):.1f}, mean out {float(out.float().mean()):.1f}, "
              f"levels in {int(frames.unique().numel())}, levels out {int(out.unique().numel())}")
elif a.shape == "blur":
    kind = "r 2 / 3 / 15, pyramids"

    def timed(what, call, calls):
        for _ in range(3):
            call()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(calls + 1)]
        ev[0].record()
        for e in ev[1:]:
            call()
            e.record()
        torch.cuda.synchronize()
        us = sorted(1e3 * x.elapsed_time(y) for x, y in zip(ev, ev[1:]))
        print(f"{what}: median {us[len(us) // 2]:.1f} us per call (min {us[0]:.1f}, max {us[-1]:.1f}), {len(us)} calls")

    sizes = {"vga1": (1, 480, 640, a.calls or 200), "vga64": (64, 480, 640, a.calls or 20), "hd": (64, 1080, 1920, a.calls or 10)}
    for b, rows, cols, calls in (sizes.values() if a.blur_size == "all" else (sizes[a.blur_size],)):
        frames = torch.nn.functional.avg_pool2d(noise(b, rows + 4, cols + 4).float()[:, None], 5, 1)[:, 0].clamp(0, 255).to(torch.uint8).contiguous()
        if a.blur_case in ("all", "blur"):
            full, half = torch.empty_like(frames), torch.empty((b, (rows + 1) // 2, (cols + 1) // 2), dtype=torch.uint8, device="cuda")
            for name, taps, step in (("r 2 step 1", [96, 64, 16], 1), ("r 2 step 2", [96, 64, 16], 2),
                                     ("r 3 step 1", fd.gaussian_taps(2.0, 3)[1], 1), ("r 15 step 1", fd.gaussian_taps(5.0)[1], 1)):
                out = half if step == 2 else full
                timed(f"fd.blur_frames {cols}x{rows}x{b} {name}", lambda: fd.blur_frames(frames, taps=taps, step=step, out=out), calls)
                print(f"  mean in {float(frames.float().mean()):.2f}, mean out {float(out.float().mean()):.2f}")
        if a.blur_case in ("all", "pyramid"):
            for kernel in ("box", "gauss"):
                timed(f"fd.build_pyramid {cols}x{rows}x{b} 3 levels {kernel}", lambda: fd.build_pyramid(frames, 3, kernel=kernel), calls)
elif a.shape == "linedesc":
    kind = "9 bands x 7 rows"
    rows, cols, S = 480, 640, 512
    for b, calls in ((64, a.calls or 20), (1, a.calls or 200)):
        frames = torch.nn.functional.avg_pool2d(noise(b, rows + 4, cols + 4).float()[:, None], 5, 1)[:, 0].clamp(0, 255).to(torch.uint8).contiguous()
        u = torch.rand((b, S, 4), generator=g, device="cuda")
        centre = u[..., :2] * torch.tensor([cols - 1.0, rows - 1.0], device="cuda")
        half = 0.5 * (20.0 + 280.0 * u[..., 2:3]) * torch.stack([torch.cos(6.2831853 * u[..., 3]), torch.sin(6.2831853 * u[..., 3])], -1)
        lines = torch.cat([centre - half, centre + half], -1).contiguous()
        out = (torch.empty((b, S, 72), device="cuda"), torch.empty((b, S, 2), device="cuda"), torch.empty((b, S), dtype=torch.uint8, device="cuda"))
        for _ in range(3):
            fd.describe_lines(frames, lines, out=out)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(calls + 1)]
        ev[0].record()
        for e in ev[1:]:
            fd.describe_lines(frames, lines, out=out)
            e.record()
        torch.cuda.synchronize()
        us = sorted(1e3 * x.elapsed_time(y) for x, y in zip(ev, ev[1:]))
        print(f"fd.describe_lines {cols}x{rows}x{b}, {S} lines per frame, {kind}: median {us[len(us) // 2]:.1f} us per call "
              f"(min {us[0]:.1f}, max {us[-1]:.1f}), {len(us)} calls; valid {float(out[2].float().mean()):.3f}")
elif a.shape == "nnmatch":
    kind = f"dim {a.dim}" + (" cross-check" if a.cross_check else "")
    B, S = 64, 240
    q = torch.nn.functional.normalize(torch.randn((B, S, a.dim), generator=g, device="cuda"), dim=2)
    t = torch.nn.functional.normalize(q.roll(17, 1) + 0.3 * torch.randn((B, S, a.dim), generator=g, device="cuda"), dim=2)
    out = (torch.empty((B, S), dtype=torch.int32, device="cuda"), torch.empty((B, S, 2), dtype=torch.float32, device="cuda"),
           torch.empty((B,), dtype=torch.int32, device="cuda"))

    def ours():
        fd.nn_match(q, t, max_ratio=0.9, cross_check=a.cross_check, out=out)

    def baseline():  # what a caller outside the C ABI writes (no validity, counts or tie rule)
        d = (q * q).sum(2)[:, :, None] + (t * t).sum(2)[:, None, :] - 2.0 * torch.bmm(q, t.transpose(1, 2))
        return torch.topk(d, 2, dim=2, largest=False)

    for name, fn in (("fd.nn_match", ours), ("torch bmm + norms + topk(2)", baseline)):
        for _ in range(3):
            fn()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range((a.calls or 20) + 1)]
        ev[0].record()
        for e in ev[1:]:
            fn()
            e.record()
        torch.cuda.synchronize()
        us = sorted(1e3 * x.elapsed_time(y) for x, y in zip(ev, ev[1:]))
        print(f"{name}, {kind}: median {us[len(us) // 2]:.1f} us per call (min {us[0]:.1f}, max {us[-1]:.1f}), {len(us)} calls")
    print("matches per frame (mean):", float(out[2].float().mean()))
else:
    kind = a.kind or "fast"
    frames = noise(64, 720, 1280)
    for _ in range(a.calls or 10):
        fd.detect_points(kind, frames, 200, 20, THR[kind])
torch.cuda.synchronize()
print("done", a.shape, kind)
