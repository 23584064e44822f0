"""fd_frames_warp on the GPU against tests/warp_ref.py: every byte of out and out_mask, no tolerance. Small
shapes (sources up to 37 x 53) at the packed store's tails and the sampler's edges."""
import ctypes

import numpy as np
import pytest

import warp_ref as W

pytestmark = pytest.mark.gpu

ROWS, COLS = 37, 53
WIDTHS = (1, 3, 4, 5, 7, 8, 9, 63, 64, 65, 67)
FRAMES = np.random.default_rng(21).integers(0, 256, (3, ROWS, COLS), dtype=np.uint8)
IDENTITY = np.eye(3).reshape(9)


@pytest.fixture(scope="module")
def fd():
    import feature_detector_amd as fd

    fd.load()
    return fd


def about_centre(rows, cols, deg, scale, out_rows=None, out_cols=None):
    """Destination -> source: rotation and scale taking the destination's centre to the source's."""
    out_rows, out_cols = out_rows or rows, out_cols or cols
    c, s = np.cos(np.deg2rad(deg)) * scale, np.sin(np.deg2rad(deg)) * scale
    A = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])
    T = lambda tx, ty: np.array([[1, 0, tx], [0, 1, ty], [0, 0, 1.0]])  # noqa: E731
    return (T((cols - 1) / 2, (rows - 1) / 2) @ A @ T(-(out_cols - 1) / 2, -(out_rows - 1) / 2)).reshape(9)


def entry(i, v):
    h = about_centre(ROWS, COLS, 30, 1.3)
    h[i] = v
    return h


HOMOGRAPHIES = {
    "identity": IDENTITY,
    "negated identity": -IDENTITY,
    "integer shift": np.array([1, 0, 5, 0, 1, -3, 0, 0, 1.0]),
    "half pixel": np.array([1, 0, 0.5, 0, 1, -0.5, 0, 0, 1.0]),
    "rotation 30 scale 1.3": about_centre(ROWS, COLS, 30, 1.3),
    # W = 1 - 0.04 x - 0.03 y changes sign inside the destination
    "perspective, W changes sign": np.array([1.1, 0.2, -3, -0.1, 0.9, 2, -0.04, -0.03, 1.0]),
    "W zero on row 2": np.array([1, 0, 0, 0, 1, 0, 0, 1, -2.0]),
    "zeros": np.zeros(9),
    "nan entry": entry(4, np.nan),
    "nan in W": entry(8, np.nan),
    "1e300 entry": entry(1, 1e300),
    "1e300 in W": entry(6, 1e300),
    "scale onto the last column and row": np.array([13, 0, 0, 0, 9, 0, 0, 0, 1.0]),  # x = 4 -> 52, y = 4 -> 36
    "one ulp right of the last column": np.array([1, 0, 2.0 ** -18, 0, 1, 0, 0, 0, 1.0]),
    "one ulp below the last row": np.array([1, 0, 0, 0, 1, 2.0 ** -18, 0, 0, 1.0]),
    "one ulp left of column 0": np.array([1, 0, -(2.0 ** -149), 0, 1, 0, 0, 0, 1.0]),
    "one ulp above row 0": np.array([1, 0, 0, 0, 1, -(2.0 ** -149), 0, 0, 1.0]),
}


def camera(dist, R=None, new_c=(26.0, 18.0), new_f=(60.0, 58.0)):
    K = np.array([[61.5, 0, 25.5], [0, 59.25, 18.25], [0, 0, 1.0]])
    nK = np.array([[new_f[0], 0, new_c[0]], [0, new_f[1], new_c[1]], [0, 0, 1.0]])
    return W.camera_params_ref(nK, K, dist, R)


def rot_y(deg):
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


CAMERAS = {
    "no distortion": camera([0, 0, 0, 0, 0]),
    "barrel": camera([-0.3, 0.1, 0, 0, 0]),
    "pincushion": camera([0.2, 0, 0, 0, 0]),
    "tangential": camera([0.05, 0, 0.02, -0.015, 0]),
    "k3": camera([-0.2, 0.05, 0, 0, 0.4]),
    "rectifying rotation 5": camera([-0.1, 0.02, 0.001, 0.002, 0], rot_y(5).T),
    "principal point outside": camera([-0.3, 0.1, 0, 0, 0], new_c=(-20.0, 50.0)),
    "zero focal length": camera([0, 0, 0, 0, 0], new_f=(0.0, 58.0)),
}


def run_device(fd, frames, params, out_shape=None, model="homography", fill=0):
    """(out, mask) of the device path, as numpy."""
    import torch

    out, mask = fd.warp_frames(torch.from_numpy(np.ascontiguousarray(frames)).cuda(), torch.from_numpy(np.asarray(params)).cuda(),
                               out_shape, model, fill, return_mask=True)
    return out.cpu().numpy(), mask.cpu().numpy()


def same(got, exp, what=""):
    for g, e, name in zip(got, exp, ("out", "mask")):
        g = g.cpu().numpy() if hasattr(g, "cpu") else np.asarray(g)
        assert g.shape == e.shape, (what, name, g.shape, e.shape)
        bad = np.argwhere(g != e)
        assert len(bad) == 0, (what, name, len(bad), bad[:5].tolist())


@pytest.mark.parametrize("src", ((1, 1), (1, 9), (9, 1), (ROWS, COLS)))
def test_destination_widths_and_rows(fd, src):
    """The packed store's tail and the wave's edges: every width with 1, 2 and 5 rows, both models."""
    frame = np.ascontiguousarray(FRAMES[0, :src[0], :src[1]])
    for cols in WIDTHS:
        for rows in (1, 2, 5):
            h = about_centre(src[0], src[1], 20, 0.8 * max(src) / max(cols, rows), rows, cols)
            exp = W.warp_ref(frame, h, (rows, cols), fill=9)
            same(run_device(fd, frame, h, (rows, cols), fill=9), exp, (src, rows, cols))
            if src == (ROWS, COLS):
                assert exp[1].any()
            nK = np.array([[30.0, 0, (cols - 1) / 2], [0, 30.0, (rows - 1) / 2], [0, 0, 1]])
            K = np.array([[25.0, 0, (src[1] - 1) / 2], [0, 25.0, (src[0] - 1) / 2], [0, 0, 1]])
            p = W.camera_params_ref(nK, K, [-0.2, 0.05, 0.01, -0.01, 0.02])
            same(run_device(fd, frame, p, (rows, cols), "camera", 9), W.warp_ref(frame, p, (rows, cols), W.CAMERA, 9),
                 ("camera", src, rows, cols))


@pytest.mark.parametrize("out_shape", ((80, 131), (11, 17)))
def test_destination_larger_and_smaller_than_source(fd, out_shape):
    h = about_centre(ROWS, COLS, -12, COLS / out_shape[1], *out_shape)
    exp = W.warp_ref(FRAMES, h, out_shape, fill=3)
    assert exp[1].mean() > 0.5
    same(run_device(fd, FRAMES, h, out_shape, fill=3), exp)


@pytest.mark.parametrize("off", (1, 2, 3))
def test_unaligned_bases(fd, off):
    """frames, out and out_mask at odd addresses inside larger device buffers whose other bytes must stay."""
    torch = pytest.importorskip("torch")
    h = torch.from_numpy(HOMOGRAPHIES["rotation 30 scale 1.3"]).cuda()
    for rows, cols in ((5, 7), (ROWS, COLS), (6, 64)):
        n = 2 * rows * cols
        exp = W.warp_ref(FRAMES[:2], HOMOGRAPHIES["rotation 30 scale 1.3"], (rows, cols), fill=200)
        src = torch.zeros(FRAMES[:2].size + 8, dtype=torch.uint8, device="cuda")
        src[off:off + FRAMES[:2].size] = torch.from_numpy(FRAMES[:2].reshape(-1)).cuda()
        fr = src[off:off + FRAMES[:2].size].view(2, ROWS, COLS)
        big_o = torch.full((n + 16,), 0xA5, dtype=torch.uint8, device="cuda")
        big_m = torch.full((n + 16,), 0xA5, dtype=torch.uint8, device="cuda")
        moff = 4 + (off + 1) % 4  # the mask's own alignment: 2, 3, 0 bytes past a dword
        out = (big_o[4 + off:4 + off + n].view(2, rows, cols), big_m[moff:moff + n].view(2, rows, cols))
        assert out[0].data_ptr() % 4 == off
        got = fd.warp_frames(fr, h, (rows, cols), fill=200, return_mask=True, out=out)
        assert got[0].data_ptr() == out[0].data_ptr()
        same(got, exp, (off, rows, cols))
        for big, o in ((big_o, 4 + off), (big_m, moff)):
            rest = torch.cat([big[:o], big[o + n:]]).cpu().numpy()
            assert (rest == 0xA5).all()
        same((fd.warp_frames(fr, h, (rows, cols), fill=200, out=out[0]), out[1]), exp)  # without a mask


@pytest.mark.parametrize("name", sorted(HOMOGRAPHIES))
def test_homographies(fd, name):
    h = HOMOGRAPHIES[name]
    for out_shape, fill in (((ROWS, COLS), 0), ((40, 67), 200), ((5, 5), 200)):
        same(run_device(fd, FRAMES[0], h, out_shape, fill=fill), W.warp_ref(FRAMES[0], h, out_shape, fill=fill), (name, out_shape))


def test_expected_homography_cases_are_what_they_claim():
    """The yardstick's side of the cases above, so that an all-fill output cannot pass for an edge case."""
    exp = lambda name, shape=(ROWS, COLS): W.warp_ref(FRAMES[0], HOMOGRAPHIES[name], shape, fill=200)  # noqa: E731
    for name in ("identity", "negated identity"):
        out, mask = exp(name)
        assert np.array_equal(out[0], FRAMES[0]) and mask.all()
    out, mask = exp("integer shift")
    assert np.array_equal(out[0, 3:, :48], FRAMES[0, :34, 5:]) and mask.sum() == 34 * 48
    out, mask = exp("perspective, W changes sign")
    assert mask.any() and not mask.all()
    out, mask = exp("W zero on row 2")
    assert not mask[0, 2].any() and (out[0, 2] == 200).all() and mask[0, 3].any()
    for name in ("zeros", "nan entry", "nan in W"):
        assert not exp(name)[1].any()
    assert exp("1e300 entry")[1][0, 0].any() and not exp("1e300 entry")[1][0, 1:].any()  # row 0 does not meet h1
    out, mask = exp("scale onto the last column and row", (5, 5))
    assert mask.all() and out[0, 4, 4] == FRAMES[0, 36, 52] and out[0, 0, 4] == FRAMES[0, 0, 52]
    out, mask = exp("one ulp right of the last column")
    assert mask[0, :, :52].all() and not mask[0, :, 52].any()
    out, mask = exp("one ulp below the last row")
    assert mask[0, :36].all() and not mask[0, 36].any()
    out, mask = exp("one ulp left of column 0")
    assert mask[0, :, 1:].all() and not mask[0, :, 0].any() and np.array_equal(out[0, :, 1:], FRAMES[0, :, 1:])
    out, mask = exp("one ulp above row 0")
    assert mask[0, 1:].all() and not mask[0, 0].any()


@pytest.mark.parametrize("name", sorted(CAMERAS))
def test_camera_models(fd, name):
    p = CAMERAS[name]
    for out_shape, fill in (((ROWS, COLS), 0), ((41, 67), 200)):
        exp = W.warp_ref(FRAMES[1], p, out_shape, W.CAMERA, fill)
        if name == "zero focal length":
            assert not exp[1].any()
        elif name != "principal point outside":
            assert exp[1].mean() > 0.4 and not np.array_equal(exp[0][0, :ROWS, :COLS], FRAMES[1])
        same(run_device(fd, FRAMES[1], p, out_shape, "camera", fill), exp, (name, out_shape))


def test_batch_of_three_models_and_shared(fd):
    hs = np.stack([HOMOGRAPHIES[n] for n in ("half pixel", "rotation 30 scale 1.3", "perspective, W changes sign")])
    exp = W.warp_ref(FRAMES, hs, (39, 66), fill=17)
    assert not np.array_equal(exp[0][0], exp[0][1])
    same(run_device(fd, FRAMES, hs, (39, 66), fill=17), exp)
    same(run_device(fd, FRAMES, hs[1], (39, 66), fill=17), W.warp_ref(FRAMES, hs[1], (39, 66), fill=17))
    cs = np.stack([CAMERAS[n] for n in ("barrel", "tangential", "rectifying rotation 5")])
    same(run_device(fd, FRAMES, cs, (39, 66), "camera", 17), W.warp_ref(FRAMES, cs, (39, 66), W.CAMERA, 17))
    same(run_device(fd, FRAMES, cs[0], (39, 66), "camera", 17), W.warp_ref(FRAMES, cs[0], (39, 66), W.CAMERA, 17))


@pytest.mark.parametrize("frames_dev", (0, 1))
@pytest.mark.parametrize("params_dev", (0, 1))
@pytest.mark.parametrize("out_dev", (0, 1))
def test_host_and_device_pointers(fd, frames_dev, params_dev, out_dev):
    """Each of frames, params and the outputs on the host or on the device, through the C ABI."""
    torch = pytest.importorskip("torch")
    from feature_detector_amd import _lib
    from feature_detector_amd._lib import fd_warp_opts

    hs = np.stack([HOMOGRAPHIES[n] for n in ("half pixel", "rotation 30 scale 1.3", "perspective, W changes sign")])
    rows, cols = 38, 61
    exp = W.warp_ref(FRAMES, hs, (rows, cols), fill=5)
    L, ctx = fd.load(), fd.default_context()
    ctx.set_stream(None)
    side = lambda a, dev: torch.from_numpy(a).cuda() if dev else a  # noqa: E731
    p = lambda a: ctypes.c_void_p(a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data)  # noqa: E731
    fr, pr = side(FRAMES, frames_dev), side(hs, params_dev)
    out, mask = side(np.full((3, rows, cols), 0xA5, np.uint8), out_dev), side(np.full((3, rows, cols), 0xA5, np.uint8), out_dev)
    torch.cuda.synchronize()
    opts = fd_warp_opts(0, 0, 5)
    _lib.check(ctx.ptr, L.fd_frames_warp(ctx.ptr, p(fr), frames_dev, 3, ROWS, COLS, ctypes.byref(opts), p(pr), params_dev, rows,
                                         cols, p(out), p(mask), out_dev))
    ctx.synchronize()
    same((out, mask), exp)
    # the Python call: outputs on the side of the frames
    got = fd.warp_frames(fr, pr, (rows, cols), fill=5, return_mask=True)
    assert all(hasattr(g, "cpu") == bool(frames_dev) for g in got)
    same(got, exp)


def test_numpy_slices_as_frames(fd):
    """A host frame batch at an odd address (a slice of a byte buffer) and a non-contiguous one."""
    buf = np.zeros(FRAMES.size + 3, np.uint8)
    buf[3:] = FRAMES.reshape(-1)
    fr = buf[3:].reshape(FRAMES.shape)
    h = HOMOGRAPHIES["rotation 30 scale 1.3"]
    same(fd.warp_frames(fr, h, (35, 51), return_mask=True), W.warp_ref(FRAMES, h, (35, 51)))
    part = FRAMES[:, 2:30, 5:44]
    same(fd.warp_frames(part, IDENTITY, return_mask=True), W.warp_ref(np.ascontiguousarray(part), IDENTITY))


def test_graph_capture(fd):
    torch = pytest.importorskip("torch")
    hs = np.stack([HOMOGRAPHIES[n] for n in ("half pixel", "rotation 30 scale 1.3", "perspective, W changes sign")])
    dfr, dp = torch.from_numpy(FRAMES).cuda(), torch.from_numpy(hs).cuda()
    out = (torch.empty((3, 40, 67), dtype=torch.uint8, device="cuda"), torch.empty((3, 40, 67), dtype=torch.uint8, device="cuda"))
    kw = dict(out_shape=(40, 67), fill=31, return_mask=True, out=out)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):  # no warm call: the stage has no workspace
        fd.warp_frames(dfr, dp, **kw)
    for step in (1, 2):  # new contents in the same tensors
        host_frames = np.ascontiguousarray(FRAMES[::-1]) if step == 1 else np.ascontiguousarray(FRAMES[:, ::-1])
        host_p = np.ascontiguousarray(hs[::-1]) if step == 1 else hs * np.float64(-0.5 * step)
        dfr.copy_(torch.from_numpy(host_frames))
        dp.copy_(torch.from_numpy(host_p))
        for o in out:
            o.fill_(0xA5)
        g.replay()
        torch.cuda.synchronize()
        same(out, W.warp_ref(host_frames, host_p, (40, 67), fill=31), step)
    del g


def test_chain_detect_match_verify_register(fd, image_png):
    """detect -> describe -> match -> verify on device tensors, then warp_frames with the verifier's device model
    as it is: q = the previous frame, t = the next, and the next frame lands on the previous one."""
    torch = pytest.importorskip("torch")
    prev_h = np.ascontiguousarray(image_png[24:264, 24:344])
    c, s = np.cos(np.deg2rad(1.0)), np.sin(np.deg2rad(1.0))
    # next[p] = prev[P p]: the content moves by P^-1
    P = np.array([[c, -s, 5.0], [s, c, -4.25], [0, 0, 1.0]]).reshape(9)
    next_h = W.warp_ref(prev_h, P)[0][0]
    dev = torch.from_numpy(np.stack([prev_h, next_h])).cuda()
    det = fd.detect_points("harris", dev, 200, 15, 30.0)
    bits, valid = fd.brief_compute(dev, det.xy, det.counts, with_valid=True)
    m = fd.brief_match(bits[0:1], bits[1:2], det.counts[0:1], det.counts[1:2], valid[0:1], valid[1:2], cross_check=True,
                       max_distance=64)
    geo = fd.verify_geometry(det.xy[0:1], det.xy[1:2], matches=m.idx, counts=det.counts[0:1], model="homography",
                             hypotheses=256, seed=3, threshold=1.5, image_size=(240, 320))
    p0 = geo.model.data_ptr()
    reg, mask = fd.warp_frames(dev[1:2], geo.model, return_mask=True)
    torch.cuda.synchronize()
    assert geo.model.data_ptr() == p0 and geo.model.is_cuda
    H = geo.model.cpu().numpy()
    assert int(geo.best[0]) >= 0 and int(geo.counts[0]) >= 10, (geo.best.tolist(), geo.counts.tolist())
    exp = W.warp_ref(next_h, H[0])
    same((reg, mask), exp)
    # the registration itself (not a bit check): the next frame warped back agrees with the previous one
    inner = exp[1][0, 20:-20, 20:-20] == 1
    diff = np.abs(exp[0][0, 20:-20, 20:-20].astype(int) - prev_h[20:-20, 20:-20].astype(int))[inner]
    print(f"chain: {int(geo.counts[0])} inliers, mean |registered - previous| {diff.mean():.3f} over {int(inner.sum())} pixels")
    assert inner.mean() > 0.9 and diff.mean() < np.abs(next_h[20:-20, 20:-20].astype(int) - prev_h[20:-20, 20:-20].astype(int)).mean()


def test_empty_destination_and_bad_arguments(fd):
    from feature_detector_amd import _lib
    from feature_detector_amd._lib import fd_warp_opts

    assert fd.warp_frames(FRAMES, IDENTITY, (0, 7)).shape == (3, 0, 7)
    L, ctx = fd.load(), fd.default_context()
    ctx.set_stream(None)
    out = np.full((3, 4, 4), 0xA5, np.uint8)
    p = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    call = lambda fr, o, pr, ot, batch=3, rows=ROWS, orows=4, ocols=4: L.fd_frames_warp(  # noqa: E731
        ctx.ptr, p(fr), 0, batch, rows, COLS, None if o is None else ctypes.byref(o), p(pr), 0, orows, ocols, p(ot), None, 0)
    ok = fd_warp_opts(0, 1, 0)
    assert call(FRAMES, ok, IDENTITY, out, orows=0) == 0 and call(FRAMES, ok, IDENTITY, out, ocols=0) == 0
    assert (out == 0xA5).all()
    bad = [(None, ok, IDENTITY, out, {}), (FRAMES, None, IDENTITY, out, {}), (FRAMES, ok, None, out, {}),
           (FRAMES, ok, IDENTITY, None, {}), (FRAMES, ok, IDENTITY, out, {"batch": 0}), (FRAMES, ok, IDENTITY, out, {"rows": 0}),
           (FRAMES, ok, IDENTITY, out, {"orows": -1}), (FRAMES, ok, IDENTITY, out, {"ocols": -1}),
           (FRAMES, fd_warp_opts(2, 1, 0), IDENTITY, out, {}), (FRAMES, fd_warp_opts(-1, 1, 0), IDENTITY, out, {}),
           (FRAMES, fd_warp_opts(0, 2, 0), IDENTITY, out, {}), (FRAMES, fd_warp_opts(0, 1, 256), IDENTITY, out, {}),
           (FRAMES, fd_warp_opts(0, 1, -1), IDENTITY, out, {})]
    for fr, o, pr, ot, kw in bad:
        with pytest.raises(fd.FdError) as e:
            _lib.check(ctx.ptr, call(fr, o, pr, ot, **kw))
        assert e.value.code == _lib.FD_ERR_INVALID and str(e.value).strip()
    with pytest.raises(ValueError):
        fd.warp_frames(FRAMES, np.zeros((2, 9)))
    with pytest.raises(ValueError):
        fd.warp_frames(FRAMES, IDENTITY, model="camera")
    with pytest.raises(ValueError):
        fd.warp_frames(FRAMES, IDENTITY, fill=300)
