"""fd_frames_equalize on the GPU against tests/equalize_ref.py: every byte of out, no tolerance. Small shapes at
the packed store's tails, the tiles' shapes, each branch of the clip and redistribution (asserted from the
reference's lim / E / r), the histogram's corners and the calling conventions."""
import ctypes

import numpy as np
import pytest

import equalize_ref as R

pytestmark = pytest.mark.gpu

ROWS, COLS = 37, 53
FRAMES = np.random.default_rng(33).integers(0, 256, (3, ROWS, COLS), dtype=np.uint8)
FRAMES[1] = (FRAMES[1] >> 3) + 90   # a low-contrast frame: bins above every limit
FRAMES[2, :, 20:] = 7               # a flat region
# the crop of the example image on which the CPU oracle alone finds more Shi-Tomasi corners after equalization
# (tests/test_equalize_host.py): rows 240..479, columns 48..367
CHAIN_CROP = (slice(240, 480), slice(48, 368))


@pytest.fixture(scope="module")
def fd():
    import feature_detector_amd as fd

    fd.load()
    return fd


def run_device(fd, frames, tiles, clip_milli):
    import torch

    out = fd.equalize_frames(torch.from_numpy(np.ascontiguousarray(frames)).cuda(), tiles, clip_milli / 1000.0)
    return out.cpu().numpy()


def same(got, exp, what=""):
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    assert got.shape == exp.shape and got.dtype == np.uint8, (what, got.shape, exp.shape)
    bad = np.argwhere(got != exp)
    assert len(bad) == 0, (what, len(bad), bad[:5].tolist(), got[tuple(bad[0])], exp[tuple(bad[0])])


def tile_infos(infos):
    return [t for frame in infos for row in frame for t in row]


@pytest.mark.parametrize("off", (1, 2, 3))
def test_store_tails_and_unaligned_bases(fd, off):
    """frames and out as slices starting `off` bytes into larger device buffers whose other bytes must stay."""
    torch = pytest.importorskip("torch")
    exp = R.equalize_ref(FRAMES[:2], (3, 2), 3000)
    n = FRAMES[:2].size
    src = torch.zeros(n + 8, dtype=torch.uint8, device="cuda")
    src[off:off + n] = torch.from_numpy(FRAMES[:2].reshape(-1)).cuda()
    fr = src[off:off + n].view(2, ROWS, COLS)
    for out_off in (off, (off + 1) % 4):  # the same alignment as the frames, and another one
        big = torch.full((n + 16,), 0xA5, dtype=torch.uint8, device="cuda")
        out = big[4 + out_off:4 + out_off + n].view(2, ROWS, COLS)
        assert out.data_ptr() % 4 == out_off and fr.data_ptr() % 4 == off
        got = fd.equalize_frames(fr, (3, 2), 3.0, out=out)
        assert got.data_ptr() == out.data_ptr()
        same(got, exp, (off, out_off))
        rest = torch.cat([big[:4 + out_off], big[4 + out_off + n:]]).cpu().numpy()
        assert (rest == 0xA5).all()


@pytest.mark.parametrize("shape,tiles,clip_milli", (
    ((61, 67), (5, 7), 3000),     # unequal tile sizes on both axes
    ((61, 67), (7, 5), 0),        # the same, unclipped AHE
    ((8, 8), (8, 8), 3000),       # tile area 1, tiles == dimension
    ((ROWS, COLS), (1, 1), 0),    # one tile, no clipping: global equalization
    ((64, 96), (32, 32), 2000),   # the maximum tile count
    ((5, 300), (2, 1), 3000),     # more than one workgroup column, rows fewer than the waves
    ((300, 5), (1, 32), 3000),    # one dword per row, many row cells
    ((1, 1), (1, 1), 3000),
))
def test_tile_shapes(fd, shape, tiles, clip_milli):
    frame = np.random.default_rng(shape[0] * 1000 + shape[1]).integers(0, 256, shape, dtype=np.uint8)
    exp = R.equalize_ref(frame, tiles, clip_milli)
    if tiles == (1, 1) and clip_milli == 0 and frame.size > 1:  # written independently: cumsum of bincount
        cdf = np.cumsum(np.bincount(frame.reshape(-1), minlength=256))
        assert np.array_equal(exp, ((cdf * 255 + frame.size // 2) // frame.size).astype(np.uint8)[frame])
    same(run_device(fd, frame, tiles, clip_milli), exp, (shape, tiles, clip_milli))


def test_limit_clamped_to_one_and_no_bin_clipped(fd):
    exp, infos = R.equalize_ref(FRAMES[0], (3, 2), 1, with_info=True)
    assert all(t["lim"] == 1 for t in tile_infos(infos))
    same(run_device(fd, FRAMES[0], (3, 2), 1), exp, "lim 1")
    exp, infos = R.equalize_ref(FRAMES[0], (1, 1), 40000, with_info=True)
    assert infos[0][0][0]["E"] == 0 and infos[0][0][0]["lim"] > 1
    same(run_device(fd, FRAMES[0], (1, 1), 40000), exp, "E 0")
    # a large limit where bins are clipped all the same: the low-contrast and the flat frame, 6 tiles
    exp, infos = R.equalize_ref(FRAMES[1:], (3, 2), 40000, with_info=True)
    assert any(t["E"] > 0 for t in tile_infos(infos))
    same(run_device(fd, FRAMES[1:], (3, 2), 40000), exp, "clip 40000")


# single-tile frames of 512 pixels: lim = clip_milli // 500. Constant: E = 512 - lim. Two-valued, 256 pixels
# each: E = 2 * (256 - lim).
@pytest.mark.parametrize("kind,clip_milli,r", (
    ("constant", 128000, 0), ("constant", 127500, 1), ("constant", 64500, 127), ("constant", 64000, 128),
    ("constant", 63500, 129), ("constant", 500, 255), ("two", 96000, 128), ("two", 64000, 0), ("two", 95500, 130),
    ("two", 64500, 254),
))
def test_redistribution_residuals(fd, kind, clip_milli, r):
    frame = np.full((16, 32), 77, np.uint8)
    if kind == "two":
        frame[:, 16:] = 201
    exp, infos = R.equalize_ref(frame, (1, 1), clip_milli, with_info=True)
    t = infos[0][0][0]
    assert t["r"] == r and t["E"] > 0 and t["lim"] == clip_milli // 500, t
    same(run_device(fd, frame, (1, 1), clip_milli), exp, (kind, clip_milli, t))


@pytest.mark.parametrize("clip_milli", (0, 3000))
def test_saturated_frames(fd, clip_milli):
    half = np.zeros((ROWS, COLS), np.uint8)
    half[:, COLS // 2:] = 255
    frames = np.stack([np.zeros((ROWS, COLS), np.uint8), np.full((ROWS, COLS), 255, np.uint8), half])
    for tiles in ((1, 1), (3, 2)):
        same(run_device(fd, frames, tiles, clip_milli), R.equalize_ref(frames, tiles, clip_milli), (tiles, clip_milli))


@pytest.mark.parametrize("tiles", ((1, 1), (2, 2)))
def test_counters_past_16_bits(fd, tiles):
    """69 632 equal pixels in one tile: a 16-bit counter would wrap."""
    frame = np.full((272, 256), 131, np.uint8)
    for clip_milli in (0, 3000):
        exp = R.equalize_ref(frame, tiles, clip_milli)
        assert clip_milli or (exp == 255).all()  # unclipped: the whole mass sits at cdf = A
        same(run_device(fd, frame, tiles, clip_milli), exp, (tiles, clip_milli))


def test_batch_of_three(fd):
    exp = R.equalize_ref(FRAMES, (3, 2), 3000)
    assert not np.array_equal(exp[0], exp[1]) and not np.array_equal(exp[1], exp[2])
    same(run_device(fd, FRAMES, (3, 2), 3000), exp)
    for b in range(3):  # no cross-talk: a frame of the batch equals the frame alone
        same(run_device(fd, FRAMES[b], (3, 2), 3000), exp[b], b)


@pytest.mark.parametrize("frames_dev", (0, 1))
@pytest.mark.parametrize("out_dev", (0, 1))
def test_host_and_device_pointers(fd, frames_dev, out_dev):
    """frames and out each on the host or on the device, through the C ABI; then the Python call."""
    torch = pytest.importorskip("torch")
    from feature_detector_amd import _lib
    from feature_detector_amd._lib import fd_equalize_opts

    exp = R.equalize_ref(FRAMES, (4, 3), 2500)
    L, ctx = fd.load(), fd.default_context()
    ctx.set_stream(None)
    side = lambda a, dev: torch.from_numpy(a).cuda() if dev else a  # noqa: E731
    p = lambda a: ctypes.c_void_p(a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data)  # noqa: E731
    fr, out = side(FRAMES.copy(), frames_dev), side(np.full(FRAMES.shape, 0xA5, np.uint8), out_dev)
    torch.cuda.synchronize()
    opts = fd_equalize_opts(4, 3, 2500)
    _lib.check(ctx.ptr, L.fd_frames_equalize(ctx.ptr, p(fr), frames_dev, 3, ROWS, COLS, ctypes.byref(opts), p(out), out_dev))
    ctx.synchronize()
    same(out, exp)
    got = fd.equalize_frames(fr, (4, 3), 2.5)  # outputs on the side of the frames
    assert hasattr(got, "cpu") == bool(frames_dev)
    same(got, exp)
    same(fr, FRAMES)  # the frames stayed


def test_preallocated_out_and_in_place(fd):
    torch = pytest.importorskip("torch")
    exp = R.equalize_ref(FRAMES, (3, 2), 3000)
    dev = torch.from_numpy(FRAMES).cuda()
    out = torch.full(FRAMES.shape, 0xA5, dtype=torch.uint8, device="cuda")
    assert fd.equalize_frames(dev, (3, 2), 3.0, out=out) is out
    same(out, exp)
    same(dev, FRAMES)
    assert fd.equalize_frames(dev, (3, 2), 3.0, out=dev) is dev  # in place on the device
    same(dev, exp)
    host = FRAMES.copy()
    assert fd.equalize_frames(host, (3, 2), 3.0, out=host) is host  # in place on the host
    same(host, exp)
    one = fd.equalize_frames(FRAMES[0], 2, None)  # [rows, cols] in, [rows, cols] out; one int; no clipping
    same(one, R.equalize_ref(FRAMES[0], (2, 2), 0))
    with pytest.raises(ValueError):
        fd.equalize_frames(dev, out=out[:2])
    with pytest.raises(ValueError):
        fd.equalize_frames(FRAMES, out=out)  # out on the other side


def test_graph_capture(fd):
    torch = pytest.importorskip("torch")
    dfr = torch.from_numpy(FRAMES).cuda()
    out = torch.empty(FRAMES.shape, dtype=torch.uint8, device="cuda")
    fd.equalize_frames(dfr, (3, 2), 3.0, out=out)  # the warm call: the workspace of the shape
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        fd.equalize_frames(dfr, (3, 2), 3.0, out=out)
    for step in (1, 2):  # new contents in the captured input
        host = np.ascontiguousarray(FRAMES[::-1]) if step == 1 else np.ascontiguousarray(FRAMES[:, ::-1, ::-1])
        dfr.copy_(torch.from_numpy(host))
        out.fill_(0xA5)
        g.replay()
        torch.cuda.synchronize()
        same(out, R.equalize_ref(host, (3, 2), 3000), step)
    del g


def test_error_codes(fd):
    from feature_detector_amd import _lib
    from feature_detector_amd._lib import fd_equalize_opts

    L, ctx = fd.load(), fd.default_context()
    ctx.set_stream(None)
    out = np.full(FRAMES.shape, 0xA5, np.uint8)
    p = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    call = lambda fr, o, ot, batch=3, rows=ROWS, cols=COLS, c=ctx.ptr: L.fd_frames_equalize(  # noqa: E731
        c, p(fr), 0, batch, rows, cols, None if o is None else ctypes.byref(o), p(ot), 0)
    ok = fd_equalize_opts(3, 2, 3000)
    assert call(FRAMES, ok, out) == 0
    assert call(FRAMES, ok, out, c=None) == _lib.FD_ERR_INVALID
    bad = [(None, ok, out, {}), (FRAMES, None, out, {}), (FRAMES, ok, None, {}), (FRAMES, ok, out, {"batch": 0}),
           (FRAMES, ok, out, {"rows": 0}), (FRAMES, ok, out, {"cols": 0}), (FRAMES, fd_equalize_opts(0, 2, 3000), out, {}),
           (FRAMES, fd_equalize_opts(33, 2, 3000), out, {}), (FRAMES, fd_equalize_opts(3, 0, 3000), out, {}),
           (FRAMES, fd_equalize_opts(3, 33, 3000), out, {}), (FRAMES, fd_equalize_opts(3, 2, -1), out, {}),
           (FRAMES, fd_equalize_opts(9, 2, 3000), out, {"cols": 8}),   # more tiles than columns
           (FRAMES, fd_equalize_opts(3, 5, 3000), out, {"rows": 4}),   # more tiles than rows
           (FRAMES, fd_equalize_opts(1, 1, 3000), out, {"batch": 1, "rows": 4097, "cols": 4096})]  # a tile above 2^24 pixels
    before = out.copy()
    for fr, o, ot, kw in bad:
        with pytest.raises(fd.FdError) as e:
            _lib.check(ctx.ptr, call(fr, o, ot, **kw))
        assert e.value.code == _lib.FD_ERR_INVALID and str(e.value).strip(), kw
    assert np.array_equal(out, before)
    with pytest.raises(ValueError):  # the Python call refuses the same tile before the library
        fd.equalize_frames(np.zeros((4097, 4096), np.uint8), 1)


def test_chain_equalize_then_detect(fd, image_png):
    """A darkened crop equalized on the device and handed to detect_points as it is: the features equal those of
    the reference-equalized frame bit for bit, and there are strictly more Shi-Tomasi corners than on the
    darkened frame at detect_points' default options."""
    torch = pytest.importorskip("torch")
    dark = np.ascontiguousarray(image_png[CHAIN_CROP]) >> 2
    exp = R.equalize_ref(dark)
    dev = torch.from_numpy(dark).cuda()
    eq = fd.equalize_frames(dev)
    res = fd.detect_points("shi_tomasi", eq, 500)
    ref = fd.detect_points("shi_tomasi", torch.from_numpy(exp).cuda(), 500)
    plain = fd.detect_points("shi_tomasi", dev, 500)
    torch.cuda.synchronize()
    same(eq, exp)
    assert np.array_equal(res.counts.cpu().numpy(), ref.counts.cpu().numpy())
    assert np.array_equal(res.features(0).view(np.uint32), ref.features(0).view(np.uint32))
    n_eq, n_dark = len(res.features(0)), len(plain.features(0))
    print(f"chain: {n_dark} Shi-Tomasi corners on the darkened crop, {n_eq} after equalization")
    assert n_eq > n_dark
