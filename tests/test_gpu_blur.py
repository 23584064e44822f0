"""fd_frames_blur / fd_pyr_build_gauss on the GPU against tests/blur_ref.py: every byte, no tolerance. k_blur's
tile is 128 output columns by 32 output rows (16 or 8 rows while a launch has fewer than 512 workgroups:
blur_ref.tile_rows restates launch_blur's rule), and a radius runs in the instance of loop bound 2, 3, 5, 8, 11
or 15 that holds it: the shapes, batches and radii below sit on those edges."""
import ctypes

import numpy as np
import pytest

import blur_ref as R
import flow_ref

pytestmark = pytest.mark.gpu

TILE_COLS = 128
ROWS, COLS = 37, 53
FRAMES = np.random.default_rng(41).integers(0, 256, (3, ROWS, COLS), dtype=np.uint8)
G5 = [20, 20, 19, 17, 15, 12, 10, 8, 6, 4, 3, 2, 1, 1, 0, 0]  # gaussian_taps(5.0): r = 15 (tests/test_blur_host.py)
# one table per kernel instance (loop bounds 2, 2, 2, 3, 5, 8, 11, 15) and a legal one that does not decrease
TAPS = {"copy": [256], "r1": [128, 64], "pyr": [96, 64, 16], "r3": [54, 49, 34, 18], "r5": [68, 58, 32, 4, 0, 0],
        "sigma2": [50, 45, 31, 17, 7, 2, 1], "r11": [26, 24, 22, 18, 14, 12, 8, 6, 5, 3, 2, 1], "sigma5": G5,
        "dip": [0, 128]}


@pytest.fixture(scope="module")
def fd():
    import feature_detector_amd as fd

    fd.load()
    assert fd.gaussian_taps(5.0) == (15, G5) and fd.gaussian_taps(2.0) == (6, TAPS["sigma2"])
    assert fd.gaussian_taps(2.0, 3) == (3, TAPS["r3"])
    for t in TAPS.values():
        R.check_taps(t)
    return fd


def run_device(fd, frames, taps, step=1):
    import torch

    return fd.blur_frames(torch.from_numpy(np.ascontiguousarray(frames)).cuda(), taps=taps, step=step).cpu().numpy()


def same(got, exp, what=""):
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    assert got.shape == exp.shape and got.dtype == np.uint8, (what, got.shape, exp.shape)
    bad = np.argwhere(got != exp)
    assert len(bad) == 0, (what, len(bad), bad[:5].tolist(), got[tuple(bad[0])], exp[tuple(bad[0])])


def noise(shape, seed=None):
    return np.random.default_rng(shape[-2] * 1000 + shape[-1] if seed is None else seed).integers(0, 256, shape, dtype=np.uint8)


@pytest.mark.parametrize("shape", ((1, 1), (1, 40), (40, 1), (3, 3), (2, 5)))
def test_multi_bounce_reflection(fd, shape):
    """Dimensions far below the radius 15: an index bounces many times."""
    frame = noise(shape)
    for step in (1, 2):
        same(run_device(fd, frame, G5, step), R.blur_ref(frame, G5, step), (shape, step))
    same(run_device(fd, frame, TAPS["pyr"]), R.blur_ref(frame, TAPS["pyr"]), shape)


@pytest.mark.parametrize("name", sorted(TAPS))
@pytest.mark.parametrize("step", (1, 2))
def test_radii_and_taps(fd, name, step):
    """Every kernel instance on a batch of three odd-sized frames (more than one tile row at 8 rows a tile)."""
    assert R.tile_rows((ROWS + step - 1) // step, (COLS + step - 1) // step, 3) == 8
    exp = R.blur_ref(FRAMES, TAPS[name], step)
    if name == "copy" and step == 1:
        assert np.array_equal(exp, FRAMES)
    same(run_device(fd, FRAMES, TAPS[name], step), exp, (name, step))


@pytest.mark.parametrize("cols", (TILE_COLS - 4, TILE_COLS - 3, TILE_COLS - 1, TILE_COLS, TILE_COLS + 1, 2 * TILE_COLS - 1,
                                  2 * TILE_COLS, 2 * TILE_COLS + 1))
def test_columns_at_the_tile_width(fd, cols):
    """One below, at and one above a multiple of the 128-column tile (and 124 / 125: where the 3 bytes a row's
    dwords may start early push the last columns into a second workgroup)."""
    frame = noise((2, 11, cols))
    for name in ("pyr", "sigma5"):
        same(run_device(fd, frame, TAPS[name]), R.blur_ref(frame, TAPS[name]), (cols, name))
    wide = noise((2, 11, 2 * cols - 1))  # step 2: the same output widths
    same(run_device(fd, wide, TAPS["pyr"], 2), R.blur_ref(wide, TAPS["pyr"], 2), (cols, "step 2"))


@pytest.mark.parametrize("rows,batch,tile", ((7, 1, 8), (8, 1, 8), (9, 1, 8), (31, 130, 16), (32, 130, 16), (33, 100, 16),
                                             (31, 300, 32), (32, 300, 32), (33, 300, 32)))
def test_rows_at_each_tile_height(fd, rows, batch, tile):
    """One below, at and one above a multiple of the tile height, at each of the three heights launch_blur picks
    (129 columns: two workgroup columns)."""
    cols = TILE_COLS + 1
    assert R.tile_rows(rows, cols, batch) == tile
    frames = noise((batch, rows, cols))
    same(run_device(fd, frames, TAPS["sigma2"]), R.blur_ref(frames, TAPS["sigma2"]), (rows, batch))
    tall = noise((batch, 2 * rows - 1, 2 * cols - 1), seed=rows)  # step 2 with the same output shape
    same(run_device(fd, tall, TAPS["pyr"], 2), R.blur_ref(tall, TAPS["pyr"], 2), (rows, batch, "step 2"))


@pytest.mark.parametrize("shape", ((5, 300), (300, 5)))
def test_thin_frames(fd, shape):
    frame = noise(shape)
    for name, step in (("pyr", 1), ("sigma5", 1), ("pyr", 2), ("sigma2", 2)):
        same(run_device(fd, frame, TAPS[name], step), R.blur_ref(frame, TAPS[name], step), (shape, name, step))


def test_values(fd):
    """All 255 at r = 15 (h reaches 65280), all 0, a 0 / 255 checkerboard, impulses in the corners and the centre."""
    full = np.full((ROWS, COLS), 255, np.uint8)
    same(run_device(fd, full, G5), full, "255")
    same(run_device(fd, full, G5, 2), full[::2, ::2], "255 step 2")
    zero = np.zeros((ROWS, COLS), np.uint8)
    same(run_device(fd, zero, G5), zero, "0")
    yy, xx = np.mgrid[0:ROWS, 0:COLS]
    checker = (((yy + xx) & 1) * 255).astype(np.uint8)
    for name in ("r1", "pyr", "dip", "sigma5"):
        for step in (1, 2):
            same(run_device(fd, checker, TAPS[name], step), R.blur_ref(checker, TAPS[name], step), ("checker", name, step))
    for y, x in ((0, 0), (0, COLS - 1), (ROWS - 1, 0), (ROWS - 1, COLS - 1), (ROWS // 2, COLS // 2)):
        imp = np.zeros((ROWS, COLS), np.uint8)
        imp[y, x] = 255
        for name in ("pyr", "sigma2", "sigma5"):
            exp = R.blur_ref(imp, TAPS[name])
            assert exp.any()
            same(run_device(fd, imp, TAPS[name]), exp, ("impulse", y, x, name))


@pytest.mark.parametrize("shape", ((37, 53), (36, 53), (37, 52), (1, 40), (1, 41)))
def test_step_two_shapes(fd, shape):
    """odd x odd, even x odd, odd x even, 1 x n: the output is ((rows + 1) // 2, (cols + 1) // 2)."""
    frame = noise((2,) + shape)
    for name in ("pyr", "sigma2", "copy"):
        got = run_device(fd, frame, TAPS[name], 2)
        assert got.shape == (2, (shape[0] + 1) // 2, (shape[1] + 1) // 2)
        same(got, R.blur_ref(frame, TAPS[name], 2), (shape, name))
    same(run_device(fd, frame, TAPS["copy"], 2), frame[:, ::2, ::2], "r = 0, step 2: decimation")


def test_batch_of_three(fd):
    exp = R.blur_ref(FRAMES, TAPS["sigma2"])
    assert not np.array_equal(exp[0], exp[1])
    same(run_device(fd, FRAMES, TAPS["sigma2"]), exp)
    for b in range(3):  # a frame of the batch equals the frame alone
        same(run_device(fd, FRAMES[b], TAPS["sigma2"]), exp[b], b)
    # the halo does not read the neighbouring frame
    pair = np.stack([np.zeros((ROWS, COLS), np.uint8), np.full((ROWS, COLS), 255, np.uint8)])
    for step in (1, 2):
        same(run_device(fd, pair, G5, step), pair[:, ::step, ::step], ("0 | 255", step))


@pytest.mark.parametrize("off", (1, 2, 3))
@pytest.mark.parametrize("step", (1, 2))
def test_store_tails_and_unaligned_bases(fd, off, step):
    """frames and out as slices starting `off` bytes into larger device buffers whose other bytes must stay."""
    torch = pytest.importorskip("torch")
    for cols in (COLS, 52):  # rows of 53 bytes: every row has its own shift; of 52 (26 out at step 2): one shift for all
        frames = np.ascontiguousarray(FRAMES[:2, :, :cols])
        exp = R.blur_ref(frames, TAPS["sigma2"], step)
        n, m = frames.size, exp.size
        src = torch.zeros(n + 8, dtype=torch.uint8, device="cuda")
        src[off:off + n] = torch.from_numpy(frames.reshape(-1)).cuda()
        fr = src[off:off + n].view(frames.shape)
        for out_off in (off, (off + 1) % 4):  # the same alignment as the frames, and another one
            big = torch.full((m + 16,), 0xA5, dtype=torch.uint8, device="cuda")
            out = big[4 + out_off:4 + out_off + m].view(exp.shape)
            assert out.data_ptr() % 4 == out_off and fr.data_ptr() % 4 == off
            got = fd.blur_frames(fr, taps=TAPS["sigma2"], step=step, out=out)
            assert got.data_ptr() == out.data_ptr()
            same(got, exp, (cols, off, out_off))
            rest = torch.cat([big[:4 + out_off], big[4 + out_off + m:]]).cpu().numpy()
            assert (rest == 0xA5).all()


@pytest.mark.parametrize("frames_dev", (0, 1))
@pytest.mark.parametrize("out_dev", (0, 1))
def test_host_and_device_pointers(fd, frames_dev, out_dev):
    """frames and out each on the host or on the device, through the C ABI; then the Python call."""
    torch = pytest.importorskip("torch")
    from feature_detector_amd import _lib
    from feature_detector_amd._lib import fd_blur_opts

    exp = R.blur_ref(FRAMES, TAPS["sigma2"])
    L, ctx = fd.load(), fd.default_context()
    ctx.set_stream(None)
    side = lambda a, dev: torch.from_numpy(a).cuda() if dev else a  # noqa: E731
    p = lambda a: ctypes.c_void_p(a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data)  # noqa: E731
    fr, out = side(FRAMES.copy(), frames_dev), side(np.full(FRAMES.shape, 0xA5, np.uint8), out_dev)
    torch.cuda.synchronize()
    opts = fd_blur_opts()
    assert L.fd_blur_taps(2.0, 0, ctypes.byref(opts)) == 0
    _lib.check(ctx.ptr, L.fd_frames_blur(ctx.ptr, p(fr), frames_dev, 3, ROWS, COLS, ctypes.byref(opts), p(out), out_dev))
    ctx.synchronize()
    same(out, exp)
    got = fd.blur_frames(fr, sigma=2.0)  # outputs on the side of the frames
    assert hasattr(got, "cpu") == bool(frames_dev)
    same(got, exp)
    same(fd.blur_frames(fr, sigma=2.0, radius=3), R.blur_ref(FRAMES, TAPS["r3"]))
    same(fr, FRAMES)  # the frames stayed


def test_preallocated_out_and_refusals(fd):
    torch = pytest.importorskip("torch")
    exp = R.blur_ref(FRAMES, TAPS["pyr"])
    dev = torch.from_numpy(FRAMES).cuda()
    out = torch.full(FRAMES.shape, 0xA5, dtype=torch.uint8, device="cuda")
    assert fd.blur_frames(dev, taps=TAPS["pyr"], out=out) is out
    same(out, exp)
    host_out = np.full(FRAMES.shape, 0xA5, np.uint8)
    assert fd.blur_frames(FRAMES, taps=TAPS["pyr"], out=host_out) is host_out
    same(host_out, exp)
    one = fd.blur_frames(FRAMES[0], taps=TAPS["pyr"], step=2)  # [rows, cols] in, [rows, cols] out
    same(one, R.blur_ref(FRAMES[0], TAPS["pyr"], 2))
    for fr in (dev, FRAMES.copy()):  # there is no in-place call, on either side
        with pytest.raises(fd.FdError) as e:
            fd.blur_frames(fr, taps=TAPS["pyr"], out=fr)
        assert e.value.code == fd._lib.FD_ERR_INVALID
    same(dev, FRAMES)
    with pytest.raises(ValueError):
        fd.blur_frames(FRAMES, taps=TAPS["pyr"], out=out)  # out on the other side
    for kw in (dict(taps=[96, 64, 17]), dict(taps=[100, 64, 16]), dict(taps=[258, -1]), dict(taps=TAPS["pyr"], step=3),
               dict(taps=TAPS["pyr"], step=0)):
        with pytest.raises(fd.FdError) as e:
            fd.blur_frames(dev, **kw)
        assert e.value.code == fd._lib.FD_ERR_INVALID and str(e.value).strip(), kw


def test_error_codes(fd):
    from feature_detector_amd import _lib
    from feature_detector_amd._lib import fd_blur_opts

    L, ctx = fd.load(), fd.default_context()
    ctx.set_stream(None)
    out = np.full(FRAMES.shape, 0xA5, np.uint8)
    p = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    call = lambda fr, o, ot, batch=3, rows=ROWS, cols=COLS, c=ctx.ptr: L.fd_frames_blur(  # noqa: E731
        c, p(fr), 0, batch, rows, cols, None if o is None else ctypes.byref(o), p(ot), 0)

    def options(radius, taps, step=1):
        o = fd_blur_opts()
        o.radius, o.step = radius, step
        for k, t in enumerate(taps):
            o.taps[k] = t
        return o

    ok = options(2, [96, 64, 16])
    assert call(FRAMES, ok, out) == 0
    same(out, R.blur_ref(FRAMES, TAPS["pyr"]))
    assert call(FRAMES, options(1, [128, 64, -5, 1000]), out) == 0  # entries above the radius are ignored
    same(out, R.blur_ref(FRAMES, TAPS["r1"]))
    assert call(FRAMES, ok, out, c=None) == _lib.FD_ERR_INVALID
    bad = [(None, ok, out, {}), (FRAMES, None, out, {}), (FRAMES, ok, None, {}), (FRAMES, ok, out, {"batch": 0}),
           (FRAMES, ok, out, {"rows": 0}), (FRAMES, ok, out, {"cols": 0}), (FRAMES, options(-1, [256]), out, {}),
           (FRAMES, options(16, [256]), out, {}), (FRAMES, options(2, [96, 64, 15]), out, {}),
           (FRAMES, options(1, [258, -1]), out, {}), (FRAMES, options(2, [96, 64, 16], 0), out, {}),
           (FRAMES, options(2, [96, 64, 16], 3), out, {}), (FRAMES, ok, FRAMES, {})]
    before = out.copy()
    for fr, o, ot, kw in bad:
        with pytest.raises(fd.FdError) as e:
            _lib.check(ctx.ptr, call(fr, o, ot, **kw))
        assert e.value.code == _lib.FD_ERR_INVALID and str(e.value).strip(), kw
    assert np.array_equal(out, before)


def test_graph_capture(fd):
    torch = pytest.importorskip("torch")
    dfr = torch.from_numpy(FRAMES).cuda()
    out = torch.empty(FRAMES.shape, dtype=torch.uint8, device="cuda")
    fd.blur_frames(dfr, taps=TAPS["sigma2"], out=out)  # the warm call of the shape
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        fd.blur_frames(dfr, taps=TAPS["sigma2"], out=out)
    host = np.ascontiguousarray(FRAMES[::-1])  # new contents in the captured input
    dfr.copy_(torch.from_numpy(host))
    out.fill_(0xA5)
    g.replay()
    torch.cuda.synchronize()
    same(out, R.blur_ref(host, TAPS["sigma2"]))
    del g


# ---- pyramid ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows,cols,levels", ((37, 53, 3), (64, 96, 6), (33, 17, 4)))
def test_gaussian_pyramid(fd, rows, cols, levels):
    torch = pytest.importorskip("torch")
    frames = noise((2, rows, cols))
    exp = R.pyr_gauss_ref(frames, levels)
    off = flow_ref.pyr_layout(2, rows, cols, levels)
    host = fd.build_pyramid(frames, levels, kernel="gauss")
    assert host.offsets == off and isinstance(host.data, np.ndarray)
    assert np.array_equal(host.data, flow_ref.pyr_pack(exp))  # (the padding stays as it was: zeros)
    dev = fd.build_pyramid(torch.from_numpy(frames).cuda(), levels, kernel="gauss")
    mixed = fd.build_pyramid(frames, levels, device_out=True, kernel="gauss")
    torch.cuda.synchronize()
    for l in range(levels):
        assert exp[l].shape == (2, rows >> l, cols >> l)
        same(host.level(l), exp[l], ("host", l))
        same(dev.level(l), exp[l], ("device", l))
        same(mixed.level(l), exp[l], ("mixed", l))
    # a preallocated device pyramid through the C ABI: the padding bytes between the levels stay
    ctx = fd.default_context()
    ctx.set_stream(None)
    pyr = torch.full((off[-1],), 0xA5, dtype=torch.uint8, device="cuda")
    dfr = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    fd._lib.check(ctx.ptr, fd.load().fd_pyr_build_gauss(ctx.ptr, ctypes.c_void_p(dfr.data_ptr()), 1, 2, rows, cols, levels,
                                                       ctypes.c_void_p(pyr.data_ptr()), 1))
    ctx.synchronize()
    want = flow_ref.pyr_pack(exp)
    pad = np.ones(off[-1], bool)
    for l in range(levels):
        pad[off[l]:off[l] + exp[l].size] = False
    want[pad] = 0xA5
    assert pad.any() and np.array_equal(pyr.cpu().numpy(), want)


def test_box_pyramid_is_unchanged(fd):
    frames = noise((2, 37, 53))
    exp = flow_ref.pyr_ref(frames, 3)
    for kw in ({}, {"kernel": "box"}):
        got = fd.build_pyramid(frames, 3, **kw)
        for l in range(3):
            same(got.level(l), exp[l], (kw, l))
    assert not np.array_equal(exp[1], R.pyr_gauss_ref(frames, 3)[1])


# ---- chains ----------------------------------------------------------------------------------------------

def test_chain_track_on_gaussian_pyramids(fd):
    """track_lk handed Gaussian Pyramids of a shifted blurred-noise pair equals flow_ref.track_one run on
    pyr_gauss_ref's levels, bit for bit."""
    rows, cols, levels = 72, 100, 3
    canvas = R.blur_ref(noise((rows + 8, cols + 8), seed=9), TAPS["sigma2"])
    prev = np.ascontiguousarray(canvas[4:4 + rows, 4:4 + cols])[None]
    nxt = np.ascontiguousarray(canvas[3:3 + rows, 6:6 + cols])[None]  # the content moves by (-2, +1)
    rng = np.random.default_rng(4)
    xy = np.stack([rng.uniform(14, cols - 15, 24), rng.uniform(14, rows - 15, 24)], -1).astype(np.float32)[None]
    xy[:, :8] = np.rint(xy[:, :8])
    kw = dict(half_window=5, max_iters=20, epsilon=0.01, min_eigen=1e-4)
    pp, pn = (fd.build_pyramid(f, levels, device_out=True, kernel="gauss") for f in (prev, nxt))
    res = fd.track_lk(pp, pn, xy, levels=levels, **kw)
    pl = [a[0].astype(np.int64) for a in R.pyr_gauss_ref(prev, levels)]
    nl = [a[0].astype(np.int64) for a in R.pyr_gauss_ref(nxt, levels)]
    tracked = 0
    for i in range(xy.shape[1]):
        out, st, err = flow_ref.track_one(pl, nl, xy[0, i], None, rows=rows, cols=cols, r=kw["half_window"],
                                          max_iters=kw["max_iters"], epsilon=kw["epsilon"], min_eigen=kw["min_eigen"],
                                          max_error=-1.0)
        assert int(res.status[0, i]) == st, i
        assert np.array_equal(np.asarray(res.xy[0, i]).view(np.uint32), np.asarray(out, np.float32).view(np.uint32)), i
        assert np.float32(res.err[0, i]).view(np.uint32) == np.float32(err).view(np.uint32), i
        tracked += st == 1
    assert tracked >= 10 and int(res.counts[0]) == tracked


def test_chain_blur_then_brief(fd, oracle, image_png):
    """blur_frames -> brief_compute on the device equals the oracle's BRIEF on blur_ref's frame, bit for bit."""
    torch = pytest.importorskip("torch")
    crop = np.ascontiguousarray(image_png[240:480, 48:368])
    kps, _ = oracle.detect(1, crop, 10, 0.1, 300, sort_mode=0)
    assert len(kps) >= 100
    r, taps = fd.gaussian_taps(2.0)
    exp_frame = R.blur_ref(crop, taps)
    smooth = fd.blur_frames(torch.from_numpy(crop).cuda(), sigma=2.0)
    xy = torch.from_numpy(kps[None]).cuda()
    counts = torch.tensor([len(kps)], dtype=torch.int32, device="cuda")
    bits = fd.brief_compute(smooth[None], xy, counts, length=256, half_patch_size=8)
    torch.cuda.synchronize()
    same(smooth, exp_frame)
    eb, _, _ = oracle.brief(exp_frame, kps, 256, 8, 0)
    assert np.array_equal(bits[0, :len(kps)].cpu().numpy().view(np.uint32), eb)
    raw, _, _ = oracle.brief(crop, kps, 256, 8, 0)
    assert not np.array_equal(raw, eb)
