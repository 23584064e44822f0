"""fd_flow_lk / fd_pyr_build at their arithmetic and shape edges, every output exactly against tests/flow_ref.py:
each k_flow_lk<ROUNDS> instance, window sums past 2^31 and 2^32, odd frame sizes with features beyond a
coarse level's last column, counts beyond the stride, and pyramids whose levels switch between k_pyr_down's
wide and narrow instances. tests/test_flow_host.py checks without a GPU that the inputs of flow_cases.py
have the properties these tests rely on."""
import numpy as np
import pytest

import flow_cases as C
import flow_ref as R
from test_gpu_flow import SENT_CNT, SENT_ERR, SENT_ST, SENT_XY, canvas, fd, features, half_shift, same, view  # noqa: F401

pytestmark = pytest.mark.gpu


# ---- tracker ---------------------------------------------------------------------------------------------

HALF_WINDOWS = list(range(1, 11))


def test_half_windows_cover_every_instance():
    assert sorted({C.rounds(r) for r in HALF_WINDOWS}) == [1, 2, 3, 4, 5, 6, 7]
    assert (C.rounds(8), C.rounds(9)) == (5, 6)


@pytest.mark.parametrize("r", HALF_WINDOWS)
@pytest.mark.parametrize("motion", ["integer", "half"])
def test_every_window_size(fd, canvas, features, r, motion):
    """half_window 1..10: every k_flow_lk<ROUNDS> instance, 5 (r = 8, n = 289) and 6 (r = 9, n = 361) among
    them, and every length of the last round's tail (n mod 64 = 9, 25, 49, 17, 57, 41, 33, 33, 41, 57)."""
    prev = view(canvas)[:1]
    nxt = (view(canvas, 2, -1) if motion == "integer" else half_shift(canvas, 1, -1))[:1]
    xy = features[:1, 6:22]  # six integral, ten fractional
    kw = dict(levels=2, half_window=r, max_iters=20, epsilon=0.01, min_eigen=1e-4)
    exp = R.flow_ref(prev, nxt, xy, **kw)
    same(fd.track_lk(prev, nxt, xy, **kw), exp)
    assert (exp[1] == 1).sum() >= 8


@pytest.mark.parametrize("r", [8, 9, 10])
@pytest.mark.parametrize("levels", [1, 2])
@pytest.mark.parametrize("fb", [-1.0, 0.5])
def test_saturated_contrast(fd, r, levels, fb):
    """0 / 255 blocks moved by (-1, -1): sum gx*gx passes 2^31 (2^32 at r = 10) and b1, b2 fall below -2^31
    (test_flow_host.py::test_saturated_frames_pass_the_32_bit_sums), so wave_sum_i32's split into 16-bit
    halves, the arithmetic shift of negative lanes and the 64-bit recombination decide the result."""
    prev, nxt = C.sat_frames()
    xy = C.sat_features()
    kw = dict(levels=levels, half_window=r, max_iters=20, min_eigen=1e-4, fb_max_dist=fb)
    exp = R.flow_ref(prev, nxt, xy, **kw)
    good = (exp[1][0] == 1) & (np.abs(exp[0][0] - xy[0] - np.array(C.SAT_SHIFT, np.float32)).max(-1) < 0.1)
    print("tracked to within 0.1 px:", good.sum())
    assert (exp[1] == 1).sum() >= 20 and good.sum() >= 20
    same(fd.track_lk(prev, nxt, xy, **kw), exp)


@pytest.mark.parametrize("r", [8, 9, 10])
def test_saturated_inverse(fd, r):
    """next = 255 - prev: nothing to find, every residual is full scale and the steps are large."""
    prev, _ = C.sat_frames()
    xy = C.sat_features()
    kw = dict(levels=2, half_window=r, max_iters=20, min_eigen=1e-4)
    exp = R.flow_ref(prev, 255 - prev, xy, **kw)
    same(fd.track_lk(prev, 255 - prev, xy, **kw), exp)


@pytest.fixture(scope="module")
def odd_pair(oracle):
    return C.blob_pair(oracle, (21, 22, 23), C.ODD_ROWS, C.ODD_COLS, (-1, -1))  # towards the far corner's inside


@pytest.mark.parametrize("levels", [3, 4])
@pytest.mark.parametrize("r", [7, 10])
def test_odd_sizes_and_the_far_edge(fd, odd_pair, levels, r):
    """97 x 131 x 3 frames down to a 12 x 16 top level: features on the last row / column of level 0 lie
    beyond the last one of the coarser levels (test_flow_host.py::test_odd_frame_features_pass_the_coarse_
    levels_last_column), and frames 1 and 2 start at odd bytes of level 0."""
    prev, nxt = odd_pair
    xy = C.odd_features()
    assert C.beyond_last_column(xy[0], C.ODD_COLS, levels)
    kw = dict(levels=levels, half_window=r, max_iters=10, min_eigen=1e-4)
    exp = R.flow_ref(prev, nxt, xy, **kw)
    same(fd.track_lk(prev, nxt, xy, **kw), exp)
    assert ((exp[1] == 1).sum(1) >= 8).all()


@pytest.mark.parametrize("extra", ["valid", "fb"])
def test_counts_beyond_the_stride(fd, oracle, extra):
    """counts[f] > stride is read as stride by k_flow_lk, k_flow_finish and the host path's copy back: no
    slot beyond the frame's own is read or written, out_counts stays <= stride."""
    torch = pytest.importorskip("torch")
    stride = 12
    prev, nxt = C.blob_pair(oracle, (31, 32, 33), C.ROWS, C.COLS, (1, 0))
    rng = np.random.default_rng(9)
    xy = np.stack([rng.uniform(14, C.COLS - 15, (3, stride)), rng.uniform(14, C.ROWS - 15, (3, stride))], -1).astype(np.float32)
    xy[:, :4] = np.rint(xy[:, :4])
    counts = np.array([stride + 5, stride, (stride + 1000) | (1 << 25) | (1 << 31)], np.int64).astype(np.int32)
    kw = dict(levels=2, half_window=5, max_iters=10, min_eigen=1e-4)
    if extra == "valid":
        kw["valid"] = (rng.random((3, stride)) < 0.7).astype(np.uint8)
    else:
        kw["fb_max_dist"] = 0.5
    init = (np.full((3, stride, 2), SENT_XY, np.float32), np.full((3, stride), SENT_ST, np.uint8),
            np.full((3, stride), SENT_ERR, np.float32))
    exp = R.flow_ref(prev, nxt, xy, counts=counts, init=init, **kw)
    assert (exp[1] != SENT_ST).all() and (exp[3] <= stride).all() and (exp[3] >= 4).all()
    # device tensors; the outputs are the middle of a longer sentinel-filled allocation each
    pad = 64
    bufs = [torch.full((pad + n + pad,), v, dtype=dt, device="cuda")
            for n, v, dt in ((3 * stride * 2, SENT_XY, torch.float32), (3 * stride, SENT_ST, torch.uint8),
                             (3 * stride, SENT_ERR, torch.float32), (3, SENT_CNT, torch.int32))]
    out = (bufs[0][pad:-pad].view(3, stride, 2), bufs[1][pad:-pad].view(3, stride), bufs[2][pad:-pad].view(3, stride),
           bufs[3][pad:-pad])
    dkw = {k: torch.from_numpy(v).cuda() if isinstance(v, np.ndarray) else v for k, v in kw.items()}
    res = fd.track_lk(torch.from_numpy(prev).cuda(), torch.from_numpy(nxt).cuda(), torch.from_numpy(xy).cuda(),
                      counts=torch.from_numpy(counts).cuda(), out=out, **dkw)
    torch.cuda.synchronize()
    same(res, exp)
    for b, v in zip(bufs, (SENT_XY, SENT_ST, SENT_ERR, SENT_CNT)):
        assert (b[:pad] == v).all() and (b[-pad:] == v).all()
    # host pointers (fresh outputs are zeros)
    same(fd.track_lk(prev, nxt, xy, counts=counts, **kw), R.flow_ref(prev, nxt, xy, counts=counts, **kw))


# ---- pyramid ---------------------------------------------------------------------------------------------

PYR_SHAPES = [(37, 40, 3),   # 40 wide with odd rows, then 20 and 10 narrow
              (18, 24, 3),   # 24 wide, 12 and 6 narrow
              (9, 8, 2),     # cols == 8: one thread per row pair, odd rows
              (33, 72, 4),   # 72 wide with odd rows, 36 and 18 narrow
              (6, 64, 2)]    # 64 wide, 3 output rows


def pyr_frames(content, batch, rows, cols):
    if content == "random":
        return np.random.default_rng(rows * cols + batch).integers(0, 256, (batch, rows, cols), dtype=np.uint8)
    if content == "white":
        return np.full((batch, rows, cols), 255, np.uint8)
    yy, xx = np.mgrid[0:rows, 0:cols]
    if content == "checker":  # 1 px cells: every box holds two of each
        return np.tile((((yy + xx) & 1) * 255).astype(np.uint8), (batch, 1, 1))
    # "mod4": multiples of 4 everywhere, plus the box's index mod 4 on the box's first pixel
    f = np.random.default_rng(rows + cols).integers(0, 64, (batch, rows, cols), dtype=np.uint8) * 4
    first = ((yy & 1) == 0) & ((xx & 1) == 0)
    return f + (first * (((yy >> 1) + (xx >> 1)) & 3)).astype(np.uint8)


def test_pyr_shapes_mix_wide_and_narrow():
    kinds = {s: ["wide" if ((s[1] >> l) & 7) == 0 else "narrow" for l in range(s[2] - 1)] for s in PYR_SHAPES}
    assert kinds[(37, 40, 3)] == ["wide", "narrow"] and kinds[(18, 24, 3)] == ["wide", "narrow"]
    assert kinds[(33, 72, 4)] == ["wide", "narrow", "narrow"] and kinds[(9, 8, 2)] == ["wide"] and kinds[(6, 64, 2)] == ["wide"]
    assert all((s[0] * s[1]) % 256 for s in PYR_SHAPES)  # batch 3: frames 1 and 2 start off the 256-byte grid


@pytest.mark.parametrize("rows,cols,levels", PYR_SHAPES)
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("content", ["random", "white", "checker", "mod4"])
def test_pyramid_wide_and_narrow(fd, rows, cols, levels, batch, content):
    torch = pytest.importorskip("torch")
    frames = pyr_frames(content, batch, rows, cols)
    exp = R.pyr_ref(frames, levels)
    if content == "white":
        assert all((e == 255).all() for e in exp)
    if content == "checker":
        assert (exp[1] == 128).all()  # (510 + 2) >> 2
    if content == "mod4":
        a = frames.astype(np.int64)[:, :rows // 2 * 2, :cols // 2 * 2]
        sums = a[:, 0::2, 0::2] + a[:, 0::2, 1::2] + a[:, 1::2, 0::2] + a[:, 1::2, 1::2]
        assert set(np.unique(sums % 4)) == {0, 1, 2, 3}
    off = R.pyr_layout(batch, rows, cols, levels)
    host = fd.build_pyramid(frames, levels)
    assert host.offsets == off and np.array_equal(host.data, R.pyr_pack(exp))
    dev = fd.build_pyramid(torch.from_numpy(frames).cuda(), levels)
    mixed = fd.build_pyramid(frames, levels, device_out=True)
    torch.cuda.synchronize()
    for l in range(levels):
        assert np.array_equal(host.level(l), exp[l])
        assert np.array_equal(dev.level(l).cpu().numpy(), exp[l])
        assert np.array_equal(mixed.level(l).cpu().numpy(), exp[l])


def test_pyramid_from_an_unaligned_device_pointer(fd):
    """Device frames that start one byte into their allocation: only the copy into level 0 reads them."""
    torch = pytest.importorskip("torch")
    frames = pyr_frames("random", 3, 37, 40)
    store = torch.zeros((1 + frames.size,), dtype=torch.uint8, device="cuda")
    src = store[1:].view(3, 37, 40)
    src.copy_(torch.from_numpy(frames))
    assert src.is_contiguous() and src.data_ptr() % 2 == 1
    dev = fd.build_pyramid(src, 3)
    torch.cuda.synchronize()
    for l, e in enumerate(R.pyr_ref(frames, 3)):
        assert np.array_equal(dev.level(l).cpu().numpy(), e)
