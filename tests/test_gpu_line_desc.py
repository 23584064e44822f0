"""fd_lines_describe on the GPU against tests/line_desc_ref.py: every bit of desc, xy and valid, no tolerance.
Geometry, borders, degenerate lines, the length clamp with sums past 2^32, the option limits, batches and
strides, the calling conventions, and the lsd_lines -> describe_lines -> nn_match chain."""
import ctypes

import numpy as np
import pytest

import line_desc_cases as C
import line_desc_ref as R
import match_guided_ref as GR
import nn_match_ref as NR

pytestmark = pytest.mark.gpu

ROWS, COLS = 48, 64
FRAME = C.noise_frame(ROWS, COLS, 11)
SENTINEL = 0xA5
SENTINEL_F = float(np.array([0xA5A5A5A5], np.uint32).view(np.float32)[0])


@pytest.fixture(scope="module")
def fd():
    import feature_detector_amd as fd

    fd.load()
    return fd


def np_(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def same(got, exp, what=""):
    """got: LineDescResult or (desc, xy, valid); exp: line_desc_ref.describe's tuple."""
    got = (got.desc, got.xy, got.valid) if hasattr(got, "desc") else got
    for name, g, e in zip(("desc", "xy", "valid"), got, exp):
        g = np_(g)
        assert g.shape == e.shape and g.dtype == e.dtype, (what, name, g.shape, e.shape, g.dtype)
        gb, eb = (g.view(np.uint32), e.view(np.uint32)) if g.dtype == np.float32 else (g, e)
        bad = np.argwhere(gb != eb)
        assert len(bad) == 0, (what, name, len(bad), bad[:5].tolist(), g[tuple(bad[0])], e[tuple(bad[0])])


def check(fd, frames, lines, counts=None, bands=9, w=7, what=""):
    """The device path on `lines` [B, S, 4 or 12] against the restatement; returns the restatement's info."""
    import torch

    frames = np.ascontiguousarray(frames if frames.ndim == 3 else frames[None])
    lines = np.ascontiguousarray(lines if lines.ndim == 3 else lines[None], np.float32)
    exp = R.describe(frames, lines, counts, bands, w)
    got = fd.describe_lines(torch.from_numpy(frames).cuda(), torch.from_numpy(lines).cuda(),
                            None if counts is None else torch.from_numpy(np.asarray(counts, np.int32)).cuda(), bands, w)
    same(got, exp[:3], what)
    return exp[3]


def test_geometry(fd):
    info = check(fd, FRAME, C.geometry_lines())[0]
    assert {d["flip"] for d in info} == {False, True} and all(d["valid"] and d["S"] != 0 for d in info)
    assert {1, 5} <= {d["N"] for d in info}  # N == 1 among them
    half = len(info) // 2  # the second half is the first with the endpoints swapped: the same bits from the GPU too
    assert all(np.array_equal(a["desc"], b["desc"]) for a, b in zip(info[:half], info[half:]))


def test_borders(fd):
    info = check(fd, FRAME, C.border_lines())[0]
    assert [d["valid"] for d in info] == [1, 1, 1, 1, 1, 0, 0]
    assert all(d["N"] > 0 and d["S"] == 0 and not d["desc"].any() for d in info[5:])  # wholly outside: sums of zero


def test_degenerate_lines(fd):
    lines = np.array([(20, 20, 20.5, 20.25), (20, 20, 20, 20), (np.nan, 5, 30, 30), (5, 5, 30, np.inf), (-np.inf, 5, 30, 30),
                      (10, 24, 50, 24)], np.float32)
    info = check(fd, FRAME, lines)[0]
    assert [d["valid"] for d in info] == [0, 0, 0, 0, 0, 1]
    flat = np.full((ROWS, COLS), 93, np.uint8)
    info = check(fd, flat, C.geometry_lines(), what="flat")[0]
    assert not any(d["valid"] for d in info) and all(d["N"] >= 1 for d in info)


def test_length_clamp_and_sums_past_32_bits(fd):
    """An 8 x 4200 frame of saturated 2 x 2 checker cells under a horizontal line of length 4160: N clamps at
    4096, |gx| = 255 at every sample, and a row's sums of gl pass 2^32."""
    y, x = np.mgrid[0:8, 0:4200]
    frame = ((((x >> 1) + (y >> 1)) & 1) * 255).astype(np.uint8)
    lines = np.array([(20, 4, 4180, 4), (4180.5, 3.5, 20.5, 3.5), (30, 3, 4100, 5)], np.float32)
    info = check(fd, frame, lines, bands=2, w=2)[0]
    assert [d["N"] for d in info] == [4096, 4096, 4070] and info[0]["vmax"] > 2 ** 32 and all(d["valid"] for d in info)
    info = check(fd, frame, lines, what="default options: most rows outside")[0]
    assert info[0]["N"] == 4096 and info[0]["valid"]
    noisy = C.noise_frame(8, 4200, 5)
    assert check(fd, noisy, lines, bands=3, w=2)[0][0]["N"] == 4096


@pytest.mark.parametrize("bands,w", ((1, 7), (2, 7), (32, 1), (32, 16), (9, 1), (3, 16), (1, 1), (1, 16)))
def test_options(fd, bands, w):
    lines = np.concatenate([C.geometry_lines()[:10], C.border_lines()[:5]])
    info = check(fd, FRAME, lines, bands=bands, w=w)[0]
    assert any(d["valid"] for d in info) and {d["flip"] for d in info if d["valid"]} == {False, True}


def test_batch_counts_and_untouched_slots(fd):
    import torch

    frames = np.stack([FRAME, C.noise_frame(ROWS, COLS, 12), C.noise_frame(ROWS, COLS, 13)])
    lines = np.stack([C.geometry_lines()[:8], C.geometry_lines()[8:16], C.geometry_lines()[16:24]])
    stride = lines.shape[1]
    # bits 25..31 of a count are ignored; a count above the stride is clamped to it
    counts = np.array([0, 1 | (1 << 25), stride | 0xFE000000], np.uint32).view(np.int32)
    exp = R.describe(frames, lines, counts, fill=SENTINEL_F, valid_fill=SENTINEL)
    assert [len(i) for i in exp[3]] == [0, 1, stride]
    out = (torch.full((3, stride, 72), SENTINEL_F, device="cuda"), torch.full((3, stride, 2), SENTINEL_F, device="cuda"),
           torch.full((3, stride), SENTINEL, dtype=torch.uint8, device="cuda"))
    got = fd.describe_lines(torch.from_numpy(frames).cuda(), torch.from_numpy(lines).cuda(), torch.from_numpy(counts).cuda(), out=out)
    assert got.desc is out[0] and got.valid is out[2]
    same(got, exp[:3], "device, sentinels")
    assert np.array_equal(np_(got.counts), counts)
    clamped = counts.copy()
    clamped[2] = stride + 5
    same(fd.describe_lines(torch.from_numpy(frames).cuda(), torch.from_numpy(lines).cuda(), torch.from_numpy(clamped).cuda(), out=out),
         exp[:3], "count above the stride")
    # the host path leaves the slots past a count as they were, too (the Python call hands in zeroed arrays)
    same(fd.describe_lines(frames, lines, counts), R.describe(frames, lines, counts)[:3], "host")
    # no cross-talk: a frame of the batch equals the frame alone
    alone = fd.describe_lines(frames[2], lines[2])
    assert np.array_equal(alone.desc[0].view(np.uint32), exp[0][2].view(np.uint32)) and alone.counts.tolist() == [stride]


def test_line_floats_12_against_4_and_lists(fd):
    import torch

    four = C.geometry_lines()
    rect = np.full((len(four), 12), 7.25, np.float32)
    rect[:, :4] = four
    exp = R.describe(FRAME[None], four[None])
    same(fd.describe_lines(torch.from_numpy(FRAME).cuda(), torch.from_numpy(rect).cuda()), exp[:3], "12 floats")
    same(fd.describe_lines(FRAME, rect), exp[:3], "12 floats, host")
    # lsd_lines' form: a list over frames of [n, 12] arrays, padded to the longest
    frames = np.stack([FRAME, FRAME])
    got = fd.describe_lines(frames, [rect[:5], rect])
    assert got.counts.tolist() == [5, len(rect)] and got.desc.shape == (2, len(rect), 72)
    exp2 = R.describe(frames, np.stack([rect, rect]), [5, len(rect)])
    same(got, exp2[:3], "list")


def test_stride_zero(fd):
    import torch

    from feature_detector_amd import _lib
    from feature_detector_amd._lib import fd_line_desc_opts

    got = fd.describe_lines(FRAME, np.zeros((1, 0, 4), np.float32))
    assert got.desc.shape == (1, 0, 72) and got.xy.shape == (1, 0, 2) and got.counts.tolist() == [0]
    got = fd.describe_lines(torch.from_numpy(FRAME).cuda(), torch.zeros((0, 12), device="cuda"))
    assert tuple(got.desc.shape) == (1, 0, 72)
    assert fd.describe_lines(np.stack([FRAME, FRAME]), [np.zeros((0, 12), np.float32)] * 2).valid.shape == (2, 0)
    L, ctx = fd.load(), fd.default_context()
    one = np.zeros(4, np.float32)  # (non-null pointers, nothing behind them is touched)
    opts = fd_line_desc_opts(9, 7)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    assert L.fd_lines_describe(ctx.ptr, p(FRAME), 0, 1, ROWS, COLS, ctypes.byref(opts), p(one), 4, None, 0, p(one), None, None, 0) == _lib.FD_OK


@pytest.mark.parametrize("frames_dev", (0, 1))
@pytest.mark.parametrize("io_dev", (0, 1))
def test_host_and_device_pointers(fd, frames_dev, io_dev):
    """frames, and lines / counts / outputs, each on the host or on the device, through the C ABI."""
    import torch

    from feature_detector_amd import _lib
    from feature_detector_amd._lib import fd_line_desc_opts

    lines = np.concatenate([C.geometry_lines()[:9], C.border_lines()])[None]
    s = lines.shape[1]
    counts = np.array([s - 2], np.int32)
    exp = R.describe(FRAME[None], lines, counts, 4, 5, fill=SENTINEL_F, valid_fill=SENTINEL)
    L, ctx = fd.load(), fd.default_context()
    ctx.set_stream(None)
    side = lambda a, dev: torch.from_numpy(a).cuda() if dev else a  # noqa: E731
    p = lambda a: None if a is None else ctypes.c_void_p(a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data)  # noqa: E731
    fr, ln, cn = side(FRAME.copy(), frames_dev), side(lines.copy(), io_dev), side(counts.copy(), io_dev)
    desc, xy = side(np.full((1, s, 32), SENTINEL_F, np.float32), io_dev), side(np.full((1, s, 2), SENTINEL_F, np.float32), io_dev)
    valid = side(np.full((1, s), SENTINEL, np.uint8), io_dev)
    torch.cuda.synchronize()
    opts = fd_line_desc_opts(4, 5)
    call = lambda x, v: L.fd_lines_describe(ctx.ptr, p(fr), frames_dev, 1, ROWS, COLS, ctypes.byref(opts), p(ln), 4, p(cn), s,  # noqa: E731
                                            p(desc), p(x), p(v), io_dev)
    _lib.check(ctx.ptr, call(xy, valid))
    ctx.synchronize()
    same((desc, xy, valid), exp[:3])
    before = np_(xy).copy(), np_(valid).copy()
    _lib.check(ctx.ptr, call(None, None))  # out_xy and out_valid skipped
    ctx.synchronize()
    same((desc, before[0], before[1]), exp[:3], "skipped outputs")
    assert np.array_equal(np_(fr), FRAME) and np.array_equal(np_(ln), lines)
    if frames_dev != io_dev:  # the Python call: outputs on the side of the lines
        got = fd.describe_lines(fr, ln, cn, 4, 5)
        assert hasattr(got.desc, "cpu") == bool(io_dev)
        same(got, R.describe(FRAME[None], lines, counts, 4, 5)[:3], "python, mixed sides")


def test_graph_capture(fd):
    import torch

    lines = np.concatenate([C.geometry_lines(), C.border_lines()])[None]
    s = lines.shape[1]
    dfr, dln = torch.from_numpy(FRAME.copy()).cuda(), torch.from_numpy(lines.copy()).cuda()
    dcn = torch.tensor([s], dtype=torch.int32, device="cuda")
    out = (torch.empty((1, s, 72), device="cuda"), torch.empty((1, s, 2), device="cuda"), torch.empty((1, s), dtype=torch.uint8, device="cuda"))
    fd.describe_lines(dfr, dln, dcn, out=out)  # the warm call
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        fd.describe_lines(dfr, dln, dcn, out=out)
    for step in (1, 2):  # new contents in the captured inputs
        frame = C.noise_frame(ROWS, COLS, 20 + step)
        ln = np.ascontiguousarray(lines[:, ::-1]) if step == 1 else lines + np.float32(0.25)
        cnt = s - 3 * step
        dfr.copy_(torch.from_numpy(frame))
        dln.copy_(torch.from_numpy(ln))
        dcn.fill_(cnt)
        for o in out:
            o.fill_(SENTINEL_F if o.dtype == torch.float32 else SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        same(out, R.describe(frame[None], ln, [cnt], fill=SENTINEL_F, valid_fill=SENTINEL)[:3], step)
    del g


def test_error_codes(fd):
    from feature_detector_amd import _lib
    from feature_detector_amd._lib import fd_line_desc_opts

    L, ctx = fd.load(), fd.default_context()
    ctx.set_stream(None)
    lines = C.geometry_lines()[:4].copy()
    desc = np.full((4, 72), SENTINEL_F, np.float32)
    p = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    ok = fd_line_desc_opts(9, 7)

    def call(fr=FRAME, o=ok, ln=lines, ds=desc, c=ctx.ptr, batch=1, rows=ROWS, cols=COLS, floats=4, stride=4):
        return L.fd_lines_describe(c, p(fr), 0, batch, rows, cols, None if o is None else ctypes.byref(o), p(ln), floats, None,
                                   stride, p(ds), None, None, 0)

    assert call() == 0
    assert call(c=None) == _lib.FD_ERR_INVALID
    before = desc.copy()
    bad = [dict(fr=None), dict(o=None), dict(ln=None), dict(ds=None), dict(o=fd_line_desc_opts(0, 7)), dict(o=fd_line_desc_opts(33, 7)),
           dict(o=fd_line_desc_opts(9, 0)), dict(o=fd_line_desc_opts(9, 17)), dict(o=fd_line_desc_opts(-1, -1)), dict(floats=5),
           dict(floats=0), dict(floats=8), dict(batch=0), dict(batch=-1), dict(stride=-1), dict(rows=2), dict(cols=2), dict(rows=0)]
    for kw in bad:
        with pytest.raises(fd.FdError) as e:
            _lib.check(ctx.ptr, call(**kw))
        assert e.value.code == _lib.FD_ERR_INVALID and str(e.value).strip(), kw
    assert np.array_equal(desc.view(np.uint32), before.view(np.uint32))
    for kw in (dict(bands=0), dict(bands=33), dict(band_width=17)):  # the Python call refuses them before the library
        with pytest.raises(ValueError):
            fd.describe_lines(FRAME, lines, **kw)
    with pytest.raises(ValueError):
        fd.describe_lines(FRAME, np.zeros((3, 5), np.float32))
    assert call(rows=3, cols=3, fr=np.zeros((3, 3), np.uint8)) == 0  # the smallest frame: one pixel has neighbours


def test_chain_detect_describe_match(fd, image_png):
    """lsd_lines on two crops offset by CHAIN_SHIFT, describe_lines on lsd_lines' lists as they are, then
    nn_match with cross-check and a ratio test, unguided and guided by the midpoints."""
    a, b = C.chain_crops(image_png)
    la, lb = fd.lsd_lines(np.stack([a, b]), min_length=C.CHAIN_MIN_LENGTH)
    da, db = fd.describe_lines(a, [la]), fd.describe_lines(b, [lb])
    ra, rb = R.describe(a[None], la[None]), R.describe(b[None], lb[None])
    same(da, ra[:3], "first crop")
    same(db, rb[:3], "second crop")
    assert da.valid.all() and db.valid.all() and da.counts.tolist() == [len(la)]
    m = fd.nn_match(da.desc, db.desc, da.counts, db.counts, da.valid, db.valid, max_ratio=C.CHAIN_RATIO, cross_check=True)
    idx, _, cnt = NR.nn_match_ref(ra[0], rb[0], q_valid=ra[2], t_valid=rb[2], max_ratio=C.CHAIN_RATIO, cross_check=True)
    assert np.array_equal(m.idx, idx) and np.array_equal(m.counts, cnt)
    n_acc, n_good, ok = C.chain_sane(m.idx[0], da.xy[0], db.xy[0])
    assert ok, (n_acc, n_good)
    moved = da.xy - np.array(C.CHAIN_SHIFT, np.float32)  # the midpoints predicted in the second crop
    g = fd.nn_match(da.desc, db.desc, da.counts, db.counts, da.valid, db.valid, max_ratio=C.CHAIN_RATIO, cross_check=True,
                    q_xy=moved, t_xy=db.xy, radius=C.CHAIN_RADIUS)
    idx, _, cnt = GR.nn_match_guided_ref(ra[0], rb[0], ra[1] - np.array(C.CHAIN_SHIFT, np.float32), rb[1], C.CHAIN_RADIUS,
                                         q_valid=ra[2], t_valid=rb[2], max_ratio=C.CHAIN_RATIO, cross_check=True)
    assert np.array_equal(g.idx, idx) and np.array_equal(g.counts, cnt)
    n_acc, n_good, ok = C.chain_sane(g.idx[0], da.xy[0], db.xy[0])
    assert ok, (n_acc, n_good)
