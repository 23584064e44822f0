"""GPU: fd_lsd_lines (GPU compact level-line lists + host region growing on worker threads) against
the line oracle (oracle/fd_oracle_lines.cpp). The float sequence is the reference's on both sides, so
the segments are compared bit for bit (all 12 rectangle fields), not just within SURVEY §8c's 0.5 px."""
import ctypes

import numpy as np
import pytest

from lsd_geometry import lsd_chunks, lsd_columns

pytestmark = pytest.mark.gpu


def _check(fd, oracle, frames, threads=0, **kw):
    """fd.lsd_lines against oracle.lsd_lines frame by frame; kw: detection options given to both."""
    frames = np.ascontiguousarray(frames)
    got = fd.lsd_lines(frames, threads=threads, **kw)
    for b in range(frames.shape[0]):
        exp = oracle.lsd_lines(frames[b], **kw)
        assert got[b].shape == exp.shape, (b, got[b].shape, exp.shape)
        assert np.array_equal(got[b].view(np.uint32), exp.view(np.uint32)), b
    return got


def test_image_png(image_png, oracle):
    import feature_detector_amd as fd

    got = _check(fd, oracle, image_png[None])
    assert len(got[0]) == 40


@pytest.mark.parametrize("rows,cols,expect", [(480, 640, 112), (1080, 1920, 792)])
def test_checker64(oracle, rows, cols, expect):
    import feature_detector_amd as fd

    img = oracle.make_frame("checker", 1234, rows, cols, 64)
    assert len(_check(fd, oracle, img[None])[0]) == expect


def test_batch_threads_and_patterns(oracle):
    import feature_detector_amd as fd

    frames = np.stack([oracle.make_frame(p, s, 240, 320, per) for p, s, per in
                       (("checker", 1, 16), ("noise", 2, 16), ("checker", 3, 40), ("checker", 4, 64),
                        ("noise", 5, 16), ("checker", 6, 24))])
    one = _check(fd, oracle, frames, threads=1)
    many = fd.lsd_lines(frames, threads=4)
    assert all(np.array_equal(a, b) for a, b in zip(one, many))


def test_ragged_and_tiny(oracle):
    import feature_detector_amd as fd

    rng = np.random.default_rng(7)
    for shape in ((37, 53), (61, 200), (5, 5), (4, 4), (3, 3), (2, 2), (2, 9), (9, 2)):
        img = (rng.integers(0, 4, shape) * 60).astype(np.uint8)
        _check(fd, oracle, img[None])


def test_ring_overflow_ramp(oracle):
    import feature_detector_amd as fd

    r, c = np.mgrid[0:400, 0:600]
    img = ((r * 3 + c * 5) % 256).astype(np.uint8)
    _check(fd, oracle, img[None])


def test_needed_zero(image_png):
    import feature_detector_amd as fd

    assert len(fd.lsd_lines(image_png[None], needed=0)[0]) == 0


def test_device_input_matches_host(oracle):
    import torch

    import feature_detector_amd as fd

    img = oracle.make_frame("checker", 9, 480, 640, 32)
    host = fd.lsd_lines(img[None])
    dev = fd.lsd_lines(torch.from_numpy(img[None]).cuda())
    assert np.array_equal(host[0], dev[0])


def test_config4_batch_spot_check(oracle):
    # BASELINE configs[3] shape: 256 frames of 1920x1080; frames 0, 127 and 255 against the oracle,
    # every frame's segments within the frame and of length >= 20
    import torch

    import feature_detector_amd as fd

    g = torch.Generator(device="cuda")
    g.manual_seed(4242)
    rows, cols, n = 1080, 1920, 256
    r = torch.arange(rows, device="cuda").view(1, rows, 1) // 64
    c = torch.arange(cols, device="cuda").view(1, 1, cols) // 64
    base = torch.where(((r + c) % 2) == 1, 180, 60)
    noise = torch.randint(-10, 11, (n, rows, cols), generator=g, device="cuda", dtype=torch.int32)
    frames = (base + noise).clamp(0, 255).to(torch.uint8)
    got = fd.lsd_lines(frames, max_lines=8192)
    assert len(got) == n
    host = frames.cpu().numpy()
    for b in (0, 127, 255):
        exp = oracle.lsd_lines(host[b])
        assert np.array_equal(got[b].view(np.uint32), exp.view(np.uint32)), b
    for seg in got:
        assert len(seg) > 0 and (seg[:, 6] >= 20).all()
        assert (seg[:, [0, 2]] > -2).all() and (seg[:, [0, 2]] < cols + 2).all()


def test_seed_order_on_gpu(oracle, monkeypatch, capfd):
    # the seed order (sorted_pixels_, feature_line_detector.cpp:88-94) comes from the GPU
    # (k_select_reference in push order) for every frame, including a ramp whose norms are all equal
    # (the introsort's equal-key paths) and a 1080p frame; the segments are the oracle's and those of
    # the host std::sort (FD_LSD_HOST_SORT=1), and with the multi-workgroup prelude (FD_LSD_WIDE=1) or
    # the order through a device buffer (FD_LSD_ORD_MAPPED=0) the same
    import feature_detector_amd as fd

    r, c = np.mgrid[0:400, 0:600]
    ramp = ((r * 3 + c * 5) % 256).astype(np.uint8)
    small = np.stack([ramp, oracle.make_frame("checker", 11, 400, 600, 24), oracle.make_frame("noise", 12, 400, 600, 16)])
    big = oracle.make_frame("checker", 13, 1080, 1920, 64)[None]
    monkeypatch.setenv("FD_DEBUG_AB", "1")
    monkeypatch.setenv("FD_LINES_TIMING", "1")
    for frames in (small, big):
        capfd.readouterr()
        got = _check(fd, oracle, frames)
        err = capfd.readouterr().err
        assert f"seed orders from the gpu {frames.shape[0]}" in err, err
        monkeypatch.setenv("FD_LSD_HOST_SORT", "1")
        host = fd.lsd_lines(frames)
        assert "seed orders from the gpu 0" in capfd.readouterr().err
        monkeypatch.delenv("FD_LSD_HOST_SORT")
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got, host))
        # the order through a device buffer and a copy instead of written into pinned host memory
        monkeypatch.setenv("FD_LSD_ORD_MAPPED", "0")
        copied = fd.lsd_lines(frames)
        assert f"seed orders from the gpu {frames.shape[0]}" in capfd.readouterr().err
        monkeypatch.delenv("FD_LSD_ORD_MAPPED")
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got, copied))
        monkeypatch.setenv("FD_LSD_WIDE", "1")
        wide = fd.lsd_lines(frames)
        assert f"seed orders from the gpu {frames.shape[0]}" in capfd.readouterr().err
        monkeypatch.delenv("FD_LSD_WIDE")
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got, wide))


def test_seed_order_guard_failure_falls_back(oracle, monkeypatch, capfd):
    # the seed sort's loop bound cut short (FD_REF_GUARD, diagnostic) right after a full GPU call of the
    # same frames: every frame must be reported unresolved -- not resolved with the previous call's order
    # still in the pinned buffer's tail -- and be sorted on the host, with the oracle's segments
    import feature_detector_amd as fd

    frames = np.stack([oracle.make_frame("checker", 21, 400, 600, 24), oracle.make_frame("noise", 22, 400, 600, 16)])
    monkeypatch.setenv("FD_DEBUG_AB", "1")
    monkeypatch.setenv("FD_LINES_TIMING", "1")
    capfd.readouterr()
    full = _check(fd, oracle, frames)
    assert f"seed orders from the gpu {frames.shape[0]}" in capfd.readouterr().err
    for guard in (1, 3):
        monkeypatch.setenv("FD_REF_GUARD", str(guard))
        got = _check(fd, oracle, frames)
        assert "seed orders from the gpu 0" in capfd.readouterr().err
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got, full))


# ---- the compact path's own outputs: the lists and is_used (fd_lsd_lines_state), the launch geometry's branches,
# ---- frames without valid pixels, the options, the rectangle capacity


def _state(fd):
    """fd_lsd_lines_state of the default context: (idx, norm, angle, used) of the last call's frame 0; the count
    first (cap = 0), as the C++ class reads it."""
    L, ctx = fd.load(), fd.default_context()
    n = ctypes.c_int64(-1)
    assert L.fd_lsd_lines_state(ctx.ptr, None, None, None, None, 0, ctypes.byref(n)) == 0
    m = n.value
    assert m >= 0
    idx, norm, ang, used = (np.full(m + 1, -5, np.int32), np.full(m + 1, -5, np.float32), np.full(m + 1, -5, np.float32),
                            np.full(m + 1, 5, np.uint8))
    p = lambda x: ctypes.c_void_p(x.ctypes.data)  # noqa: E731
    assert L.fd_lsd_lines_state(ctx.ptr, p(idx), p(norm), p(ang), p(used), m, ctypes.byref(n)) == 0
    assert n.value == m
    assert idx[m] == -5 and norm[m] == -5 and ang[m] == -5 and used[m] == 5  # nothing past the count
    return idx[:m], norm[:m], ang[:m], used[:m]


def _assert_state(fd, oracle, frame, **kw):
    idx, norm, ang, used = _state(fd)
    eidx, enorm, eang, eused = oracle.lsd_lines_state(frame, **kw)
    assert np.array_equal(idx, eidx)
    assert np.array_equal(norm.view(np.uint32), enorm.view(np.uint32))
    assert np.array_equal(ang.view(np.uint32), eang.view(np.uint32))
    assert np.array_equal(used, eused)
    return used


def _spot_frame(rows=120, cols=160):
    """Flat but for one bright pixel: 4 valid pixels, no line."""
    f = np.full((rows, cols), 90, np.uint8)
    f[rows // 2, cols // 2] = 255
    return f


@pytest.mark.parametrize("name", ["image_png", "checker_240x320", "checker_1028x48"])
def test_state_readout(oracle, image_png, name):
    """The GPU's compact lists (k_lsd_scatter + k_lsd_values) and the host's final is_used of frame 0, against
    the oracle's pixel state bit for bit; the second frame of the batch must not leak into it."""
    import feature_detector_amd as fd

    frame = {"image_png": image_png, "checker_240x320": oracle.make_frame("checker", 7, 240, 320, 24),
             "checker_1028x48": oracle.make_frame("checker", 5, 1028, 48, 24)}[name]
    other = oracle.make_frame("noise", 1, *frame.shape)
    _check(fd, oracle, np.stack([frame, other]))
    used = _assert_state(fd, oracle, frame)
    assert len(oracle.lsd_lines(frame)) > 0 and used.any() and not used.all()


def test_state_empty_first_frame_and_needed_zero(oracle):
    import feature_detector_amd as fd

    checker = oracle.make_frame("checker", 3, 120, 160, 24)
    flat = np.full((120, 160), 90, np.uint8)
    _check(fd, oracle, checker[None])
    assert len(_state(fd)[0]) > 0
    _check(fd, oracle, np.stack([flat, checker]))  # a first frame without valid pixels
    assert len(_state(fd)[0]) == 0
    _check(fd, oracle, np.stack([_spot_frame(), checker]))
    assert len(_assert_state(fd, oracle, _spot_frame())) == 4
    assert len(fd.lsd_lines(checker[None], needed=0)[0]) == 0  # needed = 0 clears the state
    assert len(_state(fd)[0]) == 0


@pytest.mark.parametrize("rows,cols,lines,chunks,columns", [
    (1027, 48, 77, 64, (1, 0, 1, 2)), (1028, 48, 77, 65, (1, 0, 1, 2)), (2052, 48, 166, 129, (1, 0, 1, 2)),
    (48, 260, 17, 3, (2, 0, 1, 9)), (48, 514, 38, 3, (3, 1, 1, 17)), (48, 520, 43, 3, (3, 1, 1, 17)),
    (48, 1030, 84, 3, (5, 3, 2, 33))])
def test_compact_geometry(oracle, rows, cols, lines, chunks, columns):
    """Compact mode (null maps, frame_base) at the scatter's one-pass / looped switch (64 | 65 chunks), in its
    third pass (129), with a second map strip, an exactly interior strip (514; 520: with dword loads) and two
    scan passes (1030): the rectangles against the oracle."""
    import feature_detector_amd as fd

    assert lsd_chunks(1, rows, cols) == (16, chunks) and lsd_columns(cols) == columns
    img = oracle.make_frame("checker", 5, rows, cols, 24)
    exp = oracle.lsd_lines(img)
    assert len(exp) == lines and lines > 0
    _check(fd, oracle, img[None])


@pytest.fixture(scope="module")
def small_batch(oracle):
    """1024 checker frames of 131x48 (seeds 0..1023) and the oracle's segments of each."""
    frames = np.stack([oracle.make_frame("checker", s, 131, 48, 24) for s in range(1024)])
    exp = [oracle.lsd_lines(f) for f in frames]
    assert len(exp[5]) == 11
    return frames, exp


@pytest.mark.parametrize("batch,geometry", [(1024, (32, 4)), (1023, (16, 8))])
def test_compact_batch_both_chunk_heights(small_batch, batch, geometry):
    """131x48 frames on both sides of the chunk-height switch (1024 x 1 x 4 >= 4096 waves): every frame's
    rectangles against the oracle."""
    import feature_detector_amd as fd

    frames, exp = small_batch
    assert lsd_chunks(batch, 131, 48) == geometry
    assert sum(len(e) > 0 for e in exp[:batch]) >= batch // 2
    got = fd.lsd_lines(frames[:batch], max_lines=64)
    assert len(got) == batch
    for b in range(batch):
        assert got[b].shape == exp[b].shape, b
        assert np.array_equal(got[b].view(np.uint32), exp[b].view(np.uint32)), b


def test_compact_batch_looped_scatter_32_row_chunks(oracle):
    """64 frames of 2052x48: 32-row chunks, 65 per column (the scatter's looped path on full row words)."""
    import feature_detector_amd as fd

    assert lsd_chunks(64, 2052, 48) == (32, 65)
    frames = np.stack([oracle.make_frame("checker", 100 + s, 2052, 48, 24) for s in range(64)])
    exp = [oracle.lsd_lines(f) for f in frames]
    assert sum(len(e) > 0 for e in exp) >= 32
    got = fd.lsd_lines(frames, max_lines=512)
    for b in range(64):
        assert got[b].shape == exp[b].shape, b
        assert np.array_equal(got[b].view(np.uint32), exp[b].view(np.uint32)), b


@pytest.mark.parametrize("host_sort", [False, True])
@pytest.mark.parametrize("threads", [1, 4])
def test_empty_frames_in_a_batch(oracle, monkeypatch, threads, host_sort):
    """Frames without valid pixels among frames with lines (equal frame_base entries in k_lsd_values' search,
    k_lsd_seed_lists with n = 0, the null FrameList), first and last in the batch; a frame with 4 valid pixels
    and no line; and an all-flat batch (no list at all). Seed order from the GPU and from the host's std::sort."""
    import feature_detector_amd as fd

    flat = np.full((120, 160), 90, np.uint8)
    checker = [oracle.make_frame("checker", s, 120, 160, 24) for s in (3, 4)]
    frames = np.stack([flat, checker[0], flat, flat, checker[1], _spot_frame()])
    valid = [len(oracle.lsd_map(f)[3]) for f in frames]
    assert [v > 0 for v in valid] == [False, True, False, False, True, True] and valid[5] == 4
    assert [len(oracle.lsd_lines(f)) > 0 for f in frames] == [False, True, False, False, True, False]
    if host_sort:
        monkeypatch.setenv("FD_DEBUG_AB", "1")
        monkeypatch.setenv("FD_LSD_HOST_SORT", "1")
    _check(fd, oracle, frames, threads=threads)
    assert len(_state(fd)[0]) == 0
    _check(fd, oracle, frames[::-1], threads=threads)  # the empty frame last, the 4-pixel frame first
    assert len(_state(fd)[0]) == 4
    got = _check(fd, oracle, np.stack([flat] * 5), threads=threads)
    assert all(len(g) == 0 for g in got) and len(_state(fd)[0]) == 0
    _check(fd, oracle, frames, threads=threads)  # and lists again after the call without any


D2R = np.float32(3.14159265358979323846) / np.float32(180.0)


@pytest.mark.parametrize("kw,lines", [(dict(min_norm=5.0), 142), (dict(min_norm=-1.0), 92),
                                      (dict(tol_rad=float(np.float32(45.0) * D2R)), 145),
                                      (dict(tol_rad=float(np.float32(10.0) * D2R)), 167),
                                      (dict(min_length=60.0), 0)])
def test_options(oracle, kw, lines):
    """Each option away from its default on a 240x320 checker: the oracle's result differs from the default's
    (167 lines), so the option matters, and the GPU path's equals it; the pixel state too."""
    import feature_detector_amd as fd

    img = oracle.make_frame("checker", 7, 240, 320, 24)
    base, exp = oracle.lsd_lines(img), oracle.lsd_lines(img, **kw)
    assert len(base) == 167 and len(exp) == lines
    assert base.shape != exp.shape or not np.array_equal(base, exp)
    _check(fd, oracle, img[None], **kw)
    _assert_state(fd, oracle, img, **kw)


@pytest.mark.parametrize("min_inlier,lines", [(0.3, 179), (0.9, 59)])
def test_option_min_inlier(oracle, min_inlier, lines):
    """min_inlier on a checker with a quarter of a noise frame added (the clean checker's count does not depend
    on it): 112 lines at the default 0.6."""
    import feature_detector_amd as fd

    noise = oracle.make_frame("noise", 3, 240, 320).astype(np.int32)
    img = (oracle.make_frame("checker", 7, 240, 320, 24).astype(np.int32) + (noise - 128) // 4).clip(0, 255).astype(np.uint8)
    assert len(oracle.lsd_lines(img)) == 112 and len(oracle.lsd_lines(img, min_inlier=min_inlier)) == lines
    _check(fd, oracle, img[None], min_inlier=min_inlier)
    _check(fd, oracle, img[None])


def test_needed_above_one_changes_nothing(oracle):
    import feature_detector_amd as fd

    img = oracle.make_frame("checker", 7, 240, 320, 24)
    one = _check(fd, oracle, img[None], needed=1)
    five = _check(fd, oracle, img[None], needed=5)
    assert len(one[0]) == 167 and np.array_equal(one[0].view(np.uint32), five[0].view(np.uint32))


def test_rectangle_capacity(oracle):
    """rect_stride below the segments found: the C call returns the true counts and writes the first rect_stride
    rectangles of each frame only; the binding raises FD_ERR_CAPACITY; the context works on."""
    import feature_detector_amd as fd
    from feature_detector_amd._lib import FD_ERR_CAPACITY, fd_lsd_opts

    checker = oracle.make_frame("checker", 3, 120, 160, 24)
    two = np.full((120, 160), 90, np.uint8)
    two[30:60, 50:72] = checker[30:60, 50:72]
    frames = np.stack([checker, np.full((120, 160), 90, np.uint8), two])
    exp = [oracle.lsd_lines(f) for f in frames]
    assert [len(e) for e in exp] == [36, 0, 2]
    L, ctx = fd.load(), fd.default_context()
    ctx.set_stream(None)
    stride, sent = 3, np.float32(-123.5)
    out = np.full((4, stride, 12), sent, np.float32)  # (a fourth frame's worth behind the batch: never written)
    cnt = np.full((3,), -9, np.int32)
    opts = fd_lsd_opts(20.0, oracle.LSD_TOL_RAD, 20.0, 0.6)
    rc = L.fd_lsd_lines(ctx.ptr, ctypes.c_void_p(frames.ctypes.data), 0, 3, 120, 160, ctypes.byref(opts), 1,
                        ctypes.c_void_p(out.ctypes.data), stride, ctypes.c_void_p(cnt.ctypes.data), 2)
    assert rc == 0
    assert cnt.tolist() == [36, 0, 2]
    for b in range(3):
        k = min(len(exp[b]), stride)
        assert np.array_equal(out[b, :k].view(np.uint32), exp[b][:k].view(np.uint32)), b
        assert (out[b, k:] == sent).all(), b
    assert (out[3] == sent).all()
    with pytest.raises(fd.FdError) as e:
        fd.lsd_lines(frames, max_lines=3)
    assert e.value.code == FD_ERR_CAPACITY
    _check(fd, oracle, frames)  # the same context, default capacity
    _assert_state(fd, oracle, frames[0])
