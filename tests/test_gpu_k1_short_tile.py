"""GPU: the short-tile corner kernel (k_corner_short) against the CPU oracle, bit for bit.

Small Harris / Shi-Tomasi launches in sorted-segment mode (tile height 3, thr >= 0) take k_corner_short: two
columns per lane, tiles of 124 columns x 3 rows, 8 waves per workgroup. Every case runs fd.detect_points
(ties="raster", the kernel under test, then the selection) and fd.point_response (the unordered candidate
list) and compares both with the oracle exactly. Detection runs with a small distance and a large need, so
that the selected features cover most of the candidates and not only the strongest few.

Cases: the tile seams in x (124 columns) and in y (3 rows), the unaligned load form (cols % 4 != 0, or a
frame pointer off by one byte), the densest candidate pattern NMS admits (the per-wave staging bound), the
prior-feature mask, batches on both sides of the dispatch boundary, and a reserved shape captured in a graph.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KIND = {"harris": 0, "shi_tomasi": 1}
THR = {"harris": 30.0, "shi_tomasi": 40.0}
NAMES = ["harris", "shi_tomasi"]
TILE_W = 124  # columns per wave of k_corner_short


@pytest.fixture(scope="module")
def fd():
    import feature_detector_amd as fd

    fd.load()
    return fd


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


def error_bits(fd):
    return np.uint32(fd.points.FRAME_GUARD | fd.points.FRAME_VALUE_RANGE | fd.points.FRAME_UNRESOLVED)


def check(fd, torch, oracle, name, frames, dist=1, need=4096, prior=None, dev=None, thr=None):
    """detect_points (raster ties) and point_response of a batch of frames against the oracle, frame by frame.
    frames: [B, R, C] uint8 (host); dev: the same frames on the device (default: a plain copy)."""
    frames = np.ascontiguousarray(frames)
    batch, rows, cols = frames.shape
    thr = THR[name] if thr is None else thr
    if dev is None:
        dev = torch.from_numpy(frames).cuda()
    res = fd.detect_points(name, dev, need, dist, thr, prior=None if prior is None else [prior] * batch, ties="raster")
    resp, idx, cnt = fd.point_response(name, dev, thr)
    torch.cuda.synchronize()
    assert not (res.frame_flags() & error_bits(fd)).any(), res.frame_flags()
    cnt = cnt.cpu().numpy()
    cache = {}
    total = 0
    for b in range(batch):
        key = frames[b].tobytes()
        if key not in cache:  # (large batches repeat a few frames)
            exp, _ = oracle.detect(KIND[name], frames[b], dist, thr, need, prior, sort_mode=1)
            cache[key] = (exp, oracle.nms(oracle.response_map(frames[b], KIND[name], thr), thr))
        exp, (er, ex, ey) = cache[key]
        assert np.array_equal(res.features(b), exp), (name, b)
        gi = idx[b, :cnt[b]].cpu().numpy().astype(np.int64)
        gr = resp[b, :cnt[b]].cpu().numpy()
        o = np.argsort(gi, kind="stable")
        assert np.array_equal(gi[o], ey.astype(np.int64) * cols + ex), (name, b)
        assert np.array_equal(gr[o].view(np.uint32), er.view(np.uint32)), (name, b)
        total += len(exp)
    return total


def seam_frame(rows, cols, seed):
    """Noise with isolated bright pixels (each the strict response maximum of its neighbourhood) on the last
    and first owned column of neighbouring 124-column tiles, and on the first and last column of the frame's
    candidate region [2, cols-3] where that leaves 4 columns to the other bright pixels of its row."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 24, (rows, cols), dtype=np.uint8)
    seams = [c for t in range(1, cols // TILE_W + 1) for c in (t * TILE_W - 1, t * TILE_W) if 2 <= c <= cols - 3]
    spots = [(c, (3, 7)[k % 2]) for k, c in enumerate(seams)]  # rows 4 apart: their 3x3 windows do not meet
    for k, c in enumerate((2, cols - 3)):
        r = (7, 3)[k]
        if all(abs(c - sc) >= 4 for sc, sr in spots if sr == r):
            spots.append((c, r))
    for c, r in spots:
        img[r, c] = 255
    return img, spots


@pytest.mark.parametrize("cols", [123, 124, 125, 126, 127, 128, 129, 248, 250])
@pytest.mark.parametrize("name", NAMES)
def test_tile_seams_in_x(fd, torch, oracle, name, cols):
    rows = 11
    for seed in range(100 + cols, 140 + cols):  # (the first noise seed that leaves every bright pixel a candidate)
        img, spots = seam_frame(rows, cols, seed)
        er, ex, ey = oracle.nms(oracle.response_map(img, KIND[name], THR[name]), THR[name])
        if set(spots) <= set(zip(ex.tolist(), ey.tolist())):
            break
    else:
        raise AssertionError("the constructed corners must be candidates on the seam columns")
    assert check(fd, torch, oracle, name, img[None]) >= len(spots)
    # (plain noise: the columns next to the seams carry candidates whose neighbours lie in the other tile)
    assert check(fd, torch, oracle, name, oracle.make_frame("noise", 150 + cols, rows, cols)[None]) > 0
    # the same frame from a pointer one byte off a dword: the byte-assembled loads whatever cols is
    buf = torch.zeros(img.size + 1, dtype=torch.uint8, device="cuda")
    odd = buf[1:].view(1, rows, cols)
    odd.copy_(torch.from_numpy(img[None]))
    assert odd.data_ptr() % 4 == 1
    check(fd, torch, oracle, name, img[None], dev=odd)


@pytest.mark.parametrize("rows", [5, 6, 7, 8, 9, 10])
@pytest.mark.parametrize("name", NAMES)
def test_tile_seams_in_y(fd, torch, oracle, name, rows):
    """1 to 6 output rows: the frame's last tile row holds 1, 2 or 3 rows."""
    img = oracle.make_frame("noise", 200 + rows, rows, 130)
    assert check(fd, torch, oracle, name, img[None]) > 0


def dense_frame(rows, cols, seed):
    """A one-pixel 0/255 checker with a seeded +-1 perturbation: strict 4-neighbour NMS can pass every other
    pixel, which is the most a wave can stage."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:rows, 0:cols]
    base = (((xx + yy) & 1) * 255).astype(np.int16)
    return np.clip(base + rng.integers(-1, 2, (rows, cols)), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("shape", [(11, 130), (480, 640)])
@pytest.mark.parametrize("name", NAMES)
def test_maximum_nms_density(fd, torch, oracle, name, shape):
    rows, cols = shape
    img = dense_frame(rows, cols, 300 + rows)
    # (thr 0: the pattern's gradients are -2 .. 2, its responses far below the detectors' usual thresholds)
    assert check(fd, torch, oracle, name, img[None], dist=1, need=4096, thr=0.0) > 40


@pytest.mark.parametrize("name", NAMES)
def test_prior_feature_mask(fd, torch, oracle, name):
    """Priors on the tile seam (columns 123 / 124) and at the frame's edge: the MASKED instance."""
    img = oracle.make_frame("noise", 400, 11, 130)
    prior = np.array([(123.0, 4.0), (124.5, 8.0), (2.0, 2.0), (60.0, 5.0), (122.0, 6.0), (127.0, 3.0), (30.0, 3.0),
                      (90.0, 7.0)], np.float32)
    n = check(fd, torch, oracle, name, img[None], dist=3, prior=prior)
    assert 0 < n < check(fd, torch, oracle, name, img[None], dist=3)


@pytest.mark.parametrize("batch", [1, 2, 5])
@pytest.mark.parametrize("name", NAMES)
def test_batches(fd, torch, oracle, name, batch):
    frames = np.stack([oracle.make_frame(("noise", "checker")[b % 2], 500 + b, 48, 64) for b in range(batch)])
    assert check(fd, torch, oracle, name, frames) > 0


@pytest.mark.parametrize("name", NAMES)
def test_dispatch_boundary(fd, torch, oracle, name):
    """Both sides of the launch size at which the tile height leaves its small-launch value 3: the tile
    height is batch * tiles_x * out_rows / 10240 rounded up to a multiple of 6 once that quotient reaches 6.
    16 x 48 frames (one tile column, 44 output rows): 1396 frames take k_corner_short, 1397 frames k_corner
    with tiles of 6 rows (batch * rows * cols stays below the 2^21 pixels from which k_corner_lp runs)."""
    rows, cols, out_rows = 48, 16, 44
    small, large = 1396, 1397
    assert small * out_rows // 10240 < 6 <= large * out_rows // 10240 and large * rows * cols < 1 << 21
    templ = [oracle.make_frame(("noise", "checker")[k % 2], 600 + k, rows, cols) for k in range(7)]
    frames = np.stack([templ[b % 7] for b in range(large)])
    n_small = check(fd, torch, oracle, name, frames[:small], need=256)
    n_large = check(fd, torch, oracle, name, frames, need=256)
    assert n_small > 0 and n_large > n_small


@pytest.mark.parametrize("name", NAMES)
def test_reserve_then_capture(fd, torch, oracle, name):
    """A reserved shape on the short-tile path, captured in a graph and replayed twice: nothing is allocated
    and no pointer changes after fd_ctx_reserve."""
    rows, cols, need, dist = 48, 250, 50, 20
    frames = np.stack([oracle.make_frame("noise", 700, rows, cols), oracle.make_frame("checker", 701, rows, cols)])
    exp = [oracle.detect(KIND[name], f, dist, THR[name], need, None, sort_mode=1)[0] for f in frames]
    assert all(len(e) > 0 for e in exp)
    ctx = fd.Context(0)
    ctx.reserve(KIND[name], len(frames), rows, cols)
    ctx.synchronize()
    dev = torch.from_numpy(frames).cuda()
    out = (torch.zeros((len(frames), need + 1, 2), dtype=torch.float32, device="cuda"),
           torch.zeros((len(frames),), dtype=torch.int32, device="cuda"),
           torch.zeros((len(frames),), dtype=torch.int32, device="cuda"))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        fd.detect_points(name, dev, need, dist, THR[name], ctx=ctx, ties="raster", out=out)
    for _ in range(2):
        for t in out:
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        xy, cnt, st = (t.cpu().numpy() for t in out)
        assert not (st.astype(np.uint32) & error_bits(fd)).any(), st
        for b in range(len(frames)):
            assert np.array_equal(xy[b, :int(cnt[b])], exp[b]), (name, b)
    del g
    ctx.close()
