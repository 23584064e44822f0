"""GPU parity of the LSD level-line map (fd_lsd_map) against the oracle: bit-exact norm, valid flag
and angle (the kernel restates glibc's fdlibm atan2f), and the column-major valid list in the
reference's scan order (sorted_pixels_ before its std::sort, feature_line_detector.cpp:71-92)."""
import numpy as np
import pytest

from lsd_geometry import lsd_chunks, lsd_columns

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fd():
    import feature_detector_amd as fd

    fd.load()
    return fd


def check_lsd(fd, oracle, img, min_norm=20.0):
    (n, a, v, idx), = fd.lsd_map(img, min_norm)
    en, ea, ev, eidx = oracle.lsd_map(img, min_norm)
    assert np.array_equal(n.view(np.uint32), en.view(np.uint32))
    assert np.array_equal(v, ev)
    assert np.array_equal(a.view(np.uint32), ea.view(np.uint32))
    assert np.array_equal(idx, eidx)
    # host std::sort of the GPU list reproduces the reference's sorted_pixels_ exactly
    assert np.array_equal(oracle.lsd_sort(n, idx, 0), oracle.lsd_sort(en, eidx, 0))
    return idx


def test_image_png(fd, oracle, image_png, ref_counts):
    idx = check_lsd(fd, oracle, image_png)
    assert len(idx) == ref_counts["image_png"]["lsd_valid"]


@pytest.mark.parametrize("rec_i", [0, 1, 2])
def test_synthetic_counts(fd, oracle, ref_counts, rec_i):
    rec = ref_counts["synthetic_lsd_valid"][rec_i]
    img = oracle.make_frame(rec["pattern"], 1234, rec["rows"], rec["cols"], rec["period"])
    idx = check_lsd(fd, oracle, img)
    assert len(idx) == rec["valid"]


@pytest.mark.parametrize("shape", [(2, 2), (3, 3), (4, 4), (5, 67), (67, 5), (100, 129), (257, 63)])
def test_ragged(fd, oracle, shape):
    img = np.random.default_rng(shape[0] * 1000 + shape[1]).integers(0, 256, shape, dtype=np.uint8)
    check_lsd(fd, oracle, img, 20.0)


def test_ragged_height_both_chunk_heights(fd, oracle):
    """37x70 frames (34 scanned rows, one 256-column strip): a single frame takes 16-row chunks (16 + 16 + 2
    rows), and from 2048 frames on (batch x strips x ceil(34 / 32) >= 4096 waves) the launch takes 32-row
    chunks (32 + 2 rows): the last chunk's row-bit word is partial in both. Dense maps and the column-major
    list of every frame against the oracle, bit for bit."""
    rows, cols, batch = 37, 70, 2048
    assert (batch - 1) * 1 * ((rows - 3 + 31) // 32) < 4096 <= batch * 1 * ((rows - 3 + 31) // 32)
    frames = np.random.default_rng(3770).integers(0, 256, (batch, rows, cols), dtype=np.uint8)
    check_lsd(fd, oracle, frames[0])
    res = fd.lsd_map(frames)
    assert len(res) == batch
    for b in range(batch):
        n, a, v, idx = res[b]
        en, ea, ev, eidx = oracle.lsd_map(frames[b])
        assert np.array_equal(n.view(np.uint32), en.view(np.uint32)), b
        assert np.array_equal(v, ev), b
        assert np.array_equal(a.view(np.uint32), ea.view(np.uint32)), b
        assert np.array_equal(idx, eidx), b


@pytest.mark.parametrize("min_norm", [0.0, 5.0, 100.0, 400.0])
def test_thresholds(fd, oracle, min_norm):
    img = np.random.default_rng(3).integers(0, 256, (120, 200), dtype=np.uint8)
    check_lsd(fd, oracle, img, min_norm)


def test_angle_domain_exhaustive(fd, oracle):
    """Every (ad, bc) gradient pair -> every half-integer (gx, gy): built as 2x2 blocks."""
    vals = []
    for ad in range(-255, 256):
        for bc in range(-255, 256):
            # I(r,c)=p, I(r+1,c+1)=p+ad, I(r,c+1)=q, I(r+1,c)=q-bc with values in [0,255]
            p = max(0, -ad)
            q = max(0, bc)
            if p + ad > 255 or q - bc > 255 or q > 255:
                continue
            vals.append((p, q, q - bc, p + ad))
    n = len(vals)
    img = np.zeros((3, 2 * n + 2), np.uint8)
    for i, (a, b, c, d) in enumerate(vals):
        img[1, 1 + 2 * i], img[1, 2 + 2 * i] = a, b
        img[2, 1 + 2 * i], img[2, 2 + 2 * i] = c, d
    img = np.concatenate([img, np.zeros((2, img.shape[1]), np.uint8)])
    check_lsd(fd, oracle, img, 0.0)


def test_batch(fd, oracle):
    frames = np.stack([oracle.make_frame("checker", s, 240, 320, 32) for s in range(5)])
    res = fd.lsd_map(frames)
    for b in range(5):
        en, ea, ev, eidx = oracle.lsd_map(frames[b])
        assert np.array_equal(res[b][3], eidx)
        assert np.array_equal(res[b][1].view(np.uint32), ea.view(np.uint32))


def test_device_path_matches_host(fd, oracle):
    """lsd_map on torch device frames (maps written whole by the kernel, no memsets) equals the host path."""
    torch = pytest.importorskip("torch")
    frames = np.stack([oracle.make_frame("checker", 60 + i, 120, 200, 64) for i in range(2)]
                      + [oracle.make_frame("noise", 70, 120, 200)])
    host = fd.lsd_map(frames)
    dev = torch.from_numpy(frames).cuda()
    out = (torch.full((3, 119, 199), 7.0, device="cuda"), torch.full((3, 119, 199), 7.0, device="cuda"),
           torch.full((3, 119, 199), 7, dtype=torch.uint8, device="cuda"),
           torch.empty((3, 119 * 199), dtype=torch.int32, device="cuda"), torch.empty((3,), dtype=torch.int64, device="cuda"))
    n, a, v, idx, cnt = fd.lsd_map(dev, out=out)
    torch.cuda.synchronize()
    for b in range(3):
        hn, ha, hv, hidx = host[b]
        assert np.array_equal(n[b].cpu().numpy().view(np.uint32), hn.view(np.uint32))
        assert np.array_equal(a[b].cpu().numpy().view(np.uint32), ha.view(np.uint32))
        assert np.array_equal(v[b].cpu().numpy(), hv)
        assert int(cnt[b]) == len(hidx)
        assert np.array_equal(idx[b, :len(hidx)].cpu().numpy(), hidx)


@pytest.mark.parametrize("shape", [(120, 200), (67, 5), (33, 257), (40, 1920)])
def test_pitched_maps(fd, oracle, shape):
    """fd_lsd_map_pitched: the default device maps (rows padded to 16 entries: aligned row stores) and a
    caller pitch (odd on purpose) equal the host path; the padding entries are never written."""
    torch = pytest.importorskip("torch")
    rows, cols = shape
    frames = np.stack([oracle.make_frame("checker", 80 + i, rows, cols, 16) for i in range(2)]
                      + [oracle.make_frame("noise", 90, rows, cols)])
    host = fd.lsd_map(frames)
    dev = torch.from_numpy(frames).cuda()
    mr, mc = rows - 1, cols - 1
    outs = [fd.lsd_map(dev)]
    pitch = mc + 5
    bufs = (torch.full((3, mr, pitch), 7.0, device="cuda"), torch.full((3, mr, pitch), 7.0, device="cuda"),
            torch.full((3, mr, pitch), 7, dtype=torch.uint8, device="cuda"))
    outs.append(fd.lsd_map(dev, out=tuple(t[..., :mc] for t in bufs) + (
        torch.empty((3, mr * mc), dtype=torch.int32, device="cuda"), torch.empty((3,), dtype=torch.int64, device="cuda"))))
    torch.cuda.synchronize()
    assert outs[0][0].stride(1) % 16 == 0 and outs[0][0].stride(1) >= mc
    for n, a, v, idx, cnt in outs:
        for b in range(3):
            hn, ha, hv, hidx = host[b]
            assert np.array_equal(n[b].cpu().numpy().view(np.uint32), hn.view(np.uint32)), b
            assert np.array_equal(a[b].cpu().numpy().view(np.uint32), ha.view(np.uint32)), b
            assert np.array_equal(v[b].cpu().numpy(), hv), b
            assert int(cnt[b]) == len(hidx)
            assert np.array_equal(idx[b, :len(hidx)].cpu().numpy(), hidx), b
    for t, fill in zip(bufs, (7.0, 7.0, 7)):
        assert bool((t[..., mc:] == fill).all())  # padding untouched
    with pytest.raises(Exception):  # a pitch below cols-1 is refused
        bad = torch.empty((3, mr, mc), device="cuda").as_strided((3, mr, mc), (mr * (mc - 1), mc - 1, 1))
        fd.lsd_map(dev, out=(bad, None, None, torch.empty((3, mr * mc), dtype=torch.int32, device="cuda"),
                             torch.empty((3,), dtype=torch.int64, device="cuda")))


def test_config4_batch_spot_check(fd, oracle):
    """BASELINE configs[3] shape (1920x1080 x256, the bench's 64-px checker + noise): the dense maps and
    the valid list of frames 0, 127 and 255 against the oracle, and every frame's count consistent."""
    torch = pytest.importorskip("torch")
    g = torch.Generator(device="cuda")
    g.manual_seed(4243)
    rows, cols, n = 1080, 1920, 256
    r = torch.arange(rows, device="cuda").view(1, rows, 1) // 64
    c = torch.arange(cols, device="cuda").view(1, 1, cols) // 64
    base = torch.where(((r + c) % 2) == 1, 180, 60)
    noise = torch.randint(-10, 11, (n, rows, cols), generator=g, device="cuda", dtype=torch.int32)
    frames = (base + noise).clamp(0, 255).to(torch.uint8)
    nm, am, vm, idx, cnt = fd.lsd_map(frames)  # the bench's layout: row-padded (aligned) maps
    torch.cuda.synchronize()
    assert nm.stride(1) == 1920  # 1919 entries padded to 16
    assert torch.equal(cnt, vm.sum(dim=(1, 2), dtype=torch.int64))
    host = frames.cpu().numpy()
    for b in (0, 127, 255):
        en, ea, ev, eidx = oracle.lsd_map(host[b])
        k = int(cnt[b])
        assert np.array_equal(nm[b].cpu().numpy().view(np.uint32), en.view(np.uint32)), b
        assert np.array_equal(vm[b].cpu().numpy(), ev), b
        assert np.array_equal(am[b].cpu().numpy().view(np.uint32), ea.view(np.uint32)), b
        assert np.array_equal(idx[b, :k].cpu().numpy(), eidx), b


# ---- the launch geometry's branches: lsd_geometry's chunk height, k_lsd_map's tile variants, k_lsd_scan's passes,
# ---- k_lsd_scatter's two paths (formulas: tests/lsd_geometry.py)


def pair_frames(oracle, seed, rows, cols, period):
    return np.stack([oracle.make_frame("noise", seed, rows, cols), oracle.make_frame("checker", seed + 1, rows, cols, period)])


def assert_frame(got, exp, tag):
    n, a, v, idx = got
    en, ea, ev, eidx = exp
    assert np.array_equal(n.view(np.uint32), en.view(np.uint32)), tag
    assert np.array_equal(v, ev), tag
    assert np.array_equal(a.view(np.uint32), ea.view(np.uint32)), tag
    assert np.array_equal(idx, eidx), tag


def device_maps(fd, torch, dev, pitch=None, min_norm=20.0):
    """fd.lsd_map on device frames -> (per-frame host tuples, the padded buffers or None). pitch None: the
    library's own maps (rows padded to 16 entries); else caller maps of that pitch, prefilled with 7."""
    b, rows, cols = dev.shape
    mr, mc = rows - 1, cols - 1
    bufs = None
    if pitch is None:
        n, a, v, idx, cnt = fd.lsd_map(dev, min_norm)
        assert n.stride(1) % 16 == 0 and n.stride(1) >= mc
    else:
        bufs = (torch.full((b, mr, pitch), 7.0, device="cuda"), torch.full((b, mr, pitch), 7.0, device="cuda"),
                torch.full((b, mr, pitch), 7, dtype=torch.uint8, device="cuda"))
        n, a, v, idx, cnt = fd.lsd_map(dev, min_norm, out=tuple(t[..., :mc] for t in bufs) + (
            torch.empty((b, mr * mc), dtype=torch.int32, device="cuda"), torch.empty((b,), dtype=torch.int64, device="cuda")))
    torch.cuda.synchronize()
    cnt = cnt.cpu().numpy()
    return [(n[i].cpu().numpy(), a[i].cpu().numpy(), v[i].cpu().numpy(), idx[i, :cnt[i]].cpu().numpy())
            for i in range(b)], bufs


@pytest.mark.parametrize("rows,chunks", [(19, 1), (20, 2), (259, 16), (260, 17), (515, 32), (516, 33), (771, 48),
                                         (772, 49), (1027, 64), (1028, 65), (1044, 66), (2100, 132)])
def test_chunk_boundaries(fd, oracle, rows, chunks):
    """Single 9-column frames of 16-row chunks on both sides of every step of k_lsd_scatter's one-pass path (16
    row-bit words per load step: 16|17, 32|33, 48|49 chunks), of its switch to the looped path (64|65), and in the
    looped path's second and third pass of 64 lanes (66, 132 chunks)."""
    assert lsd_chunks(1, rows, 9) == (16, chunks)
    for img in pair_frames(oracle, rows, rows, 9, 8):
        idx = check_lsd(fd, oracle, img)
        assert len(idx) > rows // 4  # valid pixels in every part of the column


@pytest.fixture(scope="module")
def tall_batch(oracle):
    """64 frames of 2052x9 (noise and 8-px checker alternating) and the oracle's maps of each."""
    frames = np.stack([oracle.make_frame("noise", 500 + i, 2052, 9) if i % 2 else oracle.make_frame("checker", 500 + i, 2052, 9, 8)
                       for i in range(64)])
    return frames, [oracle.lsd_map(f) for f in frames]


@pytest.mark.parametrize("batch,geometry", [(64, (32, 65)), (63, (16, 129))])
def test_looped_scatter_both_chunk_heights(fd, tall_batch, batch, geometry):
    """2052x9 frames: 64 of them take 32-row chunks (64 x 1 x 65 >= 4096), 65 per column, i.e. the scatter's looped
    path on full 32-bit row words; 63 stay on 16-row chunks, 129 per column (three passes). Every frame against
    the oracle."""
    frames, exp = tall_batch
    assert lsd_chunks(batch, 2052, 9) == geometry and geometry[1] > 64
    res = fd.lsd_map(frames[:batch])
    assert len(res) == batch
    for b in range(batch):
        assert_frame(res[b], exp[b], b)


@pytest.mark.parametrize("cols,geometry", [
    (33, (1, 0, 1, 1)), (34, (1, 0, 1, 2)), (35, (1, 0, 1, 2)),          # the scatter's 32-column wave strip
    (257, (1, 0, 1, 8)), (258, (2, 0, 1, 9)), (259, (2, 0, 1, 9)),       # a second map strip of 1 / 2 map columns
    (513, (2, 0, 1, 16)), (514, (3, 1, 1, 17)), (515, (3, 1, 1, 17)),    # strip 1 just short of / exactly interior
    (770, (4, 2, 1, 25)),                                                # strip 2 exactly interior
    (1025, (4, 2, 1, 32)), (1026, (5, 3, 2, 33)), (1027, (5, 3, 2, 33)),  # the scan's second pass of 1024 columns
    (2050, (9, 7, 3, 65))])                                              # and its third
def test_column_boundaries(fd, oracle, cols, geometry):
    """21-row frames at the column counts where the map's tile variant, the scan's pass count or the scatter's
    wave strips change: the host path, and the device path on the library's 16-padded maps and on a caller's odd
    pitch (padding untouched), all against the oracle."""
    torch = pytest.importorskip("torch")
    assert lsd_columns(cols) == geometry
    rows = 21
    frames = pair_frames(oracle, cols, rows, cols, 8)
    exp = [oracle.lsd_map(f) for f in frames]
    assert all(len(e[3]) > cols for e in exp)
    host = fd.lsd_map(frames)
    dev = torch.from_numpy(frames).cuda()
    padded, _ = device_maps(fd, torch, dev)
    pitched, bufs = device_maps(fd, torch, dev, pitch=cols - 1 + 5)
    for b in range(2):
        assert_frame(host[b], exp[b], ("host", b))
        assert_frame(padded[b], exp[b], ("padded", b))
        assert_frame(pitched[b], exp[b], ("pitched", b))
    for t, fill in zip(bufs, (7.0, 7.0, 7)):
        assert bool((t[..., cols - 1:] == fill).all())  # padding untouched


@pytest.mark.parametrize("cols", [8, 516])
def test_unaligned_frame_pointer(fd, oracle, cols):
    """cols % 4 == 0 with a frame pointer that is not 4-byte aligned (a view from byte 1 of a device buffer): the
    byte-load instance of k_lsd_map (516: with an INTERIOR strip); the same frames aligned take the dword loads."""
    torch = pytest.importorskip("torch")
    rows = 21
    assert cols % 4 == 0 and lsd_columns(cols)[1] == (1 if cols == 516 else 0)
    frames = pair_frames(oracle, 40 + cols, rows, cols, 8)
    exp = [oracle.lsd_map(f) for f in frames]
    buf = torch.zeros(frames.size + 1, dtype=torch.uint8, device="cuda")
    odd = buf[1:].view(frames.shape)
    odd.copy_(torch.from_numpy(frames))
    even = torch.from_numpy(frames).cuda()
    assert odd.is_contiguous() and odd.data_ptr() % 4 == 1 and even.data_ptr() % 4 == 0
    for dev in (odd, even):
        got, _ = device_maps(fd, torch, dev)
        for b in range(2):
            assert_frame(got[b], exp[b], (dev.data_ptr() % 4, b))


def test_saturated_strips(fd, oracle):
    """min_norm = -1 makes every scanned pixel valid, zero gradients included (atan2f(0, -0) = pi): 24x600 frames
    fill k_lsd_map's per-wave angle queue with whole rows of 256 valid columns (strip 0 but its column 0, the
    interior strip 1 completely). Noise, flat and checker; and min_norm = 0 on the noise frame."""
    rows, cols = 24, 600
    assert lsd_columns(cols)[:2] == (3, 1)
    noise = oracle.make_frame("noise", 31, rows, cols)
    flat = np.full((rows, cols), 100, np.uint8)
    en, ea, ev, eidx = oracle.lsd_map(flat, -1.0)
    assert len(eidx) == (rows - 3) * (cols - 3) and int(ev.sum()) == len(eidx)
    assert (ea.reshape(-1)[eidx].view(np.uint32) == np.float32(np.pi).view(np.uint32)).all()
    assert (en == 0).all()
    for img in (noise, flat, oracle.make_frame("checker", 32, rows, cols, 8)):
        idx = check_lsd(fd, oracle, img, -1.0)
        assert len(idx) == (rows - 3) * (cols - 3)
    check_lsd(fd, oracle, noise, 0.0)
