"""GPU: fd_png_frames (host decode threads -> one upload -> colour -> gray on the GPU) equals the host
decoder image by image, feeds detection directly, and the C++ demo's LoadImage path (PNG file in,
as the reference demo at test/test_feature_point_detector.cpp:104) gives the raw-frame results.
The second half holds the colour -> gray kernel to png_util.gray_of of the encoded samples (numpy) at
its arithmetic, pixel-stream and alignment edges, and fd_png_frames to its staging and error contract."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

from png_util import encode_png, gray_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("ch", [1, 2, 3, 4])
def test_png_frames_match_host_decode(ch, oracle):
    import torch

    import feature_detector_amd as fd

    rng = np.random.default_rng(10 + ch)
    imgs = []
    for i in range(5):
        base = oracle.make_frame("checker", 50 + i, 97, 131, 16)
        img = np.stack([np.roll(base, k, axis=1) for k in range(ch)], -1) if ch > 1 else base
        imgs.append(img)
    pngs = [encode_png(x, filters=(i % 5, 4, 1, 3, 2, 0)) for i, x in enumerate(imgs)]
    dev = fd.png_frames(pngs, threads=3)
    torch.cuda.synchronize()
    host = np.stack([fd.load_png(p) for p in pngs])
    assert np.array_equal(dev.cpu().numpy(), host)


def test_png_frames_detect(image_png, oracle):
    import torch

    import feature_detector_amd as fd

    data = open(os.path.join(ROOT, "tests", "golden", "image.png"), "rb").read()
    frames = fd.png_frames([data, data])
    res = fd.detect_points("harris", frames, 200, 20, 30.0)
    torch.cuda.synchronize()
    exp, _ = oracle.detect(0, image_png, 20, 30.0, 200, sort_mode=0)
    assert np.array_equal(res.features(0), exp) and np.array_equal(res.features(1), exp)


def test_demo_loads_png(tmp_path, image_png):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "feature_detector_amd", "api")])
    lib = os.path.join(ROOT, "feature_detector_amd", "lib")
    raw = tmp_path / "f.u8"
    image_png.tofile(raw)
    a = subprocess.run([os.path.join(lib, "fd_demo_points"), str(raw), "480", "752"], capture_output=True, text=True,
                       timeout=300)
    b = subprocess.run([os.path.join(lib, "fd_demo_points"), os.path.join(ROOT, "tests", "golden", "image.png")],
                       capture_output=True, text=True, timeout=300)
    assert a.returncode == 0 and b.returncode == 0, (a.stderr, b.stderr)
    ja = [json.loads(x) for x in a.stdout.splitlines() if x.startswith("{")]
    jb = [json.loads(x) for x in b.stdout.splitlines() if x.startswith("{")]
    assert ja == jb and len(ja) >= 4


@pytest.mark.parametrize("ch", [1, 2, 3, 4])
def test_png_frames_out_unaligned_and_checked(ch, oracle):
    """out= may start at any byte (the converter stores dwords only when both ends are 4-byte aligned,
    so offset 0 takes the packed path and offsets 1 to 3 the byte path for every quad; one channel is
    the plain upload to that address); nothing outside the view is written; a wrong shape, dtype or
    device raises before any work is queued."""
    import torch

    import feature_detector_amd as fd

    imgs = [oracle.make_frame("noise", 70 + i, 33, 50) for i in range(3)]
    if ch > 1:
        imgs = [np.stack([x, np.roll(x, 1, 0), np.roll(x, 2, 1), x[::-1]][:ch], -1) for x in imgs]
    pngs = [encode_png(x) for x in imgs]
    host = np.stack([fd.load_png(p) for p in pngs])
    assert np.array_equal(host, _expect(imgs))
    big = torch.full((host.size + 8,), 0xA5, dtype=torch.uint8, device="cuda")
    for off in (0, 1, 2, 3):
        big.fill_(0xA5)
        out = big[off:off + host.size].view(host.shape)
        fd.png_frames(pngs, out=out)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), host)
        b = big.cpu().numpy()
        assert (b[:off] == 0xA5).all() and (b[off + host.size:] == 0xA5).all()
    for rows, cols, n in ((5, 7, 2), (13, 79, 3)):
        samples = _random_samples(700 + ch, rows, cols, n, ch)
        pngs2 = [encode_png(x) for x in samples]
        exp = _expect(samples)
        big = torch.full((exp.size + 8,), 0xA5, dtype=torch.uint8, device="cuda")
        for off in (0, 1, 2, 3):
            big.fill_(0xA5)
            out = big[off:off + exp.size].view(exp.shape)
            assert out.data_ptr() % 4 == off
            fd.png_frames(pngs2, out=out)
            torch.cuda.synchronize()
            b = big.cpu().numpy()
            assert np.array_equal(b[off:off + exp.size].reshape(exp.shape), exp), (rows, cols, n, off)
            assert (b[:off] == 0xA5).all() and (b[off + exp.size:] == 0xA5).all(), (rows, cols, n, off)
    for bad in (torch.empty((3, 33, 49), dtype=torch.uint8, device="cuda"),
                torch.empty((3, 33, 50), dtype=torch.int32, device="cuda"),
                torch.empty((3, 33, 50), dtype=torch.uint8)):
        with pytest.raises(ValueError):
            fd.png_frames(pngs, out=bad)


# ------------------------------------------------- k_rgb_gray against numpy (png_util.gray_of)
# The expectation of everything below comes from the samples that were encoded, never from the
# library's own decoder. k_rgb_gray<1> is not reachable through fd_png_frames (gray input is uploaded
# straight into the frames), so the one-channel cases check that upload.
def _expect(samples):
    return np.stack([gray_of(x if x.ndim == 3 else x[:, :, None]) for x in map(np.asarray, samples)])


def _random_samples(seed, rows, cols, n, ch):
    """n images [rows, cols, ch], every channel (alpha included) independent uniform random."""
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (rows, cols, ch)).astype(np.uint8) for _ in range(n)]


def _frames_vs_numpy(samples, encode=None, **kw):
    """(fd.png_frames of the encoded samples, gray_of of the samples)."""
    import torch

    import feature_detector_amd as fd

    pngs = [encode_png(x, **(encode[i] if encode else {})) for i, x in enumerate(samples)]
    dev = fd.png_frames(pngs, **kw)
    torch.cuda.synchronize()
    return dev.cpu().numpy(), _expect(samples)


def _weighted(rgb):
    rgb = rgb.astype(np.uint32)
    return 4899 * rgb[..., 0] + 9617 * rgb[..., 1] + 1868 * rgb[..., 2]


@functools.lru_cache(maxsize=None)
def _boundary_triples():
    """From the whole 256^3 cube: 64 (R, G, B) for each residue of the weighted sum mod 2^14 at which
    the rounding decides -- 8191 (the last that rounds down), 8192 (the first that rounds up), 0, 16383."""
    v = np.arange(256, dtype=np.uint32)
    res = ((4899 * v)[:, None, None] + (9617 * v)[None, :, None] + (1868 * v)[None, None, :]) & 16383
    rng = np.random.default_rng(2024)
    out = {}
    for want in (8191, 8192, 0, 16383):
        hits = np.argwhere(res == want)
        assert len(hits) >= 64
        out[want] = hits[rng.choice(len(hits), 64, replace=False)].astype(np.uint8)
    return out


def _arithmetic_pixels(seed, count):
    """`count` RGB pixels: cube corners, single channels at the mid-range and end values, the rounding
    boundaries, the rest uniform random; in a random order, so that they fall on every byte of a quad."""
    rng = np.random.default_rng(seed)
    px = [[r, g, b] for r in (0, 255) for g in (0, 255) for b in (0, 255)]
    for k in range(3):
        for val in (1, 127, 128, 254, 255):
            px.append([val if j == k else 0 for j in range(3)])
    px = np.concatenate([np.array(px, np.uint8)] + [_boundary_triples()[w] for w in (8191, 8192, 0, 16383)])
    assert len(px) == 8 + 15 + 256 and count > len(px)
    px = np.concatenate([px, rng.integers(0, 256, (count - len(px), 3)).astype(np.uint8)])
    return px[rng.permutation(count)]


@pytest.mark.parametrize("ch", [3, 4])
def test_rgb_gray_arithmetic(ch):
    """The 14-bit fixed-point BT.601 rule, bit for bit, on pixels that tell it from its neighbours:
    a truncating shift and the float formula each differ from it on at least 32 pixels of this batch."""
    n, rows, cols = 2, 13, 31
    rgb = _arithmetic_pixels(40 + ch, n * rows * cols)
    s = _weighted(rgb)
    exact = (s + 8192) >> 14
    for want in (8191, 8192, 0, 16383):
        assert np.count_nonzero((s & 16383) == want) >= 64
    assert np.count_nonzero((s >> 14) != exact) >= 32
    as_float = np.rint(0.299 * rgb[:, 0] + 0.587 * rgb[:, 1] + 0.114 * rgb[:, 2])
    assert np.count_nonzero(as_float != exact) >= 32
    swapped = (_weighted(rgb[:, ::-1]) + 8192) >> 14  # R and B weights exchanged
    assert np.count_nonzero(swapped != exact) >= 32
    samples = rgb.reshape(n, rows, cols, 3)
    if ch == 4:
        alpha = np.random.default_rng(44).integers(0, 256, (n, rows, cols, 1)).astype(np.uint8)
        samples = np.concatenate([samples, alpha], -1)
    got, exp = _frames_vs_numpy(list(samples))
    assert np.array_equal(exp.reshape(-1), exact)
    assert np.array_equal(got, exp)


def test_gray_alpha_is_channel_0():
    samples = _random_samples(50, 13, 79, 3, 2)
    got, exp = _frames_vs_numpy(samples)
    assert np.array_equal(exp, np.stack([x[:, :, 0] for x in samples]))
    assert np.array_equal(got, exp)


SEAMS = [(1, 1, 1), (1, 1, 3), (1, 4, 1), (1, 5, 1), (3, 3, 2), (7, 9, 3), (1, 1023, 1), (32, 32, 1), (5, 205, 1),
         (13, 79, 1), (13, 79, 3)]


@pytest.mark.parametrize("ch", [2, 3, 4])
@pytest.mark.parametrize("rows,cols,n", SEAMS)
def test_rgb_gray_pixel_stream_seams(rows, cols, n, ch):
    """The batch is one stream of rows * cols * n pixels, 4 to a lane and 1024 to a block: one pixel,
    a byte tail only (3), one packed quad (4), quad + tail (5), quads across image boundaries (9-pixel
    and 63-pixel images), and 1023 / 1024 / 1025 / 1027 / 3081 pixels around the block edge."""
    got, exp = _frames_vs_numpy(_random_samples(1000 * ch + rows * cols * n, rows, cols, n, ch))
    assert got.shape == (n, rows, cols) and np.array_equal(got, exp)


def test_png_frames_staging_kept_in_context():
    """The pinned and device staging live in the context: reused, grown, reused again, skipped by a
    gray batch; a call waits for the previous call's upload before it decodes into the same pinned
    memory, so two calls without a synchronise between them both give their own images."""
    import torch

    import feature_detector_amd as fd

    ctx = fd.Context()
    first = _random_samples(61, 7, 9, 3, 3)
    for samples in (first, _random_samples(62, 32, 32, 4, 4), first, _random_samples(63, 7, 9, 3, 1),
                    _random_samples(64, 13, 79, 2, 2)):
        got, exp = _frames_vs_numpy(samples, ctx=ctx)
        assert np.array_equal(got, exp)
    a, b = _random_samples(65, 32, 32, 4, 3), _random_samples(66, 32, 32, 4, 3)
    pa, pb = [encode_png(x) for x in a], [encode_png(x) for x in b]
    da = fd.png_frames(pa, ctx=ctx)
    db = fd.png_frames(pb, ctx=ctx)
    torch.cuda.synchronize()
    assert np.array_equal(da.cpu().numpy(), _expect(a)) and np.array_equal(db.cpu().numpy(), _expect(b))
    ctx.close()


def test_png_frames_threads():
    """Any number of decode threads (1, 2, one per image, more than images, 0 = the default) gives the
    same frames, for images that differ in filters and deflate level."""
    samples = _random_samples(67, 13, 79, 5, 3)
    encode = [dict(filters=(0,), level=0), dict(filters=(4, 3), level=1), dict(filters=(1, 2, 3, 4, 0), level=9),
              dict(filters=(2,)), dict(filters=(3, 4, 1, 0, 2), level=6)]
    runs = [_frames_vs_numpy(samples, encode=encode, threads=t) for t in (1, 2, 5, 64, 0)]
    for got, exp in runs:
        assert np.array_equal(got, exp)


def _bad_batch(case):
    """(three PNG streams of which one is bad, the image index the error has to name or None)."""
    good = _random_samples(68, 7, 9, 3, 3)
    pngs = [encode_png(x) for x in good]
    if case == "size":
        pngs[1] = encode_png(_random_samples(69, 7, 10, 1, 3)[0])
    elif case == "channels":
        pngs[1] = encode_png(_random_samples(69, 7, 9, 1, 4)[0])
    elif case == "truncated_file":  # cut inside the IDAT chunk: its length runs past the end
        pngs[1] = pngs[1][:-20]
    elif case == "truncated_zstream":  # well-formed chunks, the deflate stream ends early
        pngs[1] = encode_png(good[1], z_edit=lambda z: z[:len(z) // 2])
    elif case == "filter5":
        pngs[1] = encode_png(good[1], filters=(0, 1, 5))
    elif case == "unsupported_last":
        pngs[2] = encode_png(good[2], interlace=1)
    named = {"size": 1, "channels": 1, "truncated_file": 1, "unsupported_last": 2}.get(case)
    return pngs, named


@pytest.mark.parametrize("case", ["size", "channels", "truncated_file", "truncated_zstream", "filter5",
                                  "unsupported_last"])
def test_png_frames_bad_batch(case):
    """A bad image is refused on the host (header check, or the decode before the upload): FdError with
    a message, `out` as it was, and the context converts the next batch."""
    import torch

    import feature_detector_amd as fd

    ctx = fd.Context()
    pngs, named = _bad_batch(case)
    out = torch.full((3, 7, 9), 0xA5, dtype=torch.uint8, device="cuda")
    with pytest.raises(fd.FdError) as e:
        fd.png_frames(pngs, ctx=ctx, out=out)
    msg = str(e.value).split(":", 1)[1].strip()
    assert msg and e.value.code == 1
    if named is not None:
        assert f"image {named}" in msg
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0xA5).all()
    got, exp = _frames_vs_numpy(_random_samples(70, 7, 9, 3, 3), ctx=ctx, out=out)
    assert np.array_equal(got, exp)
    ctx.close()


def test_png_frames_empty_batch_capi():
    """n = 0 through the C ABI (the binding cannot send it): FD_ERR_INVALID with a message, nothing written."""
    import ctypes

    import torch

    import feature_detector_amd as fd
    from feature_detector_amd import _lib

    ctx = fd.Context()
    samples = _random_samples(71, 7, 9, 2, 3)
    pngs = [encode_png(x) for x in samples]
    out = torch.full((2, 7, 9), 0xA5, dtype=torch.uint8, device="cuda")
    bufs = (ctypes.c_char_p * 2)(*pngs)
    lens = (ctypes.c_size_t * 2)(*[len(x) for x in pngs])
    L = _lib.load()
    rc = L.fd_png_frames(ctx.ptr, ctypes.cast(bufs, ctypes.c_void_p), ctypes.cast(lens, ctypes.c_void_p), 0, 7, 9,
                         ctypes.c_void_p(out.data_ptr()), 0)
    assert rc == _lib.FD_ERR_INVALID and L.fd_last_error(ctx.ptr)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0xA5).all()
    got, exp = _frames_vs_numpy(samples, ctx=ctx, out=out)
    assert np.array_equal(got, exp)
    ctx.close()
