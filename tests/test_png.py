"""CPU: the PNG front end (fd_png_info / fd_png_decode) against a numpy reference
decoder on encoder-made images (every row filter, every supported colour type), the reference's
examples/image.png fixture and its examples/image2.png (RGB), both kept under tests/golden/.
The colour -> gray conversion of the reference's Visualizor2D::LoadImage is un-vendored: the library's
BT.601 fixed-point rule is checked for self-consistency only (parity unpinned).
The second half feeds the parser and the filters the streams other encoders write (several IDATs, other
chunks, every deflate level, one-column / one-row images, Paeth ties) and the ones they must refuse."""
import os

import numpy as np
import pytest

from png_util import decode_png, encode_png, gray_of


@pytest.mark.parametrize("ch", [1, 2, 3, 4])
def test_roundtrip_all_filters(ch):
    import feature_detector_amd as fd

    rng = np.random.default_rng(ch)
    img = rng.integers(0, 256, (37, 53, ch) if ch > 1 else (37, 53)).astype(np.uint8)
    data = encode_png(img)
    assert fd.png_info(data) == (37, 53, ch)
    got = fd.load_png(data)
    exp = gray_of(img if img.ndim == 3 else img[:, :, None])
    assert np.array_equal(got, exp)


def test_image_png_fixture(image_png):
    import feature_detector_amd as fd

    got = fd.load_png(os.path.join(os.path.dirname(__file__), "golden", "image.png"))
    assert np.array_equal(got, image_png)


def test_reference_image2_rgb():
    import feature_detector_amd as fd

    with open(os.path.join(os.path.dirname(__file__), "golden", "image2.png"), "rb") as f:
        data = f.read()
    assert fd.png_info(data) == (480, 640, 3)
    got = fd.load_png(data)
    assert np.array_equal(got, gray_of(decode_png(data)))


def test_rejects_bad_input():
    import feature_detector_amd as fd

    data = encode_png(np.zeros((8, 8), np.uint8))
    with pytest.raises(fd.FdError):
        fd.load_png(data[:40])  # truncated
    with pytest.raises(fd.FdError):
        fd.load_png(b"not a png at all, not even close")
    bad = bytearray(data)
    bad[8 + 8 + 8] = 16  # IHDR bit depth 16
    with pytest.raises(fd.FdError):
        fd.load_png(bytes(bad))


# ------------------------------------------------------------------ the streams other encoders write
CH = [1, 2, 3, 4]
FD_ERR_INVALID, FD_ERR_CAPACITY = 1, 3


def _samples(seed, rows, cols, ch):
    return np.random.default_rng(seed).integers(0, 256, (rows, cols, ch)).astype(np.uint8)


def _check(data, samples):
    """The library's header and pixels against the numpy decoder and the samples that were encoded."""
    import feature_detector_amd as fd

    assert np.array_equal(decode_png(data), samples)  # the yardstick reads this stream
    assert fd.png_info(data) == samples.shape
    got = fd.load_png(data)
    assert got.dtype == np.uint8 and np.array_equal(got, gray_of(samples))


def _idat_sizes(data):
    pos, sizes = 8, []
    while pos + 12 <= len(data):
        n = int.from_bytes(data[pos:pos + 4], "big")
        if data[pos + 4:pos + 8] == b"IDAT":
            sizes.append(n)
        pos += 12 + n
    return sizes


def _zlen(img, **kw):
    return sum(_idat_sizes(encode_png(img, **kw)))


@pytest.mark.parametrize("ch", CH)
@pytest.mark.parametrize("split", ["middle", "bytes8", "empty_first", "empty_middle", "empty_last"])
def test_idat_concatenation(ch, split):
    """parse(): every IDAT body is appended, a zero-length one included, wherever the stream is cut."""
    img = _samples(100 + ch, 11, 13, ch)
    z = _zlen(img)
    cuts = {"middle": [z // 2], "bytes8": list(range(1, 9)), "empty_first": [0, z // 3],
            "empty_middle": [z // 2, z // 2], "empty_last": [z // 2, z]}[split]
    data = encode_png(img, idat_split=cuts)
    sizes = _idat_sizes(data)
    assert len(sizes) == len(cuts) + 1 and sum(sizes) == z
    if split == "bytes8":
        assert sizes[:8] == [1] * 8
    if split.startswith("empty"):
        assert sizes[{"empty_first": 0, "empty_middle": 1, "empty_last": -1}[split]] == 0
    _check(data, img)


@pytest.mark.parametrize("ch", CH)
@pytest.mark.parametrize("level", [0, 1, 9])
def test_deflate_levels(ch, level):
    """Stored blocks (level 0), the fast and the best compressor: inflate handles all block types."""
    img = _samples(200 + ch, 17, 19, ch)
    img[5:12] = img[4]  # repeated rows, so that levels 1 and 9 emit matches as well as literals
    data = encode_png(img, level=level)
    if level == 0:
        assert _zlen(img, level=0) > img.size + 17  # stored: nothing compressed
    _check(data, img)


@pytest.mark.parametrize("ch", CH)
def test_other_chunks_skipped(ch):
    """Ancillary chunks before and between the IDATs are skipped by their length; nothing after IEND is
    read: not garbage, and not a further IDAT (which would make the stream inflate to too much)."""
    img = _samples(300 + ch, 9, 10, ch)
    z = _zlen(img)
    gama = (b"gAMA", (45455).to_bytes(4, "big"))
    text = (b"tEXt", b"Comment\0IDAT IEND IHDR inside a body are not chunk types")
    _check(encode_png(img, before_idat=[gama, text]), img)
    _check(encode_png(img, idat_split=[z // 2], between_idat=[(b"prVt", bytes(range(37)))]), img)
    extra = encode_png(img[::-1].copy())
    late_idat = extra[extra.index(b"IDAT") - 4:extra.index(b"IEND") - 4]  # a whole, valid IDAT chunk
    trailer = b"\xde\xad\xbe\xef" * 5 + late_idat + b"\x00\x00\x00\x07junk"
    _check(encode_png(img, before_idat=[gama], idat_split=[z // 3], between_idat=[text], after_iend=trailer), img)
    _check(encode_png(img, after_iend=late_idat), img)  # chunk-aligned right after IEND


@pytest.mark.parametrize("ch", CH)
def test_filter_neighbours_outside(ch):
    """One column (a = c = 0 everywhere), one row (b = c = 0), one pixel, and first rows that use the
    filters which read the row above."""
    one_col = _samples(400 + ch, 11, 1, ch)
    _check(encode_png(one_col), one_col)  # row r: filter r % 5, every filter at least twice
    _check(encode_png(one_col, filters=(4, 3, 2, 1, 0)), one_col)
    one_row = _samples(410 + ch, 1, 23, ch)
    for ft in (0, 1, 2, 3, 4):
        _check(encode_png(one_row, filters=(ft,)), one_row)
    for ft in (0, 1, 2, 3, 4):
        px = _samples(420 + ch + ft, 1, 1, ch)
        _check(encode_png(px, filters=(ft,)), px)
    img = _samples(430 + ch, 6, 7, ch)
    _check(encode_png(img, filters=(4, 3, 1)), img)  # Paeth first
    _check(encode_png(img, filters=(3, 4, 2)), img)  # Average first


def _paeth_cases(samples):
    """(pa, pb, pc) of every byte of an all-Paeth image, as the spec defines them (Python integers)."""
    rows, cols, ch = samples.shape
    s = samples.tolist()
    at = lambda r, c, k: s[r][c][k] if r >= 0 and c >= 0 else 0
    out = []
    for r in range(rows):
        for c in range(cols):
            for k in range(ch):
                a, b, cc = at(r, c - 1, k), at(r - 1, c, k), at(r - 1, c - 1, k)
                p = a + b - cc
                out.append((abs(p - a), abs(p - b), abs(p - cc), a, b, cc))
    return out


@pytest.mark.parametrize("ch", CH)
def test_paeth_tie_orders(ch):
    """Paeth's tie-breaking order (a, then b, then c). In this 2 x 3 image the byte at (1, 1) has
    pb == pc < pa with b != c (b must win), the one at (1, 2) has pa == pb > pc (c must win, although
    pa <= pb holds), and (0, 0) has all three equal."""
    gray = np.array([[20, 40, 30], [10, 50, 77]], np.uint8)
    img = np.stack([gray + 3 * k for k in range(ch)], -1).astype(np.uint8)
    cases = _paeth_cases(img)
    assert any(pb == pc < pa and b != c for pa, pb, pc, a, b, c in cases)
    assert any(pa == pb > pc and a != b for pa, pb, pc, a, b, c in cases)
    assert any(pa == pb == pc for pa, pb, pc, a, b, c in cases)
    _check(encode_png(img, filters=(4,)), img)


def _decode_capi(data, cap, room):
    """fd_png_decode into a 0xA5-filled buffer of `room` bytes: (rc, rows, cols, buffer)."""
    import ctypes

    from feature_detector_amd import _lib

    buf = np.full(room, 0xA5, np.uint8)
    r, c = ctypes.c_int32(-1), ctypes.c_int32(-1)
    rc = _lib.load().fd_png_decode(data, len(data), ctypes.c_void_p(buf.ctypes.data), cap, ctypes.byref(r),
                                   ctypes.byref(c))
    return rc, r.value, c.value, buf


def _patch_len(data, tag, value):
    at = data.index(tag) - 4
    return data[:at] + value.to_bytes(4, "big") + data[at + 4:]


def _flip(z, at):
    return z[:at] + bytes([z[at] ^ 0x5A]) + z[at + 1:]


REJECTED = {
    "depth16": lambda img: encode_png(img, bit_depth=16),
    "depth4": lambda img: encode_png(img, bit_depth=4),
    "palette": lambda img: encode_png(img, ctype=3),
    "interlaced": lambda img: encode_png(img, interlace=1),
    "rows0": lambda img: encode_png(img, rows=0),
    "cols0": lambda img: encode_png(img, cols=0),
    "no_ihdr": lambda img: encode_png(img, ihdr=False),
    "chunk_past_end": lambda img: _patch_len(encode_png(img), b"IDAT", len(encode_png(img))),
    "chunk_past_end_by_one": lambda img: _patch_len(encode_png(img)[:-12], b"IDAT", _zlen(img) + 1),
    "chunk_len_max": lambda img: _patch_len(encode_png(img), b"IDAT", 0xFFFFFFFF),
    "zstream_half": lambda img: encode_png(img, z_edit=lambda z: z[:len(z) // 2]),
    "zstream_no_checksum": lambda img: encode_png(img, z_edit=lambda z: z[:-4]),  # all pixels out, no end
    "one_byte_few": lambda img: encode_png(img, raw_edit=lambda r: r[:-1]),
    "one_byte_many": lambda img: encode_png(img, raw_edit=lambda r: r + b"\0"),
    "filter5_last_row": lambda img: encode_png(img, filters=(0, 1, 2, 3, 4, 1, 5)),
    "zstream_corrupt_stored": lambda img: encode_png(img, level=0, z_edit=lambda z: _flip(z, len(z) // 2)),
    "zstream_corrupt_deflated": lambda img: encode_png(img, z_edit=lambda z: _flip(z, len(z) // 2)),
    "zstream_corrupt_checksum": lambda img: encode_png(img, z_edit=lambda z: _flip(z, len(z) - 1)),
}


@pytest.mark.parametrize("ch", CH)
@pytest.mark.parametrize("case", sorted(REJECTED))
def test_rejections(case, ch):
    """Each is refused by load_png with FdError and by fd_png_decode with a non-zero code, and the
    caller's buffer is as it was (a 7-row image, so that the last row is the one with filter byte 5)."""
    import feature_detector_amd as fd

    img = _samples(500 + ch, 7, 9, ch)
    _check(encode_png(img), img)  # the unbroken stream decodes
    data = REJECTED[case](img)
    with pytest.raises(fd.FdError):
        fd.load_png(data)
    npx = img.shape[0] * img.shape[1]
    rc, _, _, buf = _decode_capi(data, npx, npx + 16)
    assert rc in (FD_ERR_INVALID, FD_ERR_CAPACITY) and rc != 0
    assert (buf == 0xA5).all()
    if case in ("depth16", "depth4", "palette", "interlaced", "rows0", "cols0", "no_ihdr") or case.startswith("chunk"):
        with pytest.raises(fd.FdError):  # the header alone is enough to refuse these
            fd.png_info(data)


@pytest.mark.parametrize("ch", CH)
def test_decode_short_capacity(ch):
    """fd_png_decode with room for one pixel less than the image: FD_ERR_CAPACITY, the geometry still
    reported, nothing written at or after `cap`; with cap == npx it decodes and leaves the guard."""
    img = _samples(600 + ch, 7, 9, ch)
    data = encode_png(img)
    npx = 63
    rc, rows, cols, buf = _decode_capi(data, npx - 1, npx + 8)
    assert rc == FD_ERR_CAPACITY and (rows, cols) == (7, 9)
    assert (buf[npx - 1:] == 0xA5).all()
    rc, rows, cols, buf = _decode_capi(data, npx, npx + 8)
    assert rc == 0 and (rows, cols) == (7, 9)
    assert np.array_equal(buf[:npx].reshape(7, 9), gray_of(img)) and (buf[npx:] == 0xA5).all()
