"""GPU: k_nn_desc (fd_nn_descriptors) at its edges, against the CPU oracle's ExtractDescriptorsForSelectedFeatures
(nn_feature_point_detector.cpp:163-193, the reference's own code, which takes any channel count).

Bar: every output float equal as a bit pattern, through the C ABI into a sentinel-guarded buffer, on host and
on device pointers, for both map layouts; every slot at or past a frame's count keeps the sentinel.
Covered: channel counts on both sides of the wave's 64 lanes (the lane loop's ragged trips); maps whose inside
is one cell or empty; keypoints exactly on, and one float inside, the excluded last row and column; the
reference's quirk for -8 < x < 0 (the cell index truncates to 0, so the keypoint is inside, while the weights
come from floor); count words with flag bits, a zero count inside a batch, a count above the stride.
"""
import ctypes

import numpy as np
import pytest

from unaligned import GUARD

pytestmark = pytest.mark.gpu

F32 = np.float32
SENT = F32(-123.25)
CHANNELS = [1, 8, 63, 64, 65, 128, 200, 256, 320]  # under a wave, a wave, one past, ragged second to fifth trips
MAPS = [(2, 2), (1, 5), (5, 1), (3, 4)]            # (rows, cols): one inside cell, none, none, 2 x 3 inside cells
FLAGS = (1 << 25) | (1 << 27) | (1 << 31)


@pytest.fixture(scope="module")
def fd():
    import feature_detector_amd as fd

    fd.load()
    return fd


def axis_positions(cells):
    """Pixel coordinates along an axis of `cells` map cells: the inside is [0, 8 * (cells - 1))."""
    edge = F32(8 * (cells - 1))
    v = [edge, np.nextafter(edge, F32(-np.inf)), edge + F32(0.5)]                  # on the excluded boundary, one float inside, past it
    v += [F32(8 * i) for i in range(cells + 1)]                                    # exact multiples of 8
    v += [F32(0.0), F32(-0.0), F32(-8.0), np.nextafter(F32(-8.0), F32(np.inf)), F32(-0.5), F32(-7.999)]  # truncation against floor
    v += [F32(3.25), F32(4.0) * F32(cells) - F32(0.7), F32(-8.5), F32(1e6), F32(-1e6)]
    return np.array(v, F32)


def keypoints(rows, cols):
    """[2, S, 2]: every x of the list with every y; frame 1 holds them in another order."""
    xs, ys = axis_positions(cols), axis_positions(rows)
    xy = np.stack(np.meshgrid(xs, ys, indexing="ij"), -1).reshape(-1, 2).astype(F32)
    assert np.isfinite(xy).all() and np.abs(xy).max() <= 1e6
    return np.stack([xy, xy[np.random.default_rng(rows * 8 + cols).permutation(len(xy))]])


def word(n):
    return int(np.array([n | FLAGS], np.uint32).view(np.int32)[0])


def expected(oracle, m, xy, counts):
    B, S, C = xy.shape[0], xy.shape[1], m.shape[1]
    exp = np.full((B, S, C), SENT, F32)
    for b in range(B):
        n = min(int(np.uint32(np.int32(counts[b])) & np.uint32(0x01FFFFFF)), S)
        exp[b, :n] = oracle.nn_descriptors(m[b], xy[b, :n])
    return exp


def call(fd, m, nhwc, xy, counts, device):
    """fd_nn_descriptors through the C ABI, out between guards. m is [B, C, h, w]; with nhwc the library is
    handed the same values as [B, h, w, C]. Returns out [B, S, C] as numpy, unwritten slots sentinel."""
    L, ctx = fd.load(), fd.default_context()
    B, C, h, w = m.shape
    S = xy.shape[1]
    mm = np.ascontiguousarray(m.transpose(0, 2, 3, 1)) if nhwc else np.ascontiguousarray(m)
    cnt = np.ascontiguousarray(counts, np.int32)
    out = np.full(B * S * C + 2 * GUARD, SENT, F32)
    if device:
        import torch

        ctx.set_stream(torch.cuda.current_stream(ctx.device).cuda_stream)
        dm, dxy, dcnt, dout = (torch.from_numpy(a).cuda() for a in (mm, np.ascontiguousarray(xy), cnt, out))
        rc = L.fd_nn_descriptors(ctx.ptr, ctypes.c_void_p(dm.data_ptr()), 1, int(nhwc), B, C, h, w, ctypes.c_void_p(dxy.data_ptr()),
                                 ctypes.c_void_p(dcnt.data_ptr()), S, ctypes.c_void_p(dout.data_ptr() + 4 * GUARD), 1)
        assert rc == 0, L.fd_last_error(ctx.ptr)
        torch.cuda.synchronize()
        out = dout.cpu().numpy()
    else:
        ctx.set_stream(None)
        xy = np.ascontiguousarray(xy)
        rc = L.fd_nn_descriptors(ctx.ptr, ctypes.c_void_p(mm.ctypes.data), 0, int(nhwc), B, C, h, w, ctypes.c_void_p(xy.ctypes.data),
                                 ctypes.c_void_p(cnt.ctypes.data), S, ctypes.c_void_p(out.ctypes.data + 4 * GUARD), 0)
        assert rc == 0, L.fd_last_error(ctx.ptr)
    assert np.all(out[:GUARD] == SENT) and np.all(out[-GUARD:] == SENT), "a write outside the output"
    return out[GUARD:-GUARD].reshape(B, S, C)


@pytest.mark.parametrize("rows,cols", MAPS)
@pytest.mark.parametrize("channels", CHANNELS)
def test_channels_maps_and_boundary_keypoints(fd, oracle, channels, rows, cols):
    rng = np.random.default_rng(channels * 100 + rows * 10 + cols)
    m = rng.standard_normal((2, channels, rows, cols)).astype(F32)
    m[m == 0] = 1
    xy = keypoints(rows, cols)
    S = xy.shape[1]
    full = expected(oracle, m, xy, [S, S])
    # what the keypoints reach, by the oracle (frame 0, whose order is the list's)
    x, y = xy[0, :, 0], xy[0, :, 1]
    nz = (full[0] != 0).all(axis=1)
    assert ((full[0] != 0).any(axis=1) == nz).all()  # a descriptor is zero in every channel or in none
    if rows == 1 or cols == 1:
        assert not full.any()  # no cell is inside
    else:
        ex, ey = F32(8 * (cols - 1)), F32(8 * (rows - 1))
        assert not nz[(x == ex) | (y == ey)].any()                                   # on the excluded boundary
        assert nz[(x == np.nextafter(ex, F32(-np.inf))) & (y == np.nextafter(ey, F32(-np.inf)))].all()  # one float inside it
        quirk = (x > -8) & (x < 0) & (y > -8) & (y < 0)
        assert quirk.sum() >= 9 and nz[quirk].all()                                  # truncation: "inside" at cell (0, 0)
        assert nz[(x == F32(-0.5)) & (y == F32(3.25))].all() and nz[(x == 0) & (y == 0)].all()
        assert not nz[(x <= -8) | (y <= -8)].any() and 0 < nz.sum() < S
    for counts in ([word(S - 3), S + 9], [0, word(S)]):
        exp = expected(oracle, m, xy, counts)
        assert np.array_equal(exp[1].view(np.uint32), full[1].view(np.uint32))  # frame 1 is whole in both
        for nhwc in (False, True):
            for device in (False, True):
                got = call(fd, m, nhwc, xy, counts, device)
                assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)), (counts, nhwc, device)
