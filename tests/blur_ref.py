"""numpy restatement of fd_frames_blur / fd_pyr_build_gauss as include/fd_hip.h states them: the yardstick of
tests/test_blur_host.py, tests/test_gpu_blur.py and tests/test_cpp_blur.py.

Written unlike the kernel on purpose: whole frames, one gathered plane per tap, everything int64, the reflected
index built from the header's three lines. Nothing here knows about tiles.
"""
import numpy as np

PYR_TAPS = (96, 64, 16)


def reflect_index(i, n):
    """The header's refl(i, n) for an integer array i: 0 if n == 1; else p = 2(n-1), m = ((i mod p) + p) mod p,
    m if m < n else p - m. (C's % truncates towards zero: written with np.fmod so that the + p matters.)"""
    i = np.asarray(i, np.int64)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    m = (np.fmod(i, p) + p) % p
    return np.where(m < n, m, p - m)


def check_taps(taps):
    taps = [int(t) for t in taps]
    assert 1 <= len(taps) <= 16 and all(t >= 0 for t in taps) and taps[0] + 2 * sum(taps[1:]) == 256, taps
    return taps


def blur_ref(frames, taps, step=1):
    """fd_frames_blur of uint8 frames [B, rows, cols] or [rows, cols]: uint8 [.., (rows+step-1)//step, (cols+step-1)//step]."""
    taps = check_taps(taps)
    assert step in (1, 2)
    f = np.asarray(frames)
    assert f.dtype == np.uint8 and f.ndim in (2, 3)
    a = f.astype(np.int64)
    rows, cols = a.shape[-2:]
    r = len(taps) - 1
    xs = np.arange(0, cols, step, dtype=np.int64)  # X = step * x
    ys = np.arange(0, rows, step, dtype=np.int64)  # Y = step * y
    # horizontal pass at every source row, at the sampled columns
    h = taps[0] * a[..., :, reflect_index(xs, cols)]
    for k in range(1, r + 1):
        h = h + taps[k] * (a[..., :, reflect_index(xs - k, cols)] + a[..., :, reflect_index(xs + k, cols)])
    assert h.min() >= 0 and h.max() <= 65280
    v = taps[0] * h[..., reflect_index(ys, rows), :]
    for k in range(1, r + 1):
        v = v + taps[k] * (h[..., reflect_index(ys - k, rows), :] + h[..., reflect_index(ys + k, rows), :])
    assert v.min() >= 0 and v.max() <= 255 << 16
    out = (v + (1 << 15)) >> 16
    assert out.shape[-2:] == ((rows + step - 1) // step, (cols + step - 1) // step)
    return out.astype(np.uint8)


def pyr_gauss_ref(frames, levels):
    """fd_pyr_build_gauss: the list of levels [B, rows >> l, cols >> l] (what flow_ref.track_one and
    flow_ref.pyr_pack take): level 0 the frames, level l+1 the top-left floor-sized block of the blur of level l."""
    a = np.asarray(frames)
    if a.ndim == 2:
        a = a[None]
    out = [np.ascontiguousarray(a)]
    for _ in range(1, levels):
        below = out[-1]
        r, c = below.shape[1] >> 1, below.shape[2] >> 1
        out.append(np.ascontiguousarray(blur_ref(below, PYR_TAPS, 2)[:, :r, :c]))
    return out


def tile_rows(out_rows, out_cols, batch, lead=None):
    """The output rows of a workgroup's tile for a launch (launch_blur of fd_blur.hip): 32, halved down to 8 while
    the launch has fewer than 512 workgroups. lead: bytes a row's dwords may start early (3 unless every row is
    a whole number of dwords from an aligned base)."""
    if lead is None:
        lead = 3 if out_cols % 4 else 0
    chunks = (out_cols + lead + 127) // 128
    t = 32
    while t > 8 and chunks * ((out_rows + t - 1) // t) * min(batch, 65535) < 512:
        t //= 2
    return t
