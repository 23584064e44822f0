"""fd_frames_warp and fd_frames_equalize where a workgroup serves more than one frame, and k_eq_lut where a lane
serves more than one dword of a tile row; every byte against tests/warp_ref.py / tests/equalize_ref.py.

k_warp, k_eq_lut and k_eq_apply walk the batch as `for (b = blockIdx.y; b < batch; b += gridDim.y)` with
gridDim.y = min(batch, 65535), so the loop repeats only past 65535 frames: here 65535 + 9 frames, tiny ones. Frame
b is distinct frame b % 7 and parameter set b is set b % 7, so the expected batch is the 7 reference outputs tiled;
65535 % 7 == 1, so the two frames one workgroup serves (b and b + 65535) differ. k_eq_lut's second pass re-zeroes
the per-wave histograms and runs the workgroup scans again, k_eq_apply's re-stages the packed LUT cells in LDS.

k_eq_lut's tile-row loop `for (k = l; k < nd; k += group)` has at most 2^8 lanes per tile row: it repeats from 257
dwords per tile row, i.e. tiles of 1100 and 1150 columns here (the widest elsewhere in the suite: 256 columns)."""
import numpy as np
import pytest

import equalize_ref as R
import warp_ref as W
from test_gpu_warp import HOMOGRAPHIES

pytestmark = pytest.mark.gpu

GRID_Y = 65535           # the launches' gridDim.y limit
BATCH = GRID_Y + 9
PERIOD = 7
WHICH = np.arange(BATCH) % PERIOD
assert GRID_Y % PERIOD != 0  # frames b and b + 65535 are different frames with different parameters
SENTINEL = 0xA5

# ---- warp: source 5 x 7, destination 3 x 7 (a 7-byte row pitch: the row starts take all four alignments)
SRC, DST = (5, 7), (3, 7)
WARP_FRAMES = np.random.default_rng(65).integers(0, 256, (PERIOD,) + SRC, dtype=np.uint8)
# the homographies of tests/test_gpu_warp.py (37 x 53 frames) between this destination and this source:
# destination -> their destination (U), their source -> this source (D)
_U = np.diag([52 / (DST[1] - 1), 36 / (DST[0] - 1), 1.0])
_D = np.diag([(SRC[1] - 1) / 52, (SRC[0] - 1) / 36, 1.0])
HS = np.stack([(_D @ HOMOGRAPHIES[n].reshape(3, 3) @ _U).reshape(9) for n in (
    "identity", "negated identity", "integer shift", "half pixel", "rotation 30 scale 1.3", "perspective, W changes sign",
    "W zero on row 2")])
W_SIGN = 5  # the set whose W changes sign inside the destination


def _camera(dist, cx):
    K = np.array([[6.0, 0, 3.0], [0, 6.5, 2.0], [0, 0, 1.0]])
    nK = np.array([[5.5, 0, cx], [0, 6.0, 1.0], [0, 0, 1.0]])
    return W.camera_params_ref(nK, K, dist)


CS = np.stack([_camera(d, cx) for d, cx in (
    ([0, 0, 0, 0, 0], 3.0), ([-0.3, 0.1, 0, 0, 0], 3.0), ([0.2, 0, 0, 0, 0], 2.5), ([0.05, 0, 0.02, -0.015, 0], 3.5),
    ([-0.2, 0.05, 0, 0, 0.4], 1.0), ([-0.1, 0.02, 0.001, 0.002, 0], 5.0), ([0.4, 0, 0, 0, 0], -2.0))])
MODELS = {"homography": (W.HOMOGRAPHY, HS), "camera": (W.CAMERA, CS)}

# ---- equalize: frames 8 x 12, tiles (3, 2): one flat, one low-contrast, five noise
EQ_FRAMES = np.random.default_rng(66).integers(0, 256, (PERIOD, 8, 12), dtype=np.uint8)
EQ_FRAMES[0] = 93
EQ_FRAMES[1] = (EQ_FRAMES[1] >> 4) + 120
EQ_TILES = (3, 2)


@pytest.fixture(scope="module")
def fd():
    import feature_detector_amd as fd

    fd.load()
    return fd


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def warp_expected():
    """(out, mask) [7, 3, 7] per (model, shared): computed once, never written to."""
    exp = {}
    for model, (kind, params) in MODELS.items():
        exp[model, False] = W.warp_ref(WARP_FRAMES, params, DST, kind, fill=77)
        exp[model, True] = W.warp_ref(WARP_FRAMES, params[4], DST, kind, fill=77)
        for e in exp[model, False] + exp[model, True]:
            e.setflags(write=False)
    return exp


@pytest.fixture(scope="module")
def eq_expected():
    exp = {clip: R.equalize_ref(EQ_FRAMES, EQ_TILES, clip) for clip in (0, 3000)}
    for e in exp.values():
        e.setflags(write=False)
    return exp


def same(got, exp, what=""):
    """Every byte of the batch against the 7 expected frames tiled (or against exp as it is, if it has the batch's
    length)."""
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    if len(exp) != len(got):
        exp = exp[np.arange(len(got)) % PERIOD]
    assert got.shape == exp.shape and got.dtype == np.uint8, (what, got.shape, exp.shape)
    bad = np.argwhere(got != exp)
    assert len(bad) == 0, (what, len(bad), bad[:5].tolist(), got[tuple(bad[0])], exp[tuple(bad[0])])


def pairwise_different(frames):
    return all(not np.array_equal(frames[i], frames[j]) for i in range(len(frames)) for j in range(i))


def sentinel_views(torch, shape, offs):
    """One view of `shape` per offset, `off` bytes past a dword inside its own sentinel-filled buffer."""
    n = int(np.prod(shape))
    bufs = [torch.full((n + 16,), SENTINEL, dtype=torch.uint8, device="cuda") for _ in offs]
    views = [b[4 + o:4 + o + n].view(shape) for b, o in zip(bufs, offs)]
    assert all(v.data_ptr() % 4 == o for v, o in zip(views, offs))
    return bufs, views


def outside_untouched(torch, buf, off, n):
    rest = torch.cat([buf[:4 + off], buf[4 + off + n:]]).cpu().numpy()
    assert (rest == SENTINEL).all()


# ------------------------------------------------------------------------------------------------ warp

def test_warp_expected_outputs_tell_the_frames_apart(warp_expected):
    """The yardstick's side: 7 pairwise different outputs per case, masks neither all 0 nor all 1, and the
    perspective set's W changes sign inside the destination."""
    for (model, shared), (out, mask) in warp_expected.items():
        assert pairwise_different(out), (model, shared)
        assert mask.any() and not mask.all(), (model, shared)
    x, y = np.meshgrid(np.arange(DST[1]), np.arange(DST[0]))
    w = HS[W_SIGN][6] * x + HS[W_SIGN][7] * y + HS[W_SIGN][8]
    assert (w > 0).any() and (w < 0).any()
    assert BATCH > GRID_Y and WHICH[0] != WHICH[GRID_Y]


@pytest.mark.parametrize("shared", (False, True), ids=("per_frame", "shared"))
@pytest.mark.parametrize("with_mask", (True, False), ids=("mask", "no_mask"))
@pytest.mark.parametrize("model", ("homography", "camera"))
def test_warp_past_65535_frames(fd, torch, warp_expected, model, with_mask, shared):
    kind, params = MODELS[model]
    frames = torch.from_numpy(WARP_FRAMES[WHICH]).cuda()
    p = torch.from_numpy(np.ascontiguousarray(params[4] if shared else params[WHICH])).cuda()
    out = torch.full((BATCH,) + DST, SENTINEL, dtype=torch.uint8, device="cuda")
    mask = torch.full((BATCH,) + DST, SENTINEL, dtype=torch.uint8, device="cuda")
    exp = warp_expected[model, shared]
    if with_mask:
        fd.warp_frames(frames, p, DST, model, 77, return_mask=True, out=(out, mask))
        same(mask, exp[1], (model, shared, "mask"))
    else:
        fd.warp_frames(frames, p, DST, model, 77, out=out)
        assert (mask.cpu().numpy() == SENTINEL).all()
    same(out, exp[0], (model, shared, "out"))


@pytest.mark.parametrize("off", (1, 2, 3))
def test_warp_past_65535_frames_unaligned_outputs(fd, torch, warp_expected, off):
    """out and out_mask at bases that are no multiple of 4 (each its own) inside sentinel buffers."""
    n = BATCH * DST[0] * DST[1]
    moff = off % 3 + 1
    bufs, (out, mask) = sentinel_views(torch, (BATCH,) + DST, (off, moff))
    frames = torch.from_numpy(WARP_FRAMES[WHICH]).cuda()
    p = torch.from_numpy(np.ascontiguousarray(HS[WHICH])).cuda()
    got = fd.warp_frames(frames, p, DST, "homography", 77, return_mask=True, out=(out, mask))
    assert got[0].data_ptr() == out.data_ptr() and got[1].data_ptr() == mask.data_ptr()
    exp = warp_expected["homography", False]
    same(out, exp[0], (off, "out"))
    same(mask, exp[1], (off, "mask"))
    outside_untouched(torch, bufs[0], off, n)
    outside_untouched(torch, bufs[1], moff, n)


# -------------------------------------------------------------------------------------------- equalize

def test_equalize_expected_outputs_tell_the_frames_apart(eq_expected):
    for clip, exp in eq_expected.items():
        assert pairwise_different(exp), clip
    assert (EQ_FRAMES[0] == EQ_FRAMES[0, 0, 0]).all() and int(EQ_FRAMES[1].max()) - int(EQ_FRAMES[1].min()) < 16


@pytest.mark.parametrize("clip", (3.0, 0.0))
def test_equalize_past_65535_frames(fd, torch, eq_expected, clip):
    frames = torch.from_numpy(EQ_FRAMES[WHICH]).cuda()
    out = torch.full(tuple(frames.shape), SENTINEL, dtype=torch.uint8, device="cuda")
    assert fd.equalize_frames(frames, EQ_TILES, clip, out=out) is out
    same(out, eq_expected[int(clip * 1000)], clip)
    same(frames, EQ_FRAMES, "the frames stayed")


def test_equalize_past_65535_frames_in_place(fd, torch, eq_expected):
    frames = torch.from_numpy(EQ_FRAMES[WHICH]).cuda()
    assert fd.equalize_frames(frames, EQ_TILES, 3.0, out=frames) is frames
    same(frames, eq_expected[3000])


@pytest.mark.parametrize("off", (1, 2, 3))
def test_equalize_past_65535_frames_unaligned_bases(fd, torch, eq_expected, off):
    """frames and out `off` and `off + 1` bytes past a dword inside sentinel buffers."""
    shape = (BATCH,) + EQ_FRAMES.shape[1:]
    n = int(np.prod(shape))
    ooff = (off + 1) % 4
    bufs, (frames, out) = sentinel_views(torch, shape, (off, ooff))
    frames.copy_(torch.from_numpy(EQ_FRAMES[WHICH]))
    got = fd.equalize_frames(frames, EQ_TILES, 3.0, out=out)
    assert got.data_ptr() == out.data_ptr()
    same(out, eq_expected[3000], off)
    same(frames, EQ_FRAMES, "the frames stayed")
    outside_untouched(torch, bufs[0], off, n)
    outside_untouched(torch, bufs[1], ooff, n)


# --------------------------------------------------------------- equalize: tile rows of more than 256 dwords

def wide_frames(rows, cols):
    """Two frames: noise with a long flat run in every row (dwords of four equal bytes: one add of 4) that starts
    and ends off a dword, and plain noise."""
    fr = np.random.default_rng(rows * 10000 + cols).integers(0, 256, (2, rows, cols), dtype=np.uint8)
    fr[0, :, 301:1063] = 148  # across the 256-dword step of the loop (column 1024) in both shapes' first tile
    return fr


@pytest.mark.parametrize("off", (0, 1, 2, 3))
@pytest.mark.parametrize("clip_milli", (0, 3000))
@pytest.mark.parametrize("shape,tiles", (((3, 1100), (1, 1)), ((2, 2300), (2, 1))))
def test_equalize_tile_rows_past_256_dwords(fd, torch, shape, tiles, clip_milli, off):
    rows, cols = shape
    tile_w = cols // tiles[0]
    assert (tile_w + 3) // 4 > 256 and rows // tiles[1] < 4  # two steps of the k loop; fewer rows than sub-groups
    host = wide_frames(rows, cols)
    exp = R.equalize_ref(host, tiles, clip_milli)
    assert pairwise_different(exp)
    if tiles == (1, 1) and clip_milli == 0:  # written independently: cumsum of bincount
        for f, e in zip(host, exp):
            cdf = np.cumsum(np.bincount(f.reshape(-1), minlength=256))
            assert np.array_equal(e, ((cdf * 255 + f.size // 2) // f.size).astype(np.uint8)[f])
    bufs, (frames, out) = sentinel_views(torch, host.shape, (off, off))
    frames.copy_(torch.from_numpy(host))
    got = fd.equalize_frames(frames, tiles, clip_milli / 1000.0, out=out)
    assert got.data_ptr() == out.data_ptr()
    same(out, exp, (shape, tiles, clip_milli, off))
    same(frames, host, "the frames stayed")
    outside_untouched(torch, bufs[1], off, host.size)
