"""GPU: FAST's redo pass (FRAME_REDETECTED) with more frames than its loops take at once.

A frame whose selection runs out of emitted keys with candidates left below the adaptive emission cut is detected
and selected again in the same call. Both kernels of that pass loop over frames:
  * k_fast's redo branch (fd_points.hip) is launched with one frame's workgroups and walks the flagged frames of
    the whole batch, 64 flags per load and ballot;
  * k_select_redo (fd_select.hip) is launched with G = min(batch, 8) workgroups; workgroup w owns frames w, w + G,
    ..., 64 of them per ballot round (64 * G frames), and selects each flagged one through the same SelectLds.
tests/test_gpu_fast_cut.py redetects in batches of 3 and 4, so no workgroup selects two frames, G never falls below
the batch and neither ballot loop reaches its second round. Here the batches are 12, 70 and 520 frames.

Every frame of every call equals the oracle's SelectGoodFeatures (stable raster order, sort_mode 1) bit for bit.
The batches repeat 5 noise frames and up to 5 sparse frames; the oracle runs once per distinct frame.

The shape: the proposed cut keeps max(4 V, V + 4096) emitted keys, V = the keys down to the lowest level-0 bin the
scan gathered, which is up to one chunk of 2048 keys however small `need` is; so a cut exists only once a noise
frame has more than about 8192 FAST candidates (~19 % of the pixels on uniform noise), not 4096. Measured on the
MI355X with need 50 at distance 2, every case below at each shape: 120 x 160 (~3,100 candidates), 144 x 192
(~4,500), 160 x 208, 168 x 224, 180 x 240 (~7,200) and 192 x 256 redetect nothing (the sparse frames come out
complete at the first pass); 200 x 264 (~8,700 candidates), 208 x 280, 216 x 288 and 240 x 320 redetect every
sparse frame of every case and no noise frame. The shape is the smallest of these, 200 x 264: 4 of 4, 12 of 12,
2 of 2, 3 of 3 and 5 of 5 sparse frames redetected in the batches of 12, 12, 12 (priors), 70 and 520.
The sparse frames are flat but for a band of low-contrast noise in their top 24 rows: 24 to 33 candidates with
responses from 10.0 up (the cut lies near 10.3), fewer than `need` features, so their scan runs out with
candidates below the cut."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

THR = 10.0
ROWS, COLS = 200, 264
NEED, DIST = 50, 2
BAND, AMP = 24, 38
N_NOISE = N_SPARSE = 5
SELECT_GROUPS = 8  # k_select_redo's workgroups (launch_select, fd_select.hip)
WAVE = 64


@pytest.fixture(scope="module")
def fd():
    import feature_detector_amd as fd

    fd.load()
    return fd


def sparse_frame(rows, cols, seed):
    """Flat, with low-contrast noise in the top rows: a few weak FAST corners with the smallest running offsets."""
    img = np.full((rows, cols), 90, np.uint8)
    img[:BAND] = 90 + np.random.default_rng(seed).integers(0, AMP, (BAND, cols))
    return img


def priors(oracle, frames, dist, need):
    """Prior features (the same list for every frame): the first features of two sparse frames themselves, and a
    few points over the band and below it. Fewer than `need`, which counts them."""
    own = [oracle.detect(2, frames["s", i], dist, THR, need, None, sort_mode=1)[0][:4] for i in (0, 1)]
    rows, cols = frames["s", 0].shape
    grid = np.array([(x, y) for x in range(11, cols, cols // 3) for y in (9, rows // 2)], np.float32)
    return np.concatenate(own + [grid])


class World:
    """The distinct frames of a shape and the oracle's features per distinct frame, with and without priors."""

    def __init__(self, oracle, rows=ROWS, cols=COLS, need=NEED, dist=DIST):
        self.oracle, self.rows, self.cols, self.need, self.dist = oracle, rows, cols, need, dist
        self.frames = {("n", i): oracle.make_frame("noise", 3300 + i, rows, cols) for i in range(N_NOISE)}
        self.frames.update({("s", i): sparse_frame(rows, cols, 100 + i) for i in range(N_SPARSE)})
        self.prior = priors(oracle, self.frames, dist, need)
        self.cache = {}
        for a in self.frames.values():
            a.setflags(write=False)

    def expected(self, key, with_prior):
        if (key, with_prior) not in self.cache:
            self.cache[key, with_prior] = self.oracle.detect(2, self.frames[key], self.dist, THR, self.need,
                                                             self.prior if with_prior else None, sort_mode=1)[0]
        return self.cache[key, with_prior]

    def batch(self, n, sparse_at=()):
        """The keys of a batch of n frames: noise frame b % 5, but at sparse_at the sparse frames in turn."""
        order = sorted(sparse_at)
        return [("s", order.index(b) % N_SPARSE) if b in sparse_at else ("n", b % N_NOISE) for b in range(n)]


@pytest.fixture(scope="module")
def world(oracle):
    return World(oracle)


def check_call(fd, w, keys, feats, flags, with_prior, what):
    """One call's features and flags against the oracle and the keys' kinds; the number of redetected frames."""
    flags = np.asarray(flags).astype(np.uint32)
    assert not (flags & np.uint32(fd.points.FRAME_GUARD)).any(), (what, [hex(int(f)) for f in flags])
    redetected = (flags & np.uint32(fd.points.FRAME_REDETECTED)) != 0
    for b, key in enumerate(keys):
        assert np.array_equal(feats(b), w.expected(key, with_prior)), (what, b, key)
        assert bool(redetected[b]) == (key[0] == "s"), (what, b, key, hex(int(flags[b])))
    return int(redetected.sum())


def run_case(fd, w, batch, sparse_at, with_prior=False, device=False):
    """Settle the cut on the noise batch, redo the sparse frames in one call of the same shape and batch, then the
    noise batch again. Returns the number of frames the sparse call redetected."""
    sparse_at = set(sparse_at)
    noise_keys, mixed_keys = w.batch(batch), w.batch(batch, sparse_at)
    # the case's own conditions, on the CPU
    G = min(batch, SELECT_GROUPS)
    for key in set(mixed_keys):
        if key[0] == "s":
            assert 0 < len(w.expected(key, with_prior)) < w.need, key  # a redo that returns nothing cannot pass
    for b in sparse_at:
        for c in sparse_at:
            if b < c and b % G == c % G:  # one workgroup of k_select_redo, one after the other
                assert mixed_keys[b] != mixed_keys[c]
                assert not np.array_equal(w.expected(mixed_keys[b], with_prior), w.expected(mixed_keys[c], with_prior)), (b, c)
    prior = [w.prior] * batch if with_prior else None
    noise = np.stack([w.frames[k] for k in noise_keys])
    mixed = np.stack([w.frames[k] for k in mixed_keys])
    ctx = fd.Context(0)
    try:
        if device:
            import torch

            noise, mixed = torch.from_numpy(noise).cuda(), torch.from_numpy(mixed).cuda()
            out = (torch.empty((batch, w.need + 1, 2), dtype=torch.float32, device="cuda"),
                   torch.empty((batch,), dtype=torch.int32, device="cuda"), torch.empty((batch,), dtype=torch.int32, device="cuda"))

        def call(frames, keys, what):
            if device:
                for t in out:
                    t.zero_()
                fd.detect_points("fast", frames, w.need, w.dist, THR, prior=prior, ctx=ctx, ties="raster", out=out)
                torch.cuda.synchronize()
                xy, cnt, st = (t.cpu().numpy() for t in out)
                return check_call(fd, w, keys, lambda b: xy[b, :int(cnt[b])], st, with_prior, what)
            res = fd.detect_points("fast", frames, w.need, w.dist, THR, prior=prior, ctx=ctx, ties="raster")
            return check_call(fd, w, keys, res.features, res.frame_flags(), with_prior, what)

        for i in range(3):  # the cut settles on the noise statistics
            assert call(noise, noise_keys, f"settle {i}") == 0
        n = call(mixed, mixed_keys, "redo")
        assert call(noise, noise_keys, "after") == 0
    finally:
        ctx.close()
    print(f"redo: {w.rows}x{w.cols} need {w.need} distance {w.dist} batch {batch}: {n} of {len(sparse_at)} sparse frames redetected")
    assert n == len(sparse_at)
    return n


def test_sparse_frames_are_what_they_claim(world):
    """The yardstick's side: the sparse frames are pairwise different, each has features, fewer than `need`, and
    the priors take some of them away."""
    exp = [world.expected(("s", i), False) for i in range(N_SPARSE)]
    assert all(0 < len(e) < NEED for e in exp)
    assert all(not np.array_equal(exp[i], exp[j]) for i in range(N_SPARSE) for j in range(i))
    assert any(not np.array_equal(world.expected(("s", i), True), exp[i]) for i in range(2))
    assert all(len(world.expected(("n", i), False)) == NEED for i in range(N_NOISE))


# frames {1, 9}: workgroup 1 of k_select_redo, two frames in a row; {8}: lane 1 only of workgroup 0; {11}: the last
@pytest.mark.parametrize("device", (False, True), ids=("host", "device"))
def test_batch_12_one_workgroup_selects_two_frames(fd, world, device):
    assert 1 % SELECT_GROUPS == 9 % SELECT_GROUPS and 8 % SELECT_GROUPS == 0 and 8 // SELECT_GROUPS == 1
    run_case(fd, world, 12, {1, 9, 8, 11}, device=device)


def test_batch_12_every_frame_sparse(fd, world):
    """Each workgroup of k_select_redo takes one or two frames."""
    run_case(fd, world, 12, set(range(12)))


def test_batch_12_with_prior_features(fd, world):
    """The MASKED k_fast in the redo pass, with its prefix tables."""
    run_case(fd, world, 12, {1, 9}, with_prior=True)


def test_batch_70_second_ballot_round_of_k_fast(fd, world):
    """Frames 64 and 69 sit in the second, partial round of 64 flags of k_fast's redo loop."""
    assert 64 // WAVE == 69 // WAVE == 1 and 70 % WAVE
    run_case(fd, world, 70, {3, 64, 69})


def test_batch_520_second_round_of_k_select_redo(fd, world):
    """Frames 512 and 519 sit in the second, partial round of k_select_redo's loop over 64 * 8 frames; 519 is the
    last lane of workgroup 7 that is still inside the batch."""
    round_frames = WAVE * SELECT_GROUPS
    assert 511 // round_frames == 0 and 512 // round_frames == 519 // round_frames == 1 and 520 % round_frames
    assert (519 - round_frames) // SELECT_GROUPS == 0 and 519 % SELECT_GROUPS == SELECT_GROUPS - 1 and 519 + SELECT_GROUPS >= 520
    run_case(fd, world, 520, {0, 7, 511, 512, 519})
