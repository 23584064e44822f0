"""The SuperPoint layer kernels (K9 k_conv3x3_c1_bias_relu, K10 k_conv3x3_c64_pp, k_bias_relu / k_bias_relu_pool,
K11 k_nn_heat_softmax / k_nn_desc_normalize) bit for bit at each scheduling branch.

Inputs come from tests/nn_exact.py: integer-valued fp16 tensors whose float32 sums are exact in any order, so the
documented rounding sequence -- half(sum), half(half(sum) + bias), ReLU (NaN and -0 give +0), 2x2 max pool -- has
one right answer, computed on the CPU in float64 and compared on bit patterns. Every test asserts through
tests/nn_geometry.py the branch its shape is meant to take (K10's pipeline depth K per workgroup and its XCD remap,
the grid-stride loops' second trip, K9's pixels per step, K11's groups). Outputs lie inside a sentinel-filled
buffer whose halves before and after the tensor (and, for a channel block written into a wider tensor, the other
channels) must stay untouched."""
import ctypes

import numpy as np
import pytest

import nn_exact as E
import nn_geometry as G

pytestmark = pytest.mark.gpu

PAD, SENT16, SENT32 = 64, 0x5A5A, 0x5A5A5A5A


@pytest.fixture(scope="module")
def sp():
    import feature_detector_amd as fd
    from feature_detector_amd import superpoint

    fd.load()
    return superpoint


def dev(a, channels_last=True):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t.contiguous(memory_format=torch.channels_last) if channels_last and t.dim() == 4 else t


def guarded(n, c, h, w, dtype="float16"):
    """(buffer, channels-last [n, c, h, w] view of its middle): PAD sentinel elements on either side."""
    import torch

    it, sent = (torch.int16, SENT16) if dtype == "float16" else (torch.int32, SENT32)
    numel = n * c * h * w
    buf = torch.full((numel + 2 * PAD,), sent, dtype=it, device="cuda")
    return buf, buf[PAD:PAD + numel].view(getattr(torch, dtype)).view(n, h, w, c).permute(0, 3, 1, 2)


def assert_guard(buf):
    sent = SENT16 if buf.element_size() == 2 else SENT32
    assert bool((buf[:PAD] == sent).all()) and bool((buf[-PAD:] == sent).all()), "wrote outside the output tensor"


def assert_bits(got, ref, what):
    """got: device tensor [n, c, h, w]; ref: uint16 / uint32 array of the same shape. Reports the first
    differing element (frame, channel, pixel, expected and observed bits)."""
    import torch

    it = torch.int16 if got.element_size() == 2 else torch.int32
    g = got.view(it).cpu().numpy().view(ref.dtype)
    assert g.shape == ref.shape, (what, g.shape, ref.shape)
    if not np.array_equal(g, ref):
        bad = np.argwhere(g != ref)
        f, c, y, x = (int(v) for v in bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {ref.size} differ; first at frame {f} channel {c} pixel ({y}, {x}): "
                             f"expected {int(ref[f, c, y, x]):#06x}, observed {int(g[f, c, y, x]):#06x}")


def run_k10(sp, xd, wt, b, pool, ref, what):
    """conv64_bias_relu into a guarded output against ref [n, co, ...]."""
    n, _, h, w = xd.shape
    co = wt.shape[0]
    buf, out = guarded(n, co, h // 2 if pool else h, w // 2 if pool else w)
    sp.conv64_bias_relu(xd, dev(wt, False), dev(b), pool, out=out)
    assert_bits(out, ref, what)
    assert_guard(buf)


# one-tile frames per tile count: (unpooled, pooled) frame size; the large counts take the small frames
ONE_TILE = {1: ((8, 32), (8, 32)), 2: ((5, 17), (6, 18)), 255: ((6, 18), (6, 18)), 256: ((8, 32), (8, 32)),
            257: ((5, 17), (2, 2)), 512: ((6, 18), (6, 18)), 513: ((1, 1), (2, 2)), 769: ((5, 17), (6, 18)),
            1025: ((2, 2), (2, 2)), 1537: ((1, 1), (2, 2))}
DEPTHS = {1: {1: 1}, 2: {1: 2}, 255: {1: 255}, 256: {1: 256}, 257: {2: 1, 1: 255}, 512: {2: 256}, 513: {3: 1, 2: 255},
          769: {4: 1, 3: 255}, 1025: {5: 1, 4: 255}, 1537: {7: 1, 6: 255}}


@pytest.mark.parametrize("regime", ["exact", "rounding"])
@pytest.mark.parametrize("pool", [False, True])
@pytest.mark.parametrize("tiles", sorted(ONE_TILE))
def test_k10_one_tile_frames(sp, tiles, pool, regime):
    """n one-tile frames, all different: workgroup b runs frames L(b), L(b) + G, ...; the pipeline's prologue and
    phase branches at K = 1 .. 7, grids whose workgroups differ in K, the 255 / 256 / 257 boundary of the XCD remap,
    a single tile (group 1 idle), frames smaller than a wave's 4 x 16 patch. The exact regime has no rounding: any
    difference there is a misplaced or missing output."""
    h, w = ONE_TILE[tiles][pool]
    assert G.k10_tiles(tiles, h, w) == (1, 1, tiles) and G.k10_depth_counts(tiles, h, w) == DEPTHS[tiles]
    if tiles == 257:
        assert [b for b, k in enumerate(G.k10_depths(tiles, h, w)) if k == 2] == [0]
    x, wt, b, s = E.cached_case(regime, tiles, h, w, 100 + tiles)
    assert len({x[f].tobytes() for f in range(tiles)}) == tiles or h * w == 1
    xd = dev(x)
    for co in (64, 128):
        ref = E.relu_pool_bits(E.round_twice(s[:, :co], b[:co]), pool)
        run_k10(sp, xd, wt[:co], b[:co], pool, ref, (tiles, h, w, pool, regime, co))


@pytest.mark.parametrize("regime", ["exact", "rounding", "rounding-scaled"])
@pytest.mark.parametrize("n,h,w,pool", [(130, 9, 33, False), (130, 10, 34, False), (130, 16, 64, False), (60, 17, 65, False),
                                        (130, 10, 34, True), (60, 18, 66, True)])
def test_k10_ragged_tiles(sp, n, h, w, pool, regime):
    """Multi-tile frames whose last tiles are ragged (one row or column, two, none), K in {2, 3}."""
    assert set(G.k10_depth_counts(n, h, w)) == {2, 3}
    th, tw, _ = G.k10_tiles(n, h, w)
    assert th > 1 and tw > 1
    x, wt, b, s = E.cached_case(regime.split("-")[0], n, h, w, 7, regime.endswith("scaled"))
    xd = dev(x)
    for co in (64, 128):
        ref = E.relu_pool_bits(E.round_twice(s[:, :co], b[:co]), pool)
        run_k10(sp, xd, wt[:co], b[:co], pool, ref, (n, h, w, pool, regime, co))


def test_k10_small_grid(sp):
    """One 24 x 96 frame: 9 tiles, a grid of 9 workgroups (no remap), K = 1 each."""
    assert G.k10_tiles(1, 24, 96) == (3, 3, 9) and G.k10_depth_counts(1, 24, 96) == {1: 9}
    for regime in ("exact", "rounding"):
        x, wt, b, s = E.cached_case(regime, 1, 24, 96, 3)
        for pool in (False, True):
            for co in (64, 128):
                ref = E.relu_pool_bits(E.round_twice(s[:, :co], b[:co]), pool)
                run_k10(sp, dev(x), wt[:co], b[:co], pool, ref, (regime, pool, co))


@pytest.mark.parametrize("pool", [False, True])
def test_k10_channel_block_of_wider_output(sp, pool):
    """The C ABI with y_channels = 192, y_offset = 64: channels 64 .. 127 written, the others untouched."""
    import torch
    from feature_detector_amd import _lib

    n, h, w = 5, 10, 34
    x, wt, b = E.build("rounding", n, h, w, 64, 21)
    ref = E.conv_bias_relu_ref(x, wt, b, pool)
    xd, wp, bd = dev(x), sp.pack_conv3x3_weight(dev(wt, False)), dev(b)
    ho, wo = (h // 2, w // 2) if pool else (h, w)
    buf, out = guarded(n, 192, ho, wo)
    ctx = sp._resolve_ctx(None, xd)
    sp._bind_stream(ctx, True)
    rc = _lib.load().fd_nn_conv3x3_c64(ctx.ptr, ctypes.c_void_p(xd.data_ptr()), ctypes.c_void_p(wp.data_ptr()),
                                        ctypes.c_void_p(bd.data_ptr()), ctypes.c_void_p(out.data_ptr()), n, h, w,
                                        1 if pool else 0, 192, 64)
    _lib.check(ctx.ptr, rc)
    torch.cuda.synchronize()
    assert_bits(out[:, 64:128], ref, ("block", pool))
    o16 = out.view(torch.int16)
    assert bool((o16[:, :64] == SENT16).all()) and bool((o16[:, 128:] == SENT16).all()), "wrote outside its channel block"
    assert_guard(buf)


def special_case(regime, co):
    x, wt, b = E.build(regime, 4, 10, 34, co, 33)
    at = E.plant_specials(x, wt, b)
    return x, wt, b, at


def assert_planted(out_bits, at):
    """The unpooled outputs at the planted positions, spelled out (the full comparison covers them too)."""
    assert out_bits[at["pos_inf"]] == 0x7C00 and out_bits[at["neg_inf"]] == 0
    f, c, y, xx = at["nan_zero"]
    assert [int(out_bits[f, c, y, xx - k]) for k in range(3)] == [0, 0x7C00, 0]  # NaN, +inf, -inf
    assert out_bits[at["nan_cancel"]] == 0 and out_bits[at["cancel"]] == 0 and out_bits[at["neg_zero"]] == 0


def test_k10_special_values(sp):
    """Sums that overflow half to +-inf, NaN sums (inf * 0, inf - inf), a sum of exactly -bias and a -0 before the
    ReLU, plain and pooled: +inf stays, everything else non-positive (NaN included) is +0 -- never 0x8000."""
    import torch

    x, wt, b, at = special_case("rounding", 64)
    xd = dev(x)
    for pool in (False, True):
        ref = E.conv_bias_relu_ref(x, wt, b, pool)
        run_k10(sp, xd, wt, b, pool, ref, ("specials", pool))
    got = sp.conv64_bias_relu(xd, dev(wt, False), dev(b)).view(torch.int16).cpu().numpy().view(np.uint16)
    assert_planted(got, at)
    assert not (got & 0x8000).any()


# ------------------------------------------------------------------ K9
def run_k9(sp, x, wt, b, what):
    n, _, h, w = x.shape
    c = wt.shape[0]
    buf, out = guarded(n, c, h, w)
    sp.conv1_bias_relu(dev(x, False), dev(wt, False), dev(b), out=out)
    assert_bits(out, E.conv_bias_relu_ref(x, wt, b), what)
    assert_guard(buf)


@pytest.mark.parametrize("c", G.K9_CHANNELS)
def test_k9_channels_and_widths(sp, c):
    """Each channel count (pixels per block step 256 / (c / 8)) at widths of one pixel, two, one step, one step
    plus or minus a pixel, and the staging's limit, plain and scaled."""
    for i, w in enumerate((1, 2, 255, 256, 257, 4096)):
        h = 1 + i % 3
        geo = G.k9_geometry(2, h, w, c)
        assert geo["per"] == 256 // (c // 8) and geo["trips"] == 1 and geo["steps"] == -(-w // geo["per"])
        for scaled in (False, True):
            x, wt, b = E.build("k9", 2, h, w, c, 10 * c + i, scaled)
            run_k9(sp, x, wt, b, (c, h, w, scaled))
    assert G.k9_geometry(2, 1, 257, 8)["steps"] == 2 and G.k9_geometry(2, 1, 256, 8)["steps"] == 1


def test_k9_row_loop_second_trip(sp):
    n, h, w, c = 2800, 3, 5, 8
    assert G.k9_geometry(n, h, w, c) == dict(grid=8192, trips=2, per=256, steps=1)
    x, wt, b = E.build("k9", n, h, w, c, 77)
    run_k9(sp, x, wt, b, "second trip")


@pytest.mark.parametrize("c", [8, 64])
def test_k9_special_values(sp, c):
    import torch

    x, wt, b, at = special_case("k9", c)
    run_k9(sp, x, wt, b, ("specials", c))
    got = sp.conv1_bias_relu(dev(x, False), dev(wt, False), dev(b)).view(torch.int16).cpu().numpy().view(np.uint16)
    assert_planted(got, at)
    assert not (got & 0x8000).any()


def test_k9_refuses_wide_rows(sp):
    """Width 4097 is refused by the C ABI (the row staging holds 4096 pixels); the context works afterwards."""
    import torch
    from feature_detector_amd import _lib

    x, wt, b = E.build("k9", 1, 2, 4097, 8, 5)
    xd, wd, bd = dev(x, False), dev(wt, False), dev(b)
    buf, out = guarded(1, 8, 2, 4097)
    ctx = sp._resolve_ctx(None, xd)
    sp._bind_stream(ctx, True)
    rc = _lib.load().fd_nn_conv3x3_c1(ctx.ptr, ctypes.c_void_p(xd.data_ptr()), ctypes.c_void_p(wd.data_ptr()),
                                       ctypes.c_void_p(bd.data_ptr()), 8, ctypes.c_void_p(out.data_ptr()), 1, 2, 4097)
    assert rc == _lib.FD_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((buf == SENT16).all())  # nothing was launched
    import feature_detector_amd as fd
    with pytest.raises(fd.FdError):
        sp.conv1_bias_relu(xd, wd, bd)
    run_k9(sp, x[:, :, :, :4096], wt, b, "after the refusal")


# ------------------------------------------------------------------ bias_relu
SPECIAL_HALVES = [np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0, -1.0, 3.5, -3.5, 65504.0, -65504.0, 1000.0, -1000.0, 0.25]


@pytest.mark.parametrize("c", [8, 64])
def test_bias_relu_special_values(sp, c):
    """NaN -> +0, +inf kept, -inf and -0 -> +0, x = -bias -> +0, overflow of x + bias -> +inf; plain, pooled, in place."""
    import torch

    rng = np.random.default_rng(c)
    x = rng.choice(np.array(SPECIAL_HALVES, np.float16), (2, c, 6, 10))
    b = rng.choice(np.array([-0.0, 0.0, 1.0, -1.0, 3.5, -3.5, 1000.0, -1000.0, 65504.0], np.float16), c)
    b[:4] = np.array([-0.0, 0.0, 65504.0, 3.5], np.float16)
    assert G.bias_relu_geometry(2, 6, 10, c, False)["trips"] == 1
    xd, bd = dev(x), dev(b)
    for pool in (False, True):
        ref = E.bias_relu_ref(x, b, pool)
        assert not (ref & 0x8000).any() and (ref == 0x7C00).any() and not np.isnan(ref.view(np.float16)).any()
        buf, out = guarded(2, c, 3 if pool else 6, 5 if pool else 10)
        sp.bias_relu(xd, bd, pool, out=out)
        assert_bits(out, ref, (c, pool))
        assert_guard(buf)
    inplace = xd.clone(memory_format=torch.channels_last)
    sp.bias_relu(inplace, bd, out=inplace)
    assert_bits(inplace, E.bias_relu_ref(x, b), (c, "in place"))


@pytest.mark.parametrize("pool,side", [(False, 2050), (True, 4100)])
def test_bias_relu_second_trip(sp, pool, side):
    """More than 4,194,304 output vectors: every thread's grid-stride loop takes a second trip. Random half bit
    patterns (|x| >= 2, zeros of both signs, infinities, NaNs: with integer biases no sum is subnormal) built on the
    device; the expected bits by a 65,536-entry table per channel computed on the CPU with the same numpy rule."""
    import torch

    c = 8
    geo = G.bias_relu_geometry(1, side, side, c, pool)
    assert geo["vectors"] > 4194304 and geo["grid"] == G.ACT_GRID and geo["trips"] == 2
    b = np.array([-5, 0.0, 3, -0.0, 1000, -1000, 7, -64], np.float16)
    every = np.arange(65536, dtype=np.uint16).view(np.float16)
    lut = E.bias_relu_ref(np.ascontiguousarray(np.broadcast_to(every.reshape(1, 1, 1, -1), (1, c, 1, 65536))), b)
    lut_d = torch.from_numpy(lut.reshape(c * 65536).view(np.int16).astype(np.int32)).cuda()
    g = torch.Generator(device="cuda")
    g.manual_seed(side)
    bits = torch.randint(0, 65536, (1, side, side, c), generator=g, device="cuda", dtype=torch.int32) | 0x4000
    zero = torch.randint(0, 37, (1, side, side, c), generator=g, device="cuda", dtype=torch.int32) == 0
    bits = torch.where(zero, bits & 0x8000, bits)
    idx = bits + torch.arange(c, device="cuda", dtype=torch.int32) * 65536
    exp = lut_d.index_select(0, idx.view(-1)).view(1, side, side, c).to(torch.int16)
    del idx, zero
    if pool:
        exp = exp.view(1, side // 2, 2, side // 2, 2, c).amax(dim=(2, 4))  # (non-negative halves order as integers)
    x = torch.where(bits >= 32768, bits - 65536, bits).to(torch.int16).view(torch.float16).permute(0, 3, 1, 2)
    del bits
    assert x.is_contiguous(memory_format=torch.channels_last)
    so = side // 2 if pool else side
    buf, out = guarded(1, c, so, so)
    sp.bias_relu(x, dev(b), pool, out=out)
    torch.cuda.synchronize()
    got = out.view(torch.int16).permute(0, 2, 3, 1)
    if not torch.equal(got, exp):
        bad = (got != exp).nonzero()
        _, y, xx, ch = (int(v) for v in bad[0])
        raise AssertionError(f"{len(bad)} differ; first at pixel ({y}, {xx}) channel {ch}: expected "
                             f"{int(exp[0, y, xx, ch]) & 0xFFFF:#06x}, observed {int(got[0, y, xx, ch]) & 0xFFFF:#06x}")
    assert_guard(buf)
    assert int((exp == 0x7C00).sum()) > 0 and int((exp == 0).sum()) > 0  # (infinities kept, NaN / negative / -0 zeroed)


# ------------------------------------------------------------------ K11
def run_heat(sp, semi, bias):
    """fd_nn_heat_softmax through the C ABI into a guarded float32 map -> uint32 bits [n, 8 hc, 8 wc]."""
    import torch
    from feature_detector_amd import _lib

    n, _, hc, wc = semi.shape
    sd = dev(semi)
    bd = None if bias is None else dev(bias)
    buf, out = guarded(n, 1, 8 * hc, 8 * wc, "float32")
    ctx = sp._resolve_ctx(None, sd)
    sp._bind_stream(ctx, True)
    rc = _lib.load().fd_nn_heat_softmax(ctx.ptr, ctypes.c_void_p(sd.data_ptr()),
                                         ctypes.c_void_p(bd.data_ptr() if bd is not None else None),
                                         ctypes.c_void_p(out.data_ptr()), n, hc, wc)
    _lib.check(ctx.ptr, rc)
    torch.cuda.synchronize()
    assert_guard(buf)
    return out.view(torch.int32).cpu().numpy().view(np.uint32)[:, 0]


@pytest.mark.parametrize("wc", [31, 32, 33, 65])
def test_heat_one_hot_cells(sp, wc):
    """Cells whose logits are 0 at one channel and far below elsewhere: exp underflows to 0, so the heat is exactly
    1.0 at the hot channel's pixel of its cell and exactly 0 elsewhere, all 0 where the dustbin is hot -- the
    channel-to-pixel shuffle and the 32-cell groups (ragged, exact, one cell over) with nothing to round. A bias
    that lifts one channel above every cell's own moves the hot pixel (or, on the dustbin, empties the map)."""
    n, hc = 2, 10
    groups, last = G.heat_groups(wc)
    assert (groups, last) == {31: (1, 31), 32: (1, 32), 33: (2, 1), 65: (3, 1)}[wc]
    b_, i_, j_ = np.meshgrid(np.arange(n), np.arange(hc), np.arange(wc), indexing="ij")
    hot = (7 * i_ + 13 * j_ + b_) % 65
    assert (hot == 64).any() and len(np.unique(hot)) > 32

    def expected(hot):
        e = np.zeros((n, 8 * hc, 8 * wc), np.float32)
        live = hot < 64
        e[b_[live], 8 * i_[live] + hot[live] // 8, 8 * j_[live] + hot[live] % 8] = 1.0
        return e.view(np.uint32)

    semi = np.full((n, hc, wc, 65), -60000.0, np.float16)
    semi[b_, i_, j_, hot] = 0.0
    semi = np.ascontiguousarray(semi.transpose(0, 3, 1, 2))
    got = run_heat(sp, semi, None)
    assert np.array_equal(got, expected(hot))
    assert int((got == 0x3F800000).sum()) == int((hot < 64).sum()) and (hot == 64).any()
    zero_bias = np.zeros(65, np.float16)
    assert np.array_equal(run_heat(sp, semi, zero_bias), expected(hot))
    semi = np.where(semi == 0, np.float16(0.0), np.float16(-30000.0)).astype(np.float16)
    for moved in (37, 64):  # -30000 + 60000 = 30000 above every cell's 0 (60000 where the cell's own is lifted)
        bias = np.zeros(65, np.float16)
        bias[moved] = 60000.0
        assert np.array_equal(run_heat(sp, semi, bias), expected(np.full_like(hot, moved))), moved
    flat = run_heat(sp, np.full((n, 65, hc, wc), 5.0, np.float16), None)
    assert (flat == (np.float32(1) / np.float32(65)).view(np.uint32)).all()


@pytest.mark.parametrize("c", [8, 128, 256, 512, 1024])
def test_desc_one_channel_cells(sp, c):
    """One non-zero channel per cell: its square, the norm and the quotient are exact, so the output is exactly
    +-1 there and a zero of the input's sign elsewhere; one case per lanes-per-cell branch (8, 16, 32, 64 lanes,
    and two rounds of a 64-lane cell), a cell count that fills neither the last wave nor the last block."""
    import torch
    from feature_detector_amd import _lib

    cells = 37
    geo = G.desc_geometry(cells, c)
    assert (geo["span"], geo["rounds"]) == {8: (8, 1), 128: (16, 1), 256: (32, 1), 512: (64, 1), 1024: (64, 2)}[c]
    assert geo["waves"] % 4 and (geo["per_wave"] == 1 or geo["idle"] > 0)
    rng = np.random.default_rng(c)
    x = np.where(rng.integers(0, 2, (cells, c)) == 1, np.float16(-0.0), np.float16(0.0)).astype(np.float16)
    ch = (5 * np.arange(cells) + 3) % c
    val = ((1 + np.arange(cells) % 7) * 0.375 * np.where(np.arange(cells) % 3 == 0, -1, 1)).astype(np.float16)
    x[np.arange(cells), ch] = val
    exp = x.astype(np.float32)
    exp[np.arange(cells), ch] = np.sign(val.astype(np.float32))
    xd = dev(x)
    buf, out = guarded(1, c, 1, cells, "float32")
    ctx = sp._resolve_ctx(None, xd)
    sp._bind_stream(ctx, True)
    rc = _lib.load().fd_nn_desc_normalize(ctx.ptr, ctypes.c_void_p(xd.data_ptr()), None, ctypes.c_void_p(out.data_ptr()),
                                           cells, c)
    _lib.check(ctx.ptr, rc)
    torch.cuda.synchronize()
    got = buf[PAD:-PAD].cpu().numpy().view(np.uint32).reshape(cells, c)
    assert np.array_equal(got, exp.view(np.uint32))
    assert_guard(buf)
    t = sp.desc_normalize(xd.view(1, 1, cells, c).permute(0, 3, 1, 2))  # the wrapper, same cells
    assert np.array_equal(t.permute(0, 2, 3, 1).reshape(cells, c).view(torch.int32).cpu().numpy().view(np.uint32),
                          exp.view(np.uint32))


# ------------------------------------------------------------------ SuperPointNet.cbr
def test_forward_on_frame_wider_than_k9_rows(sp):
    """A frame wider than K9's 4096-pixel row staging: cbr leaves the first layer to the bias-free convolution +
    bias_relu branch instead of raising; outputs finite, of the right shapes, and within the fused forward's
    tolerance of the module-by-module forward (the tolerance of test_bias_relu_matches_torch)."""
    import torch
    from test_gpu_nn import _reference_forward

    net = sp.build_net(0).cuda().eval().half().to(memory_format=torch.channels_last)
    g = torch.Generator(device="cuda")
    g.manual_seed(41)
    frames = torch.randint(0, 256, (1, 1, 8, 4104), generator=g, device="cuda", dtype=torch.int32)
    x = (frames.half() / 255.0).contiguous(memory_format=torch.channels_last)
    assert x.shape[3] > G.K9_MAX_W
    with torch.inference_mode():
        heat, desc = net(x)
        rheat, rdesc = _reference_forward(net, x)
    assert tuple(heat.shape) == (1, 8, 4104) and tuple(desc.shape) == (1, 256, 1, 513)
    assert bool(torch.isfinite(heat).all()) and bool(torch.isfinite(desc).all())
    assert torch.allclose(heat, rheat, rtol=2e-2, atol=2e-3) and torch.allclose(desc, rdesc, rtol=2e-2, atol=2e-3)
