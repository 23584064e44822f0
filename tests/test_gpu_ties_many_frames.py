"""GPU: the reference tie order with more flagged frames than the wide prelude has slots.

The prelude kernels of k_select_reference (fd_select_refw.hip, FD_REFW_KERNEL) are launched with
min(batch, kRefWideSlots) x kRefWideGroups workgroups; slot j walks the flagged frames j, j + slots, ... of the
compact list that k_refw_init fills in atomic order. Elsewhere in the suite no call flags more than a handful of
frames, so `j += slots` never advances. Here FD_REF_WIDE=1 sends small frames through the prelude, and batches of
33 and 70 frames flag 33 and 66 of them: a slot takes two or three frames, one after the other, through the same
LDS; a batch of 40 with 20 flagged frames (fewer than the slots) is the control, with and without the switch.

Which calls run which prelude (fd_rt_points.cpp): fd_points_detect never sets push_order, whatever the kind, so
Harris runs the prelude with its clear / bits / wcount / wprefix / place kernels; fd_points_select always sets it,
so the same frames' Harris candidates handed to select_points (in reverse raster order) run the prelude without
them. Both then run the level kernels (lcount / lscatter / lswap), because every tie frame has more than
kRefWideMin candidates: 120 x 160 gives about 1,400 Harris candidates, 240 x 320 about 6,500, 300 x 400 about
10,300 (> 8192), so the frames are 300 x 400 with 3 x 4 stamps.

The frames that must stay unflagged are not full noise frames: 300 x 400 noise has equal Harris responses of its
own (integer gradient sums), is flagged too and would make the control flag all 40 frames. They are black frames
with six 12 x 12 patches of noise: about 90 candidates, all responses distinct (asserted), so k_select cannot meet a
tie on them, and the number of flagged frames of a batch is exactly its number of tie frames (asserted on the
status words).

FAST is run on the same batches, as the issue of this test asks, but it cannot flag a frame: its response is the
integer score plus an offset that grows with every candidate pixel, so no two responses are equal, the two tie
orders agree (asserted on the oracle's side) and the prelude's compact list stays empty. That case checks the
launch with more frames than slots and nothing to do, not the frame loop."""
import os
import re

import numpy as np
import pytest

from conftest import make_tie_frame

pytestmark = pytest.mark.gpu

ROWS, COLS, COPIES = 300, 400, (3, 4)
NEED, DIST = 200, 20
THR = {"harris": 30.0, "fast": 10.0}
KIND = {"harris": 0, "fast": 2}
TIE_SEEDS = (1, 2, 3, 4, 5)
QUIET_SEEDS = (61, 62)
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "feature_detector_amd", "csrc",
                      "fd_kernels.h")


def _const(name):
    m = re.search(r"constexpr \w+ %s = (\d+);" % name, open(HEADER).read())
    assert m, name
    return int(m.group(1))


def quiet_frame(rows, cols, seed):
    """Black, with six small patches of noise: a few dozen candidates, no two responses equal."""
    rng = np.random.default_rng(seed)
    img = np.zeros((rows, cols), np.uint8)
    for _ in range(6):
        y, x = int(rng.integers(10, rows - 30)), int(rng.integers(10, cols - 30))
        img[y:y + 12, x:x + 12] = rng.integers(0, 256, (12, 12))
    return img


# layouts: which distinct frame each batch index holds (t: tie frame t % 5, q: quiet frame q % 2)
def _layout(batch, quiet_at):
    out, t, n = [], 0, 0
    for b in range(batch):
        if b in quiet_at:
            out.append(("q", n % len(QUIET_SEEDS)))
            n += 1
        else:
            out.append(("t", t % len(TIE_SEEDS)))
            t += 1
    return out


LAYOUTS = {
    "b33_all_ties": _layout(33, ()),                       # one slot takes two frames
    "b70_quiet_at_the_seams": _layout(70, (0, 31, 32, 69)),  # 66 flagged: two or three frames per slot
    "b40_ties_at_odd": _layout(40, range(0, 40, 2)),       # 20 flagged, fewer than the slots: the control
}
CASES = [("b33_all_ties", True), ("b70_quiet_at_the_seams", True), ("b40_ties_at_odd", True), ("b40_ties_at_odd", False)]


@pytest.fixture(scope="module")
def fd():
    import feature_detector_amd as fd

    fd.load()
    return fd


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def world(oracle):
    """The distinct frames and, per distinct frame and source, the oracle's features in both orders: computed once,
    with the conditions that make the cases mean something asserted here, on the CPU."""
    slots, wide_min = _const("kRefWideSlots"), _const("kRefWideMin")
    flagged = {k: sum(1 for kind, _ in v if kind == "t") for k, v in LAYOUTS.items()}
    assert flagged["b33_all_ties"] == 33 > slots and flagged["b70_quiet_at_the_seams"] == 66 > 2 * slots
    assert flagged["b40_ties_at_odd"] == 20 < slots
    frames = {("t", i): make_tie_frame(oracle, ROWS, COLS, s, COPIES) for i, s in enumerate(TIE_SEEDS)}
    frames.update({("q", i): quiet_frame(ROWS, COLS, s) for i, s in enumerate(QUIET_SEEDS)})
    exp, lists = {}, {}
    for key, img in frames.items():
        for name in ("harris", "fast"):
            e0, cand = oracle.detect(KIND[name], img, DIST, THR[name], NEED, None, sort_mode=0)
            e1, _ = oracle.detect(KIND[name], img, DIST, THR[name], NEED, None, sort_mode=1)
            exp[name, key] = (e0, e1)
            if key[0] == "t" and name == "harris":
                assert not np.array_equal(e0, e1), ("the tie frame must separate the two orders", key)
                assert len(cand[0]) > wide_min, ("the level kernels must have work", key, len(cand[0]))
                assert len(e0) > 0
            if name == "fast":  # distinct responses by construction: nothing to resolve
                assert np.array_equal(e0, e1) and len(e0) > 0, key
        # the frame's Harris candidates, pushed in reverse raster order
        r, x, y = oracle.nms(oracle.response_map(img, 0, THR["harris"]), THR["harris"])
        lists[key] = (np.ascontiguousarray(r[::-1]), np.ascontiguousarray(x[::-1]), np.ascontiguousarray(y[::-1]))
        e0 = oracle.select(*lists[key], ROWS, COLS, DIST, NEED, None, sort_mode=0)
        e1 = oracle.select(*lists[key], ROWS, COLS, DIST, NEED, None, sort_mode=1)
        exp["custom", key] = (e0, e1)
        if key[0] == "t":
            assert not np.array_equal(e0, e1) and len(r) > wide_min and len(e0) > 0, key
        else:  # no two equal responses: the frame cannot be flagged
            assert len(np.unique(r)) == len(r) > 0 and len(e0) > 0, key
    # the tie frames differ from each other (a slot's second frame must not pass with its first frame's result)
    ties = [exp["harris", ("t", i)][0] for i in range(len(TIE_SEEDS))]
    assert all(not np.array_equal(ties[i], ties[j]) for i in range(len(ties)) for j in range(i))
    for a in frames.values():
        a.setflags(write=False)
    return frames, lists, exp


def _dev_lists(torch, lists):
    cap = max(len(l[0]) for l in lists)
    t = [np.zeros((len(lists), cap), dt) for dt in (np.float32, np.int32, np.int32)]
    for i, l in enumerate(lists):
        for k in range(3):
            t[k][i, :len(l[k])] = l[k]
    counts = np.array([len(l[0]) for l in lists], np.int64)
    return tuple(torch.from_numpy(a).cuda() for a in (*t, counts))


def _check(fd, layout, exp, source, ref, dev, ras):
    P = fd.points
    for what, res in (("host", ref), ("device", dev)):
        flags = res.frame_flags()
        assert not (flags & np.uint32(P.FRAME_GUARD | P.FRAME_UNRESOLVED)).any(), (what, [hex(int(f)) for f in flags])
        for b, key in enumerate(layout):
            np.testing.assert_array_equal(res.features(b), exp[source, key][0], err_msg=f"{source} {what} frame {b} {key}")
            if source != "fast":  # exactly the tie frames are flagged, and resolved
                want = np.uint32(P.FRAME_TIES | P.FRAME_RESOLVED) if key[0] == "t" else np.uint32(0)
                assert flags[b] & np.uint32(P.FRAME_TIES | P.FRAME_RESOLVED) == want, (what, b, key, hex(int(flags[b])))
    for b, key in enumerate(layout):
        np.testing.assert_array_equal(ras.features(b), exp[source, key][1], err_msg=f"{source} raster frame {b} {key}")


@pytest.mark.parametrize("source", ["harris", "custom", "fast"])
@pytest.mark.parametrize("layout,wide", CASES, ids=[f"{k}-{'wide' if w else 'auto'}" for k, w in CASES])
def test_more_flagged_frames_than_prelude_slots(fd, torch, world, monkeypatch, layout, wide, source):
    frames, lists, exp = world
    if wide:
        monkeypatch.setenv("FD_DEBUG_AB", "1")  # (the library reads A/B switches only with it)
        monkeypatch.setenv("FD_REF_WIDE", "1")
    else:
        monkeypatch.delenv("FD_REF_WIDE", raising=False)
    lay = LAYOUTS[layout]
    if source == "custom":
        host = [lists[key] for key in lay]
        ref = fd.select_points(host, ROWS, COLS, NEED, DIST, ties="reference")
        ras = fd.select_points(host, ROWS, COLS, NEED, DIST, ties="raster")
        # device lists and outputs: no host fallback behind the GPU emulation (FRAME_UNRESOLVED would raise)
        dev = fd.select_points(_dev_lists(torch, host), ROWS, COLS, NEED, DIST, ties="reference")
    else:
        host = np.stack([frames[key] for key in lay])
        ref = fd.detect_points(source, host, NEED, DIST, THR[source])
        ras = fd.detect_points(source, host, NEED, DIST, THR[source], ties="raster")
        dev = fd.detect_points(source, torch.from_numpy(host).cuda(), NEED, DIST, THR[source], ties="reference")
    torch.cuda.synchronize()
    dev.check()
    _check(fd, lay, exp, source, ref, dev, ras)
