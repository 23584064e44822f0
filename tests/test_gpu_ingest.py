"""GPU: the pipelined ingest (fd_ingest_*) returns exactly what fd_points_detect
returns for the same frames, across slots reused round-robin with several submits in flight."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

THR = {"harris": 30.0, "shi_tomasi": 40.0, "fast": 10.0}
KIND = {"harris": 0, "shi_tomasi": 1, "fast": 2}


@pytest.mark.parametrize("name", ["harris", "shi_tomasi", "fast"])
def test_ingest_matches_oracle(oracle, name):
    import feature_detector_amd as fd

    rows, cols, batch, depth = 240, 320, 3, 3
    ing = fd.Ingest(name, rows, cols, batch=batch, depth=depth, need=150, min_feature_distance=9)
    frames = [np.stack([oracle.make_frame("noise" if (k + b) % 2 else "checker", 900 + 7 * k + b, rows, cols)
                        for b in range(batch)]) for k in range(7)]
    got = {}
    for k in range(len(frames)):
        slot = k % depth
        if k >= depth:
            got[k - depth] = ing.wait(slot)
        ing.frames(slot)[:] = frames[k]
        ing.submit(slot)
    for k in range(len(frames) - depth, len(frames)):
        got[k] = ing.wait(k % depth)
    for k, fr in enumerate(frames):
        for b in range(batch):
            exp = oracle.detect(KIND[name], fr[b], 9, THR[name], 150, sort_mode=1)[0]
            np.testing.assert_array_equal(got[k][b], exp)
    ing.close()


def test_ingest_misuse():
    import feature_detector_amd as fd

    ing = fd.Ingest("harris", 64, 64, batch=1, depth=2)
    with pytest.raises(fd.FdError):
        ing.wait(0)  # nothing submitted
    ing.frames(0)[:] = 7
    ing.submit(0)
    with pytest.raises(fd.FdError):
        ing.submit(0)  # still pending
    assert [len(x) for x in ing.wait(0)] == [0]  # flat frame: no candidates
    ing.close()


# ------------------------------------------------------------- slots, options and the C ABI's edges
# Small frames (48 x 64 and the odd-width 31 x 50), every submitted frame from its own seed, so that a
# mixed-up slot or a stale buffer shows. The options differ from the defaults and change the result.
SHAPES = [(48, 64), (31, 50)]
DIST = 5
THR2 = {"harris": 1.0e8, "shi_tomasi": 20000.0, "fast": 16.0}


def _frame(oracle, seed, rows, cols):
    return oracle.make_frame("noise", seed, rows, cols)


def _expect(oracle, name, frame, need=150):
    return oracle.detect(KIND[name], frame, DIST, THR2[name], need, sort_mode=1)[0]


def _ingest(name, rows, cols, batch, depth):
    import feature_detector_amd as fd

    return fd.Ingest(name, rows, cols, batch=batch, depth=depth, need=150, min_feature_distance=DIST,
                     min_valid_response=THR2[name])


@pytest.mark.parametrize("rows,cols", SHAPES)
@pytest.mark.parametrize("name", ["harris", "shi_tomasi", "fast"])
def test_ingest_one_slot_in_sequence(oracle, name, rows, cols):
    """depth 1, batch 1: four frames through the only slot, each collected before the next is written;
    every detector; distance and threshold that are not the defaults and that change the features."""
    frames = [_frame(oracle, 2000 + 10 * KIND[name] + k + rows, rows, cols) for k in range(4)]
    exp = [_expect(oracle, name, f) for f in frames]
    default = oracle.detect(KIND[name], frames[0], 20, THR[name], 150, sort_mode=1)[0]
    tighter = oracle.detect(KIND[name], frames[0], DIST, THR[name], 150, sort_mode=1)[0]
    assert len(exp[0]) > 0 and len(default) != len(tighter) and len(tighter) != len(exp[0])  # both options matter
    ing = _ingest(name, rows, cols, 1, 1)
    for f, e in zip(frames, exp):
        ing.frames(0)[0] = f
        ing.submit(0)
        got = ing.wait(0)
        assert len(got) == 1
        np.testing.assert_array_equal(got[0], e)
    ing.close()


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_ingest_waits_out_of_order_and_slot_reuse(oracle, rows, cols):
    """depth 3, batch 2: three submits in flight, collected as 2, 0, 1; then slot 1 alone is refilled
    and resubmitted; what wait() returned before for the other slots is a copy and stays as it was."""
    name = "harris"
    ing = _ingest(name, rows, cols, 2, 3)
    frames = {(s, b): _frame(oracle, 3000 + 2 * s + b + rows, rows, cols) for s in range(3) for b in range(2)}
    for s in range(3):
        for b in range(2):
            ing.frames(s)[b] = frames[s, b]
        ing.submit(s)
    got = {s: ing.wait(s) for s in (2, 0, 1)}
    for s in range(3):
        for b in range(2):
            np.testing.assert_array_equal(got[s][b], _expect(oracle, name, frames[s, b]))
    kept = {s: [x.copy() for x in got[s]] for s in (0, 2)}
    new = [_frame(oracle, 3100 + b + rows, rows, cols) for b in range(2)]
    for b in range(2):
        ing.frames(1)[b] = new[b]
    ing.submit(1)
    again = ing.wait(1)
    for b in range(2):
        e = _expect(oracle, name, new[b])
        assert not np.array_equal(e, got[1][b])  # the new frames have other features
        np.testing.assert_array_equal(again[b], e)
    for s in (0, 2):
        for b in range(2):
            np.testing.assert_array_equal(got[s][b], kept[s][b])
    ing.close()


def test_ingest_unsubmitted_slots(oracle):
    """depth 4, two slots ever used: wait on a slot that was never submitted raises, the used slots
    are right, and close() is clean with two slots untouched."""
    import feature_detector_amd as fd

    rows, cols, name = 31, 50, "shi_tomasi"
    ing = _ingest(name, rows, cols, 1, 4)
    frames = [_frame(oracle, 3200 + s, rows, cols) for s in range(2)]
    for s in range(2):
        ing.frames(s)[0] = frames[s]
        ing.submit(s)
    for s in (2, 3):
        with pytest.raises(fd.FdError):
            ing.wait(s)
    for s in (1, 0):
        np.testing.assert_array_equal(ing.wait(s)[0], _expect(oracle, name, frames[s]))
    with pytest.raises(fd.FdError):
        ing.wait(0)  # collected already
    ing.close()
    ing.close()


def _capi():
    import ctypes

    import feature_detector_amd as fd
    from feature_detector_amd import _lib

    return ctypes, fd, _lib, _lib.load()


def test_ingest_capacity_capi(oracle):
    """out_stride smaller than the features found (the binding always passes need + 1, so only the C ABI
    gets here): fd_ingest_wait gives FD_ERR_CAPACITY, the slot is free again, and the next frame through
    it is right."""
    ctypes, fd, _lib, L = _capi()
    rows, cols = 48, 64
    noise = _frame(oracle, 3300, rows, cols)
    assert len(oracle.detect(0, noise, DIST, 30.0, 150, sort_mode=1)[0]) > 8
    ctx = fd.Context()
    g = ctypes.c_void_p()
    assert L.fd_ingest_create(ctx.ptr, 0, 1, rows, cols, 2, 150, 8, ctypes.byref(g)) == _lib.FD_OK and g.value
    addr = L.fd_ingest_frames(g, 0)
    view = np.frombuffer((ctypes.c_uint8 * (rows * cols)).from_address(addr), np.uint8).reshape(rows, cols)
    opts = _lib.fd_point_opts(DIST, 30.0)
    xy, cnt = ctypes.c_void_p(), ctypes.c_void_p()
    view[:] = noise
    assert L.fd_ingest_submit(g, 0, ctypes.byref(opts)) == _lib.FD_OK
    assert L.fd_ingest_wait(g, 0, ctypes.byref(xy), ctypes.byref(cnt)) == _lib.FD_ERR_CAPACITY
    assert xy.value is None and cnt.value is None  # no results handed out with the error
    assert L.fd_ingest_submit(g, 0, ctypes.byref(opts)) == _lib.FD_OK  # not "still pending"
    assert L.fd_ingest_wait(g, 0, ctypes.byref(xy), ctypes.byref(cnt)) == _lib.FD_ERR_CAPACITY
    view[:] = 7
    assert L.fd_ingest_submit(g, 0, ctypes.byref(opts)) == _lib.FD_OK
    assert L.fd_ingest_wait(g, 0, ctypes.byref(xy), ctypes.byref(cnt)) == _lib.FD_OK
    assert xy.value and ctypes.cast(cnt, ctypes.POINTER(ctypes.c_int32))[0] == 0
    # a frame with at most 8 features fits: the features themselves, through the same slot
    few = np.full((rows, cols), 7, np.uint8)
    few[10:30, 12:40] = 200
    exp = oracle.detect(0, few, DIST, 30.0, 150, sort_mode=1)[0]
    assert 0 < len(exp) <= 8
    view[:] = few
    assert L.fd_ingest_submit(g, 0, ctypes.byref(opts)) == _lib.FD_OK
    assert L.fd_ingest_wait(g, 0, ctypes.byref(xy), ctypes.byref(cnt)) == _lib.FD_OK
    n = ctypes.cast(cnt, ctypes.POINTER(ctypes.c_int32))[0]
    pts = np.ctypeslib.as_array(ctypes.cast(xy, ctypes.POINTER(ctypes.c_float)), (8, 2))
    assert n == len(exp)
    np.testing.assert_array_equal(pts[:n], exp)
    L.fd_ingest_destroy(g)
    ctx.close()


def test_ingest_argument_checks_capi():
    """fd_ingest_create refuses each bad argument with FD_ERR_INVALID and hands out no ingest; the slot
    calls refuse a slot outside [0, depth) and NULL options."""
    ctypes, fd, _lib, L = _capi()
    ctx = fd.Context()
    good = dict(kind=0, batch=1, rows=48, cols=64, depth=2, need=150, out_stride=151)
    for bad in (dict(depth=0), dict(depth=65), dict(batch=0), dict(rows=0), dict(out_stride=0), dict(kind=-1),
                dict(kind=3)):
        a = dict(good, **bad)
        g = ctypes.c_void_p()
        rc = L.fd_ingest_create(ctx.ptr, a["kind"], a["batch"], a["rows"], a["cols"], a["depth"], a["need"],
                                a["out_stride"], ctypes.byref(g))
        assert rc == _lib.FD_ERR_INVALID and g.value is None, bad
    a = good
    assert L.fd_ingest_create(ctx.ptr, a["kind"], a["batch"], a["rows"], a["cols"], a["depth"], a["need"],
                              a["out_stride"], None) == _lib.FD_ERR_INVALID
    g = ctypes.c_void_p()
    assert L.fd_ingest_create(ctx.ptr, a["kind"], a["batch"], a["rows"], a["cols"], a["depth"], a["need"],
                              a["out_stride"], ctypes.byref(g)) == _lib.FD_OK and g.value
    opts = _lib.fd_point_opts(DIST, 30.0)
    xy, cnt = ctypes.c_void_p(), ctypes.c_void_p()
    for slot in (-1, a["depth"]):
        assert L.fd_ingest_frames(g, slot) is None
        assert L.fd_ingest_submit(g, slot, ctypes.byref(opts)) == _lib.FD_ERR_INVALID
        assert L.fd_ingest_wait(g, slot, ctypes.byref(xy), ctypes.byref(cnt)) == _lib.FD_ERR_INVALID
    assert L.fd_ingest_frames(g, 0) and L.fd_ingest_frames(g, a["depth"] - 1)
    assert L.fd_ingest_submit(g, 0, None) == _lib.FD_ERR_INVALID
    assert L.fd_ingest_wait(g, 0, ctypes.byref(xy), ctypes.byref(cnt)) == _lib.FD_ERR_INVALID  # nothing was queued
    assert xy.value is None and cnt.value is None
    L.fd_ingest_destroy(g)
    ctx.close()
