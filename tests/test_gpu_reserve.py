"""GPU: the workspace contract of a context.

* fd_ctx_reserve sizes everything fd_points_detect needs for a shape, so a fresh context can capture the
  call into a hipGraph right after it, with no eager call in between (a captured call must not allocate:
  growing the workspace under capture fails). The shape, 2 x 120 x 160, takes k_corner with the sorted
  segment lists and the in-kernel gather (the branch with the most buffers); FAST at this size uses the run
  table and the cut words. need 50 / distance 20 keep the occupancy grid in LDS, so nothing is sized by
  the call's options.
* Closing a context frees its whole workspace: contexts created and closed one after another leave no
  more device memory in use than one context's workspace.
"""
import numpy as np
import pytest

from conftest import make_tie_frame

pytestmark = pytest.mark.gpu

THR = {"harris": 30.0, "shi_tomasi": 40.0, "fast": 10.0}
KIND = {"harris": 0, "shi_tomasi": 1, "fast": 2}
ROWS, COLS, NEED, DIST = 120, 160, 50, 20


@pytest.fixture(scope="module")
def fd():
    import feature_detector_amd as fd

    fd.load()
    return fd


def _reserve_capture_replay(fd, oracle, name, frames, ties, sort_mode):
    import torch

    exp = [oracle.detect(KIND[name], f, DIST, THR[name], NEED, None, sort_mode=sort_mode)[0] for f in frames]
    assert all(len(e) > 0 for e in exp)
    ctx = fd.Context(0)
    if ties == "reference":  # reserve sizes the reference order's scratch only when the context has that order
        ctx.set_tie_order("reference")
    ctx.reserve(KIND[name], len(frames), ROWS, COLS)
    ctx.synchronize()  # reserve's fills ran on the context's own stream; the capture does not wait for it
    dev = torch.from_numpy(frames).cuda()
    out = (torch.zeros((len(frames), NEED + 1, 2), dtype=torch.float32, device="cuda"),
           torch.zeros((len(frames),), dtype=torch.int32, device="cuda"),
           torch.zeros((len(frames),), dtype=torch.int32, device="cuda"))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        fd.detect_points(name, dev, NEED, DIST, THR[name], ctx=ctx, ties=ties, out=out)
    for _ in range(2):
        for t in out:
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        xy, cnt, st = (t.cpu().numpy() for t in out)
        assert not (st.astype(np.uint32) & np.uint32(fd.points.FRAME_GUARD)).any(), st
        for b in range(len(frames)):
            assert np.array_equal(xy[b, :int(cnt[b])], exp[b]), (name, b)
    del g
    ctx.close()


@pytest.mark.parametrize("name", ["harris", "shi_tomasi", "fast"])
def test_reserve_then_capture_raster(fd, oracle, name):
    pytest.importorskip("torch")
    frames = np.stack([oracle.make_frame("noise", 9100, ROWS, COLS), oracle.make_frame("checker", 9101, ROWS, COLS)])
    _reserve_capture_replay(fd, oracle, name, frames, "raster", 1)


@pytest.mark.parametrize("name", ["harris", "shi_tomasi", "fast"])
def test_reserve_then_capture_reference(fd, oracle, name):
    pytest.importorskip("torch")
    tie = make_tie_frame(oracle, ROWS, COLS, seed=9102, copies=(3, 4))
    if name != "fast":  # (the stamps' responses are bit-identical for the corner detectors: the orders differ)
        e0 = oracle.detect(KIND[name], tie, DIST, THR[name], NEED, None, sort_mode=0)[0]
        e1 = oracle.detect(KIND[name], tie, DIST, THR[name], NEED, None, sort_mode=1)[0]
        assert not np.array_equal(e0, e1), "the constructed frame must separate the two orders"
    frames = np.stack([tie, oracle.make_frame("checker", 9103, ROWS, COLS)])
    _reserve_capture_replay(fd, oracle, name, frames, "reference", 0)


def test_context_churn_frees_the_workspace(fd, oracle):
    """20 contexts, each used for one host-frame point, line and BRIEF call and closed: the device memory in
    use afterwards has grown by no more than the workspace of one of them (measured on the first), i.e.
    closing a context frees every buffer it owns. A 1080p frame: its buffers are device allocations of their
    own (4 MB and more each), so the measure does not depend on what the runtime's sub-allocator for small
    blocks has cached from earlier tests (with a 64x96 frame the whole workspace fitted into one cached
    2 MB block and measured 0 bytes once more tests ran before this one)."""
    torch = pytest.importorskip("torch")
    img = oracle.make_frame("checker", 9104, 1080, 1920)

    def use(ctx):
        res = fd.detect_points("harris", img, 20, 5, 30.0, ctx=ctx)
        fd.lsd_lines(img, ctx=ctx)
        uv = np.zeros((1, 20, 2), np.float32)
        uv[0, :, :] = (48.0, 32.0)
        uv[0, :int(res.counts[0])] = res.features(0)
        fd.brief_compute(img, uv, length=256, half_patch_size=8, ctx=ctx)

    warm = fd.Context(0)  # (loads the kernels' code objects and torch's own state: not workspace)
    use(warm)
    warm.close()
    torch.cuda.synchronize()
    free_before = torch.cuda.mem_get_info()[0]
    workspace = None
    for i in range(20):
        ctx = fd.Context(0)
        use(ctx)
        if i == 0:
            workspace = free_before - torch.cuda.mem_get_info()[0]
        ctx.close()
    grown = free_before - torch.cuda.mem_get_info()[0]
    print(f"workspace of one context: {workspace} bytes; in use after 20 contexts: {grown} bytes more")
    assert workspace > 0
    assert grown <= workspace, (grown, workspace)
