"""The argument checks of the Python binding, pinned: for every public wrapper the exception type and the full
message of the errors the wrapper itself raises, the order of its checks (argument sets that are wrong twice), that
out= comes back as the same object, and the type and shape of a fresh result on either side.

Shapes are the smallest that reach the check: frames 8 x 8 and 2 x 8 x 8, slot arrays of stride 4, activations
[1, 64, 4, 4]. Checks that fire before any context or library call carry no marker; the rest are marked gpu. Every
case is an error raised in Python; none reaches a kernel with bad arguments.
"""
import numpy as np
import pytest

import feature_detector_amd as fd
from feature_detector_amd import superpoint as sp

U8, RANK = "frames must be uint8", "frames must be [rows, cols] or [batch, rows, cols]"
EMPTY, SIDE = "frames must not be empty", "out must be on the side of the frames"
HOST_OUT = "out= is for device tensors"
OTHER_CTX = "context is on device 1 but the inputs are on device 0"
TAPS = [96, 64, 16]
F8, B8 = np.zeros((8, 8), np.uint8), np.zeros((2, 8, 8), np.uint8)
XY, XYZ = np.zeros((4, 2), np.float32), np.zeros((4, 3), np.float32)
BITS, DESC = np.zeros((4, 8), np.int32), np.zeros((4, 8), np.float32)
H9 = np.eye(3).reshape(9)


def out_msg(shape):
    return f"out must be a contiguous uint8 array of shape {shape}"


def raises(exc, msg, fn, *args, **kwargs):
    with pytest.raises(exc) as e:
        fn(*args, **kwargs)
    assert type(e.value) is exc and str(e.value) == msg, (type(e.value), str(e.value))


class OtherDevice:  # a context object claiming another GPU
    device = 1
    ptr = None


# every wrapper that takes frames first, as a call on the frames alone
FRAME_CALLS = {
    "detect_points": lambda f: fd.detect_points("harris", f, 10),
    "point_candidates": lambda f: fd.point_candidates("harris", f),
    "point_response": lambda f: fd.point_response("harris", f),
    "lsd_map": lambda f: fd.lsd_map(f),
    "lsd_lines": lambda f: fd.lsd_lines(f),
    "blur_frames": lambda f: fd.blur_frames(f, taps=TAPS),
    "equalize_frames": lambda f: fd.equalize_frames(f),
    "warp_frames": lambda f: fd.warp_frames(f, H9),
    "describe_lines": lambda f: fd.describe_lines(f, np.zeros((1, 4, 4), np.float32)),
    "brief_compute": lambda f: fd.brief_compute(f, XY),
    "refine_points": lambda f: fd.refine_points(f, XY),
    "build_pyramid": lambda f: fd.build_pyramid(f, 1),
}


@pytest.mark.parametrize("name", sorted(FRAME_CALLS))
def test_frames_dtype_and_rank(name):
    raises(TypeError, U8, FRAME_CALLS[name], np.zeros((8, 8), np.float32))
    raises(ValueError, RANK, FRAME_CALLS[name], np.zeros((1, 1, 8, 8), np.uint8))


def bad_host_outs(shape):
    """Host arrays that are not `a contiguous writeable uint8 array of shape`."""
    ro = np.zeros(shape, np.uint8)
    ro.flags.writeable = False
    return {"shape": np.zeros(shape + (1,), np.uint8), "dtype": np.zeros(shape, np.float32),
            "strided": np.zeros(shape[:-1] + (2 * shape[-1],), np.uint8)[..., ::2], "read-only": ro,
            "no array": np.zeros(shape, np.uint8).tolist()}


def test_blur_frames_host_checks():
    raises(ValueError, EMPTY, fd.blur_frames, np.zeros((0, 8), np.uint8), taps=TAPS)
    raises(ValueError, EMPTY, fd.blur_frames, np.zeros((0, 8, 8), np.uint8), taps=TAPS)
    raises(ValueError, EMPTY, fd.blur_frames, np.zeros((2, 8, 0), np.uint8), taps=TAPS)
    raises(ValueError, "give either sigma or taps", fd.blur_frames, F8)
    raises(ValueError, "give either sigma or taps", fd.blur_frames, F8, sigma=1.0, taps=TAPS)
    raises(ValueError, "taps must have radius + 1 entries", fd.blur_frames, F8, radius=1, taps=TAPS)
    raises(ValueError, "taps must have 1 to 16 entries: w[0], ..., w[radius]", fd.blur_frames, F8, taps=[1] * 17)
    for frames, step, shape in ((F8, 1, (8, 8)), (B8, 1, (2, 8, 8)), (B8, 2, (2, 4, 4))):
        for what, out in bad_host_outs(shape).items():
            raises(ValueError, out_msg(shape), fd.blur_frames, frames, taps=TAPS, step=step, out=out)
    # wrong twice: the earlier check speaks
    bad = np.zeros((3, 3), np.float32)
    raises(TypeError, U8, fd.blur_frames, np.zeros((0, 8), np.float32), taps=TAPS, out=bad)
    raises(ValueError, EMPTY, fd.blur_frames, np.zeros((0, 8), np.uint8), out=bad)
    raises(ValueError, "give either sigma or taps", fd.blur_frames, F8, out=bad)
    raises(ValueError, "taps must have radius + 1 entries", fd.blur_frames, F8, radius=1, taps=TAPS, out=bad)


def test_equalize_frames_host_checks():
    raises(ValueError, EMPTY, fd.equalize_frames, np.zeros((0, 8), np.uint8))
    raises(ValueError, EMPTY, fd.equalize_frames, np.zeros((0, 8, 8), np.uint8))
    raises(ValueError, "tiles must be (tiles_x, tiles_y) or one int", fd.equalize_frames, F8, tiles=(2, 2, 2))
    tiles = "tiles must be in [1, min(32, cols)] x [1, min(32, rows)]"
    raises(ValueError, tiles, fd.equalize_frames, F8, tiles=0)
    raises(ValueError, tiles, fd.equalize_frames, F8, tiles=(9, 2))
    raises(ValueError, "clip_limit must be in [0, 2e6]", fd.equalize_frames, F8, clip_limit=-1.0)
    raises(ValueError, "clip_limit must be in [0, 2e6]", fd.equalize_frames, F8, clip_limit=float("nan"))
    for frames, shape in ((F8, (8, 8)), (B8, (2, 8, 8))):
        for what, out in bad_host_outs(shape).items():
            raises(ValueError, out_msg(shape), fd.equalize_frames, frames, tiles=2, out=out)
    bad = np.zeros((3, 3), np.float32)
    raises(TypeError, U8, fd.equalize_frames, np.zeros((0, 8), np.float32), tiles=0, out=bad)
    raises(ValueError, EMPTY, fd.equalize_frames, np.zeros((0, 8), np.uint8), tiles=0, out=bad)
    raises(ValueError, tiles, fd.equalize_frames, F8, tiles=0, clip_limit=-1.0, out=bad)
    raises(ValueError, "clip_limit must be in [0, 2e6]", fd.equalize_frames, F8, clip_limit=-1.0, out=bad)


def test_checks_before_the_context():
    models = "model must be one of ['camera', 'homography']"
    raises(ValueError, models, fd.warp_frames, F8, H9, model="affine")
    raises(ValueError, models, fd.warp_frames, np.zeros((8, 8), np.float32), H9, model="affine", fill=300)
    raises(ValueError, 'kernel must be "box" or "gauss"', fd.build_pyramid, F8, kernel="tri")
    raises(ValueError, 'kernel must be "box" or "gauss"', fd.build_pyramid, np.zeros((8, 8), np.float32), kernel="tri")
    raises(TypeError, "point_response takes device frames", fd.point_response, "harris", F8)
    raises(TypeError, "point_response takes device frames", fd.point_response, "harris", F8, append=True)
    raises(ValueError, "a list of lines carries its own counts", fd.describe_lines, F8, [np.zeros((2, 4))], counts=[2])
    raises(TypeError, U8, fd.describe_lines, np.zeros((8, 8), np.float32), [np.zeros((2, 4))], counts=[2])
    raises(ValueError, "a list of lines must hold [n, 4] or [n, 12] arrays of one width", fd.describe_lines, F8, [np.zeros(4)])
    for match, a in ((fd.brief_match, BITS), (fd.nn_match, DESC)):
        raises(ValueError, "guided matching needs q_xy, t_xy and radius together", match, a, a, q_xy=XY)
        raises(ValueError, "model-gated matching needs q_xy and t_xy", match, a, a, model=H9)
        raises(ValueError, "model_kind must be one of ['fundamental', 'homography']", match, a, a, q_xy=XY, t_xy=XY,
               model=H9, model_kind="affine")
    two_view = "model must be one of ['fundamental', 'homography']"
    raises(ValueError, two_view, fd.verify_geometry, XY, XY, model="affine")
    raises(ValueError, two_view, fd.refit_geometry, XY, XY, None, model="affine")
    kinds = "kind must be one of ['rigid', 'similarity']"
    raises(ValueError, kinds, fd.align_points, XYZ, XYZ, kind="affine")


LAYER_X = {
    "bias_relu": "bias_relu: x must be a channels-last float16 [N, C, H, W] device tensor",
    "heat_softmax": "heat_softmax: semi must be a channels-last float16 [N, 65, Hc, Wc] device tensor",
    "desc_normalize": "desc_normalize: desc must be a channels-last float16 [N, C, Hc, Wc] device tensor, C % 8 == 0",
    "conv1_bias_relu": "conv1_bias_relu: x must be a [N, 1, H, W] float16 device tensor",
    "conv64_bias_relu": "conv64_bias_relu: x must be a channels-last float16 [N, 64, H, W] device tensor",
}


def activation(torch, c=64, h=4, w=4, dtype=None, device="cpu"):
    x = torch.zeros((1, c, h, w), dtype=dtype or torch.float16, device=device)
    return x.contiguous(memory_format=torch.channels_last)


def layer_calls(torch, device):
    """Each layer call as a function of its activation, with a well-formed filter and bias."""
    w1 = torch.zeros((64, 1, 3, 3), dtype=torch.float16, device=device)
    w64 = torch.zeros((64, 64, 3, 3), dtype=torch.float16, device=device)
    b64 = torch.zeros((64,), dtype=torch.float16, device=device)
    return {"bias_relu": lambda x: sp.bias_relu(x, b64), "heat_softmax": lambda x: sp.heat_softmax(x),
            "desc_normalize": lambda x: sp.desc_normalize(x), "conv1_bias_relu": lambda x: sp.conv1_bias_relu(x, w1, b64),
            "conv64_bias_relu": lambda x: sp.conv64_bias_relu(x, w64, b64)}


def test_layer_calls_refuse_host_activations():
    import torch

    for name, call in layer_calls(torch, "cpu").items():
        c = {"heat_softmax": 65, "conv1_bias_relu": 1}.get(name, 64)
        raises(ValueError, LAYER_X[name], call, activation(torch, c))
    raises(ValueError, LAYER_X["bias_relu"], sp.bias_relu, np.zeros((1, 64, 4, 4), np.float16), None)


# ------------------------------------------------------------------------------------------------ with a GPU
@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def is_dev(torch, t, shape, dtype):
    return isinstance(t, torch.Tensor) and t.is_cuda and tuple(t.shape) == tuple(shape) and t.dtype == dtype


def is_host(a, shape, dtype):
    return isinstance(a, np.ndarray) and a.shape == tuple(shape) and a.dtype == dtype


@pytest.mark.gpu
def test_context_on_another_device(torch):
    d8, dxy, dbits, x = dev(torch, F8), dev(torch, XY), dev(torch, BITS), activation(torch, device="cuda")
    ctx = OtherDevice()
    calls = [lambda: fd.detect_points("harris", d8, 10, ctx=ctx), lambda: fd.point_response("harris", d8, ctx=ctx),
             lambda: fd.lsd_map(d8, ctx=ctx), lambda: fd.lsd_lines(d8, ctx=ctx),
             lambda: fd.blur_frames(d8, taps=TAPS, ctx=ctx), lambda: fd.equalize_frames(d8, tiles=2, ctx=ctx),
             lambda: fd.blur_frames(F8, taps=TAPS, out=d8, ctx=ctx),  # (the side of out is checked first)
             lambda: fd.warp_frames(d8, H9, ctx=ctx), lambda: fd.warp_frames(F8, dev(torch, H9), ctx=ctx),
             lambda: fd.build_pyramid(d8, 1, ctx=ctx), lambda: fd.describe_lines(d8, np.zeros((1, 4, 4), np.float32), ctx=ctx),
             lambda: fd.brief_compute(d8, dxy, ctx=ctx), lambda: fd.refine_points(F8, dxy, ctx=ctx),
             lambda: fd.track_lk(F8, F8, dxy, levels=1, ctx=ctx), lambda: fd.brief_match(dbits, dbits, ctx=ctx),
             lambda: fd.nn_match(dev(torch, DESC), dev(torch, DESC), ctx=ctx), lambda: fd.verify_geometry(dxy, dxy, ctx=ctx),
             lambda: fd.transform_points(dev(torch, np.zeros(13)), dev(torch, XYZ), ctx=ctx),
             lambda: sp.nn_select(dev(torch, np.zeros((8, 8), np.float32)), ctx=ctx),
             lambda: sp.bias_relu(x, torch.zeros(64), ctx=ctx), lambda: sp.conv64_bias_relu(x, torch.zeros((64, 64, 3, 3)), torch.zeros(64), ctx=ctx)]
    for i, call in enumerate(calls):
        if i == 6:
            raises(ValueError, SIDE, call)
        else:
            raises(ValueError, OTHER_CTX, call)
    # wrong twice: the context is resolved before warp_frames looks at params, after blur_frames looks at out
    raises(ValueError, OTHER_CTX, fd.warp_frames, d8, dev(torch, H9).float(), ctx=ctx)
    raises(ValueError, out_msg((8, 8)), fd.blur_frames, d8, taps=TAPS, out=dev(torch, B8), ctx=ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("stage", ["blur", "equalize"])
def test_frame_stage_out(torch, stage):
    call = (lambda f, **k: fd.blur_frames(f, taps=TAPS, **k)) if stage == "blur" else (lambda f, **k: fd.equalize_frames(f, tiles=2, **k))
    d8, db8 = dev(torch, F8), dev(torch, B8)
    raises(ValueError, SIDE, call, F8, out=torch.empty((8, 8), dtype=torch.uint8, device="cuda"))
    raises(ValueError, SIDE, call, d8, out=np.zeros((8, 8), np.uint8))
    raises(ValueError, SIDE, call, d8, out=torch.empty((8, 8), dtype=torch.uint8))  # (a torch tensor in host memory)
    raises(ValueError, SIDE, call, d8, out=np.zeros((3, 3), np.float32))  # wrong twice: the side first
    raises(ValueError, SIDE, call, B8, out=torch.empty((3,), device="cuda"))
    for what, out in {"shape": torch.empty((8, 9), dtype=torch.uint8, device="cuda"),
                      "dtype": torch.empty((8, 8), dtype=torch.int8, device="cuda"),
                      "strided": torch.empty((8, 16), dtype=torch.uint8, device="cuda")[:, ::2]}.items():
        raises(ValueError, out_msg((8, 8)), call, d8, out=out)
    raises(ValueError, out_msg((2, 8, 8)), call, db8, out=torch.empty((8, 8), dtype=torch.uint8, device="cuda"))
    for frames, shape in ((F8, (8, 8)), (B8, (2, 8, 8))):
        assert is_host(call(frames), shape, np.uint8)
        assert is_dev(torch, call(dev(torch, frames)), shape, torch.uint8)
        out = np.zeros(shape, np.uint8)
        assert call(frames, out=out) is out
        out = torch.empty(shape, dtype=torch.uint8, device="cuda")
        assert call(dev(torch, frames), out=out) is out
    if stage == "blur":
        assert is_host(fd.blur_frames(B8, taps=TAPS, step=2), (2, 4, 4), np.uint8)
        assert is_dev(torch, fd.blur_frames(db8, sigma=1.0, step=2), (2, 4, 4), torch.uint8)
        raises(ValueError, out_msg((2, 4, 4)), fd.blur_frames, db8, taps=TAPS, step=2, out=torch.empty_like(db8))
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_warp_frames_checks(torch):
    d8, dh = dev(torch, F8), dev(torch, H9)
    raises(TypeError, "params must be float64", fd.warp_frames, F8, dh.float())
    raises(ValueError, "params must be [9] or [1, 9] for model 'homography'", fd.warp_frames, F8, np.zeros(8))
    raises(ValueError, "params must be [22] or [2, 22] for model 'camera'", fd.warp_frames, B8, np.zeros((1, 22)), model="camera")
    raises(ValueError, "out_shape must not be negative", fd.warp_frames, F8, H9, out_shape=(-1, 8))
    raises(ValueError, HOST_OUT, fd.warp_frames, F8, H9, out=np.zeros((1, 8, 8), np.uint8))
    raises(ValueError, "fill must be in [0, 255]", fd.warp_frames, F8, H9, fill=300)
    one, two = "out must be contiguous tensors: uint8 (1, 8, 8)", "out must be contiguous tensors: uint8 (1, 8, 8), uint8 (1, 8, 8)"
    o8 = torch.empty((8, 8), dtype=torch.uint8, device="cuda")
    o18, m18 = o8.clone()[None], o8.clone()[None]
    raises(ValueError, one, fd.warp_frames, d8, H9, out=o8)
    raises(ValueError, one, fd.warp_frames, d8, H9, out=o18.int())
    raises(ValueError, two, fd.warp_frames, d8, H9, return_mask=True, out=(o18,))
    raises(ValueError, two, fd.warp_frames, d8, H9, return_mask=True, out=(o18, o8))
    # wrong twice
    raises(TypeError, "params must be float64", fd.warp_frames, F8, dh.float(), out_shape=(-1, 8), fill=300)
    raises(ValueError, "out_shape must not be negative", fd.warp_frames, F8, H9, out_shape=(-1, 8), out=o8, fill=300)
    raises(ValueError, HOST_OUT, fd.warp_frames, F8, H9, out=o18, fill=300)
    raises(ValueError, one, fd.warp_frames, d8, H9, out=o8, fill=300)
    assert fd.warp_frames(d8, H9, out=o18) is o18
    got = fd.warp_frames(d8, dh, return_mask=True, out=(o18, m18))
    assert isinstance(got, tuple) and got[0] is o18 and got[1] is m18
    assert is_host(fd.warp_frames(F8, H9), (1, 8, 8), np.uint8)
    assert is_host(fd.warp_frames(B8, H9, out_shape=(4, 6)), (2, 4, 6), np.uint8)
    assert is_host(fd.warp_frames(B8, H9, out_shape=(0, 6)), (2, 0, 6), np.uint8)
    out, mask = fd.warp_frames(B8, H9, return_mask=True)
    assert is_host(out, (2, 8, 8), np.uint8) and is_host(mask, (2, 8, 8), np.uint8)
    assert is_dev(torch, fd.warp_frames(d8, H9), (1, 8, 8), torch.uint8)
    out, mask = fd.warp_frames(dev(torch, B8), dh, return_mask=True)
    assert is_dev(torch, out, (2, 8, 8), torch.uint8) and is_dev(torch, mask, (2, 8, 8), torch.uint8)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_point_response_and_maps(torch):
    d8, db8 = dev(torch, F8), dev(torch, B8)
    raises(TypeError, "point_candidates takes host frames", fd.point_candidates, "harris", d8)
    raises(ValueError, "append=True needs out=(resp, idx, counts)", fd.point_response, "harris", d8, append=True)
    for kind, cap in (("harris", 96), ("fast", 64)):
        resp, idx, counts = fd.point_response(kind, db8)
        assert is_dev(torch, resp, (2, cap), torch.float32) and is_dev(torch, idx, (2, cap), torch.int32)
        assert is_dev(torch, counts, (2,), torch.int32)
    got = fd.point_response("harris", db8, out=(resp, idx, counts))
    assert got[0] is resp and got[1] is idx and got[2] is counts
    got = fd.point_response("harris", db8, out=(resp, idx, counts), append=True)
    assert got[0] is resp and got[1] is idx and got[2] is counts

    res = fd.lsd_map(B8)
    assert isinstance(res, list) and len(res) == 2 and len(res[0]) == 4
    assert is_host(res[0][0], (7, 7), np.float32) and is_host(res[0][1], (7, 7), np.float32) and is_host(res[0][2], (7, 7), np.uint8)
    assert res[0][3].dtype == np.int32 and res[0][3].ndim == 1
    norm, ang, val, idx, cnt = out = fd.lsd_map(db8)
    assert is_dev(torch, norm, (2, 7, 7), torch.float32) and is_dev(torch, ang, (2, 7, 7), torch.float32)
    assert is_dev(torch, val, (2, 7, 7), torch.uint8) and norm.stride() == (112, 16, 1)
    assert is_dev(torch, idx, (2, 49), torch.int32) and is_dev(torch, cnt, (2,), torch.int64)
    assert fd.lsd_map(db8, out=out) is out
    maps = "lsd_map: maps must be [2, 7, 7] with unit column stride and rows packed at one pitch"
    raises(ValueError, maps, fd.lsd_map, db8, out=(norm[:1], ang, val, idx, cnt))
    raises(ValueError, maps, fd.lsd_map, db8, out=(norm, ang.transpose(1, 2), val, idx, cnt))
    raises(ValueError, "lsd_map: norm / angle / valid must share one row pitch", fd.lsd_map, db8,
           out=(norm, ang.contiguous(), val, idx, cnt))
    raises(ValueError, maps, fd.lsd_map, db8, out=(norm[:1], ang.contiguous(), val, idx, cnt))  # wrong twice
    lines = fd.lsd_lines(B8)
    assert isinstance(lines, list) and len(lines) == 2 and is_host(lines[0], (0, 12), np.float32)
    lines = fd.lsd_lines(db8)
    assert isinstance(lines, list) and len(lines) == 2 and is_host(lines[1], (0, 12), np.float32)

    raises(ValueError, "device frames give a device pyramid", fd.build_pyramid, d8, 1, device_out=False)
    raises(ValueError, 'kernel must be "box" or "gauss"', fd.build_pyramid, d8, 1, device_out=False, kernel="tri")
    for kernel in ("box", "gauss"):
        p = fd.build_pyramid(B8, 2, kernel=kernel)
        assert isinstance(p, fd.Pyramid) and is_host(p.data, (p.offsets[-1],), np.uint8) and p.level(1).shape == (2, 4, 4)
        assert is_dev(torch, fd.build_pyramid(B8, 2, device_out=True, kernel=kernel).data, (p.offsets[-1],), torch.uint8)
        assert is_dev(torch, fd.build_pyramid(db8, 2, kernel=kernel).data, (p.offsets[-1],), torch.uint8)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_png_frames_out(torch):
    from png_util import encode_png

    pngs = [encode_png(np.full((8, 8), 7 * i, np.uint8)) for i in range(2)]
    assert is_dev(torch, fd.png_frames(pngs), (2, 8, 8), torch.uint8)
    out = torch.empty((2, 8, 8), dtype=torch.uint8, device="cuda")
    assert fd.png_frames(pngs, out=out) is out
    msg = "png_frames: out must be a contiguous uint8 cuda:0 tensor of shape (2, 8, 8), got {} {} on {}"
    raises(ValueError, msg.format((2, 8, 9), "torch.uint8", "cuda:0"), fd.png_frames, pngs,
           out=torch.empty((2, 8, 9), dtype=torch.uint8, device="cuda"))
    raises(ValueError, msg.format((2, 8, 8), "torch.int8", "cuda:0"), fd.png_frames, pngs, out=out.to(torch.int8))
    raises(ValueError, msg.format((2, 8, 8), "torch.uint8", "cpu"), fd.png_frames, pngs, out=out.cpu())
    raises(ValueError, msg.format((2, 8, 8), "torch.uint8", "cuda:0"), fd.png_frames, pngs,
           out=torch.empty((2, 8, 16), dtype=torch.uint8, device="cuda")[..., ::2])
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_slot_stage_checks(torch):
    d8, dxy, dbits, ddesc = dev(torch, F8), dev(torch, XY), dev(torch, BITS), dev(torch, DESC)
    lines = np.zeros((1, 4, 4), np.float32)
    # out= on a host call
    for call in (lambda o: fd.refine_points(F8, XY, out=o), lambda o: fd.track_lk(F8, F8, XY, levels=1, out=o),
                 lambda o: fd.describe_lines(F8, lines, out=o), lambda o: fd.brief_match(BITS, BITS, out=o),
                 lambda o: fd.nn_match(DESC, DESC, out=o), lambda o: fd.verify_geometry(XY, XY, out=o),
                 lambda o: fd.solve_pnp(XYZ, XY, (1.0, 1.0, 0.0, 0.0), out=o), lambda o: fd.align_points(XYZ, XYZ, out=o),
                 lambda o: fd.transform_points(np.zeros(13), XYZ, out=o[0])):
        raises(ValueError, HOST_OUT, call, (np.zeros((1, 4, 3), np.float32),))
    # a device out= that does not fit
    o = (torch.empty((1, 4), dtype=torch.int32, device="cuda"),)
    raises(ValueError, "out must be contiguous tensors: float32 (1, 4, 2), uint8 (1, 4), int32 (1,)", fd.refine_points, d8, dxy, out=o)
    raises(ValueError, "out must be contiguous tensors: float32 (1, 4, 2), uint8 (1, 4), float32 (1, 4), int32 (1,)",
           fd.track_lk, d8, d8, dxy, levels=1, out=o)
    raises(ValueError, "out must be contiguous tensors: float32 (1, 4, 72), float32 (1, 4, 2), uint8 (1, 4)",
           fd.describe_lines, d8, dev(torch, lines), out=o)
    raises(ValueError, "out must be contiguous int32 tensors of shapes (1, 4), (1, 4, 2), (1,)", fd.brief_match, dbits, dbits, out=o)
    raises(ValueError, "out must be contiguous tensors: int32 (1, 4), float32 (1, 4, 2), int32 (1,)", fd.nn_match, ddesc, ddesc, out=o)
    raises(ValueError, "out must be contiguous tensors: float64 (1, 9), uint8 (1, 4), int32 (1,), int32 (1,)",
           fd.verify_geometry, dxy, dxy, out=o)
    raises(ValueError, "out must be contiguous tensors: float32 (1, 4, 3)", fd.transform_points, dev(torch, np.zeros(13)),
           dev(torch, XYZ), out=o[0])
    raises(ValueError, "out must be a contiguous int32 tensor of shape (1, 4, 8)", fd.brief_compute, d8, dxy, out=o[0])
    # the two sides of a call
    raises(ValueError, "q_bits and t_bits must both be device tensors or both host arrays", fd.brief_match, BITS, dbits)
    raises(ValueError, "q_desc and t_desc must both be device tensors or both host arrays", fd.nn_match, ddesc, DESC)
    raises(ValueError, "q_xy must be on the side (host / device) of the descriptors", fd.brief_match, BITS, BITS, q_xy=dxy, t_xy=XY, radius=1.0)
    raises(ValueError, "model must be on the side (host / device) of the descriptors", fd.nn_match, DESC, DESC, q_xy=XY, t_xy=XY,
           model=dev(torch, H9))
    raises(ValueError, "t_xy must be on the side (host / device) of q_xy", fd.verify_geometry, XY, dxy)
    raises(ValueError, "t_xy must be on the side (host / device) of q_xy", fd.verify_geometry, dxy, XY, out=o)
    raises(ValueError, "guess must be on the side (host / device) of xy", fd.track_lk, F8, F8, XY, guess=dxy, levels=1)
    raises(ValueError, "points, point_valid and the given result must be on the side (host / device) of t_xy",
           fd.solve_pnp, dev(torch, XYZ), XY, (1.0, 1.0, 0.0, 0.0))
    raises(ValueError, "t_xyz, the masks and the given result must be on the side (host / device) of q_xyz",
           fd.align_points, XYZ, dev(torch, XYZ))
    raises(ValueError, "model, valid and counts must be on the side (host / device) of xyz", fd.transform_points,
           dev(torch, np.zeros(13)), XYZ)
    # dtype, rank and batch of the slot arrays
    raises(TypeError, "xy must be float32", fd.refine_points, F8, XY.astype(np.float64))
    raises(ValueError, "xy must be [batch, S, 2] or [S, 2]", fd.refine_points, F8, XYZ)
    raises(ValueError, "xy and the frames must have the same batch", fd.refine_points, B8, XY)
    raises(TypeError, "xy must be float32", fd.track_lk, d8, d8, dxy.double(), levels=1)
    raises(ValueError, "xy and the frames must have the same batch", fd.track_lk, B8, B8, XY, levels=1)
    raises(ValueError, "prev and next must have the same batch, rows and cols", fd.track_lk, F8, B8, XY, levels=1)
    raises(ValueError, "uv must be [batch, S, 2] matching frames", fd.brief_compute, F8, XYZ)
    raises(ValueError, "uv must be [batch, S, 2] matching frames", fd.brief_compute, B8, XY)
    raises(TypeError, "lines must be float32", fd.describe_lines, F8, lines.astype(np.float64))
    raises(ValueError, "lines must be [batch, S, 4 or 12] or [S, 4 or 12]", fd.describe_lines, F8, np.zeros((4, 5), np.float32))
    raises(ValueError, "lines and the frames must have the same batch", fd.describe_lines, B8, lines)
    raises(ValueError, "bands must be in [1, 32] and band_width in [1, 16]", fd.describe_lines, F8, lines, bands=0)
    raises(TypeError, "q_bits must be int32 or uint32 words", fd.brief_match, BITS.astype(np.float32), BITS)
    raises(ValueError, "t_bits must be [batch, S, 8] or [S, 8]", fd.brief_match, BITS, BITS[:, :4])
    raises(ValueError, "q_bits and t_bits must have the same batch", fd.brief_match, BITS, np.zeros((2, 4, 8), np.int32))
    raises(TypeError, "t_desc must be float32", fd.nn_match, ddesc, ddesc.double())
    raises(ValueError, "q_desc must be [batch, S, dim] or [S, dim]", fd.nn_match, np.zeros((1, 1, 4, 8), np.float32), DESC)
    raises(ValueError, "q_desc and t_desc must have the same dim", fd.nn_match, DESC, DESC[:, :4])
    raises(TypeError, "q_xy must be float32", fd.verify_geometry, XY.astype(np.float64), XY)
    raises(ValueError, "q_xy and t_xy must have the same batch", fd.verify_geometry, XY, np.zeros((2, 4, 2), np.float32))
    raises(ValueError, "without matches slot i pairs with slot i: t_xy needs at least as many slots as q_xy",
           fd.verify_geometry, XY, XY[:2])
    # results: a host call ignores brief_compute's out=; the matchers return out= as it is
    r = fd.brief_match(BITS, BITS)
    assert is_host(r.idx, (1, 4), np.int32) and is_host(r.dist, (1, 4, 2), np.int32) and is_host(r.counts, (1,), np.int32)
    r = fd.nn_match(ddesc, ddesc)
    assert is_dev(torch, r.idx, (1, 4), torch.int32) and is_dev(torch, r.dist, (1, 4, 2), torch.float32)
    assert is_dev(torch, r.counts, (1,), torch.int32)
    o = (torch.empty((1, 4), dtype=torch.int32, device="cuda"), torch.empty((1, 4, 2), dtype=torch.int32, device="cuda"),
         torch.empty((1,), dtype=torch.int32, device="cuda"))
    r = fd.brief_match(dbits, dbits, out=o)
    assert r.idx is o[0] and r.dist is o[1] and r.counts is o[2]
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_nn_wrappers(torch):
    heat = np.zeros((2, 8, 8), np.float32)
    xy, cnt = sp.nn_select(heat)
    assert is_host(xy, (2, 241, 2), np.float32) and is_host(cnt, (2,), np.int32)
    xy, cnt = sp.nn_select(dev(torch, heat), sp.Options(kMaxNumberOfDetectedFeatures=3))
    assert is_dev(torch, xy, (2, 4, 2), torch.float32) and is_dev(torch, cnt, (2,), torch.int32)
    got = sp.nn_select(dev(torch, heat), out=(xy, cnt))
    assert got[0] is xy and got[1] is cnt
    raises(ValueError, "prior must have one entry per frame", sp.nn_select, heat, prior=[XY])
    kp, sc = np.zeros((1, 4, 2), np.int64), np.zeros((1, 4), np.float32)
    raises(ValueError, "keypoints must be [B, K, 2] matching scores [B, K]", sp.nn_select_list, np.zeros((1, 4, 3), np.int64), sc, 8, 8)
    raises(ValueError, "keypoints must be [B, K, 2] matching scores [B, K]", sp.nn_select_list, dev(torch, kp)[:, :3], dev(torch, sc), 8, 8)
    xy, cnt, d = sp.nn_select_list(kp, sc, 8, 8, descriptors=np.zeros((1, 4, 8), np.float32))
    assert is_host(xy, (1, 241, 2), np.float32) and is_host(cnt, (1,), np.int32) and is_host(d, (1, 241, 8), np.float32)
    xy, cnt, d = sp.nn_select_list(dev(torch, kp), dev(torch, sc), 8, 8)
    assert is_dev(torch, xy, (1, 241, 2), torch.float32) and is_dev(torch, cnt, (1,), torch.int32) and d is None
    dmap = np.zeros((1, 8, 2, 2), np.float32)
    assert is_host(sp.nn_descriptors(dmap, XY[None]), (1, 4, 8), np.float32)
    assert is_dev(torch, sp.nn_descriptors(dev(torch, dmap), dev(torch, XY[None])), (1, 4, 8), torch.float32)
    out = torch.zeros((1, 4, 8), dtype=torch.float32, device="cuda")
    assert sp.nn_descriptors(dev(torch, dmap), dev(torch, XY[None]), out=out) is out
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_layer_call_checks(torch):
    cl, f16 = torch.channels_last, torch.float16
    x, x1, x65 = activation(torch, device="cuda"), activation(torch, 1, device="cuda"), activation(torch, 65, device="cuda")
    odd = activation(torch, 64, 3, 4, device="cuda")
    b64, b63 = torch.zeros(64), torch.zeros(63)
    w1, w64 = torch.zeros((64, 1, 3, 3), dtype=f16), torch.zeros((64, 64, 3, 3), dtype=f16)
    calls = layer_calls(torch, "cuda")
    # the activation: dtype, rank, channels, layout
    for name, call in calls.items():
        c = {"heat_softmax": 65, "conv1_bias_relu": 1}.get(name, 64)
        good = activation(torch, c, device="cuda")
        bad = [good.float(), good[0], good.cpu() if name in ("bias_relu", "heat_softmax", "desc_normalize") else good.float()]
        if c != 1:
            bad.append(good.contiguous())  # plain NCHW
        bad.append(activation(torch, {"bias_relu": 64, "desc_normalize": 12}.get(name, 2), device="cuda"))
        for t in bad[:-1] + ([] if name == "bias_relu" else bad[-1:]):
            raises(ValueError, LAYER_X[name], call, t)
    # bias_relu
    raises(ValueError, "bias_relu: pooling needs even H and W", sp.bias_relu, odd, b64, pool=True)
    out_br = "bias_relu: out must be a channels-last float16 [1, 64, 4, 4] tensor on cuda:0"
    for out in (torch.empty_like(x).float(), torch.empty_like(x)[:, :, :2], torch.empty_like(x).contiguous(), torch.empty_like(x).cpu()):
        raises(ValueError, out_br, sp.bias_relu, x, b64, out=out)
    raises(ValueError, "bias_relu: out must be a channels-last float16 [1, 64, 2, 2] tensor on cuda:0", sp.bias_relu, x, b64, pool=True, out=x)
    raises(ValueError, "bias_relu: bias has 63 values for 64 channels", sp.bias_relu, x, b63)
    raises(ValueError, "bias_relu: pooling needs even H and W", sp.bias_relu, odd, b63, pool=True, out=x)  # wrong three times
    raises(ValueError, out_br, sp.bias_relu, x, b63, out=x.float())
    # heads
    raises(ValueError, "heat_softmax: bias must hold 65 values", sp.heat_softmax, x65, b64)
    raises(ValueError, "desc_normalize: bias must hold 64 values", sp.desc_normalize, x, b63)
    # conv1_bias_relu
    w_c1 = "conv1_bias_relu: weight must be [C, 1, 3, 3] float16 and bias C values"
    raises(ValueError, w_c1, sp.conv1_bias_relu, x1, w1.float(), b64)
    raises(ValueError, w_c1, sp.conv1_bias_relu, x1, w64, b64)
    raises(ValueError, w_c1, sp.conv1_bias_relu, x1, w1, b63)
    out_c1 = "conv1_bias_relu: out must be a channels-last float16 [1, 64, 4, 4] tensor"
    for out in (torch.empty_like(x).float(), torch.empty_like(x)[:, :, :2], torch.empty_like(x).contiguous()):
        raises(ValueError, out_c1, sp.conv1_bias_relu, x1, w1, b64, out=out)
    raises(ValueError, w_c1, sp.conv1_bias_relu, x1, w1, b63, out=x.float())
    # conv64_bias_relu
    w_c64 = "conv64_bias_relu: weight must be [64 k, 64, 3, 3] and bias as many values"
    raises(ValueError, w_c64, sp.conv64_bias_relu, x, torch.zeros((32, 64, 3, 3), dtype=f16), torch.zeros(32))
    raises(ValueError, w_c64, sp.conv64_bias_relu, x, torch.zeros((64, 32, 3, 3), dtype=f16), b64)
    raises(ValueError, w_c64, sp.conv64_bias_relu, x, w64, b63)
    raises(ValueError, "conv64_bias_relu: pooling needs even H and W", sp.conv64_bias_relu, odd, w64, b64, pool=True)
    out_c64 = "conv64_bias_relu: out must be a channels-last float16 [1, 64, 4, 4] tensor"
    for out in (torch.empty_like(x).float(), torch.empty_like(x)[:, :, :2], torch.empty_like(x).contiguous()):
        raises(ValueError, out_c64, sp.conv64_bias_relu, x, w64, b64, out=out)
    packed = "conv64_bias_relu: packed must be 1 float16 [9, 64, 64] blocks on cuda:0"
    blk = torch.zeros((9, 64, 64), dtype=f16, device="cuda")
    for p in ([blk.float()], [blk.cpu()], [blk[:8]], [blk, blk], []):
        raises(ValueError, packed, sp.conv64_bias_relu, x, w64, b64, packed=p)
    raises(ValueError, w_c64, sp.conv64_bias_relu, x, w64, b63, pool=True, out=x.float(), packed=[])
    raises(ValueError, "conv64_bias_relu: pooling needs even H and W", sp.conv64_bias_relu, odd, w64, b64, pool=True, out=x.float(), packed=[])
    raises(ValueError, out_c64, sp.conv64_bias_relu, x, w64, b64, out=x.float(), packed=[])
    assert tuple(sp.pack_conv3x3_weight(w64).shape) == (9, 64, 64) and sp.pack_conv3x3_weight(w64).is_contiguous()

    # results
    def is_act(t, shape, dtype=f16):
        return is_dev(torch, t, shape, dtype) and t.is_contiguous(memory_format=cl)

    assert is_act(sp.bias_relu(x, b64), (1, 64, 4, 4)) and is_act(sp.bias_relu(x, b64, pool=True), (1, 64, 2, 2))
    assert is_dev(torch, sp.heat_softmax(x65), (1, 32, 32), torch.float32)
    assert is_dev(torch, sp.heat_softmax(x65, torch.zeros(65)), (1, 32, 32), torch.float32)
    assert is_act(sp.desc_normalize(x), (1, 64, 4, 4), torch.float32) and is_act(sp.desc_normalize(x, b64), (1, 64, 4, 4), torch.float32)
    assert is_act(sp.conv1_bias_relu(x1, w1, b64), (1, 64, 4, 4))
    assert is_act(sp.conv1_bias_relu(x1.contiguous(), w1.cuda(), b64), (1, 64, 4, 4))  # plain NCHW passes here
    assert is_act(sp.conv64_bias_relu(x, w64, b64), (1, 64, 4, 4)) and is_act(sp.conv64_bias_relu(x, w64, b64, pool=True), (1, 64, 2, 2))
    assert is_act(sp.conv64_bias_relu(x, w64, b64, packed=[blk]), (1, 64, 4, 4))
    out = torch.empty_like(x)
    assert sp.bias_relu(x, b64, out=out) is out and sp.bias_relu(x, b64, out=x) is x
    assert sp.conv1_bias_relu(x1, w1, b64, out=out) is out and sp.conv64_bias_relu(x, w64, b64, out=out) is out
    torch.cuda.synchronize()
