"""The NN stages over the C ABI: the selection and descriptor post-processing behind fd_nn_select / fd_nn_select_list /
fd_nn_descriptors, and the SuperPoint layer kernels (fd_nn_bias_relu, fd_nn_heat_softmax, fd_nn_desc_normalize,
fd_nn_conv3x3_c1, fd_nn_conv3x3_c64). The networks that call them are in superpoint.py.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._context import Context, bind_stream, invoke, is_device_tensor, resolve_ctx
from ._lib import fd_nn_opts
from ._slots import ptr


@dataclass
class Options:
    """NNFeaturePointDetector::Options (nn_feature_point_detector.h:22-31)."""
    kInvalidBoundary: int = 3
    kMinFeatureDistance: int = 15
    kMaxImageRows: int = 480
    kMaxImageCols: int = 752
    kMaxNumberOfDetectedFeatures: int = 240
    kMinResponse: float = 0.1
    kModelType: str = "kSuperpointHeatmap"
    kComputeDescriptors: bool = False


def _opts(o: Options, max_response: float = 1.0) -> fd_nn_opts:
    return fd_nn_opts(int(o.kInvalidBoundary), int(o.kMinFeatureDistance), int(o.kMaxNumberOfDetectedFeatures),
                      float(o.kMinResponse), float(max_response))


def _prior_arrays(prior, b):
    """Per-frame prior features (list of (n_i, 2) (x, y) arrays) -> (flat float32 [sum, 2], counts int32)."""
    if prior is None:
        return None, None
    if len(prior) != b:
        raise ValueError("prior must have one entry per frame")
    pcnt = np.array([len(p) for p in prior], np.int32)
    pflat = (np.ascontiguousarray(np.concatenate([np.asarray(p, np.float32).reshape(-1, 2) for p in prior]))
             if pcnt.sum() > 0 else np.zeros((1, 2), np.float32))
    return pflat, pcnt


def nn_select(heat, options: Options | None = None, prior=None, out=None, ctx: Context | None = None,
              max_response: float = 1.0):
    """fd_nn_select on heatmaps [B, H, W] float32 (numpy, or a torch device tensor -> device outputs).

    max_response: declared upper bound of the heatmap (1.0: softmax probabilities); float('inf') for
    arbitrary maps (coarser selection keys). A value above it fails the call.
    Returns (xy [B, max+1, 2] float32, counts [B] int32): new features per frame, selection order.
    prior: None or a list (per frame) of (n_i, 2) float arrays of (x, y), host memory.
    """
    o = options or Options()
    ctx = resolve_ctx(ctx, heat)
    opts = _opts(o, max_response)
    on_dev = is_device_tensor(heat)
    if on_dev:
        import torch

        heat = heat.to(torch.float32).contiguous()
    else:
        heat = np.ascontiguousarray(heat, np.float32)
    if heat.ndim == 2:
        heat = heat[None]
    b, r, c = (int(v) for v in heat.shape)
    stride = max(int(o.kMaxNumberOfDetectedFeatures), 1) + 1
    pflat, pcnt = _prior_arrays(prior, b)
    if on_dev:
        if out is None:
            out = (torch.empty((b, stride, 2), dtype=torch.float32, device=heat.device),
                   torch.empty((b,), dtype=torch.int32, device=heat.device))
        xy, cnt = out
        stride = xy.shape[1]
    else:
        xy = np.zeros((b, stride, 2), np.float32)
        cnt = np.zeros((b,), np.int32)
    invoke(ctx, on_dev, "fd_nn_select", ptr(heat), 1 if on_dev else 0, b, r, c, ctypes.byref(opts), ptr(pflat), ptr(pcnt),
           ptr(xy), int(stride), ptr(cnt), 1 if on_dev else 0)
    return xy, cnt


def nn_select_list(keypoints, scores, rows: int, cols: int, counts=None, options: Options | None = None, prior=None,
                   descriptors=None, out=None, ctx: Context | None = None):
    """fd_nn_select_list: the keypoint-list models' selection (DirectlySelectGoodFeaturesWithDescriptors).

    keypoints [B, K, 2] int64 (u, v) in a rows x cols frame, scores [B, K] float32, counts [B] int64
    (None: K each),
    descriptors [B, K, D] float32 or None. numpy inputs give numpy outputs; torch device tensors give
    device outputs (current stream). Returns (xy [B, max+1, 2], counts [B] int32, desc [B, max+1, D] or
    None): the new features per frame in selection order and their descriptor rows.
    prior: None or a list (per frame) of (n_i, 2) float arrays of (x, y), host memory.
    """
    o = options or Options()
    on_dev = is_device_tensor(scores)
    ctx = resolve_ctx(ctx, scores)
    opts = _opts(o, float("inf"))
    stride = max(int(o.kMaxNumberOfDetectedFeatures), 1) + 1
    pflat, pcnt = _prior_arrays(prior, int(scores.shape[0]))
    if on_dev:
        import torch

        kp = keypoints.to(torch.int64).contiguous()
        sc = scores.to(torch.float32).contiguous()
        b, k = (int(v) for v in sc.shape)
        cnt_in = (torch.full((b,), k, dtype=torch.int64, device=sc.device) if counts is None
                  else counts.to(torch.int64).contiguous())
        dd = None if descriptors is None else descriptors.to(torch.float32).contiguous()
        dim = 0 if dd is None else int(dd.shape[2])
        if out is None:
            out = (torch.empty((b, stride, 2), dtype=torch.float32, device=sc.device),
                   torch.empty((b,), dtype=torch.int32, device=sc.device),
                   None if dd is None else torch.zeros((b, stride, dim), dtype=torch.float32, device=sc.device))
        xy, cnt, dout = out
        stride = xy.shape[1]
    else:
        kp = np.ascontiguousarray(keypoints, np.int64)
        sc = np.ascontiguousarray(scores, np.float32)
        b, k = sc.shape
        cnt_in = np.full((b,), k, np.int64) if counts is None else np.ascontiguousarray(counts, np.int64)
        dd = None if descriptors is None else np.ascontiguousarray(descriptors, np.float32)
        dim = 0 if dd is None else dd.shape[2]
        xy = np.zeros((b, stride, 2), np.float32)
        cnt = np.zeros((b,), np.int32)
        dout = None if dd is None else np.zeros((b, stride, dim), np.float32)
    if tuple(kp.shape) != (b, k, 2):
        raise ValueError("keypoints must be [B, K, 2] matching scores [B, K]")
    invoke(ctx, on_dev, "fd_nn_select_list", ptr(kp), ptr(sc), ptr(cnt_in), int(k), 1 if on_dev else 0, b, int(rows), int(cols),
           ctypes.byref(opts), ptr(pflat), ptr(pcnt), ptr(dd), int(dim), ptr(dout), ptr(xy), int(stride), ptr(cnt),
           1 if on_dev else 0)
    return xy, cnt, dout


def _activation(x, name, arg, dims, on_device, channels_ok, suffix=""):
    """Refuse anything but a channels-last float16 [N, C, H, W] activation on the device. on_device: the wrapper's own
    device test, channels_ok: its test of C; name, arg, dims and suffix word the message."""
    import torch

    if not (on_device(x) and x.dtype == torch.float16 and x.dim() == 4 and channels_ok(x.shape[1])
            and x.is_contiguous(memory_format=torch.channels_last)):
        raise ValueError(f"{name}: {arg} must be a channels-last float16 {dims} device tensor{suffix}")


def _is_cuda(x):
    return x.is_cuda


def _any(c):
    return True


def _output(out, name, shape, x, same_device=False):
    """The channels-last float16 result of `shape`: a fresh tensor on x's device, or the caller's out=, checked (with
    same_device also for being a tensor on x's device)."""
    import torch

    if out is None:
        return torch.empty(shape, dtype=torch.float16, device=x.device, memory_format=torch.channels_last)
    if not ((not same_device or (is_device_tensor(out) and out.device == x.device)) and out.dtype == torch.float16
            and tuple(out.shape) == shape and out.is_contiguous(memory_format=torch.channels_last)):
        raise ValueError(f"{name}: out must be a channels-last float16 {list(shape)} tensor" + (f" on {x.device}" if same_device else ""))
    return out


def _bias(bias, device, n=None, msg=None):
    """bias as contiguous float16 values on `device` (None stays None); with n, any other count is ValueError(msg)."""
    import torch

    if bias is None:
        return None
    if n is not None and bias.numel() != n:
        raise ValueError(msg)
    return bias.detach().to(device=device, dtype=torch.float16).contiguous()


def bias_relu(x, bias, pool: bool = False, out=None, ctx: Context | None = None):
    """fd_nn_bias_relu: relu(x + bias) (and the 2x2 max pool when pool) of a channels-last fp16
    activation [N, C, H, W] on the device, in one pass (torch's current stream). x is the output of a
    bias-free convolution; the result equals PyTorch's separate half-precision add / ReLU (/ MaxPool2d(2,
    2)) ops on it, bit for bit (not a conv-with-bias, whose bias is added before the rounding to half;
    and a NaN sum gives 0 here). out: preallocated result (may be x itself when not pooling)."""
    _activation(x, "bias_relu", "x", "[N, C, H, W]", is_device_tensor, _any)
    n, c, h, w = x.shape
    if pool and (h % 2 or w % 2):
        raise ValueError("bias_relu: pooling needs even H and W")
    out = _output(out, "bias_relu", (n, c, h // 2, w // 2) if pool else (n, c, h, w), x, same_device=True)
    b = _bias(bias, x.device, c, f"bias_relu: bias has {bias.numel()} values for {c} channels")
    invoke(resolve_ctx(ctx, x), True, "fd_nn_bias_relu", ptr(x), ptr(b), int(b.numel()), ptr(out), int(n), int(h), int(w), int(c),
           1 if pool else 0)
    return out


def heat_softmax(semi, bias=None, ctx: Context | None = None):
    """fd_nn_heat_softmax: SuperPoint's detector-head output from convPb's logits [N, 65, Hc, Wc]
    (channels-last fp16, on the device): softmax over the 65 channels in float, the dustbin dropped,
    pixel_shuffle(8) -> heat [N, 8 Hc, 8 Wc] float32, in one pass (PyTorch: float copy, softmax, slice,
    shuffle). bias (65 values): added to semi in half first (semi from a bias-free convolution). Within
    float rounding of torch.softmax((semi + bias).float(), 1)[:, :-1] shuffled."""
    import torch

    _activation(semi, "heat_softmax", "semi", "[N, 65, Hc, Wc]", is_device_tensor, lambda c: c == 65)
    n, _, hc, wc = semi.shape
    b = _bias(bias, semi.device, 65, "heat_softmax: bias must hold 65 values")
    heat = torch.empty((n, 8 * hc, 8 * wc), dtype=torch.float32, device=semi.device)
    invoke(resolve_ctx(ctx, semi), True, "fd_nn_heat_softmax", ptr(semi), ptr(b), ptr(heat), int(n), int(hc), int(wc))
    return heat


def desc_normalize(desc, bias=None, ctx: Context | None = None):
    """fd_nn_desc_normalize: SuperPoint's descriptor-head output from convDb's [N, C, Hc, Wc] (channels-last
    fp16, on the device): each cell's vector over its L2 norm (clamped to 1e-12) in float -> [N, C, Hc, Wc]
    float32 channels-last, in one pass (PyTorch: float copy, norm, division). bias (C values): added in
    half first (desc from a bias-free convolution). Within float rounding of d.float() /
    d.float().norm(dim=1, keepdim=True).clamp_min(1e-12), d = desc + bias."""
    import torch

    _activation(desc, "desc_normalize", "desc", "[N, C, Hc, Wc]", is_device_tensor, lambda c: c % 8 == 0, ", C % 8 == 0")
    n, c, hc, wc = desc.shape
    b = _bias(bias, desc.device, c, f"desc_normalize: bias must hold {c} values")
    out = torch.empty((n, c, hc, wc), dtype=torch.float32, device=desc.device, memory_format=torch.channels_last)
    invoke(resolve_ctx(ctx, desc), True, "fd_nn_desc_normalize", ptr(desc), ptr(b), ptr(out), int(n) * int(hc) * int(wc), int(c))
    return out


def conv1_bias_relu(x, weight, bias, out=None, ctx: Context | None = None):
    """fd_nn_conv3x3_c1: the encoder's first layer (1 input channel, 3x3, stride 1, padding 1) with its bias
    and ReLU in one pass: x [N, 1, H, W] fp16 on the device -> [N, C, H, W] fp16 channels-last. The 9
    products are summed in float and rounded to half, then the bias is added in float and rounded (as the
    bias-free convolution followed by bias_relu); within fp16 rounding of PyTorch's convolution + ReLU.
    W <= 4096 (the kernel's row staging); a wider frame is refused."""
    import torch

    # (its own check: a plain-contiguous x passes too, and the message names no layout)
    if not (x.is_cuda and x.dtype == torch.float16 and x.dim() == 4 and x.shape[1] == 1
            and (x.is_contiguous() or x.is_contiguous(memory_format=torch.channels_last))):
        raise ValueError("conv1_bias_relu: x must be a [N, 1, H, W] float16 device tensor")
    n, _, h, w = x.shape
    c = weight.shape[0]
    if tuple(weight.shape) != (c, 1, 3, 3) or weight.dtype != torch.float16 or bias.numel() != c:
        raise ValueError("conv1_bias_relu: weight must be [C, 1, 3, 3] float16 and bias C values")
    out = _output(out, "conv1_bias_relu", (n, c, h, w), x)
    ctx = resolve_ctx(ctx, x)
    wt = weight.detach().to(device=x.device, dtype=torch.float16).contiguous()  # (the kernel reads it on x's device)
    invoke(ctx, True, "fd_nn_conv3x3_c1", ptr(x), ptr(wt), ptr(_bias(bias, x.device)), c, ptr(out), n, h, w)
    return out


def pack_conv3x3_weight(weight):
    """[C_out, C_in, 3, 3] -> [9 taps (ky, kx)][C_out][C_in] contiguous (fd_nn_conv3x3_c64's filter layout)."""
    return weight.detach().permute(2, 3, 0, 1).reshape(9, weight.shape[0], weight.shape[1]).contiguous()


def conv64_bias_relu(x, weight, bias, pool: bool = False, out=None, ctx: Context | None = None, packed=None):
    """fd_nn_conv3x3_c64: 3x3 convolution from 64 channels to a multiple of 64 (stride 1, padding 1) + bias +
    ReLU (+ 2x2 max pool) on the matrix cores, one call per 64-output-channel block: x [N, 64, H, W] fp16
    channels-last on the device -> [N, C_out, H(/2), W(/2)] fp16 channels-last. fp16 products summed in
    float, the sum rounded to half, then the bias added in float and rounded (as the bias-free
    convolution + bias_relu path). packed: the filter's blocks already in pack_conv3x3_weight's layout
    (a list, one per 64 output channels; reused across calls)."""
    import torch

    _activation(x, "conv64_bias_relu", "x", "[N, 64, H, W]", _is_cuda, lambda c: c == 64)
    n, c, h, w = x.shape
    co = weight.shape[0]
    if co % 64 or tuple(weight.shape) != (co, 64, 3, 3) or bias.numel() != co:
        raise ValueError("conv64_bias_relu: weight must be [64 k, 64, 3, 3] and bias as many values")
    if pool and (h % 2 or w % 2):
        raise ValueError("conv64_bias_relu: pooling needs even H and W")
    out = _output(out, "conv64_bias_relu", (n, co, h // 2, w // 2) if pool else (n, co, h, w), x)
    if packed is None:
        packed = [pack_conv3x3_weight(weight[k:k + 64].to(device=x.device, dtype=torch.float16)) for k in range(0, co, 64)]
    elif any(wp.device != x.device or wp.dtype != torch.float16 or tuple(wp.shape) != (9, 64, 64) for wp in packed) \
            or len(packed) != co // 64:
        raise ValueError(f"conv64_bias_relu: packed must be {co // 64} float16 [9, 64, 64] blocks on {x.device}")
    b = _bias(bias, x.device)
    ctx = resolve_ctx(ctx, x)
    bind_stream(ctx, True)  # once, then one call per block
    for blk, wp in enumerate(packed):
        rc = _lib.load().fd_nn_conv3x3_c64(ctx.ptr, ptr(x), ptr(wp), ptr(b[blk * 64:(blk + 1) * 64]), ptr(out), n, h, w,
                                            1 if pool else 0, co, blk * 64)
        _lib.check(ctx.ptr, rc)
    return out


def nn_descriptors(desc_map, xy, counts=None, out=None, ctx: Context | None = None):
    """fd_nn_descriptors: desc_map [B, C, h, w] float32, xy [B, S, 2] -> descriptors [B, S, C].

    Host arrays give numpy outputs; torch device tensors give device outputs (current stream)."""
    ctx = resolve_ctx(ctx, desc_map, xy)
    on_dev, layout = is_device_tensor(desc_map), 0
    if on_dev:
        import torch

        m = desc_map.to(torch.float32)
        b, ch, h, w = (int(v) for v in m.shape)
        # a channels-last map (the network's output) is read in place; anything else as NCHW
        if m.is_contiguous(memory_format=torch.channels_last) and not m.is_contiguous():
            layout = 1
        else:
            m = m.contiguous()
        xy = xy.to(torch.float32).contiguous()
        s = int(xy.shape[1])
        cnt = None if counts is None else counts.to(torch.int32).contiguous()
        res = out if out is not None else torch.zeros((b, s, ch), dtype=torch.float32, device=m.device)
    else:
        m = np.ascontiguousarray(desc_map, np.float32)
        b, ch, h, w = m.shape
        xy = np.ascontiguousarray(np.asarray(xy, np.float32).reshape(b, -1, 2))
        s = xy.shape[1]
        cnt = None if counts is None else np.ascontiguousarray(np.asarray(counts, np.int32).reshape(b))
        res = np.zeros((b, s, ch), np.float32)
    invoke(ctx, on_dev, "fd_nn_descriptors", ptr(m), 1 if on_dev else 0, layout, b, ch, h, w, ptr(xy), ptr(cnt), s, ptr(res),
           1 if on_dev else 0)
    return res
