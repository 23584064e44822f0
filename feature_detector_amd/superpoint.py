"""NN keypoints + descriptors: the networks in PyTorch-ROCm, the post-processing in
the HIP kernels behind fd_nn_select / fd_nn_select_list / fd_nn_descriptors and the layer kernels (nn_layers.py).

Mirrors feature_detector::NNFeaturePointDetector (src/nn_feature_point_detector/
nn_feature_point_detector.h:12-86) for its four model types (ModelType, :15-20):
  Initialize()                          nn_feature_point_detector.cpp:10-57 (network + one warm-up run)
  DetectGoodFeaturesWithDescriptor()    nn_feature_point_detector_superpoint.cpp:8-112 / _disk.cpp:8-112
    InferenceSession                    -> the network (fp16 convs through MIOpen, fp32 outputs); DISK
                                           models take the gray frame as RGB (:96-99)
    heatmap models (kSuperpointHeatmap, kDiskHeatmap):
      CreateMask + candidates + selection -> fd_nn_select (GPU, std::multimap order)
      ExtractDescriptorsForSelectedFeatures -> fd_nn_descriptors for the priors and the new features
                                           (the reference describes every entry of all_pixel_uv)
    keypoint-list models (kSuperpointNms, kDiskNms: NMS in the graph):
      ArgSort + DirectlySelectGoodFeaturesWithDescriptors -> fd_nn_select_list (GPU selection +
                                           descriptor-row gather; new features only, as :223-227)

The reference loads trained ONNX models (onnx_models/*.onnx) that are not available here
(.MISSING_LARGE_BLOBS), and ONNX Runtime is absent: the networks are the published SuperPoint
architecture and a DISK-shaped U-Net with seeded random weights, with in-graph NMS + top-K heads for
the list models, so keypoints from them are meaningful for throughput only. The post-processing is
bit-exact to the oracle's restatement on any given network output.
"""
from __future__ import annotations

import os
from dataclasses import dataclass

import numpy as np

# (the stream binder and context resolver under their earlier names: the layer tests launch kernels through them)
from ._context import bind_stream as _bind_stream, resolve_ctx as _resolve_ctx  # noqa: F401
from .nn_layers import (Options, bias_relu, conv1_bias_relu, conv64_bias_relu, desc_normalize, heat_softmax, nn_descriptors,  # noqa: F401
                        nn_select, nn_select_list, pack_conv3x3_weight)

MODEL_TYPES = ("kSuperpointHeatmap", "kSuperpointNms", "kDiskHeatmap", "kDiskNms")  # ModelType (:15-20)
DESCRIPTOR_DIM = {"superpoint": 256, "disk": 128}  # SuperpointDescriptorType / DiskDescriptorType


def simple_nms(heat, radius: int):
    """In-graph NMS of the keypoint-list models (the max-pool suppression SuperPoint/DISK exports use):
    a score survives where it is the maximum of its (2r+1)^2 window, twice refined around the kept ones."""
    import torch
    import torch.nn.functional as F

    def mp(x):
        return F.max_pool2d(x, kernel_size=2 * radius + 1, stride=1, padding=radius)

    x = heat[:, None]
    zeros = torch.zeros_like(x)
    keep = x == mp(x)
    for _ in range(2):
        supp = mp(keep.float()) > 0
        supp_x = torch.where(supp, zeros, x)
        keep = keep | ((supp_x == mp(supp_x)) & ~supp)
    return torch.where(keep, x, zeros)[:, 0]


def top_k_keypoints(heat, k: int):
    """heat [B, H, W] -> (keypoints [B, k, 2] int64 (u, v), scores [B, k] float32), best first."""
    import torch

    b, h, w = heat.shape
    sc, idx = heat.reshape(b, -1).topk(min(k, h * w), dim=1)
    kp = torch.stack([idx % w, idx // w], dim=2).to(torch.int64)
    return kp, sc.float()


def build_net(seed: int = 0, head_gain: float = 100.0, nms: bool = False, top_k: int = 1024):
    """SuperPoint (DeTone et al. 2018): shared VGG encoder (1/8 resolution, 128 channels), detector
    head (65-way cell softmax -> full-resolution heatmap) and descriptor head (256-d, L2-normalised).
    Seeded random weights (the trained model is not available offline). With default init the
    65-way softmax is nearly uniform (every value ~1/65 < kMinResponse), so the detector head's
    logits are scaled by head_gain: at 100, ~5 % of a noise frame's pixels exceed 0.1 (a few
    thousand candidates per 640x480 frame), so that selection does the work a trained model gives it.
    nms=True (kSuperpointNms): the heatmap goes through simple_nms (radius 4) and top_k keypoints are
    returned with their scores and bilinearly sampled, normalised descriptors."""
    import torch
    from torch import nn

    class SuperPointNet(nn.Module):
        def __init__(self):
            super().__init__()
            c1, c2, c3, c4, c5, d1 = 64, 64, 128, 128, 256, 256
            self.pool = nn.MaxPool2d(2, 2)
            self.relu = nn.ReLU(inplace=True)
            self.conv1a = nn.Conv2d(1, c1, 3, 1, 1)
            self.conv1b = nn.Conv2d(c1, c1, 3, 1, 1)
            self.conv2a = nn.Conv2d(c1, c2, 3, 1, 1)
            self.conv2b = nn.Conv2d(c2, c2, 3, 1, 1)
            self.conv3a = nn.Conv2d(c2, c3, 3, 1, 1)
            self.conv3b = nn.Conv2d(c3, c3, 3, 1, 1)
            self.conv4a = nn.Conv2d(c3, c4, 3, 1, 1)
            self.conv4b = nn.Conv2d(c4, c4, 3, 1, 1)
            self.convPa = nn.Conv2d(c4, c5, 3, 1, 1)
            self.convPb = nn.Conv2d(c5, 65, 1, 1, 0)
            self.convDa = nn.Conv2d(c4, c5, 3, 1, 1)
            self.convDb = nn.Conv2d(c5, d1, 1, 1, 0)

        def cbr(self, conv, x, pool=False):
            """conv -> ReLU (-> MaxPool2d(2, 2)): fp16 channels-last activations run the convolution
            without its bias and fd_nn_bias_relu for bias, ReLU and pooling in one pass (PyTorch would make
            three or four elementwise passes over the activation); other inputs take the torch modules."""
            if x.dtype == torch.float16 and x.is_cuda and conv.in_channels == 1 and conv.kernel_size == (3, 3) \
                    and conv.stride == (1, 1) and conv.padding == (1, 1) and conv.out_channels in (8, 16, 32, 64, 128, 256) \
                    and x.dim() == 4 and x.shape[1] == 1 and x.shape[3] <= 4096 and not pool:
                # first layer: write-bound (9 MACs per output), one pass instead of convolution + bias pass
                # (fd_nn_conv3x3_c1 stages rows of up to 4096 pixels; wider frames take the branches below)
                return conv1_bias_relu(x.contiguous(), conv.weight, conv.bias)
            if x.dtype == torch.float16 and x.is_cuda and conv.in_channels == 64 and conv.out_channels % 64 == 0 \
                    and conv.kernel_size == (3, 3) and conv.stride == (1, 1) and conv.padding == (1, 1) \
                    and x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last) \
                    and (not pool or (x.shape[2] % 2 == 0 and x.shape[3] % 2 == 0)):
                # 64 -> 64 k layers on the matrix cores with bias, ReLU and pooling in the epilogue
                # one packed copy per layer, replaced when the weight changes (in-place update, reload, device)
                tag = (conv.weight.data_ptr(), conv.weight._version, x.device)
                cache = self.__dict__.setdefault("_fd_packed", {})
                hit = cache.get(id(conv))
                if hit is None or hit[0] != tag:
                    hit = (tag, [pack_conv3x3_weight(conv.weight[k:k + 64].to(device=x.device, dtype=torch.float16))
                                 for k in range(0, conv.out_channels, 64)])
                    cache[id(conv)] = hit
                return conv64_bias_relu(x, conv.weight, conv.bias, pool, packed=hit[1])
            if x.dtype == torch.float16 and x.is_cuda and x.is_contiguous(memory_format=torch.channels_last) \
                    and conv.out_channels % 8 == 0:
                y = torch.nn.functional.conv2d(x, conv.weight, None, conv.stride, conv.padding)
                if y.is_contiguous(memory_format=torch.channels_last):
                    return bias_relu(y, conv.bias, pool, out=None if pool else y)
                x = y + conv.bias.view(1, -1, 1, 1)
                x = self.relu(x)
                return self.pool(x) if pool else x
            x = self.relu(conv(x))
            return self.pool(x) if pool else x

        @staticmethod
        def fused_heads(semi, desc):
            """The heads' output stages run as fd_nn_heat_softmax / fd_nn_desc_normalize when the logits are
            channels-last fp16 on the device."""
            return (semi.is_cuda and semi.dtype == torch.float16 and semi.shape[1] == 65
                    and semi.is_contiguous(memory_format=torch.channels_last)
                    and desc.is_cuda and desc.dtype == torch.float16 and desc.shape[1] % 8 == 0
                    and desc.is_contiguous(memory_format=torch.channels_last))

        def first_layers(self, x):
            """conv1a -> ReLU -> conv1b -> ReLU -> MaxPool2d(2, 2), layer by layer through cbr (conv1a's
            write-bound pass, then conv1b on the matrix cores). conv1a recomputed inside conv1b's tiles (the
            full-resolution activation never written) measured slower in both K10 forms -- 4.75-4.78 vs
            4.68-4.79 ms per 64-frame forward in round 5, 4.19-4.38 vs 4.09-4.13 ms once conv1b kept two tiles
            in flight per CU (profiles/r05_sp_ab.txt, r06_sp_fused_ab.txt) -- and was removed."""
            return self.cbr(self.conv1b, self.cbr(self.conv1a, x), pool=True)

        def forward(self, x):
            """x: [B, 1, H, W] in [0, 1] -> (heatmap [B, H, W] f32, descriptors [B, 256, H/8, W/8] f32), or
            with nms (keypoints [B, K, 2] int64, scores [B, K] f32, descriptors [B, K, 256] f32)."""
            x = self.first_layers(x)
            x = self.cbr(self.conv2b, self.cbr(self.conv2a, x), pool=True)
            x = self.cbr(self.conv3b, self.cbr(self.conv3a, x), pool=True)
            x = self.cbr(self.conv4b, self.cbr(self.conv4a, x))
            xp, xd = self.cbr(self.convPa, x), self.cbr(self.convDa, x)
            semi = desc = None
            if xp.is_cuda and xp.dtype == torch.float16 and xd.dtype == torch.float16:
                # bias-free head convolutions: their biases go into the output stages below
                semi = torch.nn.functional.conv2d(xp, self.convPb.weight, None, self.convPb.stride, self.convPb.padding)
                desc = torch.nn.functional.conv2d(xd, self.convDb.weight, None, self.convDb.stride, self.convDb.padding)
                if self.fused_heads(semi, desc):  # the heads' output stages in one pass each (fd_nn.hip)
                    heat, desc = heat_softmax(semi, self.convPb.bias), desc_normalize(desc, self.convDb.bias)
                    semi = None
                else:
                    semi = semi + self.convPb.bias.view(1, -1, 1, 1)
                    desc = desc + self.convDb.bias.view(1, -1, 1, 1)
            else:
                semi, desc = self.convPb(xp), self.convDb(xd)
            if semi is not None:
                prob = torch.softmax(semi.float(), dim=1)[:, :-1]
                heat = torch.nn.functional.pixel_shuffle(prob, 8)[:, 0]
                desc = desc.float()
                desc = desc / desc.norm(dim=1, keepdim=True).clamp_min(1e-12)
            if not nms:
                return heat, desc
            kp, sc = top_k_keypoints(simple_nms(heat, 4), top_k)
            h, w = heat.shape[1:]
            # descriptor at each keypoint: bilinear on the 1/8 map at the cell-centred position
            grid = torch.stack([(kp[..., 0].float() + 0.5) / w * 2 - 1, (kp[..., 1].float() + 0.5) / h * 2 - 1], -1)
            d = torch.nn.functional.grid_sample(desc, grid[:, None], mode="bilinear", align_corners=False)[:, :, 0]
            d = d / d.norm(dim=1, keepdim=True).clamp_min(1e-12)
            return kp, sc, d.transpose(1, 2).contiguous()

    torch.manual_seed(seed)
    net = SuperPointNet()
    with torch.no_grad():
        net.convPb.weight.mul_(head_gain)
        net.convPb.bias.mul_(head_gain)
    return net


def build_disk(seed: int = 0, nms: bool = False, top_k: int = 1024, head_gain: float = 8.0):
    """DISK-shaped network (Tyszkiewicz et al. 2020): a U-Net on the RGB frame whose full-resolution
    output holds 128 descriptor channels and one detection channel. Seeded random weights (the
    trained disk.onnx is not available); the detection logits are scaled by head_gain and pass a
    sigmoid, so a few percent of a noise frame's pixels exceed kMinResponse. nms=True (kDiskNms):
    simple_nms (radius 2) + top_k keypoints with the descriptor rows at their pixels."""
    import torch
    from torch import nn

    def block(ci, co):
        return nn.Sequential(nn.Conv2d(ci, co, 3, 1, 1), nn.ReLU(inplace=True), nn.Conv2d(co, co, 3, 1, 1),
                             nn.ReLU(inplace=True))

    class DiskNet(nn.Module):
        def __init__(self):
            super().__init__()
            ch = (32, 64, 64, 128)
            self.enc = nn.ModuleList([block(3, ch[0]), block(ch[0], ch[1]), block(ch[1], ch[2]), block(ch[2], ch[3])])
            self.up = nn.ModuleList([nn.ConvTranspose2d(ch[3], ch[2], 2, 2), nn.ConvTranspose2d(ch[2], ch[1], 2, 2),
                                     nn.ConvTranspose2d(ch[1], ch[0], 2, 2)])
            self.dec = nn.ModuleList([block(2 * ch[2], ch[2]), block(2 * ch[1], ch[1]), block(2 * ch[0], ch[0])])
            self.head = nn.Conv2d(ch[0], 129, 1)
            self.pool = nn.MaxPool2d(2, 2)

        def forward(self, x):
            """x: [B, 3, H, W] in [0, 1] -> (heatmap [B, H, W] f32, descriptors [B, 128, H, W] f32), or
            with nms (keypoints [B, K, 2] int64, scores [B, K] f32, descriptors [B, K, 128] f32)."""
            skips = []
            for i, e in enumerate(self.enc):
                x = e(x if i == 0 else self.pool(x))
                skips.append(x)
            for u, d, sk in zip(self.up, self.dec, reversed(skips[:-1])):
                x = d(torch.cat([u(x), sk], dim=1))
            out = self.head(x).float()
            heat = torch.sigmoid(out[:, 128] * head_gain)
            desc = out[:, :128]
            desc = desc / desc.norm(dim=1, keepdim=True).clamp_min(1e-12)
            if not nms:
                return heat, desc
            kp, sc = top_k_keypoints(simple_nms(heat, 2), top_k)
            b = torch.arange(desc.shape[0], device=desc.device)[:, None]
            d = desc.permute(0, 2, 3, 1)[b, kp[..., 1], kp[..., 0]]
            return kp, sc, d.contiguous()

    torch.manual_seed(seed)
    return DiskNet()


@dataclass
class NNResult:
    """DetectGoodFeaturesWithDescriptor's outputs for a batch: xy [B, S, 2] / counts [B] (the new
    features), descriptors [B, S, D] (their rows), prior_descriptors [B, P, D] (heatmap models: the
    reference's descriptors of the incoming features, all_pixel_uv[0..P), per frame counts as the
    priors given; None for the keypoint-list models, whose reference returns new rows only). Unpacks as
    (xy, counts, descriptors)."""
    xy: object
    counts: object
    descriptors: object
    prior_descriptors: object = None

    def __iter__(self):
        return iter((self.xy, self.counts, self.descriptors))


class NNFeaturePointDetector:
    """NNFeaturePointDetector (nn_feature_point_detector.h:12-86), batched, on one GPU."""

    def __init__(self, options: Options | None = None, device: int = 0, dtype: str = "fp16", seed: int = 0,
                 top_k: int = 1024):
        self._options = options or Options()
        self.device = device
        self.dtype = dtype
        self.seed = seed
        self.top_k = top_k
        self.net = None

    def options(self) -> Options:
        return self._options

    @property
    def is_disk(self) -> bool:
        return self._options.kModelType.startswith("kDisk")

    @property
    def is_list_model(self) -> bool:
        return self._options.kModelType.endswith("Nms")

    def Initialize(self) -> bool:
        """nn_feature_point_detector.cpp:10-57: build the model's network, run it once on an all-ones image."""
        import torch

        mt = self._options.kModelType
        if mt not in MODEL_TYPES:
            raise ValueError(f"unknown kModelType {mt!r} (one of {MODEL_TYPES})")
        dev = torch.device("cuda", self.device)
        net = (build_disk(self.seed, nms=self.is_list_model, top_k=self.top_k) if self.is_disk
               else build_net(self.seed, nms=self.is_list_model, top_k=self.top_k))
        net = net.to(dev).eval()
        if self.dtype == "fp16":
            net = net.half()
        self.net = net.to(memory_format=torch.channels_last)
        # MIOpen solver choice (measured with tools/sp_find_probe.py, 64x640x480 fp16): exhaustive find
        # (benchmark=True) picks solvers worth 14.3 ms per 64 frames against 17.1 ms for immediate mode
        # (benchmark=False), but its first use also times the naive direct solver on every
        # conv shape (~30 s). That solver never wins, so it is left out of the search unless the caller
        # set the variable: first find ~10 s, ~0.6 s once MIOpen's user find-db holds the shapes.
        os.environ.setdefault("MIOPEN_DEBUG_CONV_DIRECT_NAIVE_CONV_FWD", "0")
        torch.backends.cudnn.benchmark = True
        ones = torch.ones((1, self._options.kMaxImageRows, self._options.kMaxImageCols), dtype=torch.uint8, device=dev)
        self.InferenceSession(ones)
        return True

    def InferenceSession(self, frames):
        """frames: u8 [B, H, W] device tensor (H, W multiples of 8) -> the network's outputs: heatmap
        models (heatmap f32 [B, H, W], descriptor map f32 [B, D, h, w]); list models (keypoints
        int64 [B, K, 2], scores f32 [B, K], descriptors f32 [B, K, D]). DISK models see the gray frame as
        RGB (OnnxRuntime::ConvertGrayImageToRgbTensor, nn_feature_point_detector.cpp:96-99)."""
        import torch

        x = frames.unsqueeze(1).to(torch.float16 if self.dtype == "fp16" else torch.float32) / 255.0
        if self.is_disk:
            x = x.expand(-1, 3, -1, -1)
        x = x.contiguous(memory_format=torch.channels_last)
        with torch.inference_mode():
            return self.net(x)

    def DetectGoodFeaturesWithDescriptor(self, frames, prior=None) -> NNResult:
        """nn_feature_point_detector_superpoint.cpp:8-112 / nn_feature_point_detector_disk.cpp:8-112 for a
        batch of device frames [B, H, W]. prior: None or a list (per frame) of (n_i, 2) (x, y) arrays
        (the incoming all_pixel_uv). Returns an NNResult on the device."""
        import torch

        if self.net is None:
            raise RuntimeError("Initialize() first")
        o = self._options
        out = self.InferenceSession(frames)
        if self.is_list_model:
            kp, sc, dl = out
            xy, cnt, d = nn_select_list(kp, sc, int(frames.shape[1]), int(frames.shape[2]), None, o, prior, dl)
            return NNResult(xy, cnt, d, None)
        heat, desc = out
        xy, cnt = nn_select(heat, o, prior)
        d = nn_descriptors(desc, xy, cnt)
        pd = None
        if prior is not None:  # ExtractDescriptorsForSelectedFeatures runs over all_pixel_uv (priors first)
            p = max(max((len(q) for q in prior), default=0), 1)
            pxy = np.zeros((len(prior), p, 2), np.float32)
            for i, q in enumerate(prior):
                q = np.asarray(q, np.float32).reshape(-1, 2)
                pxy[i, :len(q)] = q
            pcnt = torch.tensor([len(q) for q in prior], dtype=torch.int32, device=desc.device)
            pd = nn_descriptors(desc, torch.from_numpy(pxy).to(desc.device), pcnt)
        return NNResult(xy, cnt, d, pd)


SuperPointDetector = NNFeaturePointDetector  # (kSuperpointHeatmap by default)
