"""ALIKED on the MI355X: the extractor upstream LightGlue recommends with `LightGlue(features="aliked")`.

Same module tree / parameter names as the reference class (`lightglue/aliked.py:612-694`), built from `nn.Conv2d` /
`nn.BatchNorm2d` only (no torchvision, no kornia), so a released `aliked-n16.pth` / `aliked-n32.pth` loads with
`load_state_dict(strict=True)`, and the same `forward({"image"[, "image_size"]})` contract (`:740-760`).  Everything runs in
`lightglue_amd/csrc/lg_aliked.hip` behind the `lg_aliked_*` C entry points: the encoder, aggregation and score head
(`lg_aliked_encode`), DKD (`lg_aliked_detect`) and SDDH (`lg_aliked_describe`), all exact fp32; each takes one io struct of named fields whose `flags` carry its variants.  No CPU fallback.  As for
SuperPoint, `extract(img, resize=...)` resizes on the device first (`preprocess.ImagePreprocessor`) and maps the keypoints back.

Images of DIFFERENT sizes run in one ragged batch: a canvas with image b in its top-left corner plus `valid_size` (`forward`, `encode`, `detect`, `describe`; the
`LG_EXTRACT_RAGGED` flag of the three stages' io structs).  Each image keeps its own padding to a multiple of 32, and its result is bit-identical to the B = 1 call on its crop;
`extract_batch` builds the feature store of a mixed photo set that way (`superpoint.plan_image_batches`)."""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace
from typing import Optional, Sequence

import torch
from torch import nn

from . import _cabi
from .glue import extracted_to_image_frame
from .preprocess import ImagePreprocessor
from .superpoint import check_image_set, extract_groups
from .superpoint_head import check_descriptor_dtype, check_sizes, device_sizes, sizes_on_device


class DeformableConv2d(nn.Module):
    """Parameter holder of the reference's DeformableConv2d (aliked.py:282-336; mask=False, bias=False)."""

    def __init__(self, cin: int, cout: int):
        super().__init__()
        self.offset_conv = nn.Conv2d(cin, 18, 3, 1, 1, bias=True)
        self.regular_conv = nn.Conv2d(cin, cout, 3, 1, 1, bias=False)


def _conv(cin, cout, conv_type):
    return nn.Conv2d(cin, cout, 3, 1, 1, bias=False) if conv_type == "conv" else DeformableConv2d(cin, cout)


class ConvBlock(nn.Module):
    def __init__(self, cin, cout, conv_type="conv"):
        super().__init__()
        self.conv1 = _conv(cin, cout, conv_type)
        self.bn1 = nn.BatchNorm2d(cout)
        self.conv2 = _conv(cout, cout, conv_type)
        self.bn2 = nn.BatchNorm2d(cout)


class ResBlock(ConvBlock):
    def __init__(self, cin, cout, conv_type="conv"):
        super().__init__(cin, cout, conv_type)
        self.downsample = nn.Conv2d(cin, cout, 1)


class SDDH(nn.Module):
    def __init__(self, dims: int, n_pos: int):
        super().__init__()
        self.offset_conv = nn.Sequential(nn.Conv2d(dims, 2 * n_pos, 3, 1, 0, bias=True), nn.SELU(inplace=True),
                                         nn.Conv2d(2 * n_pos, 2 * n_pos, 1, 1, 0, bias=True))
        self.sf_conv = nn.Conv2d(dims, dims, 1, 1, 0, bias=False)
        self.register_parameter("agg_weights", nn.Parameter(torch.rand(n_pos, dims, dims)))


def _abi_names():
    """State-dict names in the order lg_aliked_pack_weights takes them (include/lightglue_amd.h)."""
    bn = lambda p: [f"{p}.weight", f"{p}.bias", f"{p}.running_mean", f"{p}.running_var"]  # noqa: E731
    names = ["block1.conv1.weight", *bn("block1.bn1"), "block1.conv2.weight", *bn("block1.bn2")]
    names += ["block2.conv1.weight", *bn("block2.bn1"), "block2.conv2.weight", *bn("block2.bn2"), "block2.downsample.weight", "block2.downsample.bias"]
    for b in ("block3", "block4"):
        names += [f"{b}.conv1.offset_conv.weight", f"{b}.conv1.offset_conv.bias", f"{b}.conv1.regular_conv.weight", *bn(f"{b}.bn1"),
                  f"{b}.conv2.offset_conv.weight", f"{b}.conv2.offset_conv.bias", f"{b}.conv2.regular_conv.weight", *bn(f"{b}.bn2"),
                  f"{b}.downsample.weight", f"{b}.downsample.bias"]
    names += [f"conv{i}.weight" for i in range(1, 5)] + [f"score_head.{i}.weight" for i in (0, 2, 4, 6)]
    names += ["desc_head.offset_conv.0.weight", "desc_head.offset_conv.0.bias", "desc_head.offset_conv.2.weight", "desc_head.offset_conv.2.bias",
              "desc_head.sf_conv.weight", "desc_head.agg_weights"]
    return names


_ABI_NAMES = _abi_names()


class ALIKED(nn.Module):
    default_conf = {"model_name": "aliked-n16", "max_num_keypoints": -1, "detection_threshold": 0.2, "nms_radius": 2,   # ref :613-618
                    # extension: element type of the returned descriptors.  torch.float16 = the fp32 descriptors rounded once, on store, by SDDH's last kernel
                    # (half the bytes of a feature store; LightGlue reads them in place).  A storage format, opt-in: outside the matcher's 1e-3 score bar (README)
                    "descriptor_dtype": torch.float32}
    # c1, c2, c3, c4, dim, K, M  (ref :624-630)
    cfgs = {
        "aliked-t16": [8, 16, 32, 64, 64, 3, 16],
        "aliked-n16": [16, 32, 64, 128, 128, 3, 16],
        "aliked-n16rot": [16, 32, 64, 128, 128, 3, 16],
        "aliked-n32": [16, 32, 64, 128, 128, 3, 32],
    }
    n_limit_max = 20000
    required_data_keys = ["image"]

    def __init__(self, weights: Optional[dict] = None, **conf):
        """`weights`: a state dict with the reference's names (e.g. torch.load('aliked-n16.pth')), loaded with strict=True; None = PyTorch's
        default init (the released files come from the network, which this class never touches)."""
        super().__init__()
        self.conf = SimpleNamespace(**{**self.default_conf, **conf})
        name = self.conf.model_name
        if name == "aliked-t16":
            raise ValueError("aliked-t16 is not built (8-channel layers, 64-d descriptors; LightGlue has no weights for it)")
        if name not in self.cfgs:
            raise ValueError(f"unknown ALIKED model {name!r}; built: aliked-n16, aliked-n16rot, aliked-n32")
        if self.conf.nms_radius < 1 or self.conf.nms_radius > 8:
            raise ValueError("nms_radius must be in [1, 8]")
        if self.conf.max_num_keypoints is not None and self.conf.max_num_keypoints > self.n_limit_max:
            raise ValueError(f"max_num_keypoints must be at most {self.n_limit_max}")
        check_descriptor_dtype(self.conf.descriptor_dtype)
        c1, c2, c3, c4, dim, K, M = self.cfgs[name]
        self.n_pos = M
        # module tree of the reference (registration order included: state_dict keys come out in the same order)
        self.block1 = ConvBlock(3, c1, "conv")
        self.block2 = ResBlock(c1, c2, "conv")
        self.block3 = ResBlock(c2, c3, "dcn")
        self.block4 = ResBlock(c3, c4, "dcn")
        self.conv1 = nn.Conv2d(c1, dim // 4, 1, bias=False)
        self.conv2 = nn.Conv2d(c2, dim // 4, 1, bias=False)
        self.conv3 = nn.Conv2d(c3, dim // 4, 1, bias=False)
        self.conv4 = nn.Conv2d(dim, dim // 4, 1, bias=False)
        self.score_head = nn.Sequential(nn.Conv2d(dim, 8, 1, bias=False), nn.SELU(inplace=True), nn.Conv2d(8, 4, 3, 1, 1, bias=False), nn.SELU(inplace=True),
                                        nn.Conv2d(4, 4, 3, 1, 1, bias=False), nn.SELU(inplace=True), nn.Conv2d(4, 1, 3, 1, 1, bias=False))
        self.desc_head = SDDH(dim, M)
        if weights is not None:
            self.load_state_dict(weights, strict=True)
        self._packed = None   # (signature, packed device buffer)

    # ------------------------------------------------------------------ detector settings of the reference's DKD (ref :680-689)
    def _dkd(self):
        c = self.conf
        mnk = c.max_num_keypoints if c.max_num_keypoints is not None else -1
        top_k = -1 if c.detection_threshold > 0 else mnk
        n_limit = mnk if mnk > 0 else self.n_limit_max
        return top_k, float(c.detection_threshold), n_limit

    # ------------------------------------------------------------------ weights -> kernel layout (BatchNorm folded)
    def _params(self, device):
        sd = self.state_dict(keep_vars=True)
        sig = (str(device),) + tuple((sd[n]._version, sd[n].data_ptr()) for n in _ABI_NAMES)
        if self._packed is not None and self._packed[0] == sig:
            return self._packed[1]
        lib = _cabi.load()
        with torch.cuda.device(device):
            tensors = [sd[n].detach().to(device=device, dtype=torch.float32).contiguous() for n in _ABI_NAMES]
            nbytes = lib.lg_aliked_packed_bytes(self.n_pos)
            packed = torch.empty((nbytes,), device=device, dtype=torch.uint8)
            arr = (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
            stream = torch.cuda.current_stream(device)
            _cabi.check(lib.lg_aliked_pack_weights(self.n_pos, arr, len(tensors), packed.data_ptr(), nbytes, C.c_void_p(stream.cuda_stream)))
            stream.synchronize()   # the temporaries may be freed after this
        self._packed = (sig, packed)
        return packed

    @staticmethod
    def _check_image(image):
        if image.device.type != "cuda":
            raise RuntimeError("lightglue_amd.ALIKED runs on MI355X (ROCm device type 'cuda') only; there is no CPU fallback. "
                               f"Got an image on {image.device}.")
        assert image.dim() == 4 and image.shape[1] in (1, 3), "image must be [B, 1|3, H, W]"

    # ------------------------------------------------------------------ encoder + score head
    @torch.no_grad()
    def encode(self, image: torch.Tensor, valid_size=None):
        """image [B, 1|3, H, W] -> (scores [B, H, W], level maps): ref extract_dense_map (:696-738) without the dense feature map, which
        lg_aliked_describe recomputes per keypoint from the four 32-channel level maps.

        `valid_size` (ragged batch): `[B, 2]` `(w, h)`, integers with 8 <= size <= canvas — `image` is then a canvas and image b its top-left h_b x w_b corner,
        padded to a multiple of 32 on its own (centred, replicated from ITS border).  Nothing outside an image is read (the padding may hold anything).  Inside
        h_b x w_b the scores, and inside the image's padded level extents `(Hp_b >> s, Wp_b >> s)` the `level_maps(levels, (B, H, W))` of the canvas, are
        bit-identical to the call on the crop; scores outside are 0, level maps outside unspecified."""
        sizes = None if valid_size is None else check_sizes(valid_size, image.shape[0], image.shape[-2:], 8, "valid_size")
        return self._encode(image, sizes)

    def _encode(self, image: torch.Tensor, sizes):
        """encode with `sizes` = None, validated host rows (check_sizes) or the int32 device array made from them"""
        self._check_image(image)
        device = image.device
        image = image.detach().to(dtype=torch.float32).contiguous()
        bsz, ch, h, w = image.shape
        lib = _cabi.load()
        packed = self._params(device)
        nlev = lib.lg_aliked_levels_bytes(bsz, h, w)
        nws = lib.lg_aliked_workspace_bytes(bsz, h, w, self.n_pos)
        if nlev <= 0 or nws <= 0:   # refused sizes: let the encode call report why
            nlev, nws = max(nlev, 1), max(nws, 1)
        levels = torch.empty((nlev,), device=device, dtype=torch.uint8)
        work = torch.empty((nws,), device=device, dtype=torch.uint8)
        scores = torch.empty((bsz, h, w), device=device, dtype=torch.float32)
        sizes = device_sizes(sizes, device)
        io = _cabi.LgAlikedEncodeIO(batch=bsz, channels=ch, h=h, w=w, n_pos=self.n_pos, flags=_cabi.LG_EXTRACT_RAGGED if sizes is not None else 0,
                                    image=image.data_ptr(), sizes=None if sizes is None else sizes.data_ptr(), packed=packed.data_ptr(), levels=levels.data_ptr(),
                                    workspace=work.data_ptr(), workspace_bytes=nws, scores=scores.data_ptr())
        with torch.cuda.device(device):
            _cabi.check(lib.lg_aliked_encode(C.byref(io), C.c_void_p(torch.cuda.current_stream(device).cuda_stream)))
        return scores, levels

    @staticmethod
    def level_maps(levels: torch.Tensor, shape):
        """The four level maps x1 .. x4 inside the opaque `levels` buffer of `encode` / `describe` for images of `shape` = (B, H, W): float32
        views [B, Hp >> s, Wp >> s, 32] for s = 0, 1, 3, 5 (NHWC, after conv1 .. conv4 + SELU) that share its memory, so a caller can read
        the encoder's levels or write its own.  Restates the layout of lg_aliked.hip: Hp, Wp from InputPadder(divis_by=32) (`frame_of`), each
        level's size rounded up to 256 bytes (`level_layout`); the total is checked against lg_aliked_levels_bytes."""
        bsz, h, w = shape
        hp, wp = h + ((h // 32 + 1) * 32 - h) % 32, w + ((w // 32 + 1) * 32 - w) % 32
        dims = [(bsz, hp >> s, wp >> s, 32) for s in (0, 1, 3, 5)]
        offsets, used = [], 0
        for d in dims:
            offsets.append(used)
            used += (4 * d[0] * d[1] * d[2] * d[3] + 255) // 256 * 256
        total = _cabi.load().lg_aliked_levels_bytes(bsz, h, w)
        assert used == total and levels.dtype == torch.uint8 and levels.dim() == 1 and levels.numel() >= total, \
            f"level layout: {used} bytes restated here, lg_aliked_levels_bytes says {total}, the buffer has {levels.numel()}"
        return [levels[o:o + 4 * d[0] * d[1] * d[2] * d[3]].view(torch.float32).view(d) for o, d in zip(offsets, dims)]

    @torch.no_grad()
    def detect(self, scores: torch.Tensor, image_size: Optional[torch.Tensor] = None, valid_size=None):
        """DKD (ref :94-262) on a score map [B, H, W] -> keypoints [B, cap, 2] (pixels), scores [B, cap], normalised keypoints [B, cap, 2], counts [B].

        `valid_size` (ragged batch, `[B, 2]` `(w, h)`; not together with `image_size`): `scores` is a canvas, the score map of image b its top-left corner and
        whatever lies outside it is ignored.  Each image is detected as its own batch of one — keypoints in its own frame, the mean-threshold fallback decided
        per image — bit-identical to the call on the crop."""
        if valid_size is not None and image_size is not None:
            raise ValueError("valid_size and image_size cannot be given together: a ragged batch takes every border from valid_size")
        sizes = None if valid_size is None else check_sizes(valid_size, scores.shape[0], scores.shape[-2:], 8, "valid_size")
        return self._detect(scores, image_size, sizes)

    def _detect(self, scores: torch.Tensor, image_size, sizes):
        bsz, h, w = scores.shape
        device = scores.device
        top_k, th, n_limit = self._dkd()
        cap = top_k if top_k > 0 else n_limit
        lib = _cabi.load()
        nws = max(lib.lg_aliked_detect_workspace_bytes(bsz, h, w, cap), 1)
        work = torch.empty((nws,), device=device, dtype=torch.uint8)
        kpts = torch.empty((bsz, cap, 2), device=device, dtype=torch.float32)
        kscores = torch.empty((bsz, cap), device=device, dtype=torch.float32)
        knorm = torch.empty((bsz, cap, 2), device=device, dtype=torch.float32)
        counts = torch.empty((bsz,), device=device, dtype=torch.int32)
        size_ptr = None
        if image_size is not None:
            image_size = image_size.to(device=device, dtype=torch.float32).reshape(bsz, 2).contiguous()
            size_ptr = image_size.data_ptr()
        sizes = device_sizes(sizes, device)
        io = _cabi.LgAlikedDetectIO(batch=bsz, h=h, w=w, flags=_cabi.LG_EXTRACT_RAGGED if sizes is not None else 0, scores=scores.data_ptr(),
                                    sizes=None if sizes is None else sizes.data_ptr(), image_size=size_ptr, nms_radius=int(self.conf.nms_radius), scores_th=th,
                                    top_k=top_k, n_limit=n_limit, capacity=cap, workspace=work.data_ptr(), workspace_bytes=nws, keypoints=kpts.data_ptr(),
                                    kp_scores=kscores.data_ptr(), kp_norm=knorm.data_ptr(), counts=counts.data_ptr())
        with torch.cuda.device(device):
            _cabi.check(lib.lg_aliked_detect(C.byref(io), C.c_void_p(torch.cuda.current_stream(device).cuda_stream)))
        return kpts, kscores, knorm, counts

    @torch.no_grad()
    def describe(self, levels: torch.Tensor, shape, knorm: torch.Tensor, counts: torch.Tensor, dtype: Optional[torch.dtype] = None, valid_size=None):
        """SDDH (ref :479-609): descriptors [B, N, 128] of the normalised keypoints knorm [B, N, 2]; rows >= counts[b] are zero.  `dtype`: torch.float32, or
        torch.float16 = the same values rounded once on store (`LG_EXTRACT_DESC_F16`); None = conf.descriptor_dtype.  `valid_size` (ragged batch): `shape` is
        the canvas and `levels` what `encode(canvas, valid_size)` returned; knorm is normalised in each image's own frame."""
        sizes = None if valid_size is None else check_sizes(valid_size, shape[0], shape[1:], 8, "valid_size")
        return self._describe(levels, shape, knorm, counts, dtype, sizes)

    def _describe(self, levels, shape, knorm, counts, dtype, sizes):
        dtype = check_descriptor_dtype(self.conf.descriptor_dtype if dtype is None else dtype)
        bsz, h, w = shape
        n = knorm.shape[1]
        device = knorm.device
        out = torch.empty((bsz, n, 128), device=device, dtype=dtype)   # every row is written (padding rows with zeros)
        if n == 0:
            return out
        lib = _cabi.load()
        packed = self._params(device)
        knorm = knorm.contiguous()
        nws = max(lib.lg_aliked_describe_workspace_bytes(bsz * n, self.n_pos), 1)
        work = torch.empty((nws,), device=device, dtype=torch.uint8)
        sizes = device_sizes(sizes, device)
        flags = (_cabi.LG_EXTRACT_RAGGED if sizes is not None else 0) | (_cabi.LG_EXTRACT_DESC_F16 if dtype is torch.float16 else 0)
        io = _cabi.LgAlikedDescribeIO(batch=bsz, h=h, w=w, n_pos=self.n_pos, flags=flags, levels=levels.data_ptr(), sizes=None if sizes is None else sizes.data_ptr(),
                                      packed=packed.data_ptr(), kp_norm=knorm.data_ptr(), counts=counts.data_ptr(), n=n, workspace=work.data_ptr(),
                                      workspace_bytes=nws, descriptors=out.data_ptr())
        with torch.cuda.device(device):
            _cabi.check(lib.lg_aliked_describe(C.byref(io), C.c_void_p(torch.cuda.current_stream(device).cuda_stream)))
        return out

    # ------------------------------------------------------------------ the reference's forward
    @torch.no_grad()
    def forward(self, data: dict) -> dict:
        """ref :740-760.  Returns keypoints [B, N, 2] (pixel frame), keypoint_scores [B, N], descriptors [B, N, 128] and — extension for ragged
        batches — num_keypoints [B]; rows beyond an image's count are zero (the reference's torch.stack only handles equal counts).

        Optional `data["valid_size"]` (`[B, 2]` `(w, h)`, integers; validated on the host, ValueError names the offending image; not together with
        `image_size`): a ragged batch of images of DIFFERENT sizes, image b in the top-left h_b x w_b corner of the canvas `data["image"]`.  Rows
        < num_keypoints[b] are then bit-identical to the B = 1 call on that crop, keypoints in the image's own frame; absent, the path is exactly the uniform one."""
        for key in self.required_data_keys:
            assert key in data, f"Missing key {key} in data"
        image = data["image"]
        sizes = None
        if data.get("valid_size") is not None:
            if data.get("image_size") is not None:
                raise ValueError("valid_size and image_size cannot be given together: a ragged batch takes every border from valid_size")
            sizes = check_sizes(data["valid_size"], image.shape[0], image.shape[-2:], 8, "valid_size")
        self._check_image(image)
        bsz, _, h, w = image.shape
        if sizes is not None:
            sizes = sizes_on_device(sizes, image.device)      # one upload for the three stages
        scores, levels = self._encode(image, sizes)
        kpts, kscores, knorm, counts = self._detect(scores, data.get("image_size"), sizes)
        nmax = int(counts.cpu().max()) if counts.numel() else 0   # (a copy, not a reduction kernel)
        kpts, kscores, knorm = kpts[:, :nmax].contiguous(), kscores[:, :nmax].contiguous(), knorm[:, :nmax].contiguous()
        desc = self._describe(levels, (bsz, h, w), knorm, counts, None, sizes)
        return {"keypoints": kpts, "keypoint_scores": kscores, "descriptors": desc, "num_keypoints": counts}

    preprocess_conf = {"resize": None}   # NOT the reference's 1024 (aliked.py:631-633): see extract()

    @torch.no_grad()
    def extract(self, img: torch.Tensor, **conf) -> dict:
        """Perform extraction with online resizing (ref utils.py:136-147): ImagePreprocessor(**{**self.preprocess_conf, **conf}) on the device
        (lightglue_amd/preprocess.py: one HIP kernel), forward on the resized image, keypoints mapped back to the original image's pixel frame,
        `(k + 0.5) / scale - 0.5`, and `image_size` = the ORIGINAL (w, h).  Deliberate difference: `preprocess_conf["resize"]` is None here, not the
        reference's 1024, so `extract(img)` keeps using the image at its own size (and returns exactly what it did before resizing existed);
        the upstream behaviour is one keyword away: `extract(img, resize=1024)`, `match_pair(..., resize=1024)`."""
        if img.dim() == 3:
            img = img[None]
        assert img.dim() == 4 and img.shape[0] == 1
        h, w = img.shape[-2:]
        resized, scales = ImagePreprocessor(**{**self.preprocess_conf, **conf})(img)
        feats = self.forward({"image": resized})
        if tuple(resized.shape[-2:]) != (h, w):
            return extracted_to_image_frame(feats, (h, w), scales)
        feats["image_size"] = torch.tensor([[w, h]], dtype=torch.float32, device=img.device)
        return feats

    @torch.no_grad()
    def extract_batch(self, images: Sequence[torch.Tensor], batch_size: int = 8, order: str = "size", **conf) -> dict:
        """`extract` for a set of images of DIFFERENT sizes at batched speed: the feature store `collate_features([self.extract(i, **conf) for i in images])`
        would give, key for key and bit for bit — keypoints [K, N, 2] in each ORIGINAL image's pixel frame, keypoint_scores, descriptors
        (conf.descriptor_dtype), num_keypoints [K], image_size [K, 2] = original (w, h); N = the largest count, padding rows zero — ready for
        `LightGlue.match_pairs`.  The contract of `SuperPoint.extract_batch`: each image ([C, H_i, W_i] / [1, C, H_i, W_i], float32 or uint8, C = 1 | 3) is
        preprocessed with `{**preprocess_conf, **conf}`: the target sizes are planned on the host and grouped by `plan_image_batches` (at most `batch_size` per
        group), each group is resized / converted into the top-left corners of one zeroed canvas by ONE kernel (`ImagePreprocessor.to_canvas`) and extracted in
        ONE ragged `forward` (`valid_size`).  A group that mixes 1- and 3-channel images runs on a 3-channel canvas, the one channel written to all three
        planes: the first convolution broadcasts one channel to three itself, so this changes nothing."""
        images = check_image_set(images, "ALIKED")
        prep = ImagePreprocessor(**{**self.preprocess_conf, **conf})
        return extract_groups(self.forward, prep, images, batch_size, order, None)
