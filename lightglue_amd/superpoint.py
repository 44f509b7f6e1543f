"""SuperPoint on the MI355X: the extractor that produces the matcher's `(B, N, 256)` inputs.

Same module tree / parameter names as the reference class (`lightglue/superpoint.py:98-145`: conv1a ... convDb), so the
released `superpoint_v1.pth` loads with `load_state_dict` unchanged, and the same `forward({"image": ...})` contract
(`:147-232`).  Everything runs in `lightglue_amd/csrc/`: the conv stack as exact-fp32 MFMA implicit GEMMs
(`lg_sp_encoder.hip`, `lg_sp_encode`), keypoint extraction (`lg_sp_detect`: NMS, borders, threshold, top-k) and the
descriptor head (`lg_sp_sample_descriptors`).  No CPU fallback.  `extract(img, resize=...)` resizes on the device first (`preprocess.ImagePreprocessor`,
`lg_preprocess.hip`) and maps the keypoints back like the reference's `Extractor.extract`; image FILE I/O (cv2) stays out of scope.

Images of DIFFERENT sizes run in one ragged batch: a canvas with image b in its top-left corner plus `valid_size` (`forward`, `encode`; the `LG_EXTRACT_RAGGED` flag of the three stages' io structs),
every image's result bit-identical to the B = 1 call on its crop; `extract_batch` builds the feature store of a mixed photo set that way (`plan_image_batches`)."""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace
from typing import List, Optional, Sequence, Tuple

import torch
from torch import nn

from . import _cabi
from .glue import extracted_to_image_frame
from .preprocess import ImagePreprocessor
from .superpoint_head import _detect, _run as _descriptor_run, check_descriptor_dtype, check_sizes, device_sizes, sizes_on_device

def plan_image_batches(sizes_hw: Sequence[Tuple[int, int]], batch_size: int = 8, max_workspace_bytes: Optional[int] = None,
                       order: str = "size", workspace_bytes=None) -> List[Tuple[List[int], Tuple[int, int]]]:
    """Group images of sizes `sizes_hw[i] = (h_i, w_i)` into ragged batches for `SuperPoint.extract_batch`: a list of `(indices, (Hc, Wc))`
    that covers every index exactly once, with at most `batch_size` indices per group and the group's canvas = the elementwise maximum of
    its sizes.  Pure host arithmetic and deterministic.  `order="size"` (default) walks the images sorted by (h, w) descending, ties by index,
    so that equal and similar sizes share a canvas and little of it is padding; `order="input"` keeps the given order.  A group is closed when
    it is full or when the next image would push the conv stack's workspace, `lg_sp_encode_workspace_bytes(n, Hc, Wc)`, above
    `max_workspace_bytes`; a single image that alone exceeds the cap raises ValueError.  `workspace_bytes`: the byte function `(n, Hc, Wc) -> int` the cap
    is measured with, for another extractor (`ALIKED.extract_batch` passes its own encoder's); None = SuperPoint's, as above."""
    if batch_size < 1:
        raise ValueError("batch_size must be at least 1")
    if order not in ("size", "input"):
        raise ValueError("order must be 'size' or 'input'")
    sizes = [(int(h), int(w)) for h, w in sizes_hw]
    for i, (h, w) in enumerate(sizes):
        if h < 8 or w < 8:
            raise ValueError(f"image {i} is {h} x {w}: the extractors need at least 8 x 8")
    nbytes = (workspace_bytes or _cabi.load().lg_sp_encode_workspace_bytes) if max_workspace_bytes is not None else None
    todo = sorted(range(len(sizes)), key=lambda i: (-sizes[i][0], -sizes[i][1], i)) if order == "size" else list(range(len(sizes)))
    groups: List[Tuple[List[int], Tuple[int, int]]] = []
    cur: List[int] = []
    hc = wc = 0
    for i in todo:
        h, w = sizes[i]
        if nbytes is not None and nbytes(1, h, w) > max_workspace_bytes:
            raise ValueError(f"image {i} ({h} x {w}) alone needs {nbytes(1, h, w)} bytes of conv workspace, above max_workspace_bytes = {max_workspace_bytes}")
        nh, nw = max(hc, h), max(wc, w)
        if cur and (len(cur) == batch_size or (nbytes is not None and nbytes(len(cur) + 1, nh, nw) > max_workspace_bytes)):
            groups.append((cur, (hc, wc)))
            cur, nh, nw = [], h, w
        cur.append(i)
        hc, wc = nh, nw
    if cur:
        groups.append((cur, (hc, wc)))
    return groups


def check_image_set(images: Sequence[torch.Tensor], who: str) -> List[torch.Tensor]:
    """The images of an `extract_batch` call as [1, C, H, W] tensors, or the first refusal: an empty set, dimensions, device, channels, dtype (in that order)"""
    images = list(images)
    if not images:
        raise ValueError("extract_batch needs at least one image")
    out = []
    for i, img in enumerate(images):
        if img.dim() == 3:
            img = img[None]
        if img.dim() != 4 or img.shape[0] != 1:
            raise ValueError(f"image {i} must be [C, H, W] or [1, C, H, W], got {tuple(img.shape)}")
        if img.device.type != "cuda":
            raise RuntimeError(f"lightglue_amd.{who} runs on MI355X (ROCm device type 'cuda') only; there is no CPU fallback. "
                               f"Got image {i} on {img.device}.")
        if img.shape[1] not in (1, 3):
            raise ValueError(f"image {i} must have 1 or 3 channels, got {img.shape[1]}")
        if img.dtype not in (torch.float32, torch.uint8):
            raise TypeError(f"image {i} must be float32 or uint8, got {img.dtype}")
        out.append(img)
    return out


def extract_groups(forward, prep: ImagePreprocessor, images, batch_size: int, order: str, channels: Optional[int]) -> dict:
    """`extract_batch` of both extractors after validation: the images' plans under `prep` (host), `plan_image_batches` on the planned target sizes, then per
    group ONE `prep.to_canvas` (one kernel: every image resized / converted into its corner of the zeroed canvas; `channels` as `to_canvas` takes it) and ONE
    ragged `forward`; the collated store in the images' own order"""
    device = images[0].device
    plans = prep.plan_images([tuple(t.shape[-2:]) for t in images])
    groups = plan_image_batches([(p.h_out, p.w_out) for p in plans], batch_size, order=order)
    parts = []
    for idx, (hc, wc) in groups:
        canvas, valid, scales = prep.to_canvas([images[i] for i in idx], channels=channels, canvas_size=(hc, wc))
        feats = forward({"image": canvas, "valid_size": valid})
        kp, counts = feats["keypoints"], feats["num_keypoints"]
        resized = [not plans[i].identity for i in idx]      # extract maps keypoints back only then
        if any(resized):      # back to the original frame, (k + 0.5) / scale - 0.5 (extracted_to_image_frame), for the images that were resized
            sc = scales.to(kp.dtype)[:, None, :]
            moved = (kp + 0.5) / sc - 0.5
            kp = torch.where(torch.tensor(resized, device=device)[:, None, None], moved, kp)
            kp = torch.where((torch.arange(kp.shape[1], device=device)[None, :] < counts[:, None])[..., None], kp, torch.zeros_like(kp))      # padding rows stay zero
        parts.append((idx, kp, feats["keypoint_scores"], feats["descriptors"], counts))
    k, nmax = len(images), max(p[1].shape[1] for p in parts)
    order = torch.tensor([i for p in parts for i in p[0]], device=device)
    def gather(j, tail):
        buf = parts[0][j].new_zeros((k, nmax) + tail)
        for p in parts:
            buf[torch.tensor(p[0], device=device), : p[j].shape[1]] = p[j]
        return buf
    out = {"keypoints": gather(1, (2,)), "descriptors": gather(3, (parts[0][3].shape[-1],)), "keypoint_scores": gather(2, ())}
    out["image_size"] = torch.tensor([[p.w_in, p.h_in] for p in plans], dtype=torch.float32).to(device)
    counts = torch.empty((k,), dtype=torch.int32, device=device)
    counts[order] = torch.cat([p[4] for p in parts])
    out["num_keypoints"] = counts
    return out


_LAYERS = ("conv1a", "conv1b", "conv2a", "conv2b", "conv3a", "conv3b", "conv4a", "conv4b", "convPa", "convPb", "convDa", "convDb")


class SuperPoint(nn.Module):
    default_conf = {"descriptor_dim": 256, "nms_radius": 4, "max_num_keypoints": None, "detection_threshold": 0.0005,
                    "remove_borders": 4,   # ref :108-114
                    # extension: "fp32" = exact f32 MFMA convolutions (default); "f16x3" = split-f16 operands, three f16 MFMAs per product, fp32 accumulation (22 operand bits:
                    # below an fp32 convolution's summation-order noise, cf. the reference's own GPU default of TF32 convolutions) at several times the f32 MFMA rate
                    "conv_precision": "fp32",
                    # extension: element type of the returned descriptors.  torch.float16 = the fp32 descriptors rounded once, on store, by the head's last kernel
                    # (half the bytes of a feature store; LightGlue reads them in place).  A storage format, opt-in: outside the matcher's 1e-3 score bar (README)
                    "descriptor_dtype": torch.float32}
    required_data_keys = ["image"]

    def __init__(self, weights: Optional[dict] = None, **conf):
        """`weights`: a state dict with the reference's names (e.g. torch.load('superpoint_v1.pth')); None = PyTorch's default
        init (the released file is network-only, ref :143-144, and there is no network here)."""
        super().__init__()
        self.conf = SimpleNamespace(**{**self.default_conf, **conf})
        c1, c2, c3, c4, c5 = 64, 64, 128, 128, 256
        self.conv1a = nn.Conv2d(1, c1, 3, 1, 1); self.conv1b = nn.Conv2d(c1, c1, 3, 1, 1)
        self.conv2a = nn.Conv2d(c1, c2, 3, 1, 1); self.conv2b = nn.Conv2d(c2, c2, 3, 1, 1)
        self.conv3a = nn.Conv2d(c2, c3, 3, 1, 1); self.conv3b = nn.Conv2d(c3, c3, 3, 1, 1)
        self.conv4a = nn.Conv2d(c3, c4, 3, 1, 1); self.conv4b = nn.Conv2d(c4, c4, 3, 1, 1)
        self.convPa = nn.Conv2d(c4, c5, 3, 1, 1); self.convPb = nn.Conv2d(c5, 65, 1, 1, 0)
        self.convDa = nn.Conv2d(c4, c5, 3, 1, 1); self.convDb = nn.Conv2d(c5, self.conf.descriptor_dim, 1, 1, 0)
        if self.conf.descriptor_dim != 256:
            raise ValueError("lightglue_amd builds descriptor_dim = 256 only")
        if self.conf.conv_precision not in ("fp32", "f16x3"):
            raise ValueError("conv_precision must be 'fp32' or 'f16x3'")
        if self.conf.max_num_keypoints is not None and self.conf.max_num_keypoints <= 0:
            raise ValueError("max_num_keypoints must be positive or None")   # ref :146-147
        check_descriptor_dtype(self.conf.descriptor_dtype)
        if weights is not None:
            self.load_state_dict(weights)
        self._packed = None   # (signature, [24 device tensors])

    # ------------------------------------------------------------------ weights -> kernel layout
    def _params(self, device):
        split = self.conf.conv_precision == "f16x3"
        sig = (str(device), split) + tuple((p._version, p.data_ptr()) for p in self.parameters())
        if self._packed is not None and self._packed[0] == sig:
            return self._packed[1]
        lib = _cabi.load()
        out = []
        with torch.cuda.device(device):
            stream = torch.cuda.current_stream(device).cuda_stream
            for name in _LAYERS:
                conv = getattr(self, name)
                w = conv.weight.detach().to(device=device, dtype=torch.float32).contiguous()
                cout, cin, k, _ = w.shape
                dst = torch.empty(w.numel(), device=device, dtype=torch.float32)
                pack = lib.lg_sp_pack_conv_weight_split if (split and name != "conv1a") else lib.lg_sp_pack_conv_weight   # (the split form fills the same bytes: two f16 planes)
                _cabi.check(pack(w.data_ptr(), cout, cin, k, dst.data_ptr(), C.c_void_p(stream)))
                out += [dst, conv.bias.detach().to(device=device, dtype=torch.float32).contiguous()]
            torch.cuda.current_stream(device).synchronize()   # `w` temporaries may be freed after this
        self._packed = (sig, out)
        return out

    # ------------------------------------------------------------------ conv stack
    @torch.no_grad()
    def encode(self, image: torch.Tensor, valid_size=None):
        """image [B, 1, H, W] (or [B, 3, H, W]: converted like kornia's rgb_to_grayscale, ref :155-156) ->
        (scores [B, H // 8 * 8, W // 8 * 8], dense raw descriptors [B, 256, H // 8, W // 8]) — ref :159-184 and :213-214.  Any
        H, W >= 8: the three 2 x 2 max-pools floor like the reference's nn.MaxPool2d, so the score map is cropped to whole 8 x 8 cells.

        `valid_size` (ragged batch): `[B, 2]` `(w, h)`, integers with 8 <= size <= canvas — `image` is then a canvas and image b its top-left
        h_b x w_b corner.  Nothing outside an image is read (the padding may hold anything); inside `(h_b // 8 * 8, w_b // 8 * 8)` the scores and inside
        `(h_b // 8, w_b // 8)` the descriptors are bit-identical to the call on the crop; scores outside are 0, descriptors outside unspecified."""
        sizes = None if valid_size is None else check_sizes(valid_size, image.shape[0], image.shape[-2:], 8, "valid_size")
        return self._encode(image, sizes)

    def _encode(self, image: torch.Tensor, sizes):
        """encode with `sizes` = None, validated host rows (check_sizes) or the int32 device array made from them"""
        if image.device.type != "cuda":
            raise RuntimeError("lightglue_amd.SuperPoint runs on MI355X (ROCm device type 'cuda') only; there is no CPU fallback. "
                               f"Got an image on {image.device}.")
        if image.shape[1] == 3:
            r, g, b = image[:, 0:1], image[:, 1:2], image[:, 2:3]
            image = 0.299 * r + 0.587 * g + 0.114 * b
        assert image.dim() == 4 and image.shape[1] == 1, "image must be [B, 1|3, H, W]"
        device = image.device
        image = image.detach().to(dtype=torch.float32).contiguous()
        bsz, _, h, w = image.shape
        assert h >= 8 and w >= 8, "image must be at least 8 x 8"
        lib = _cabi.load()
        params = self._params(device)
        arr = (C.c_void_p * 24)(*[t.data_ptr() for t in params])
        nbytes = lib.lg_sp_encode_workspace_bytes(bsz, h, w)
        work = torch.empty((nbytes,), device=device, dtype=torch.uint8)
        scores = torch.empty((bsz, h // 8 * 8, w // 8 * 8), device=device, dtype=torch.float32)
        dense = torch.empty((bsz, 256, h // 8, w // 8), device=device, dtype=torch.float32)
        sizes = device_sizes(sizes, device)
        flags = (_cabi.LG_EXTRACT_RAGGED if sizes is not None else 0) | (_cabi.LG_EXTRACT_SPLIT if self.conf.conv_precision == "f16x3" else 0)
        io = _cabi.LgSpEncodeIO(batch=bsz, h=h, w=w, flags=flags, image=image.data_ptr(), sizes=None if sizes is None else sizes.data_ptr(), params=arr,
                                workspace=work.data_ptr(), workspace_bytes=nbytes, scores=scores.data_ptr(), desc_map=dense.data_ptr())
        with torch.cuda.device(device):
            _cabi.check(lib.lg_sp_encode(C.byref(io), C.c_void_p(torch.cuda.current_stream(device).cuda_stream)))
        return scores, dense

    # ------------------------------------------------------------------ the reference's forward
    @torch.no_grad()
    def forward(self, data: dict) -> dict:
        """ref :147-232.  Returns keypoints [B, N, 2] (x, y), keypoint_scores [B, N], descriptors [B, N, 256] (conf.descriptor_dtype) and — extension for
        ragged batches — num_keypoints [B] (rows beyond an image's count are padding; with max_num_keypoints and enough
        detections every image has exactly that many, as the reference's torch.stack requires).

        Optional `data["valid_size"]` (`[B, 2]` `(w, h)`, integers; validated on the host, ValueError names the offending image): a ragged batch of images
        of DIFFERENT sizes, image b in the top-left h_b x w_b corner of the canvas `data["image"]`.  Rows < num_keypoints[b] are then bit-identical to the
        B = 1 call on that crop, keypoints in the image's own frame; absent, the path is exactly the uniform one."""
        for key in self.required_data_keys:
            assert key in data, f"Missing key {key} in data"
        c = self.conf
        image = data["image"]
        img_sizes = score_sizes = None
        if data.get("valid_size") is not None:
            rows = check_sizes(data["valid_size"], image.shape[0], image.shape[-2:], 8, "valid_size")
            if image.device.type == "cuda":      # (a CPU image raises in _encode)
                both = sizes_on_device(rows + [[w // 8 * 8, h // 8 * 8] for w, h in rows], image.device)      # one upload: the images, then their score maps
                img_sizes, score_sizes = both[: len(rows)], both[len(rows):]
        scores, dense = self._encode(image, img_sizes)
        kpts, kscores, counts = _detect(scores, c.nms_radius, c.remove_borders, c.detection_threshold, c.max_num_keypoints, None, score_sizes)
        nmax = int(counts.max().item()) if counts.numel() else 0
        kpts, kscores = kpts[:, :nmax].contiguous(), kscores[:, :nmax].contiguous()
        if bool((counts < nmax).any()):   # ragged batch: rows beyond an image's count are padding — zero them (descriptor_head does the same)
            live = torch.arange(nmax, device=counts.device)[None, :] < counts[:, None]
            # (a select, not a product: the rows past a count are unwritten memory, and NaN * 0 is NaN)
            kpts = torch.where(live[..., None], kpts, 0.0); kscores = torch.where(live, kscores, 0.0)
        desc = _descriptor_run(kpts, dense, 8, True, counts, c.descriptor_dtype, img_sizes)
        return {"keypoints": kpts, "keypoint_scores": kscores, "descriptors": desc, "num_keypoints": counts}   # counts: consumed by LightGlue.forward

    preprocess_conf = {"resize": None}   # NOT the reference's 1024 (superpoint.py:115-117): see extract()

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
        `LightGlue.match_pairs`.  `images`: [C, H_i, W_i] / [1, C, H_i, W_i] tensors, everything `extract` accepts.  Each is preprocessed with
        `{**preprocess_conf, **conf}`: the target sizes are planned on the host and grouped by `plan_image_batches` (at most `batch_size` per group), each group is
        resized / converted into the top-left corners of one canvas by ONE kernel (`ImagePreprocessor.to_canvas`) and extracted in ONE ragged `forward` (`valid_size`).  `order`: the planner's — "size" puts like sizes together
        (little padding), "input" batches the images as they come."""
        images = check_image_set(images, "SuperPoint")
        prep = ImagePreprocessor(**{**self.preprocess_conf, **conf})
        return extract_groups(self.forward, prep, images, batch_size, order, 1)      # 3-channel images turn gray in the kernel, as encode does per image
