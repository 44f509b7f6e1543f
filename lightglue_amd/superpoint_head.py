"""SuperPoint descriptor head on the MI355X: the step between the SuperPoint conv stack and
the matcher.  Mirrors the reference's `sample_descriptors` (lightglue/superpoint.py:80-95) and the descriptor tail
of `SuperPoint.forward` (:216-228); both run in `lightglue_amd/csrc/lg_superpoint.hip` through
`lg_sp_sample_descriptors` and `lg_sp_detect` (include/lightglue_amd.h): one entry point each, taking an io struct whose `flags` say whether the batch is ragged
(`LG_EXTRACT_RAGGED`: `sizes` is read) and whether the descriptors are stored as float16 (`LG_EXTRACT_DESC_F16`).  The conv stack stays out of scope.
No CPU fallback: CPU tensors raise."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _cabi


def check_descriptor_dtype(dtype) -> torch.dtype:
    """The element types an extractor writes its descriptors in: float32 (default) or float16 (rounded once, on store, by the last kernel)."""
    if dtype not in (torch.float32, torch.float16):
        raise ValueError(f"descriptor_dtype must be torch.float32 or torch.float16, got {dtype}")
    return dtype


def check_sizes(sizes, batch: int, canvas_hw, minimum: int = 8, what: str = "valid_size") -> list:
    """Host-side validation of the per-image extents of a ragged batch: `sizes` is `[batch, 2]` `(w, h)` — a tensor, an array or nested
    sequences — integer-valued, with `minimum <= h <= canvas_hw[0]` and `minimum <= w <= canvas_hw[1]`.  Returns them as a list of
    `[w, h]` Python ints; raises ValueError naming the first offending image.  (The kernels clamp what they are given into the canvas;
    this is the check proper, made where the sizes are host integers.  A device tensor is copied to the host for it.)"""
    t = torch.as_tensor(sizes).detach().cpu()
    if t.dim() != 2 or tuple(t.shape) != (batch, 2):
        raise ValueError(f"{what} must have shape [{batch}, 2] = (w, h) per image, got {tuple(t.shape)}")
    if t.dtype == torch.bool or t.is_complex():
        raise ValueError(f"{what} must hold integers, got {t.dtype}")
    if t.is_floating_point():
        bad = ((t != t.round()) | ~torch.isfinite(t)).any(dim=1).nonzero()
        if bad.numel():
            i = int(bad[0])
            raise ValueError(f"{what}[{i}] = {t[i].tolist()} is not integer-valued")
    rows = [[int(v) for v in row] for row in t.tolist()]
    hc, wc = int(canvas_hw[0]), int(canvas_hw[1])
    for i, (w, h) in enumerate(rows):
        if w < minimum or h < minimum:
            raise ValueError(f"{what}[{i}] = (w {w}, h {h}) is below the minimum of {minimum}")
        if w > wc or h > hc:
            raise ValueError(f"{what}[{i}] = (w {w}, h {h}) does not fit the canvas (w {wc}, h {hc})")
    return rows


def sizes_on_device(rows: list, device) -> torch.Tensor:
    """int32 `[B, 2]` device array of validated `(w, h)` rows: the `sizes` field of a stage's io under LG_EXTRACT_RAGGED"""
    return torch.tensor(rows, dtype=torch.int32).reshape(-1, 2).to(device)


def device_sizes(sizes, device) -> Optional[torch.Tensor]:
    """None, validated host rows (check_sizes) or the int32 device array made from them -> that device array (or None)"""
    return sizes if sizes is None or torch.is_tensor(sizes) else sizes_on_device(sizes, device)


def _run(keypoints: torch.Tensor, dense: torch.Tensor, s: int, normalize_dense: bool,
         num_keypoints: Optional[torch.Tensor], dtype: torch.dtype = torch.float32, sizes: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`sizes`: None, or the VALIDATED int32 device array `[B, 2]` of the images' `(w, h)` (`sizes_on_device(check_sizes(...))`): `dense` is then a canvas"""
    check_descriptor_dtype(dtype)
    if dense.device.type != "cuda":
        raise RuntimeError("lightglue_amd.superpoint_head runs on MI355X (ROCm device type 'cuda') only; there is no "
                           f"CPU fallback. Got a descriptor map on {dense.device}.")
    b, c, h, w = dense.shape
    assert keypoints.shape[0] == b and keypoints.shape[-1] == 2, "keypoints must be [B, N, 2]"
    device = dense.device
    f32 = lambda t: t.detach().to(device=device, dtype=torch.float32).contiguous()
    dense, keypoints = f32(dense), f32(keypoints)
    n = keypoints.shape[1]
    num = None
    if num_keypoints is not None:
        num = torch.as_tensor(num_keypoints).to(device=device, dtype=torch.int32).contiguous()
        assert num.shape == (b,)
    out = torch.empty((b, n, c), device=device, dtype=dtype)
    work = torch.empty((b, h, w, c), device=device, dtype=torch.float32)
    ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream(device).cuda_stream
        flags = (_cabi.LG_EXTRACT_RAGGED if sizes is not None else 0) | (_cabi.LG_EXTRACT_DESC_F16 if dtype is torch.float16 else 0)
        io = _cabi.LgSpSampleIO(batch=b, channels=c, h=h, w=w, flags=flags, desc_map=ptr(dense), sizes=ptr(sizes), keypoints=ptr(keypoints), num=ptr(num),
                                n=n, cell=int(s), normalize_dense=int(normalize_dense), workspace=ptr(work), out=ptr(out))
        _cabi.check(_cabi.load().lg_sp_sample_descriptors(C.byref(io), C.c_void_p(stream)))
    return out


def sample_descriptors(keypoints: torch.Tensor, descriptors: torch.Tensor, s: int = 8, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """Same contract as the reference function (superpoint.py:80-95): `keypoints [b, N, 2]` pixel (x, y),
    `descriptors [b, c, h, w]` -> L2-normalised bilinear samples `[b, c, N]` (a transposed view of the kernel's
    matcher-ready `[b, N, c]` output).  Unlike the reference, `keypoints` is not modified in place.  `dtype=torch.float16`: the fp32 result
    rounded once on store (`LG_EXTRACT_DESC_F16`), bit-identical to `.half()` of the fp32 output."""
    return _run(keypoints, descriptors, s, False, None, dtype).transpose(1, 2)


def descriptor_head(keypoints: torch.Tensor, dense_descriptors: torch.Tensor, s: int = 8,
                    num_keypoints: Optional[torch.Tensor] = None, dtype: torch.dtype = torch.float32, sizes=None) -> torch.Tensor:
    """Descriptor tail of SuperPoint.forward (superpoint.py:216-228) for a whole (ragged) batch: dense L2
    normalisation over channels, sampling at the keypoints, final normalisation, `[B, N, 256]` layout.
    `dense_descriptors` is the raw `convDb` output `[B, 256, H/8, W/8]`; rows >= num_keypoints[b] come back zero.  `dtype` as for `sample_descriptors`.
    `sizes` (ragged batch): `[B, 2]` `(w, h)` of the IMAGES; `dense_descriptors` is then the canvas `SuperPoint.encode(image, valid_size)` returns and the map
    of image b its top-left `(h_b // s, w_b // s)` corner, which alone is read: rows < num_keypoints[b] are bit-identical to the call on that crop."""
    if sizes is not None:
        h, w = dense_descriptors.shape[-2:]
        sizes = sizes_on_device(check_sizes(sizes, dense_descriptors.shape[0], (h * s + s - 1, w * s + s - 1), s, "sizes"), dense_descriptors.device)
    return _run(keypoints, dense_descriptors, s, True, num_keypoints, dtype, sizes)


def detect_keypoints(scores: torch.Tensor, nms_radius: int = 4, remove_borders: int = 4, detection_threshold: float = 0.0005,
                     max_num_keypoints: Optional[int] = None, capacity: Optional[int] = None, sizes=None):
    """Keypoint extraction of SuperPoint.forward (superpoint.py:186-218) on the dense score map `scores [B, H, W]`
    (after softmax / depth-to-space, :176-184): simple_nms, border removal, threshold, optional top-k.

    Returns `(keypoints [B, C, 2] float (x, y), keypoint_scores [B, C], num_keypoints [B] int32)` — a ragged batch in
    the form `LightGlue.forward` / `descriptor_head` take (`num_keypoints`); rows >= num_keypoints[b] are undefined.
    C = `capacity` (default: max_num_keypoints, or 1/8 of the pixels when it is None).  Without top-k, raises if an
    image has more detections than `capacity` rows (the internal candidate buffer always holds every pixel).

    `sizes` (ragged batch): `[B, 2]` `(w, h)` of the SCORE maps; `scores` is then a canvas whose top-left `h_b x w_b` corner is the map of image b.
    Whatever lies outside is never read — it is max_pool2d's -inf padding, and the far borders are the map's — so the result is exactly that of
    the call on each crop, keypoints in the crop's own frame."""
    if sizes is not None and scores.device.type == "cuda":
        sizes = sizes_on_device(check_sizes(sizes, scores.shape[0], scores.shape[-2:], 1, "sizes"), scores.device)
    return _detect(scores, nms_radius, remove_borders, detection_threshold, max_num_keypoints, capacity, sizes)


def _detect(scores: torch.Tensor, nms_radius: int, remove_borders: int, detection_threshold: float, max_num_keypoints: Optional[int],
            capacity: Optional[int], sizes: Optional[torch.Tensor]):
    """detect_keypoints with `sizes` already validated and on the device (int32 `[B, 2]`), or None"""
    if scores.device.type != "cuda":
        raise RuntimeError("lightglue_amd.superpoint_head runs on MI355X (ROCm device type 'cuda') only; there is no "
                           f"CPU fallback. Got scores on {scores.device}.")
    if max_num_keypoints is not None and max_num_keypoints <= 0:
        raise ValueError("max_num_keypoints must be positive or None")   # ref superpoint.py:143-144
    b, h, w = scores.shape
    device = scores.device
    scores = scores.detach().to(dtype=torch.float32).contiguous()
    k = int(max_num_keypoints) if max_num_keypoints is not None else 0
    cap = int(capacity) if capacity is not None else (k if k > 0 else max(1, h * w // 8))
    maxc = h * w   # candidates before top-k: worst case every pixel (8 bytes each, twice the score map)
    lib = _cabi.load()
    nbytes = lib.lg_sp_detect_workspace_bytes(b, h, w, maxc)
    work = torch.empty((nbytes,), device=device, dtype=torch.uint8)
    kpts = torch.empty((b, cap, 2), device=device, dtype=torch.float32)
    kscores = torch.empty((b, cap), device=device, dtype=torch.float32)
    counts = torch.empty((b,), device=device, dtype=torch.int32)
    totals = torch.empty((b,), device=device, dtype=torch.int32)
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream(device).cuda_stream
        io = _cabi.LgSpDetectIO(batch=b, h=h, w=w, flags=_cabi.LG_EXTRACT_RAGGED if sizes is not None else 0, scores=scores.data_ptr(),
                                sizes=None if sizes is None else sizes.data_ptr(), nms_radius=int(nms_radius), remove_borders=int(remove_borders),
                                detection_threshold=float(detection_threshold), max_keypoints=k, capacity=cap, max_candidates=maxc, workspace=work.data_ptr(),
                                workspace_bytes=nbytes, keypoints=kpts.data_ptr(), kp_scores=kscores.data_ptr(), counts=counts.data_ptr(), totals=totals.data_ptr())
        _cabi.check(lib.lg_sp_detect(C.byref(io), C.c_void_p(stream)))
    if k == 0:
        worst = int(totals.max().item())
        if worst > cap:
            raise RuntimeError(f"{worst} detections in one image exceed `capacity` = {cap} output rows; pass a larger one")
    return kpts, kscores, counts
