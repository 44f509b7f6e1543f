"""SIFT feature stores (the reference's `lightglue/sift.py:17-56, 177-194`; the SIFT detector itself — cv2 / pycolmap — is out of scope): what turns raw SIFT
detections, as COLMAP, pycolmap or OpenCV hand them over, into a store `LightGlue(features="sift").match_pairs` reads in place.

  * `sift_to_rootsift`: the descriptor transform the SIFT LightGlue weights expect, one HIP launch on fp32 / float16 / uint8 rows.  A store can also carry it as
    `descriptor_transform = "rootsift"`: the engine then applies the same device code where the descriptors enter it, and uint8 rows stay uint8 in memory.
  * `filter_dog_point`: duplicate removal (several orientations per point) and optional NMS, on the device, for one image or a ragged set.
  * `sift_features`: filter, top-k, gather -> the store `collate_features` would give.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _cabi

_KIND = {torch.float32: 0, torch.float16: 1, torch.uint8: 2}


def _stream_ptr(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def sift_to_rootsift(x: torch.Tensor, eps: float = 1e-6, out_dtype=None) -> torch.Tensor:
    """RootSIFT of every row of `x` [..., D]: L1-normalise, clip at eps, sqrt, L2-normalise (ref sift.py:53-56).  Device tensors (fp32 / float16 / uint8 rows,
    D a multiple of 4 up to 256) go through ONE launch of `lg_rootsift`, which reads the rows in their storage format; `out_dtype` torch.float32 (default) or
    torch.float16 (the fp32 result rounded once).  A CPU tensor takes the reference's torch expression.  Only eps = 1e-6 is built on the device."""
    out_dtype = torch.float32 if out_dtype is None else out_dtype
    if out_dtype not in (torch.float32, torch.float16):
        raise ValueError(f"out_dtype must be torch.float32 or torch.float16, got {out_dtype}")
    if x.device.type != "cuda":
        y = torch.nn.functional.normalize(x.to(torch.float32), p=1, dim=-1, eps=eps)     # (.to: a copy unless fp32 already, and normalize never writes its input)
        y = y.clip_(min=eps).sqrt_()
        return torch.nn.functional.normalize(y, p=2, dim=-1, eps=eps).to(out_dtype)
    if eps != 1e-6:
        raise ValueError("sift_to_rootsift on the device is built for eps = 1e-6 only")
    if x.dtype not in _KIND:
        x = x.to(torch.float32)
    D = int(x.shape[-1]) if x.dim() else 0
    if x.dim() < 1 or D < 4 or D > 256 or D % 4:
        raise ValueError(f"sift_to_rootsift on the device needs rows of 4 .. 256 values, a multiple of 4; got shape {tuple(x.shape)}")
    x = x.detach().contiguous()
    if x.data_ptr() % (4 * x.element_size()):      # the kernel loads four elements at a time
        x = x.clone()
    out = torch.empty(x.shape, device=x.device, dtype=out_dtype)
    rows = x.numel() // D
    with torch.cuda.device(x.device):
        _cabi.check(_cabi.load().lg_rootsift(x.data_ptr(), _KIND[x.dtype], rows, D, out.data_ptr(), int(out_dtype is torch.float16), _stream_ptr(x.device)))
    return out


def _f32(t, device):
    return torch.as_tensor(t).detach().to(device=device, dtype=torch.float32).contiguous()


def filter_dog_point(points, scales, angles, image_shape, nms_radius, scores=None, num_keypoints=None):
    """The reference's `filter_dog_point` (sift.py:17-50) on the device -> `keep`, the int64 indices of the detections that stay, ascending (np.where's order).

    One image: points [N, 2] (x, y), scales / angles / scores [N], image_shape (h, w).  With s = scores if given, else scales, and the pixel
    p_i = (round_half_even(y_i - 0.5), round_half_even(x_i - 0.5)):  keep i iff s_i equals max(0, max s at p_i) (so s < 0 drops out); among those iff |angle_i| is
    the lowest at p_i; and, with nms_radius > 0, iff the value kept at p_i is the maximum of the (2 r + 1)^2 window clipped to the image.  Every comparison is
    exact and the result does not depend on any order.  A detection whose pixel lies outside h x w is DROPPED (the reference wraps a negative index and raises on
    a large one).

    Ragged batch: points [K, N, 2], scales / angles / scores [K, N], num_keypoints [K] (None: N each), image_shape one (h, w) or K of them (sequence or [K, 2]
    tensor) -> (keep [K, N] int64: the kept indices of image k in ascending order, then -1; counts [K] int64)."""
    points = torch.as_tensor(points)
    device = points.device
    if device.type != "cuda":
        raise RuntimeError(f"lightglue_amd.filter_dog_point runs on MI355X (ROCm device type 'cuda') only; got points on {device}")
    single = points.dim() == 2
    if single:
        assert num_keypoints is None, "num_keypoints belongs to the batched form (points [K, N, 2])"
    pts = _f32(points, device)
    pts = pts[None] if single else pts
    assert pts.dim() == 3 and pts.shape[-1] == 2, f"points must have shape [N, 2] or [K, N, 2], got {tuple(points.shape)}"
    K, N = int(pts.shape[0]), int(pts.shape[1])

    def per_point(t, name):
        t = _f32(t, device).reshape(1, -1) if single else _f32(t, device)
        assert tuple(t.shape) == (K, N), f"{name} must have shape {[N] if single else [K, N]}, got {tuple(t.shape)}"
        return t
    sc, an = per_point(scales, "scales"), per_point(angles, "angles")
    sco = None if scores is None else per_point(scores, "scores")
    shape = torch.as_tensor(image_shape).detach().to("cpu", torch.int64).reshape(-1, 2)      # host integers: they size the workspace
    assert shape.shape[0] in (1, K), f"image_shape must be one (h, w) or {K} of them"
    shape = shape.expand(K, 2)
    max_h, max_w = max(int(shape[:, 0].max()), 1), max(int(shape[:, 1].max()), 1)
    nms_radius = int(nms_radius)
    keep = torch.empty((K, N), device=device, dtype=torch.int64)
    counts = torch.empty((K,), device=device, dtype=torch.int32)
    if K == 0:
        return keep, counts.to(torch.int64)
    sizes = shape.to(torch.int32).contiguous().to(device)
    num = None if num_keypoints is None else torch.as_tensor(num_keypoints).detach().to(device=device, dtype=torch.int32).contiguous()
    assert num is None or num.shape == (K,), f"num_keypoints must have shape [{K}]"
    lib = _cabi.load()
    nbytes = int(lib.lg_sift_filter_workspace_bytes(K, N, max_h, max_w))
    ws = torch.empty((max(nbytes, 256),), device=device, dtype=torch.uint8)      # (the caching allocator's blocks are 512-byte aligned)
    ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()
    with torch.cuda.device(device):
        _cabi.check(lib.lg_sift_filter(ptr(pts), ptr(sc), ptr(an), ptr(sco), ptr(num), sizes.data_ptr(), K, N, max_h, max_w, nms_radius,
                                       ws.data_ptr(), ws.numel(), ptr(keep), counts.data_ptr(), _stream_ptr(device)))
    if single:
        return keep[0, : int(counts[0])]
    return keep, counts.to(torch.int64)


def sift_features(keypoints, scales, oris, descriptors, image_size, scores=None, nms_radius: Optional[int] = 0, max_num_keypoints: Optional[int] = 4096,
                  rootsift="on_entry") -> dict:
    """Raw SIFT detections of K images -> a feature store for `LightGlue(features="sift")` (what the reference's `SIFT.extract_single_image` does behind its
    detector, sift.py:177-194, then `collate_features`).

    Per image (a tensor each, or a list of K of them): keypoints [N, 2], scales / oris [N], descriptors [N, D] in any dtype (uint8 stays uint8), scores [N] or
    None; image_size (w, h), one or K of them.  Steps: `filter_dog_point` (nms_radius None skips it); when scores are given and more than max_num_keypoints
    remain, the best by score (torch.topk: descending); gather.  rootsift = "on_entry": the store carries descriptor_transform = "rootsift" and the engine
    transforms every row where it reads it — the descriptors stay as stored; True: `sift_to_rootsift` now, fp32 descriptors; False: neither.

    Returns {keypoints [K, Nmax, 2], scales, oris, keypoint_scores (with scores) [K, Nmax], descriptors [K, Nmax, D], image_size [K, 2], num_keypoints [K]}."""
    from .glue import collate_features
    if rootsift not in ("on_entry", True, False):
        raise ValueError(f"rootsift must be 'on_entry', True or False, got {rootsift!r}")
    as_list = lambda v: list(v) if isinstance(v, (list, tuple)) else [v]
    kps, scs, ors, dss = as_list(keypoints), as_list(scales), as_list(oris), as_list(descriptors)
    K = len(kps)
    scos = [None] * K if scores is None else as_list(scores)
    sizes = torch.as_tensor(image_size).detach().to("cpu", torch.int64).reshape(-1, 2)
    assert len(scs) == len(ors) == len(dss) == len(scos) == K and sizes.shape[0] in (1, K), "every per-image argument must hold the same number of images"
    sizes = sizes.expand(K, 2)
    assert all(s is None for s in scos) or all(s is not None for s in scos), "scores for every image or for none"
    keeps = [None] * K
    if nms_radius is not None and K:      # ONE ragged call for all K images: one workspace, one host synchronisation (the counts)
        device = kps[0].device
        counts = [int(kp.shape[0]) for kp in kps]
        N = max(counts)

        def padded(ts, *tail):            # [K, N, ...]; what lies past an image's count is never read
            buf = torch.zeros((K, N) + tail, device=device, dtype=torch.float32)
            for k, t in enumerate(ts):
                buf[k, : counts[k]] = torch.as_tensor(t).to(device=device, dtype=torch.float32)
            return buf
        keep, kept = filter_dog_point(padded(kps, 2), padded(scs), padded(ors), sizes.flip(1), nms_radius,
                                      scores=None if scos[0] is None else padded(scos), num_keypoints=torch.tensor(counts))
        keeps = [keep[k, :c] for k, c in enumerate(kept.tolist())]
    items = []
    for k in range(K):
        w, h = int(sizes[k, 0]), int(sizes[k, 1])
        f = {"keypoints": kps[k], "scales": scs[k], "oris": ors[k], "descriptors": dss[k]}
        if scos[k] is not None:
            f["keypoint_scores"] = scos[k]
        if keeps[k] is not None:
            f = {key: v[keeps[k]] for key, v in f.items()}
        if scos[k] is not None and max_num_keypoints is not None and f["keypoints"].shape[0] > max_num_keypoints:
            best = torch.topk(f["keypoint_scores"], int(max_num_keypoints)).indices
            f = {key: v[best] for key, v in f.items()}
        if rootsift is True:
            f["descriptors"] = sift_to_rootsift(f["descriptors"])
        f["image_size"] = torch.tensor([w, h], dtype=torch.float32)
        items.append(f)
    store = collate_features(items)
    if rootsift == "on_entry":
        store["descriptor_transform"] = "rootsift"
    return store
