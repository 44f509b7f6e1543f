"""Extractor -> matcher plumbing: behaviour of the reference's `rbd`, `batch_to_device` and
`match_pair` helpers (reference `lightglue/utils.py:55-69, 150-165`), written for this package.  `match_pair` accepts any object
with the reference's `extract(image, **preprocess) -> dict` contract (`lightglue/utils.py:136-147`); this package's extractors honour
`**preprocess` (`resize=`, `side=`, `antialias=`, `align_corners=`) through `preprocess.ImagePreprocessor` on the device.  Image file
I/O is out of scope.  `extracted_to_image_frame` is the keypoint / image_size step of `extract` on its own, for callers who resized by
other means."""
from __future__ import annotations

from typing import Any, Callable, Dict

import torch

from ._call import descriptor_transform


def _apply_to_tensors(obj: Any, fn: Callable[[torch.Tensor], torch.Tensor]) -> Any:
    """Rebuild nested dict / list / tuple containers with `fn` applied to every tensor leaf."""
    if torch.is_tensor(obj):
        return fn(obj)
    if isinstance(obj, dict):
        return {key: _apply_to_tensors(val, fn) for key, val in obj.items()}
    if isinstance(obj, (list, tuple)):
        return [_apply_to_tensors(val, fn) for val in obj]
    return obj  # str, int, None, ...


def batch_to_device(batch: Dict[str, Any], device: str = "cpu", non_blocking: bool = True) -> Dict[str, Any]:
    """Detached copy of every tensor in `batch` on `device`."""
    return _apply_to_tensors(batch, lambda t: t.detach().to(device=device, non_blocking=non_blocking))


def prefetch_to_device(batches, device="cuda", depth: int = 2):
    """Host batches -> device batches, up to `depth` of them AHEAD of the consumer, copied on a separate HIP stream (no reference counterpart: the reference's
    callers do `batch_to_device` on the compute stream, `lightglue/utils.py:63-69`).  For a matcher fed from host memory — features arriving over the network or from
    an extractor on another device — the host-to-device copy of batch i + 1 then runs under the forward of batch i instead of in front of it (cfg #2: 68 MB per batch,
    about 1.2 ms over PCIe against a 7.4 ms forward; measured by `bench.py`'s `pcie_inclusive` block).  Tensors that are not in pinned memory are staged through a pinned
    copy first (a pageable source would make the copy synchronous); pass pinned tensors to avoid that extra host pass.  Every yielded batch is ordered behind its copy on
    the stream that is current when it is consumed, and its device memory is handed to that stream (`record_stream`), so nothing else is needed before `matcher(batch)`."""
    import collections
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("prefetch_to_device copies to an MI355X (ROCm device type 'cuda')")
    if depth < 1:
        raise ValueError("depth must be >= 1")
    copy_stream = torch.cuda.Stream(device)
    queue = collections.deque()

    def stage(batch):
        def to_dev(t):
            if t.is_cuda:
                return t
            src = t.detach()
            if not src.is_pinned():
                src = src.contiguous().pin_memory()
            return src.to(device, non_blocking=True), src
        keep = []
        def conv(t):
            r = to_dev(t)
            if isinstance(r, tuple):
                keep.append(r[1])
                return r[0]
            return r
        with torch.cuda.stream(copy_stream):
            dev = _apply_to_tensors(batch, conv)
            done = torch.cuda.Event()
            done.record(copy_stream)
        return dev, done, keep           # `keep`: the pinned sources stay alive until the copy has been waited for

    def release(item):
        dev, done, _keep = item
        cur = torch.cuda.current_stream(device)
        cur.wait_event(done)
        _apply_to_tensors(dev, lambda t: (t.record_stream(cur), t)[1] if t.is_cuda else t)
        return dev

    for batch in batches:
        queue.append(stage(batch))
        if len(queue) > depth:
            yield release(queue.popleft())
    while queue:
        yield release(queue.popleft())


def rbd(data: Dict[str, Any]) -> Dict[str, Any]:
    """Strip the leading batch dimension: tensors and per-batch lists/tuples yield their first item, scalars
    (e.g. `stop`) pass through."""
    out = {}
    for key, val in data.items():
        indexable = torch.is_tensor(val) or isinstance(val, (list, tuple))
        out[key] = val[0] if indexable else val
    return out


def match_pair(extractor, matcher, image0: torch.Tensor, image1: torch.Tensor, device: str = "cuda", **preprocess):
    """Extract both images, match them, and return (feats0, feats1, matches01) without batch dimension on `device`."""
    feats = [extractor.extract(img, **preprocess) for img in (image0, image1)]
    matches01 = matcher({"image0": feats[0], "image1": feats[1]})
    feats0, feats1, matches01 = (batch_to_device(rbd(d), device) for d in (feats[0], feats[1], matches01))
    return feats0, feats1, matches01


def extracted_to_image_frame(feats: Dict[str, Any], original_hw, scales: torch.Tensor) -> Dict[str, Any]:
    """The last two steps of the reference's `Extractor.extract` (`lightglue/utils.py:142-147`) for an extractor that
    ran on a RESIZED image: keypoints go back to the original image's pixel frame, `(k + 0.5) / scales - 0.5`, and
    `image_size` = original (width, height) is attached — the two fields the matcher's keypoint normalisation reads
    (`lightglue.py:32-43`).  `original_hw` = (H, W) of the image before resizing, `scales` = resized / original per axis
    (x, y) as the reference's ImagePreprocessor returns it."""
    kp = feats["keypoints"]
    scales = torch.as_tensor(scales, dtype=kp.dtype, device=kp.device)
    out = dict(feats)
    out["keypoints"] = (kp + 0.5) / scales[None] - 0.5
    h, w = int(original_hw[0]), int(original_hw[1])
    out["image_size"] = torch.tensor([[w, h]], dtype=kp.dtype, device=kp.device)
    return out


_PER_KEYPOINT = ("keypoints", "descriptors", "scales", "oris", "keypoint_scores")


def collate_features(feats: list) -> Dict[str, Any]:
    """Stack per-image feature dicts with DIFFERENT keypoint counts into one ragged batch for `LightGlue.forward`.

    Each item follows the extractor contract (reference `lightglue/utils.py:136-147`), with or without the leading
    batch dimension of 1: `keypoints [N_i,2]`, `descriptors [N_i,D]`, optional `scales`/`oris`/`keypoint_scores
    [N_i]` and `image_size [2]`.  Per-keypoint tensors are zero-padded to max N_i and `num_keypoints [B]` carries
    the true counts; the engine never reads the padding (the reference instead pads with ones and masks every
    attention call, `lightglue.py:46-55, 512-520`, and only inside `compile()`d B=1 calls).  Descriptors stay float16 / uint8
    when every item stores them so, else fp32; `descriptor_transform` (None | "rootsift") is carried when all items agree."""
    items = []
    for f in feats:
        kp = f["keypoints"]
        items.append(rbd(f) if kp.dim() == 3 else f)
    counts = [int(f["keypoints"].shape[0]) for f in items]
    nmax = max(counts) if counts else 0
    out: Dict[str, Any] = {}
    for key in _PER_KEYPOINT:
        if not all(key in f for f in items):
            continue
        first = items[0][key]
        dtype = first.dtype
        if key == "descriptors" and dtype in (torch.float16, torch.uint8) and not all(f[key].dtype is dtype for f in items):
            dtype = torch.float32   # float16 / uint8 only when EVERY item stores it: a float16 first item must not round the fp32 ones behind it
        buf = first.new_zeros((len(items), nmax) + tuple(first.shape[1:]), dtype=dtype)
        for b, f in enumerate(items):
            buf[b, : counts[b]] = f[key]
        out[key] = buf
    if all("image_size" in f for f in items):
        out["image_size"] = torch.stack([torch.as_tensor(f["image_size"], dtype=torch.float32).reshape(2) for f in items]).to(out["keypoints"].device)
    out["num_keypoints"] = torch.tensor(counts, dtype=torch.int32, device=out["keypoints"].device)
    transforms = {descriptor_transform(f, f"feats[{b}]") for b, f in enumerate(items)}
    if len(transforms) > 1:
        raise ValueError(f"descriptor_transform differs between the items ({sorted(map(str, transforms))}): one store has one transform")
    if transforms and transforms != {None}:
        out["descriptor_transform"] = transforms.pop()
    return out


def _as_store(feats):
    """a feature store as it is; a list of per-image dicts collated into one"""
    return collate_features(feats) if isinstance(feats, (list, tuple)) else feats


def _trimmed(res: dict, b: int, n0: int, n1: int, stop) -> dict:
    """pair b of a batched result as an `rbd`-style dict, trimmed to the pair's own keypoint counts"""
    return {
        "matches0": res["matches0"][b, :n0], "matches1": res["matches1"][b, :n1],
        "matching_scores0": res["matching_scores0"][b, :n0], "matching_scores1": res["matching_scores1"][b, :n1],
        "matches": res["matches"][b], "scores": res["scores"][b],
        "prune0": res["prune0"][b, :n0], "prune1": res["prune1"][b, :n1],
        "stop": stop,
    }


def match_batch(matcher, feats0: list, feats1: list) -> list:
    """Match B independent image pairs with ragged keypoint counts in ONE forward; returns one `rbd`-style result
    dict per pair, trimmed to that pair's own keypoint counts (what B separate `matcher(...)` calls would give)."""
    assert len(feats0) == len(feats1)
    batch0, batch1 = collate_features(feats0), collate_features(feats1)
    res = matcher({"image0": batch0, "image1": batch1})
    n0, n1 = batch0["num_keypoints"].tolist(), batch1["num_keypoints"].tolist()
    stop = res["stop"]
    return [_trimmed(res, b, n0[b], n1[b], int(stop[b]) if torch.is_tensor(stop) else stop) for b in range(len(feats0))]


def match_pairs(matcher, feats, pairs, feats1=None) -> list:
    """Match a pair list over extracted images: pair (i, j) matches image i of `feats` against image j of `feats1` (None: of `feats` too).  `feats` / `feats1`:
    a feature store (the output of an extractor on an image batch, or of `collate_features`) or a list of per-image dicts, which is collated ONCE — the
    matcher then reads every pair's rows in the store (`LightGlue.match_pairs`: nothing is stacked per pair, and the list may be longer than one engine
    call).  Returns one `rbd`-style result dict per pair, trimmed to that pair's own keypoint counts, as `match_batch` does."""
    store0, store1 = _as_store(feats), None if feats1 is None or feats1 is feats else _as_store(feats1)
    res = matcher.match_pairs(store0, pairs, store1)
    def counts(store):
        num = store.get("num_keypoints")
        return [int(store["keypoints"].shape[1])] * int(store["keypoints"].shape[0]) if num is None else torch.as_tensor(num).tolist()
    c0 = counts(store0)
    c1 = c0 if store1 is None else counts(store1)
    stop = res["stop"]
    stops = stop.tolist() if torch.is_tensor(stop) else [stop]
    return [_trimmed(res, b, c0[i], c1[j], int(stops[b])) for b, (i, j) in enumerate(torch.as_tensor(pairs).reshape(-1, 2).tolist())]


def verify_pairs(verifier, result, feats, pairs, feats1=None) -> dict:
    """Geometric verification of what `matcher.match_pairs(feats, pairs, feats1)` returned (`result`: its dict or its `DeferredMatches`), by a
    `TwoViewVerifier`: the same stores (or lists of per-image dicts, collated once) and the same pair list; only `keypoints` and `num_keypoints` are read.
    Returns the verifier's dict: models [P, 3, 3], inliers0 [P, N0], num_inliers [P], matches0 (-1 off the inliers), matches, best_hypothesis."""
    store0, store1 = _as_store(feats), None if feats1 is None or feats1 is feats else _as_store(feats1)
    return verifier.verify_pairs(store0, pairs, result, store1)


def estimate_poses(estimator, result, feats, pairs, cameras, feats1=None, cameras1=None) -> dict:
    """Relative pose from what `matcher.match_pairs(feats, pairs, feats1)` returned (`result`: its dict or its `DeferredMatches`), by a
    `RelativePoseEstimator`: the same stores (or lists of per-image dicts, collated once), the same pair list and one camera per image of either store
    ([K, 4] (fx, fy, cx, cy) or [K, 3, 3]; cameras1 None: `cameras`).  Returns the estimator's dict: R [P, 3, 3], t [P, 3], E, models, inliers0, num_inliers,
    num_in_front, matches0 (-1 off the inliers), matches, best_hypothesis."""
    store0, store1 = _as_store(feats), None if feats1 is None or feats1 is feats else _as_store(feats1)
    return estimator.estimate_pairs(store0, pairs, result, cameras, store1, cameras1)


def estimate_absolute_poses(estimator, result, feats, pairs, cameras, points3d, feats1=None, pool: bool = True) -> dict:
    """Absolute pose of the query images from what `matcher.match_pairs(feats, pairs, feats1)` returned (`result`: its dict or its `DeferredMatches`), by an
    `AbsolutePoseEstimator`: the same stores (or lists of per-image dicts, collated once), the same pair list (query, database), one camera per query image
    ([K, 4] (fx, fy, cx, cy) or [K, 3, 3]) and the world point of every database keypoint row (points3d [K1, N1, 3], NaN where a row has none).  pool: all
    pairs of one query form ONE 2-D - 3-D problem (how localisation runs PnP); without it one problem per pair.  Returns the estimator's dict: R [G, 3, 3],
    t [G, 3], num_inliers, best_hypothesis, queries [G], group_of_pair [P], and per pair inliers0, pair_num_inliers, matches0 (-1 off the inliers), matches."""
    store0, store1 = _as_store(feats), None if feats1 is None or feats1 is feats else _as_store(feats1)
    return estimator.estimate_pairs(store0, pairs, result, cameras, points3d, store1, pool=pool)


def triangulate_tracks(triangulator, result, feats, pairs, cameras, poses) -> dict:
    """Tracks and their world points from what `matcher.match_pairs(feats, pairs)` or a verifier over the same list returned (`result`: a dict, a
    `DeferredMatches` or matches0 itself), by a `Triangulator`: the same store (or a list of per-image dicts, collated once), the same pair list — both
    columns index the one store —, one camera ([K, 4] (fx, fy, cx, cy) or [K, 3, 3]) and one known pose ([K, 3, 4] (R | t) or (R, t)) per image.  Returns the
    triangulator's dict; its points3d [K, N, 3] is what `estimate_absolute_poses` takes as points3d."""
    return triangulator.triangulate(_as_store(feats), pairs, result, cameras, poses)


def bundle_adjust(adjuster, tracks, feats, cameras, poses, constant_pose, constant_camera=None) -> dict:
    """Joint refinement of the free poses and of all track points from what `triangulate_tracks` returned (`tracks`: its dict, or (track_id, xyz)), by a
    `BundleAdjuster`: the same store (or a list of per-image dicts, collated once), the same cameras and poses, and the images whose pose is held fixed
    (constant_pose: a [K] bool mask or image indices; at least one, two fix scale) and, with an adjuster built with refine_focal=True, the images whose focal
    length is held (constant_camera: None, a mask or indices).  Returns the adjuster's dict; its points3d [K, N, 3] is what
    `estimate_absolute_poses` takes as points3d."""
    return adjuster.adjust(_as_store(feats), tracks, cameras, poses, constant_pose, constant_camera)


def estimate_global_poses(estimator, relative, pairs, num_images, **kw) -> dict:
    """One pose per image from what `estimate_poses` returned over the same pair list (`relative`: its dict, or (R, t)), by a `GlobalPoseEstimator`: rotation
    and position averaging over the view graph of `num_images` images; **kw: origin, baseline, weights.  Returns the estimator's dict; its poses [K, 3, 4] are
    what `triangulate_tracks` and `bundle_adjust` take, its origin and baseline the two images to hold constant there (the same gauge and scale)."""
    return estimator.estimate(pairs, relative, num_images, **kw)


def position_from_tracks(positioner, tracks, feats, cameras, poses, constant_pose=None) -> dict:
    """Camera centres and track points from the tracks of `Triangulator.build_tracks` (`tracks`: its dict, or (track_id, T)) and the rotations of
    `estimate_global_poses` (`poses`: its dict — origin and baseline are then held —, [K, 3, 4] or (R, t)), by a `GlobalPositioner`: the same store (or a list
    of per-image dicts, collated once) and cameras; constant_pose: a [K] bool mask or image indices, at least two.  Returns the positioner's dict: its poses are
    what `triangulate_tracks` takes, (track_id, xyz) what `bundle_adjust` takes as `tracks`, points3d what `estimate_absolute_poses` takes."""
    return positioner.solve(_as_store(feats), tracks, cameras, poses, constant_pose)


def cm_prune(prune):
    """RGBA colour per keypoint from the matcher's ``prune0`` / ``prune1`` output (the layer at which a point was
    dropped; points alive to the end carry the maximum) — the consumer the reference ships for that output
    (``lightglue/viz2d.py:33-39`` with its ``cm_BlRdGn`` ramp, :22-31): survivors blue, the others red (dropped after
    layer 1) -> yellow -> green (layer 10).  Pure numpy: returns ``[N, 4]`` floats in [0, 1] for any plotting backend."""
    import numpy as np
    p = np.asarray(prune.detach().cpu() if isinstance(prune, torch.Tensor) else prune, dtype=np.float64)
    t = np.where(p == p.max(), -1.0, (p - 1.0) / 9.0)              # -1 marks the survivors
    up = 2.0 * np.clip(t, 0.0, 1.0)[..., None]                       # red (0) -> green (1)
    ramp = up * np.array([0.0, 1.0, 0.0, 1.0]) + (2.0 - up) * np.array([1.0, 0.0, 0.0, 1.0])
    dn = -2.0 * np.clip(t, -1.0, 0.0)[..., None]                     # red (0) -> blue (-1)
    blue = dn * np.array([0.0, 0.1, 1.0, 1.0]) + (2.0 - dn) * np.array([1.0, 0.0, 0.0, 1.0])
    return np.clip(np.where(t[..., None] < 0.0, blue, ramp), 0.0, 1.0)
