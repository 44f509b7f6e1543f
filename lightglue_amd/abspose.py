"""Absolute pose of query cameras against a known model on the device: P3P RANSAC with a fixed hypothesis budget over 2-D - 3-D matches, on the kernels of
`csrc/lg_abspose.hip` behind `lg_abspose_estimate` (include/lightglue_amd.h holds the definition).  It reads what a matcher leaves on the device — the query
keypoint store, the pair list and `matches0` — in place, plus one world point per database keypoint row and one pinhole camera (fx, fy, cx, cy) per query
image.  A problem is one pair, or — `pool=True`, how localisation runs PnP — all pairs of one query image: their 2-D - 3-D matches form ONE list.  Any number
of pairs in ONE call with ONE host synchronisation, and every problem's result is a function of its own correspondences, its camera, the configuration and
the seed alone."""
from __future__ import annotations

from typing import Optional

import torch
from torch import nn

from . import _cabi, _call
from ._readers import as_cameras


class _Store1:
    """what the estimator reads of the database side: the shape of points3d1 and num_keypoints"""
    __slots__ = ("K", "N", "num")


def _database_side(points3d1, feats1: Optional[dict], device, fallback: Optional[dict] = None):
    pts = torch.as_tensor(points3d1)
    if pts.dim() != 3 or pts.shape[-1] != 3:
        raise ValueError(f"points3d1 must have shape [K1, N1, 3], got {tuple(pts.shape)}")
    if pts.dtype is not torch.float32 or pts.device != device or not pts.is_contiguous():
        pts = pts.detach().to(device=device, dtype=torch.float32).contiguous()
    s = _Store1()
    s.K, s.N, s.num = int(pts.shape[0]), int(pts.shape[1]), None
    src = feats1 if feats1 is not None else fallback
    num = None if src is None else src.get("num_keypoints")
    if feats1 is None and num is not None and tuple(torch.as_tensor(num).shape) != (s.K,):
        num = None                                         # the query store's counts say nothing about another store
    if num is not None:
        num = torch.as_tensor(num).detach().to(device=device, dtype=torch.int32).contiguous()
        assert tuple(num.shape) == (s.K,), f"feats1: num_keypoints must have shape [{s.K}]"
        s.num = num.clamp(0, s.N)
    return pts, s


def group_by_query(image0) -> tuple:
    """The pooling of a pair list by its image-0 index, on the host: (group_offsets [G + 1], group_pairs [P], queries [G] ascending, group_of_pair [P]).
    A stable sort: inside a problem the pairs keep the order of the list."""
    q = torch.as_tensor(image0).detach().cpu().to(torch.int64).reshape(-1)
    order = torch.sort(q, stable=True)[1]
    queries, inverse, counts = torch.unique(q, sorted=True, return_inverse=True, return_counts=True)
    offsets = torch.zeros(len(queries) + 1, dtype=torch.int64)
    offsets[1:] = torch.cumsum(counts, 0)
    return offsets.to(torch.int32), order.to(torch.int32), queries, inverse


class AbsolutePoseEstimator(nn.Module):
    """threshold: the inlier reprojection error in pixels.  num_hypotheses: the fixed budget of 3-point samples, a multiple of 256 in [256, 65536].  refine: five
    Gauss-Newton steps on the winner's inliers, kept if the inlier count does not drop.  seed: the only source of randomness."""
    required_data_keys = ("image0",)

    def __init__(self, threshold: float = 3.0, num_hypotheses: int = 1024, refine: bool = True, seed: int = 0):
        super().__init__()
        self.threshold, self.num_hypotheses, self.seed = _call.ransac_settings(threshold, num_hypotheses, seed)
        self.refine = bool(refine)

    # ------------------------------------------------------------------ the call path
    def _launch(self, device, s0, s1, pts, P: int, index, image0, result, cameras0, pool: bool, poses=None, return_candidates: bool = False) -> dict:
        """P pairs in ONE lg_abspose_estimate call on the current stream, then the dict behind the one host synchronisation of the call.  image0 [P]: the
        image-0 index of every pair (host or device), read on the host only to pool."""
        m0 = _call.as_matches0(result, P, s0.N, device)
        cam0 = as_cameras(cameras0, s0.K, device, "cameras0")
        H = self.num_hypotheses
        flags = (_cabi.LG_ABSPOSE_REFINE if self.refine else 0) | (0 if index is None else _cabi.LG_FLAG_INDEXED)
        G, groups, queries, group_of_pair = P, None, torch.as_tensor(image0).to(torch.int64), torch.arange(P)
        if pool and P:
            offsets, order, queries, group_of_pair = group_by_query(image0)
            G = len(queries)
            groups = torch.cat([offsets, order]).to(device)                  # ONE upload: group_offsets [G + 1] | group_pairs [P]
            flags |= _cabi.LG_ABSPOSE_GROUPED
        if poses is not None:
            poses = torch.as_tensor(poses)
            assert poses.dim() == 4 and poses.shape[0] == G and tuple(poses.shape[2:]) == (3, 4), f"poses must have shape [{G}, H, 3, 4] (R | t), got {tuple(poses.shape)}"
            H = int(poses.shape[1])
            poses = poses.detach().to(device=device, dtype=torch.float32).contiguous()
            flags |= _cabi.LG_ABSPOSE_GIVEN_POSES
        inl = torch.empty((P, s0.N), device=device, dtype=torch.uint8)
        verified = torch.empty((P, s0.N), device=device, dtype=torch.int64)
        ints = torch.empty((2 * G + 2 * P,), device=device, dtype=torch.int32)   # num_inliers [G] | best_hypothesis [G] | pair_num_inliers [P] | status [P]
        R, t = torch.empty((G, 3, 3), device=device, dtype=torch.float32), torch.empty((G, 3), device=device, dtype=torch.float32)
        cand = torch.empty((G, H, _cabi.LG_ABSPOSE_ROOTS, 3, 4), device=device, dtype=torch.float32) if return_candidates else None
        p, (index0, index1), at = _call._ptr, _call.index_ptrs(index), lambda k: ints.data_ptr() + 4 * k
        io = lambda ws, nbytes: _cabi.LgAbsposeIO(
            pairs=P, n0=s0.N, n1=s1.N, images0=s0.K, images1=s1.K, groups=G, flags=flags, threshold=self.threshold, num_hypotheses=H, seed=self.seed,
            kpts0=p(s0.kpts), points3d1=p(pts), num0=p(s0.num), num1=p(s1.num), index0=index0, index1=index1, matches0=p(m0), cameras0=p(cam0),
            group_offsets=None if groups is None else groups.data_ptr(), group_pairs=None if groups is None else groups.data_ptr() + 4 * (G + 1),
            poses_in=p(poses), workspace=ws, workspace_bytes=nbytes,
            rotations=p(R), translations=p(t), num_inliers=at(0), best_hypothesis=at(G), candidates=p(cand),
            inliers0=p(inl), pair_num_inliers=at(2 * G), matches0_out=p(verified), status=at(2 * G + P))
        _call.device_call(device, "lg_abspose_estimate", "lg_abspose_workspace_bytes", (P, s0.N, H, flags), io, skip=not P)
        host = ints.tolist()                  # THE host sync of the call: the ragged lists need their sizes
        mask = inl.bool()
        matches = _call.ragged_matches(mask, verified, host[2 * G:2 * G + P])
        out = {"R": R, "t": t, "num_inliers": ints[:G].long(), "best_hypothesis": ints[G:2 * G].long(), "queries": queries, "group_of_pair": group_of_pair,
               "inliers0": mask, "pair_num_inliers": ints[2 * G:2 * G + P].long(), "matches0": verified, "matches": matches}
        if return_candidates:
            out["candidates"] = cand
        return _call.raise_with_outputs(host[2 * G + P:], out)

    @torch.no_grad()
    def forward(self, data: dict, result, cameras0, points3d1) -> dict:
        """{"image0": feats}, feats = {keypoints [B, N0, 2], num_keypoints [B] (optional)} (an "image1" entry gives the database side's num_keypoints), the
        matcher's result for these B pairs (its dict, a `DeferredMatches` or matches0 [B, N0] itself), the cameras of the B query images ([B, 4]
        (fx, fy, cx, cy) or [B, 3, 3]) and the world points of the B database images' keypoint rows [B, N1, 3] (a row with a non-finite coordinate has none).
        B problems.  Returns R [B, 3, 3] and t [B, 3] (X_cam = R X_world + t), num_inliers [B], best_hypothesis [B] (-1: no pose), inliers0 [B, N0] bool,
        pair_num_inliers [B], matches0 [B, N0] (the inlier matches, -1 elsewhere), matches List[[S_i, 2]], queries, group_of_pair."""
        assert "image0" in data, "Missing key image0 in data"
        feats0 = data["image0"]
        device = feats0["keypoints"].device
        _call.require_gpu(device, "keypoints")
        s0 = _call.build_side(feats0, device, "image0")
        pts, s1 = _database_side(points3d1, data.get("image1"), device)
        assert s1.K == s0.K, f"image0 and points3d1 must hold the same number of images, got {s0.K} and {s1.K}"
        return self._launch(device, s0, s1, pts, s0.K, None, torch.arange(s0.K), result, cameras0, False)

    def _open(self, feats0: dict, pairs, points3d1, feats1, validate: bool):
        device = feats0["keypoints"].device
        _call.require_gpu(device, "keypoints")
        s0 = _call.build_side(feats0, device, "feats0")
        pts, s1 = _database_side(points3d1, feats1, device, feats0)
        pt = _call.pair_list(pairs, s0.K, s1.K, validate)
        return device, s0, s1, pts, int(pt.shape[0]), _call.device_index(pt, device), pt[:, 0]

    @torch.no_grad()
    def estimate_pairs(self, feats0: dict, pairs, result, cameras0, points3d1, feats1: Optional[dict] = None, *, pool: bool = False, validate: bool = True,
                       return_candidates: bool = False) -> dict:
        """The pair list of `match_pairs` posed: pair p = (i, j) reads the keypoints and the camera of query image i of the store `feats0` / `cameras0`, the
        world points points3d1[j] ([K1, N1, 3]) of database image j and row p of `result`'s matches0; of `feats1` (None: `feats0`, where it has K1 images)
        only num_keypoints is read.  pool=False: one problem per pair.  pool=True: the pairs with the same image-0 index form ONE problem (group_offsets /
        group_pairs are built on the host by a stable sort and uploaded once).  Returns per problem R [G, 3, 3], t [G, 3], num_inliers [G], best_hypothesis
        [G] and queries [G] (the image-0 index of each problem, ascending when pooled; pairs[:, 0] otherwise), group_of_pair [P], and per pair in input order
        inliers0, pair_num_inliers, matches0, matches.  ONE host synchronisation, no chunking.  `validate` as in `match_pairs`.  return_candidates: also
        `candidates` [G, num_hypotheses, 4, 3, 4], every root's (R | t) in the world frame."""
        device, s0, s1, pts, P, index, image0 = self._open(feats0, pairs, points3d1, feats1, validate)
        return self._launch(device, s0, s1, pts, P, index, image0, result, cameras0, pool, return_candidates=return_candidates)

    @torch.no_grad()
    def score_poses(self, feats0: dict, pairs, result, cameras0, points3d1, poses, feats1: Optional[dict] = None, *, pool: bool = False, validate: bool = True) -> dict:
        """Scoring against given poses (LG_ABSPOSE_GIVEN_POSES): no sampling, no solving — hypothesis h of problem g is poses[g, h] ([G, H, 3, 4] (R | t) in
        the world frame, H a multiple of 256) as it stands, and the winner is the one with the most inliers, the lowest h on a tie."""
        device, s0, s1, pts, P, index, image0 = self._open(feats0, pairs, points3d1, feats1, validate)
        return self._launch(device, s0, s1, pts, P, index, image0, result, cameras0, pool, poses=poses)
