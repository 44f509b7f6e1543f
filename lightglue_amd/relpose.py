"""Relative pose of calibrated pairs on the device: 5-point essential-matrix RANSAC with a fixed hypothesis budget, then (R, t) by cheirality, on the kernels of
`csrc/lg_relpose.hip` behind `lg_relpose_estimate` (include/lightglue_amd.h holds the definition).  It reads what a matcher leaves on the device — the keypoint
stores, the pair list and `matches0` — in place, plus one pinhole camera (fx, fy, cx, cy) per image; any number of pairs in ONE call with ONE host
synchronisation, and every pair's result is a function of its own correspondences, its two cameras, the configuration and the seed alone."""
from __future__ import annotations

from typing import Optional

import torch
from torch import nn

from . import _cabi, _call
from ._readers import as_cameras


class RelativePoseEstimator(nn.Module):
    """threshold: the inlier Sampson distance in pixels.  num_hypotheses: the fixed budget of 5-point samples, a multiple of 256 in [256, 65536].  refine: one
    least-squares refit of E on the winner's inliers, projected onto the essential manifold, kept if the inlier count does not drop.  seed: the only source
    of randomness."""
    required_data_keys = ("image0", "image1")

    def __init__(self, threshold: float = 3.0, num_hypotheses: int = 1024, refine: bool = True, seed: int = 0):
        super().__init__()
        self.threshold, self.num_hypotheses, self.seed = _call.ransac_settings(threshold, num_hypotheses, seed)
        self.refine = bool(refine)

    # ------------------------------------------------------------------ the call path
    def _launch(self, device, s0, s1, P: int, index, result, cameras0, cameras1, return_candidates: bool = False) -> dict:
        """P pairs in ONE lg_relpose_estimate call on the current stream, then the dict behind the one host synchronisation of the call."""
        m0 = _call.as_matches0(result, P, s0.N, device)
        cam0 = as_cameras(cameras0, s0.K, device, "cameras0")
        cam1 = cam0 if cameras1 is None and s1.K == s0.K else as_cameras(cameras0 if cameras1 is None else cameras1, s1.K, device, "cameras1")
        H = self.num_hypotheses
        flags = (_cabi.LG_RELPOSE_REFINE if self.refine else 0) | (0 if index is None else _cabi.LG_FLAG_INDEXED)
        inl = torch.empty((P, s0.N), device=device, dtype=torch.uint8)
        verified = torch.empty((P, s0.N), device=device, dtype=torch.int64)
        ints = torch.empty((4, P), device=device, dtype=torch.int32)            # [0] = num_inliers, [1] = best_hypothesis, [2] = status, [3] = num_in_front
        R, t = torch.empty((P, 3, 3), device=device, dtype=torch.float32), torch.empty((P, 3), device=device, dtype=torch.float32)
        E, F = torch.empty((P, 3, 3), device=device, dtype=torch.float32), torch.empty((P, 3, 3), device=device, dtype=torch.float32)
        cand = torch.empty((P, H, _cabi.LG_RELPOSE_ROOTS, 3, 3), device=device, dtype=torch.float32) if return_candidates else None
        p, (index0, index1) = _call._ptr, _call.index_ptrs(index)
        io = lambda ws, nbytes: _cabi.LgRelPoseIO(
            pairs=P, n0=s0.N, n1=s1.N, images0=s0.K, images1=s1.K, flags=flags, threshold=self.threshold, num_hypotheses=H, seed=self.seed,
            kpts0=p(s0.kpts), kpts1=p(s1.kpts), num0=p(s0.num), num1=p(s1.num), index0=index0, index1=index1,
            matches0=p(m0), cameras0=p(cam0), cameras1=p(cam1), workspace=ws, workspace_bytes=nbytes,
            rotations=p(R), translations=p(t), essentials=p(E), models=p(F), candidates=p(cand),
            inliers0=p(inl), num_inliers=ints[0].data_ptr(), matches0_out=p(verified),
            best_hypothesis=ints[1].data_ptr(), num_in_front=ints[3].data_ptr(), status=ints[2].data_ptr())
        _call.device_call(device, "lg_relpose_estimate", "lg_relpose_workspace_bytes", (P, s0.N, H, flags), io, skip=not P)
        host = ints.tolist()                  # THE host sync of the call: the ragged lists need their sizes
        mask = inl.bool()
        matches = _call.ragged_matches(mask, verified, host[0])
        out = {"R": R, "t": t, "E": E, "models": F, "inliers0": mask, "num_inliers": ints[0].long(), "num_in_front": ints[3].long(), "matches0": verified,
               "matches": matches, "best_hypothesis": ints[1].long()}
        if return_candidates:
            out["candidates"] = cand
        return _call.raise_with_outputs(host[2], out)

    @torch.no_grad()
    def forward(self, data: dict, result, cameras0, cameras1) -> dict:
        """{"image0": feats, "image1": feats}, feats = {keypoints [B, N, 2], num_keypoints [B] (optional)}, the matcher's result for these B pairs (its dict, a
        `DeferredMatches` or matches0 [B, N0] itself) and the cameras of the B images of either side ([B, 4] (fx, fy, cx, cy) or [B, 3, 3]).  Returns R [B, 3, 3]
        and t [B, 3] (X1 = R X0 + t, |t| = 1), E [B, 3, 3], models [B, 3, 3] (the pixel-space F), inliers0 [B, N0] bool, num_inliers [B], num_in_front [B],
        matches0 [B, N0] (the inlier matches, -1 elsewhere), matches List[[S_i, 2]], best_hypothesis [B] (-1: no model)."""
        device, s0, s1 = _call.batch_sides(data, self.required_data_keys, _call.build_side)        # keypoints [B, N, 2] and num_keypoints: nothing else is read
        return self._launch(device, s0, s1, s0.K, None, result, cameras0, cameras1)

    @torch.no_grad()
    def estimate_pairs(self, feats0: dict, pairs, result, cameras0, feats1: Optional[dict] = None, cameras1=None, *, validate: bool = True,
                       return_candidates: bool = False) -> dict:
        """The pair list of `match_pairs` posed: pair p = (i, j) reads the keypoints and the camera of image i of the store `feats0` / `cameras0` and of image j
        of `feats1` / `cameras1` (None: of `feats0` / `cameras0` too) in place through the index, and row p of `result`'s matches0.  Outputs allocated once for
        all P pairs, ONE host synchronisation, no chunking.  `validate` as in `match_pairs`: without it an index outside its store gives LG_ERR_INDEX for that
        pair (raised after the call).  return_candidates: also `candidates` [P, num_hypotheses, 10, 3, 3], the pixel-space F of every root of every sample."""
        same, P, index = _call.store_pairs(feats0, pairs, feats1, validate)
        device, s0, s1 = _call.sides(feats0, feats0 if same else feats1, ("feats0", "feats1"), _call.build_side)
        return self._launch(device, s0, s1, P, index, result, cameras0, cameras1, return_candidates)
