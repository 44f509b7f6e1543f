"""Two-view geometric verification of match lists on the device: RANSAC with a fixed hypothesis budget for a homography or a fundamental matrix per pair, on the
kernels of `csrc/lg_twoview.hip` behind `lg_twoview_verify` (include/lightglue_amd.h holds the definition).  It reads what a matcher leaves on the device — the
keypoint stores, the pair list and `matches0` — in place, runs any number of pairs in ONE call with ONE host synchronisation, and every pair's result is a
function of its own correspondences, the configuration and the seed alone: the same bits wherever the pair stands in a list."""
from __future__ import annotations

from typing import Optional

import torch
from torch import nn

from . import _cabi, _call

MODELS = {"homography": _cabi.LG_TWOVIEW_HOMOGRAPHY, "fundamental": _cabi.LG_TWOVIEW_FUNDAMENTAL}


class TwoViewVerifier(nn.Module):
    """model: "homography" (x1 ~ H x0, 4-point samples) or "fundamental" (x1^T F x0 = 0, 7-point samples).  threshold: the inlier distance in keypoint units
    (reprojection error for H, Sampson distance for F).  num_hypotheses: the fixed budget, a multiple of 256 in [256, 65536].  refine: one least-squares refit
    on the winner's inliers, kept if the inlier count does not drop.  seed: the only source of randomness."""
    required_data_keys = ("image0", "image1")

    def __init__(self, model: str = "fundamental", threshold: float = 3.0, num_hypotheses: int = 1024, refine: bool = True, seed: int = 0):
        super().__init__()
        if model not in MODELS:
            raise ValueError(f"model must be one of {sorted(MODELS)}, got {model!r}")
        self.model, self.refine = model, bool(refine)
        self.threshold, self.num_hypotheses, self.seed = _call.ransac_settings(threshold, num_hypotheses, seed)

    # ------------------------------------------------------------------ the call path
    def _launch(self, device, s0, s1, P: int, index, result, models=None) -> dict:
        """P pairs in ONE lg_twoview_verify call on the current stream, then the dict behind the one host synchronisation of the call."""
        m0 = _call.as_matches0(result, P, s0.N, device)
        H = self.num_hypotheses
        flags = MODELS[self.model] | (_cabi.LG_TWOVIEW_REFINE if self.refine else 0) | (0 if index is None else _cabi.LG_FLAG_INDEXED)
        if models is not None:
            assert models.dim() == 4 and models.shape[0] == P and tuple(models.shape[2:]) == (3, 3), f"models must have shape [{P}, H, 3, 3], got {tuple(models.shape)}"
            H = int(models.shape[1])
            models = models.detach().to(device=device, dtype=torch.float32).contiguous()
            flags |= _cabi.LG_TWOVIEW_GIVEN_MODELS
        out_models = torch.empty((P, 3, 3), device=device, dtype=torch.float32)
        inl = torch.empty((P, s0.N), device=device, dtype=torch.uint8)
        verified = torch.empty((P, s0.N), device=device, dtype=torch.int64)
        ints = torch.empty((3, P), device=device, dtype=torch.int32)          # [0] = num_inliers, [1] = best_hypothesis, [2] = status
        p, (index0, index1) = _call._ptr, _call.index_ptrs(index)
        io = lambda ws, nbytes: _cabi.LgTwoViewIO(
            pairs=P, n0=s0.N, n1=s1.N, images0=s0.K, images1=s1.K, flags=flags, threshold=self.threshold, num_hypotheses=H, seed=self.seed,
            kpts0=p(s0.kpts), kpts1=p(s1.kpts), num0=p(s0.num), num1=p(s1.num), index0=index0, index1=index1,
            matches0=p(m0), models_in=p(models), workspace=ws, workspace_bytes=nbytes,
            models=p(out_models), inliers0=p(inl), num_inliers=ints[0].data_ptr(), matches0_out=p(verified),
            best_hypothesis=ints[1].data_ptr(), status=ints[2].data_ptr())
        _call.device_call(device, "lg_twoview_verify", "lg_twoview_workspace_bytes", (P, s0.N, flags), io, skip=not P)
        host = ints.tolist()                  # THE host sync of the call: the ragged lists need their sizes
        mask = inl.bool()
        matches = _call.ragged_matches(mask, verified, host[0])
        out = {"models": out_models, "inliers0": mask, "num_inliers": ints[0].long(), "matches0": verified, "matches": matches, "best_hypothesis": ints[1].long()}
        return _call.raise_with_outputs(host[2], out)

    @torch.no_grad()
    def forward(self, data: dict, result) -> dict:
        """{"image0": feats, "image1": feats}, feats = {keypoints [B, N, 2], num_keypoints [B] (optional)}, and the matcher's result for these B pairs (its dict,
        a `DeferredMatches` or matches0 [B, N0] itself).  Returns models [B, 3, 3], inliers0 [B, N0] bool, num_inliers [B], matches0 [B, N0] (the verified
        matches, -1 elsewhere), matches List[[S_i, 2]], best_hypothesis [B] (-1: no model)."""
        device, s0, s1 = _call.batch_sides(data, self.required_data_keys, _call.build_side)        # keypoints [B, N, 2] and num_keypoints: nothing else is read
        return self._launch(device, s0, s1, s0.K, None, result)

    @torch.no_grad()
    def verify_pairs(self, feats0: dict, pairs, result, feats1: Optional[dict] = None, *, validate: bool = True) -> dict:
        """The pair list of `match_pairs` verified: pair p = (i, j) reads the keypoints of image i of the store `feats0` and image j of `feats1` (None: of
        `feats0` too) in place through the index, and row p of `result`'s matches0.  Outputs allocated once for all P pairs, ONE host synchronisation, no
        chunking.  `validate` as in `match_pairs`: without it an index outside its store gives LG_ERR_INDEX for that pair (raised after the call)."""
        same, P, index = _call.store_pairs(feats0, pairs, feats1, validate)
        device, s0, s1 = _call.sides(feats0, feats0 if same else feats1, ("feats0", "feats1"), _call.build_side)
        return self._launch(device, s0, s1, P, index, result)

    @torch.no_grad()
    def score_models(self, feats0: dict, pairs, result, models: torch.Tensor, feats1: Optional[dict] = None, *, validate: bool = True) -> dict:
        """Verification against given geometry (LG_TWOVIEW_GIVEN_MODELS): no sampling, no solving — hypothesis h of pair p is models[p, h] ([P, H, 3, 3], H a
        multiple of 256) as it stands, and the winner is the one with the most inliers, the lowest h on a tie."""
        same, P, index = _call.store_pairs(feats0, pairs, feats1, validate)
        device, s0, s1 = _call.sides(feats0, feats0 if same else feats1, ("feats0", "feats1"), _call.build_side)
        return self._launch(device, s0, s1, P, index, result, models=models)
