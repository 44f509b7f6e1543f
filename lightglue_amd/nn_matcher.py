"""The weight-free matcher: (mutual) nearest neighbour with Lowe's ratio test and a distance threshold, on the kernels of `csrc/lg_nn.hip` behind
`lg_nn_match` (include/lightglue_amd.h holds the definition).  It is the baseline a LightGlue result is compared with, the matcher for descriptors no LightGlue
checkpoint covers (any dim that is a multiple of 16 up to 256) and the quickest check of a freshly written feature store.  Same feature stores, storage formats
(fp32 / float16 / uint8, `descriptor_transform="rootsift"`), pair lists and output dict as `LightGlue`, so `glue.match_pair`, `glue.match_batch` and
`glue.match_pairs` take it unchanged.  The similarity matrix is never materialised: the only scratch of a call is the normalised copy of the stores' rows."""
from __future__ import annotations

import functools
from typing import Optional

import torch
from torch import nn

from . import _cabi, _call


# one side of a call: descriptors [K, N, D] of any D, num_keypoints and descriptor_transform; nothing else is read.  Both sides: the same D
_READ = dict(build=functools.partial(_call.build_side, keypoints=False, descriptors="any"), key="descriptors")


def _same_dim(s0, s1):
    assert s0.desc.shape[2] == s1.desc.shape[2], f"descriptor dims differ: {s0.desc.shape[2]} and {s1.desc.shape[2]}"


class NearestNeighborMatcher(nn.Module):
    """mutual: keep (i, j) only if j is i's nearest neighbour AND i is j's.  ratio_threshold in (0, 1] or None: keep a row only if d1 <= ratio^2 * d2, d the squared
    distance 2 (1 - sim) to the nearest / second nearest neighbour.  distance_threshold > 0 or None: keep a row only if d1 <= distance^2."""
    required_data_keys = ("image0", "image1")

    def __init__(self, mutual: bool = True, ratio_threshold: Optional[float] = None, distance_threshold: Optional[float] = None):
        super().__init__()
        if ratio_threshold is not None and not 0.0 < float(ratio_threshold) <= 1.0:
            raise ValueError(f"ratio_threshold must lie in (0, 1] or be None, got {ratio_threshold!r}")
        if distance_threshold is not None and not float(distance_threshold) > 0.0:
            raise ValueError(f"distance_threshold must be > 0 or None, got {distance_threshold!r}")
        self.mutual = bool(mutual)
        self.ratio_threshold = None if ratio_threshold is None else float(ratio_threshold)
        self.distance_threshold = None if distance_threshold is None else float(distance_threshold)

    # ------------------------------------------------------------------ the call path
    def _launch(self, device, s0, s1, P: int, index, defer: bool):
        """P pairs in ONE lg_nn_match call on the current stream, then the dict behind the one host synchronisation of the call (or a `DeferredMatches`).
        `index`: int32 [2, P] image indices into the sides (LG_FLAG_INDEXED), None for pair p = (image p, image p)."""
        o = _call.Outputs(P, s0.N, s1.N, device, pruning=False)
        if not self.mutual and s0.N > s1.N:          # without the mutual check every row of image 0 may match: the list needs n0 rows, not min(n0, n1)
            o.mlist64 = torch.empty((P, s0.N, 2), device=device, dtype=torch.int64)
            o.mscore_list = torch.empty((P, s0.N), device=device, dtype=torch.float32)
        dim, p, (index0, index1) = int(s0.desc.shape[2]), _call._ptr, _call.index_ptrs(index)
        flags = ((0 if index is None else _cabi.LG_FLAG_INDEXED) | (_cabi.LG_FLAG_NN_MUTUAL if self.mutual else 0) | s0.flags(0) | s1.flags(1))
        io = lambda ws, nbytes: _cabi.LgNnIO(
            pairs=P, n0=s0.N, n1=s1.N, dim=dim, flags=flags,
            ratio_threshold=self.ratio_threshold or 0.0, distance_threshold=self.distance_threshold or 0.0,
            desc0=p(s0.desc), desc1=p(s1.desc), num0=p(s0.num), num1=p(s1.num), index0=index0, index1=index1, images0=s0.K, images1=s1.K,
            workspace=ws, workspace_bytes=nbytes,
            raw0=p(o.m0), raw1=p(o.m1), matches0=p(o.m0_64), matches1=p(o.m1_64), scores0=p(o.ms0), scores1=p(o.ms1),
            matches=p(o.mlist64), match_scores=p(o.mscore_list), list_rows=int(o.mscore_list.shape[1]),
            n_matches=o.stop_nm[1].data_ptr(), status=o.stop_nm[2].data_ptr(), stop=o.stop_nm[0].data_ptr(), stop_i64=p(o.stop64),
            prune0=p(o.prune0), prune1=p(o.prune1))
        with torch.cuda.device(device):       # the scratch is the normalised rows of the stores, independent of P: no floor under its size
            stream = _call.device_call(device, "lg_nn_match", "lg_nn_workspace_bytes", (s0.K, s1.K, s0.N, s1.N, dim, flags), io, skip=not P, floor=0)
            return o.finish(stream, defer)

    @torch.no_grad()
    def forward(self, data: dict) -> dict:
        """{"image0": feats, "image1": feats}, feats = {descriptors [B, N, D] (fp32, or float16 / uint8 read in place), num_keypoints [B] (optional),
        descriptor_transform None | "rootsift" (optional)}; `keypoints` may be absent.  Returns the dict of `LightGlue.forward`: matches0 [B, M] int64,
        matching_scores0 [B, M], matches1 / matching_scores1 [B, N], matches List[[S_i, 2]], scores List[[S_i]], stop (0), prune0 / prune1 (zeros)."""
        device, s0, s1 = _call.batch_sides(data, self.required_data_keys, check=_same_dim, **_READ)
        return self._launch(device, s0, s1, s0.K, None, False)

    @torch.no_grad()
    def match_pairs(self, feats0: dict, pairs, feats1: Optional[dict] = None, *, deferred: bool = False, validate: bool = True):
        """`LightGlue.match_pairs` for this matcher, same contract: pair p = (i, j) matches image i of the store `feats0` against image j of `feats1` (None: of
        `feats0` too), read in place through the index; outputs allocated once for all P pairs; ONE host synchronisation, none with `deferred=True`
        (a `DeferredMatches`); `validate` as there.  Bit-identical to `forward` on the stacked tensors {k: v[index]}.  No chunking: any P is one call."""
        same, P, index = _call.store_pairs(feats0, pairs, feats1, validate, "descriptors")
        device, s0, s1 = _call.sides(feats0, feats0 if same else feats1, ("feats0", "feats1"), check=_same_dim, **_READ)
        return self._launch(device, s0, s1, P, index, deferred)
