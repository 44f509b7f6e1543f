"""The weight-free matcher: (mutual) nearest neighbour with Lowe's ratio test and a distance threshold, on the kernels of `csrc/lg_nn.hip` behind
`lg_nn_match` (include/lightglue_amd.h holds the definition).  It is the baseline a LightGlue result is compared with, the matcher for descriptors no LightGlue
checkpoint covers (any dim that is a multiple of 16 up to 256) and the quickest check of a freshly written feature store.  Same feature stores, storage formats
(fp32 / float16 / uint8, `descriptor_transform="rootsift"`), pair lists and output dict as `LightGlue`, so `glue.match_pair`, `glue.match_batch` and
`glue.match_pairs` take it unchanged.  The similarity matrix is never materialised: the only scratch of a call is the normalised copy of the stores' rows."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch
from torch import nn

from . import _cabi, _call


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

    # ------------------------------------------------------------------ one side of a call
    @staticmethod
    def _side(feats: dict, device, what: str) -> _call.Side:
        """{descriptors [K, N, D], num_keypoints [K] (optional), descriptor_transform (optional)} -> the `_call.Side` of it; nothing else is read."""
        desc = feats["descriptors"]
        assert desc.dim() == 3, f"{what}: descriptors must have shape [K, N, D], got {tuple(desc.shape)}"
        s = _call.Side()
        s.K, s.N = int(desc.shape[0]), int(desc.shape[1])
        s.desc = _call._engine_descriptors(desc, device)
        s.rootsift = _call.descriptor_transform(feats, what) == "rootsift"
        s.kpts = s.size = s.scales = s.oris = s.num = None
        num = feats.get("num_keypoints")
        if num is not None:
            num = torch.as_tensor(num).detach().to(device=device, dtype=torch.int32).contiguous()
            assert num.shape == (s.K,), f"{what}: num_keypoints must have shape [{s.K}]"
            s.num = num.clamp(0, s.N)
        return s

    def _sides(self, feats0: dict, feats1: dict, names=("feats0", "feats1")):
        device = feats0["descriptors"].device
        _call.require_gpu(device, "descriptors")
        s0 = self._side(feats0, device, names[0])
        s1 = s0 if feats1 is feats0 else self._side(feats1, device, names[1])
        assert s0.desc.shape[2] == s1.desc.shape[2], f"descriptor dims differ: {s0.desc.shape[2]} and {s1.desc.shape[2]}"
        return device, s0, s1

    # ------------------------------------------------------------------ the call path
    def _launch(self, device, s0, s1, P: int, index, defer: bool):
        """P pairs in ONE lg_nn_match call on the current stream, then the dict behind the one host synchronisation of the call (or a `DeferredMatches`).
        `index`: int32 [2, P] image indices into the sides (LG_FLAG_INDEXED), None for pair p = (image p, image p)."""
        o = _call.Outputs(P, s0.N, s1.N, device, pruning=False)
        if not self.mutual and s0.N > s1.N:          # without the mutual check every row of image 0 may match: the list needs n0 rows, not min(n0, n1)
            o.mlist64 = torch.empty((P, s0.N, 2), device=device, dtype=torch.int64)
            o.mscore_list = torch.empty((P, s0.N), device=device, dtype=torch.float32)
        with torch.cuda.device(device):
            stream = torch.cuda.current_stream(device)
            if P:
                lib = _cabi.load()
                dim = int(s0.desc.shape[2])
                flags = ((0 if index is None else _cabi.LG_FLAG_INDEXED) | (_cabi.LG_FLAG_NN_MUTUAL if self.mutual else 0) | s0.flags(0) | s1.flags(1))
                nbytes = lib.lg_nn_workspace_bytes(s0.K, s1.K, s0.N, s1.N, dim, flags)      # -1: outside the envelope — lg_nn_match below says why
                ws = torch.empty((max(nbytes, 0),), device=device, dtype=torch.uint8)       # the normalised rows of the stores: independent of P
                p = _call._ptr
                io = _cabi.LgNnIO(
                    pairs=P, n0=s0.N, n1=s1.N, dim=dim, flags=flags,
                    ratio_threshold=self.ratio_threshold or 0.0, distance_threshold=self.distance_threshold or 0.0,
                    desc0=p(s0.desc), desc1=p(s1.desc), num0=p(s0.num), num1=p(s1.num),
                    index0=None if index is None else index[0].data_ptr(), index1=None if index is None else index[1].data_ptr(), images0=s0.K, images1=s1.K,
                    workspace=p(ws), workspace_bytes=max(nbytes, 0),
                    raw0=p(o.m0), raw1=p(o.m1), matches0=p(o.m0_64), matches1=p(o.m1_64), scores0=p(o.ms0), scores1=p(o.ms1),
                    matches=p(o.mlist64), match_scores=p(o.mscore_list), list_rows=int(o.mscore_list.shape[1]),
                    n_matches=o.stop_nm[1].data_ptr(), status=o.stop_nm[2].data_ptr(), stop=o.stop_nm[0].data_ptr(), stop_i64=p(o.stop64),
                    prune0=p(o.prune0), prune1=p(o.prune1))
                _cabi.check(lib.lg_nn_match(C.byref(io), C.c_void_p(stream.cuda_stream)))
            return o.finish(stream, defer)

    @torch.no_grad()
    def forward(self, data: dict) -> dict:
        """{"image0": feats, "image1": feats}, feats = {descriptors [B, N, D] (fp32, or float16 / uint8 read in place), num_keypoints [B] (optional),
        descriptor_transform None | "rootsift" (optional)}; `keypoints` may be absent.  Returns the dict of `LightGlue.forward`: matches0 [B, M] int64,
        matching_scores0 [B, M], matches1 / matching_scores1 [B, N], matches List[[S_i, 2]], scores List[[S_i]], stop (0), prune0 / prune1 (zeros)."""
        for key in self.required_data_keys:
            assert key in data, f"Missing key {key} in data"
        device, s0, s1 = self._sides(data["image0"], data["image1"], self.required_data_keys)
        assert s0.K == s1.K, f"image0 and image1 must hold the same number of images, got {s0.K} and {s1.K}"
        return self._launch(device, s0, s1, s0.K, None, False)

    @torch.no_grad()
    def match_pairs(self, feats0: dict, pairs, feats1: Optional[dict] = None, *, deferred: bool = False, validate: bool = True):
        """`LightGlue.match_pairs` for this matcher, same contract: pair p = (i, j) matches image i of the store `feats0` against image j of `feats1` (None: of
        `feats0` too), read in place through the index; outputs allocated once for all P pairs; ONE host synchronisation, none with `deferred=True`
        (a `DeferredMatches`); `validate` as there.  Bit-identical to `forward` on the stacked tensors {k: v[index]}.  No chunking: any P is one call."""
        same = feats1 is None or feats1 is feats0
        K0 = int(feats0["descriptors"].shape[0])
        K1 = K0 if same else int(feats1["descriptors"].shape[0])
        pt = _call.pair_list(pairs, K0, K1, validate)
        P = int(pt.shape[0])
        device, s0, s1 = self._sides(feats0, feats0 if same else feats1)
        index = pt.to(device=device, dtype=torch.int32).t().contiguous() if P else None     # [2, P]: index0 | index1
        return self._launch(device, s0, s1, P, index, deferred)
