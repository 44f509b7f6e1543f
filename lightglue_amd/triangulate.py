"""Tracks and multi-view triangulation with known poses on the device, on the kernels of `csrc/lg_triangulate.hip` behind `lg_triangulate`
(include/lightglue_amd.h holds the definition).  It reads what a matcher or a verifier leaves on the device — ONE keypoint store, the pair list over it and
`matches0` — in place, plus one pinhole camera (fx, fy, cx, cy) and one pose (R | t), X_cam = R X_world + t, per image.  Tracks are the connected components of
the match graph; each is triangulated from all its views.  `points3d [K, N, 3]` (NaN where a row has no point) is what `AbsolutePoseEstimator` takes as
points3d1.  Any number of pairs in ONE call with ONE host synchronisation; every output is a function of the edge set alone, not of the list's order.
`robust=True` (`lg_triangulate_robust`): a consensus over every component's views and up to `max_tracks` tracks out of one component, so that a wrong match
costs an outlier node and not the track."""
from __future__ import annotations

import torch
from torch import nn

from . import _cabi, _call
from ._readers import as_cameras, as_poses

STATES = ("none", "triangulated", "conflict", "too_long", "degenerate", "behind", "reprojection", "angle")    # node_state 0 .. 7
ROBUST_STATES = STATES + ("outlier",)                    # node_state 0 .. 8 of the robust mode: 8 is a node its component's tracks left over (2 does not occur)


class Triangulator(nn.Module):
    """max_reproj_error: the largest reprojection error, in pixels, an observation of an accepted track may have.  min_angle: the smallest angle, in degrees,
    the widest pair of rays of an accepted track must have.  max_track_length: a longer track is reported too long, in [2, 1024].  refine: five Gauss-Newton
    steps on the reprojection error from the linear start.  robust: per component a consensus over its views from `num_hypotheses` two-view hypotheses per
    round, and up to `max_tracks` tracks (rounds) out of one component (lg_triangulate_robust): a wrong match leaves an outlier node (state 8) behind, not a
    rejected track, and two tracks it merged come apart again.  A failed round 0 still rejects the component, and a node is not re-admitted after the fit."""

    def __init__(self, max_reproj_error: float = 4.0, min_angle: float = 1.5, max_track_length: int = 128, refine: bool = True, robust: bool = False,
                 num_hypotheses: int = 64, max_tracks: int = 2):
        super().__init__()
        self.num_hypotheses = _call.int_in("num_hypotheses", num_hypotheses, 1, _cabi.LG_TRI_MAX_HYPOTHESES)       # these integers take True as 1
        self.max_tracks, self.robust = _call.int_in("max_tracks", max_tracks, 1, _cabi.LG_TRI_MAX_TRACKS), bool(robust)
        self.max_reproj_error = _call.positive("max_reproj_error", max_reproj_error)
        if not 0.0 <= float(min_angle) < 180.0:
            raise ValueError(f"min_angle must lie in [0, 180), got {min_angle!r}")
        self.max_track_length = _call.int_in("max_track_length", max_track_length, 2, _cabi.LG_TRI_MAX_TRACK_LENGTH)
        self.min_angle, self.refine = float(min_angle), bool(refine)

    # ------------------------------------------------------------------ the call path
    def _launch(self, feats: dict, pairs, result, cameras, poses, validate: bool, tracks_only: bool) -> dict:
        """ONE lg_triangulate (robust: lg_triangulate_robust) call on the current stream, then the dict behind the one host synchronisation of the call"""
        device = feats["keypoints"].device
        _call.require_gpu(device, "keypoints")
        s = _call.build_side(feats, device, "feats")
        K, N = int(s.K), int(s.N)
        pt = _call.pair_list(pairs, K, K, validate)
        P, index = int(pt.shape[0]), _call.device_index(pt, device)
        m0 = _call.as_matches0(result, P, N, device)
        cam = pose = None
        if not tracks_only:
            cam, pose = as_cameras(cameras, K, device, "cameras"), as_poses(poses, K, device)
        flags = (_cabi.LG_TRI_REFINE if self.refine else 0) | (_cabi.LG_TRI_TRACKS_ONLY if tracks_only else 0)
        cap = K * N // 2                                                   # a track has at least two nodes
        pts = None if tracks_only else torch.empty((K, N, 3), device=device, dtype=torch.float32)
        track_id = torch.empty((K, N), device=device, dtype=torch.int64)
        state = torch.empty((K, N), device=device, dtype=torch.uint8)
        per_track = torch.empty((max(cap, 1), 5), device=device, dtype=torch.float32)      # xyz [cap, 3] | track_error [cap] | track_length [cap] (int32 bits)
        robust = self.robust                                                    # (never with tracks_only: build_tracks refuses)
        extra = 2 if robust else 0                                              # robust: | outlier nodes | components with more than one track, at the end
        ints = torch.zeros((9 + P + extra,), device=device, dtype=torch.int32)  # T | tracks per state [8] | status [P]
        p, (index0, index1), base = _call._ptr, _call.index_ptrs(index), per_track.data_ptr()

        def make_io(ws, nbytes):
            io = _cabi.LgTriangulateIO(
                pairs=P, n=N, images=K, flags=flags, max_reproj_error=self.max_reproj_error, min_angle=self.min_angle, max_track_length=self.max_track_length,
                kpts=p(s.kpts), num=p(s.num), index0=index0, index1=index1, matches0=p(m0), cameras=p(cam), poses=p(pose), workspace=ws, workspace_bytes=nbytes,
                points3d=p(pts), track_id=p(track_id), node_state=p(state), xyz=base, track_error=base + 12 * cap, track_length=base + 16 * cap,
                counts=ints.data_ptr(), status=None if not P else ints.data_ptr() + 36)
            if robust:
                io = _cabi.LgTriangulateRobustIO(base=io, num_hypotheses=self.num_hypotheses, max_tracks=self.max_tracks, outlier_counts=ints.data_ptr() + 4 * (9 + P))
            return io
        entry = ("lg_triangulate_robust", "lg_triangulate_robust_workspace_bytes", (K, N, self.max_tracks)) if robust else ("lg_triangulate", "lg_triangulate_workspace_bytes", (K, N, flags))
        _call.device_call(device, *entry, make_io)
        host = ints.tolist()                  # THE host sync of the call: the per-track outputs need their number
        T = host[0]
        flat = per_track.view(-1)
        out = {"track_id": track_id, "node_state": state, "num_tracks": T, "track_length": flat[4 * cap:4 * cap + T].view(torch.int32).long(),
               "state_counts": dict(zip(STATES, host[1:9])), "status": ints[9:9 + P]}
        if robust:
            out.update(num_outliers=host[9 + P], num_split=host[10 + P])
        if not tracks_only:
            out.update(points3d=pts, xyz=flat[:3 * T].view(T, 3), track_error=flat[3 * cap:3 * cap + T])
        return _call.raise_with_outputs(host[9:9 + P], out)

    @torch.no_grad()
    def triangulate(self, feats: dict, pairs, result, cameras, poses, *, validate: bool = True) -> dict:
        """feats = {keypoints [K, N, 2], num_keypoints [K] (optional)}: ONE store, indexed by both columns of `pairs` [P, 2] (host or device); `result`: either
        matcher's dict, a `DeferredMatches`, the dict of `TwoViewVerifier` / `RelativePoseEstimator` (its verified matches0) or matches0 [P, N] itself — only
        matches0 is read; cameras [K, 4] (fx, fy, cx, cy) or [K, 3, 3]; poses [K, 3, 4] (R | t) or (R [K, 3, 3], t [K, 3]), X_cam = R X_world + t.  Returns
        points3d [K, N, 3] float32 (the track's point at every row of a triangulated track, NaN elsewhere: what `AbsolutePoseEstimator` takes as points3d1),
        track_id [K, N] int64 (dense in [0, T) in ascending order of the track's lowest node, -1 elsewhere), node_state [K, N] uint8 (`STATES`), num_tracks = T,
        xyz [T, 3], track_length [T], track_error [T] (mean reprojection error in pixels), state_counts (tracks per state), status [P].  ONE host
        synchronisation.  `validate` as in `match_pairs`; a pair (a, a), an index outside the store or an image whose camera or pose fails the camera rule
        raises LightGlueAmdError after the call, with `err.outputs` holding the outputs of everything else.  With `robust` also num_outliers (the nodes of
        state 8, `ROBUST_STATES`) and num_split (the components that gave more than one track); state_counts then counts the tracks under "triangulated" and,
        under every other state, the components whose first round failed with it."""
        return self._launch(feats, pairs, result, cameras, poses, validate, False)

    forward = triangulate

    @torch.no_grad()
    def build_tracks(self, feats: dict, pairs, result, *, validate: bool = True) -> dict:
        """Tracks only (LG_TRI_TRACKS_ONLY): no cameras, no poses, no geometry.  node_state holds 0 .. 3 (1: a clean track), track_id numbers every clean
        track; returns track_id, node_state, num_tracks, track_length, state_counts, status.  There are no tracks without geometry in the robust mode."""
        if self.robust:
            raise ValueError("build_tracks has no robust mode: the consensus over a component's views needs cameras and poses (use triangulate)")
        return self._launch(feats, pairs, result, None, None, validate, True)
