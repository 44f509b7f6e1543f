"""Camera centres and track points from tracks on the device, on the kernels of `csrc/lg_positioning.hip` behind `lg_positioning_solve`
(include/lightglue_amd.h holds the definition).  It keeps the rotations it is given — `GlobalPoseEstimator`'s, say — and solves the centres of all free
images and the points of all tracks jointly from the viewing rays of every observation, with at least two images held to fix origin, orientation and scale:
reweighted linear least squares, Schur complement onto the centres, dense Cholesky, fp64.  It reads the keypoint store and the labels of
`Triangulator.build_tracks` in place; `(track_id, xyz)` of its dict is what `BundleAdjuster.adjust` takes, `points3d` what `AbsolutePoseEstimator` takes.
ONE call with ONE host synchronisation."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch
from torch import nn

from . import _cabi, _call
from .bundle import as_constant, as_track_id
from .relpose import as_cameras
from .triangulate import as_poses

# node_state 0 .. 9, image_state 0 .. 5
STATES = ("none", "inlier", "bad_image", "too_long", "peeled", "not_connected", "degenerate", "outlier", "no_point", "no_solution")
IMAGE_STATES = ("posed", "held", "too_few_tracks", "not_connected", "bad_image", "no_solution")
NO_GAUGE = "constant_pose must hold at least two images with finite poses and distinct centres: they fix origin, orientation and scale"


def as_labels(tracks, K: int, N: int, device):
    """(track_id [K, N] int64 on `device`, T) from the dict of `Triangulator.build_tracks` / `triangulate` (track_id, num_tracks) or a tuple (track_id, T)"""
    if isinstance(tracks, dict):
        for k in ("track_id", "num_tracks"):
            if k not in tracks:
                raise ValueError(f"tracks is a dict without {k!r}: pass the Triangulator's dict or a tuple (track_id [K, N], T)")
        tracks = (tracks["track_id"], tracks["num_tracks"])
    if not isinstance(tracks, (tuple, list)) or len(tracks) != 2:
        raise ValueError("tracks must be the Triangulator's dict or a tuple (track_id [K, N], T)")
    tid, T = as_track_id(tracks[0], K, N, device), tracks[1]
    if isinstance(T, bool) or torch.is_tensor(T) or int(T) != T or not 0 <= int(T) <= K * N // 2:
        raise ValueError(f"the number of tracks must be an integer in [0, K N / 2 = {K * N // 2}] (a track has at least two observations), got {T!r}")
    return tid, int(T)


class GlobalPositioner(nn.Module):
    """num_iterations: the fixed budget of reweighted solves, in [6, 100].  angle_scale: the robust scale (degrees between an observation's ray and the
    direction to its point) the reweighting ends at (it starts wide and halves down to it).  max_angle_error: an observation further than this (degrees) from
    its point at the final state is an outlier; no solve follows the classification."""

    def __init__(self, num_iterations: int = 12, angle_scale: float = 1.0, max_angle_error: float = 2.0):
        super().__init__()
        lo, hi = _cabi.LG_PG_MIN_ITERATIONS, _cabi.LG_BA_MAX_ITERATIONS
        if isinstance(num_iterations, bool) or int(num_iterations) != num_iterations or not lo <= int(num_iterations) <= hi:
            raise ValueError(f"num_iterations must be an integer in [{lo}, {hi}], got {num_iterations!r}")
        for name, v in (("angle_scale", angle_scale), ("max_angle_error", max_angle_error)):
            if not 0.0 < float(v) < float("inf"):
                raise ValueError(f"{name} must be > 0 degrees, got {v!r}")
        self.num_iterations, self.angle_scale, self.max_angle_error = int(num_iterations), float(angle_scale), float(max_angle_error)

    @torch.no_grad()
    def solve(self, feats: dict, tracks, cameras, poses, constant_pose=None) -> dict:
        """feats = {keypoints [K, N, 2], num_keypoints [K] (optional)}: the store the tracks were built over; `tracks`: the dict of
        `Triangulator.build_tracks` / `triangulate` (track_id, num_tracks are read) or (track_id [K, N], T); cameras [K, 4] (fx, fy, cx, cy) or [K, 3, 3];
        poses [K, 3, 4] (R | t), (R [K, 3, 3], t [K, 3]) or `GlobalPoseEstimator`'s dict (its poses; constant_pose then defaults to [origin, baseline]): R is
        read of every image, t of the held ones only; constant_pose: a [K] bool mask or the indices of the held images — at least two, with finite poses and
        distinct centres (ValueError otherwise: on the host before the GPU is touched where the poses live on the host, else behind the call).  Returns poses
        [K, 3, 4] (R the input's bits, t = -R c; t NaN where an image got no centre, all NaN for a bad image), xyz [T, 3] (NaN: no point), points3d [K, N, 3],
        track_id [K, N] (the input label at every inlier observation, -1 elsewhere), node_state [K, N] uint8 (`STATES`), image_state [K] uint8
        (`IMAGE_STATES`), angle_error [K, N] (degrees, NaN where not evaluated), status [K] (LG_ERR_CAMERA per bad image), num_posed, num_points,
        num_outliers, num_degenerate, iterations, positions_ok.  ONE host synchronisation."""
        device = feats["keypoints"].device
        s = _call.build_side(feats, device, "feats")
        K, N = int(s.K), int(s.N)
        if not 2 <= K <= _cabi.LG_BA_MAX_IMAGES:
            raise ValueError(f"the store must hold between 2 and {_cabi.LG_BA_MAX_IMAGES} images, got {K}")
        if isinstance(poses, dict):
            for k in ("poses", "origin", "baseline"):
                if k not in poses:
                    raise ValueError(f"poses is a dict without {k!r}: pass GlobalPoseEstimator's dict, [K, 3, 4] or a tuple (R, t)")
            if constant_pose is None:
                if poses["baseline"] is None:
                    raise ValueError("poses is GlobalPoseEstimator's dict without a baseline: no second image to hold (pass constant_pose)")
                constant_pose = [int(poses["origin"]), int(poses["baseline"])]
            poses = poses["poses"]
        if constant_pose is None:
            raise ValueError(NO_GAUGE)
        const = as_constant(constant_pose, K)
        if int(const.sum()) < 2:
            raise ValueError(NO_GAUGE)
        tid, T = as_labels(tracks, K, N, device)
        host_poses = (poses[0] if isinstance(poses, (tuple, list)) else poses)
        on_host = not (torch.is_tensor(host_poses) and host_poses.device.type != "cpu")
        cam, pose = as_cameras(cameras, K, device, "cameras"), as_poses(poses, K, device)
        if on_host:                                    # the gauge, from the inputs as they lie on the host
            P = (pose if pose.device.type == "cpu" else as_poses(poses, K, torch.device("cpu")))[const].double()
            centres = -torch.einsum("kji,kj->ki", P[:, :, :3], P[:, :, 3])
            good = centres[torch.isfinite(P).all(2).all(1)]
            if len(good) < 2 or bool((good == good[0]).all()):
                raise ValueError(NO_GAUGE)
        _call.require_gpu(device, "keypoints")          # behind every shape check: those need no device
        const = const.to(device=device, dtype=torch.uint8)
        poses_out = torch.empty((K, 3, 4), device=device, dtype=torch.float32)
        xyz = torch.empty((T, 3), device=device, dtype=torch.float32)
        pts = torch.empty((K, N, 3), device=device, dtype=torch.float32)
        tid_out = torch.empty((K, N), device=device, dtype=torch.int64)
        state = torch.empty((K, N), device=device, dtype=torch.uint8)
        image_state = torch.empty((K,), device=device, dtype=torch.uint8)
        err = torch.empty((K, N), device=device, dtype=torch.float32)
        small = torch.zeros((16 + K,), device=device, dtype=torch.int32)          # summary [8] fp64 | status [K]
        with torch.cuda.device(device):
            stream = torch.cuda.current_stream(device)
            lib = _cabi.load()
            nbytes = lib.lg_positioning_workspace_bytes(K, N, T, 0)                # -1: outside the envelope — the call below says why
            ws = torch.empty((max(nbytes, 256),), device=device, dtype=torch.uint8)
            p = _call._ptr
            io = _cabi.LgPositioningIO(
                n=N, images=K, tracks=T, flags=0, num_iterations=self.num_iterations, angle_scale=self.angle_scale, max_angle_error=self.max_angle_error,
                kpts=p(s.kpts), num=p(s.num), track_id=p(tid), cameras=p(cam), poses=p(pose), constant_pose=p(const), workspace=p(ws),
                workspace_bytes=max(nbytes, 0), poses_out=p(poses_out), xyz=p(xyz), points3d=p(pts), track_id_out=p(tid_out), node_state=p(state),
                image_state=p(image_state), angle_error=p(err), summary=small.data_ptr(), status=small.data_ptr() + 64)
            _cabi.check(lib.lg_positioning_solve(C.byref(io), C.c_void_p(stream.cuda_stream)))
            host = small.cpu().numpy()                # THE host sync of the call
        summary = host[:16].view(np.float64)
        if not summary[5]:
            raise ValueError(NO_GAUGE)
        return {"poses": poses_out, "xyz": xyz, "points3d": pts, "track_id": tid_out, "node_state": state, "image_state": image_state, "angle_error": err,
                "status": small[16:], "num_posed": int(summary[0]), "num_points": int(summary[1]), "num_outliers": int(summary[2]),
                "iterations": int(summary[3]), "positions_ok": bool(summary[4]), "num_degenerate": int(summary[6])}

    forward = solve
