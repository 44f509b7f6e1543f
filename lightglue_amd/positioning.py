"""Camera centres and track points from tracks on the device, on the kernels of `csrc/lg_positioning.hip` behind `lg_positioning_solve`
(include/lightglue_amd.h holds the definition).  It keeps the rotations it is given — `GlobalPoseEstimator`'s, say — and solves the centres of all free
images and the points of all tracks jointly from the viewing rays of every observation, with at least two images held to fix origin, orientation and scale:
reweighted linear least squares, Schur complement onto the centres, dense Cholesky, fp64.  It reads the keypoint store and the labels of
`Triangulator.build_tracks` in place; `(track_id, xyz)` of its dict is what `BundleAdjuster.adjust` takes, `points3d` what `AbsolutePoseEstimator` takes.
ONE call with ONE host synchronisation."""
from __future__ import annotations

import torch
from torch import nn

from . import _cabi, _call
from ._readers import as_cameras, as_constant, as_labels, as_poses

# node_state 0 .. 9, image_state 0 .. 5
STATES = ("none", "inlier", "bad_image", "too_long", "peeled", "not_connected", "degenerate", "outlier", "no_point", "no_solution")
IMAGE_STATES = ("posed", "held", "too_few_tracks", "not_connected", "bad_image", "no_solution")
NO_GAUGE = "constant_pose must hold at least two images with finite poses and distinct centres: they fix origin, orientation and scale"


class GlobalPositioner(nn.Module):
    """num_iterations: the fixed budget of reweighted solves, in [6, 100].  angle_scale: the robust scale (degrees between an observation's ray and the
    direction to its point) the reweighting ends at (it starts wide and halves down to it).  max_angle_error: an observation further than this (degrees) from
    its point at the final state is an outlier; no solve follows the classification."""

    def __init__(self, num_iterations: int = 12, angle_scale: float = 1.0, max_angle_error: float = 2.0):
        super().__init__()
        self.num_iterations = _call.int_in("num_iterations", num_iterations, _cabi.LG_PG_MIN_ITERATIONS, _cabi.LG_BA_MAX_ITERATIONS, refuse_bool=True)
        self.angle_scale, self.max_angle_error = _call.positive("angle_scale", angle_scale, " degrees"), _call.positive("max_angle_error", max_angle_error, " degrees")

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
        status, summary_ptr, status_ptr, read = _call.summary_status(8, K, device)
        p = _call._ptr
        io = lambda ws, nbytes: _cabi.LgPositioningIO(
            n=N, images=K, tracks=T, flags=0, num_iterations=self.num_iterations, angle_scale=self.angle_scale, max_angle_error=self.max_angle_error,
            kpts=p(s.kpts), num=p(s.num), track_id=p(tid), cameras=p(cam), poses=p(pose), constant_pose=p(const), workspace=ws,
            workspace_bytes=nbytes, poses_out=p(poses_out), xyz=p(xyz), points3d=p(pts), track_id_out=p(tid_out), node_state=p(state),
            image_state=p(image_state), angle_error=p(err), summary=summary_ptr, status=status_ptr)
        _call.device_call(device, "lg_positioning_solve", "lg_positioning_workspace_bytes", (K, N, T, 0), io)
        summary = read()[0]                           # THE host sync of the call
        if not summary[5]:
            raise ValueError(NO_GAUGE)
        return {"poses": poses_out, "xyz": xyz, "points3d": pts, "track_id": tid_out, "node_state": state, "image_state": image_state, "angle_error": err,
                "status": status, "num_posed": int(summary[0]), "num_points": int(summary[1]), "num_outliers": int(summary[2]),
                "iterations": int(summary[3]), "positions_ok": bool(summary[4]), "num_degenerate": int(summary[6])}

    forward = solve
