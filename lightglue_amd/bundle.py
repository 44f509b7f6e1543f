"""Bundle adjustment of poses, points and (opt-in) per-image focal lengths on the device, on the kernels of `csrc/lg_bundle.hip` behind `lg_bundle_adjust`,
with a robust loss or filter rounds `lg_bundle_adjust_robust`, and with `refine_focal=True` `lg_bundle_adjust_focal` (include/lightglue_amd.h holds the three definitions).  It reads what `Triangulator` returns — `track_id [K, N]` and `xyz [T, 3]` over ONE keypoint store — in place, plus one pinhole camera
(fx, fy, cx, cy) and one pose (R | t), X_cam = R X_world + t, per image, and refines all free poses and all track points jointly: Levenberg-Marquardt on the
sum of squared pixel reprojection errors, Schur complement, dense Cholesky, fp64.  Intrinsics are fixed unless `refine_focal=True`: then every image carries
one more unknown, the logarithm of a common scale of fx and fy (cx, cy stay), held or free per image by `constant_camera` independently of its pose, and the
dict holds `cameras [K, 4]`, which every other estimator takes as it is.  Principal point, distortion, shared intrinsics and a prior stay out.
`solver="pcg"` replaces the dense Cholesky by matrix-free preconditioned conjugate gradients on the reduced camera system (`lg_bundle_adjust_pcg`, block-Jacobi
preconditioner, fp64) and lifts the bound of 256 images to 4096.  ONE call with ONE host synchronisation; `points3d
[K, N, 3]` (NaN where a row is no active observation) is what `AbsolutePoseEstimator` takes as points3d1."""
from __future__ import annotations

import numpy as np
import torch
from torch import nn

from . import _cabi, _call
from ._readers import as_cameras, as_constant, as_poses, as_tracks

STATES = ("none", "active", "bad_image", "non_finite_point", "behind", "short_track", "too_long", "filtered")    # node_state 0 .. 7 (7: the robust mode's filter)
IMAGE_STATUS = {_cabi.LG_ERR_CAMERA: "a camera whose focal length is not finite and > 0, whose principal point is not finite, or a non-finite pose (LG_ERR_CAMERA): "
                                     "its observations were left out"}     # status [K] of an adjust call (the only code lg_bundle.hip writes there beside LG_OK)


class BundleAdjuster(nn.Module):
    """num_iterations: the fixed budget of Levenberg-Marquardt iterations, in [1, 100].  initial_damping: lambda of the first iteration.  function_tolerance:
    the call converges after a trial with |cost - cost_new| <= function_tolerance cost.  At least one image must be held constant; two constant images fix the
    scale of the reconstruction, with one the damping holds it (it may drift slowly).
    loss: "squared", "huber" or "cauchy" on the pixel error, with loss_scale (c, pixels) where the loss bends; filter_rounds in [0, 4]: after each of that
    many stages of num_iterations the observations above max_reproj_error (pixels) are dropped (node_state 7) and the rest is adjusted again.  The defaults
    (squared, no filter) call `lg_bundle_adjust` as before; anything else calls `lg_bundle_adjust_robust`.
    refine_focal: every image carries one more unknown d, a step sets fx <- fx exp(d), fy <- fy exp(d) (the aspect ratio and the sign stay, cx and cy are not
    touched); `adjust` then takes `constant_camera` and returns `cameras` and `num_free_cameras`, on `lg_bundle_adjust_focal`, with every loss and filter
    setting meaning what it means without it.  False (the default) changes nothing.
    solver: "cholesky" (the default: the dense factorisation, at most 256 images, nothing changes) or "pcg": every Levenberg-Marquardt step is solved by at
    most max_cg_iterations (in [1, 1000]) iterations of preconditioned conjugate gradients, stopped once the preconditioned residual norm sqrt(r.z) has
    fallen to cg_tolerance (in (0, 1)) times its start; up to 4096 images, with every loss and filter setting (`lg_bundle_adjust_pcg`), not with
    refine_focal.  num_iterations x (filter_rounds + 1) x max_cg_iterations may not exceed 20000: the call enqueues that many solver iterations.  The dict
    then counts them in `cg_iterations`, and in `cg_unconverged` the Levenberg-Marquardt iterations whose solve ended on the budget.  With "cholesky"
    max_cg_iterations and cg_tolerance are not read and therefore not examined, like the robust settings under the defaults."""

    def __init__(self, num_iterations: int = 10, initial_damping: float = 1e-4, function_tolerance: float = 1e-6, loss: str = "squared", loss_scale: float = 2.0,
                 filter_rounds: int = 0, max_reproj_error: float = 4.0, refine_focal: bool = False, solver: str = "cholesky", max_cg_iterations: int = 100,
                 cg_tolerance: float = 1e-6):
        super().__init__()
        if not isinstance(refine_focal, (bool, np.bool_)):
            raise ValueError(f"refine_focal must be a bool, got {refine_focal!r}")
        # the defaults are not examined further (what the C side does not read is not refused), and the robust settings are ONE attribute: an nn.Module
        # pays for every attribute it sets, and this constructor sits inside callers' loops
        if not (loss == "squared" and type(filter_rounds) is int and filter_rounds == 0):
            if loss not in _cabi.LG_BA_LOSS:
                raise ValueError(f"loss must be one of {sorted(_cabi.LG_BA_LOSS)}, got {loss!r}")
            rounds = _call.int_in("filter_rounds", filter_rounds, 0, _cabi.LG_BA_MAX_FILTER_ROUNDS, refuse_bool=True)
            if loss != "squared":
                _call.positive("loss_scale", loss_scale, " with a robust loss")
            if rounds > 0:
                _call.positive("max_reproj_error", max_reproj_error, " with filter_rounds > 0")
        pcg = None                                          # or (max_cg_iterations, cg_tolerance): the last entry of the one attribute
        if solver != "cholesky":
            if solver != "pcg":
                raise ValueError(f"solver must be 'cholesky' or 'pcg', got {solver!r}")
            if refine_focal:
                raise ValueError("solver='pcg' does not refine focal lengths: refine_focal needs solver='cholesky'")
            if not isinstance(cg_tolerance, (int, float, np.floating)) or not 0.0 < float(cg_tolerance) < 1.0:
                raise ValueError(f"cg_tolerance must be a number in (0, 1), got {cg_tolerance!r}")
            pcg = (_call.int_in("max_cg_iterations", max_cg_iterations, 1, _cabi.LG_BA_PCG_MAX_CG_ITERATIONS, refuse_bool=True), float(cg_tolerance))
        self.robust = (loss, float(loss_scale), int(filter_rounds), float(max_reproj_error), loss != "squared" or filter_rounds > 0, bool(refine_focal), pcg)
        self.num_iterations = _call.int_in("num_iterations", num_iterations, 1, _cabi.LG_BA_MAX_ITERATIONS)        # takes True as 1, as it always has
        if pcg and self.num_iterations * (int(filter_rounds) + 1) * pcg[0] > _cabi.LG_BA_PCG_MAX_SOLVER_ITERATIONS:
            raise ValueError(f"num_iterations x (filter_rounds + 1) x max_cg_iterations must not exceed {_cabi.LG_BA_PCG_MAX_SOLVER_ITERATIONS} (the call enqueues "
                             f"that many solver iterations), got {self.num_iterations} x {int(filter_rounds) + 1} x {pcg[0]}")
        self.initial_damping, self.function_tolerance = _call.positive("initial_damping", initial_damping), _call.positive("function_tolerance", function_tolerance)

    loss = property(lambda self: self.robust[0])
    loss_scale = property(lambda self: self.robust[1])
    filter_rounds = property(lambda self: self.robust[2])
    max_reproj_error = property(lambda self: self.robust[3])
    refine_focal = property(lambda self: self.robust[5])
    solver = property(lambda self: "pcg" if self.robust[6] else "cholesky")
    max_cg_iterations = property(lambda self: self.robust[6][0] if self.robust[6] else None)
    cg_tolerance = property(lambda self: self.robust[6][1] if self.robust[6] else None)

    @property
    def robust_entry(self) -> bool:
        """the C entry point adjust() takes: lg_bundle_adjust_robust also accepts the plain settings and then returns lg_bundle_adjust's bytes (the tests
        set this to compare the two on one call)"""
        return self.robust[4]

    @robust_entry.setter
    def robust_entry(self, value):
        self.robust = self.robust[:4] + (bool(value),) + self.robust[5:]

    @torch.no_grad()
    def adjust(self, feats: dict, tracks, cameras, poses, constant_pose, constant_camera=None) -> dict:
        """feats = {keypoints [K, N, 2], num_keypoints [K] (optional)}: the store the tracks were built over; `tracks`: `Triangulator`'s dict or
        (track_id [K, N], xyz [T, 3]); cameras [K, 4] (fx, fy, cx, cy) or [K, 3, 3]; poses [K, 3, 4] (R | t) or (R [K, 3, 3], t [K, 3]); constant_pose: a [K]
        bool mask or the indices of the images whose pose is held fixed (at least one: ValueError otherwise; two fix scale).  Returns poses [K, 3, 4], xyz
        [T, 3], points3d [K, N, 3] (NaN where a row is no active observation), node_state [K, N] uint8 (`STATES`), observation_error [K, N] (pixels, NaN where
        not active), initial_cost, final_cost, num_iterations (run), num_accepted, converged, num_observations, num_filtered, num_filter_stages (both 0 without
        a filter), status [K]; with solver="pcg" also cg_iterations and cg_unconverged.  With refine_focal: constant_camera (None: no camera is held; else a [K] bool mask or image indices, parsed like
        constant_pose) names the images whose focal length is held, independently of the poses, and the dict also holds cameras [K, 4] float32 (fx, fy
        refined where the camera was free; cx, cy and every camera that never moved are the input's bits: what `Triangulator`, `AbsolutePoseEstimator` and
        `RelativePoseEstimator` take as cameras) and num_free_cameras.  Without refine_focal constant_camera must be None.  ONE host synchronisation.  An
        image whose camera or pose fails the camera rule raises LightGlueAmdError after the call, with `err.outputs` holding the outputs of everything else."""
        device = feats["keypoints"].device
        s = _call.build_side(feats, device, "feats")
        K, N = int(s.K), int(s.N)
        const = as_constant(constant_pose, K)
        loss, loss_scale, filter_rounds, max_reproj_error, robust, focal, pcg = self.robust
        if constant_camera is not None and not focal:
            raise ValueError("constant_camera needs refine_focal=True: without it every camera is held")
        const_cam = as_constant(constant_camera, K, "constant_camera") if constant_camera is not None else None
        tid, xyz = as_tracks(tracks, K, N, device)
        cam, pose = as_cameras(cameras, K, device, "cameras"), as_poses(poses, K, device)
        _call.require_gpu(device, "keypoints")          # behind every shape check: those need no device
        T = int(xyz.shape[0])
        const = const.to(device=device, dtype=torch.uint8)
        poses_out = torch.empty((K, 3, 4), device=device, dtype=torch.float32)
        xyz_out = torch.empty((T, 3), device=device, dtype=torch.float32)
        pts = torch.empty((K, N, 3), device=device, dtype=torch.float32)
        state = torch.empty((K, N), device=device, dtype=torch.uint8)
        err = torch.empty((K, N), device=device, dtype=torch.float32)
        status, summary_ptr, status_ptr, read = _call.summary_status(12, K, device)       # lg_bundle_adjust writes 8 of the 12 doubles
        cameras_out = torch.empty((K, 4), device=device, dtype=torch.float32) if focal else None
        held = const_cam.to(device=device, dtype=torch.uint8) if const_cam is not None else None
        p = _call._ptr

        def make_io(ws, nbytes):      # the plain struct, wrapped once for the robust entry point and once more for the focal one
            io = _cabi.LgBundleIO(
                n=N, images=K, tracks=T, flags=0, num_iterations=self.num_iterations, initial_damping=self.initial_damping,
                function_tolerance=self.function_tolerance, kpts=p(s.kpts), num=p(s.num), track_id=p(tid), xyz=p(xyz), cameras=p(cam), poses=p(pose),
                constant_pose=p(const), workspace=ws, workspace_bytes=nbytes, poses_out=p(poses_out), xyz_out=p(xyz_out), points3d=p(pts),
                node_state=p(state), observation_error=p(err), summary=summary_ptr, status=status_ptr)
            if robust or focal or pcg:
                io = _cabi.LgBundleRobustIO(base=io, loss=_cabi.LG_BA_LOSS[loss], filter_rounds=filter_rounds, loss_scale=loss_scale, max_reproj_error=max_reproj_error)
            if pcg:
                return _cabi.LgBundlePcgIO(base=io, max_cg_iterations=pcg[0], pad=0, cg_tolerance=pcg[1])
            return _cabi.LgBundleFocalIO(base=io, constant_camera=p(held) if held is not None else None, cameras_out=p(cameras_out)) if focal else io
        entry = (("lg_bundle_adjust_pcg", "lg_bundle_pcg_workspace_bytes") if pcg else ("lg_bundle_adjust_focal", "lg_bundle_focal_workspace_bytes") if focal
                 else ("lg_bundle_adjust_robust", "lg_bundle_robust_workspace_bytes") if robust else ("lg_bundle_adjust", "lg_bundle_workspace_bytes"))
        _call.device_call(device, *entry, (K, N, T, 0), make_io)
        summary, host_status = read()             # THE host sync of the call
        out = {"poses": poses_out, "xyz": xyz_out, "points3d": pts, "node_state": state, "observation_error": err,
               "initial_cost": float(summary[0]), "final_cost": float(summary[1]), "num_iterations": int(summary[2]), "num_accepted": int(summary[3]),
               "converged": bool(summary[4]), "num_observations": int(summary[5]), "num_filtered": int(summary[8]), "num_filter_stages": int(summary[9]),
               "status": status}
        if pcg:
            out["cg_iterations"], out["cg_unconverged"] = int(summary[7]), int(summary[11])
        if focal:
            out["cameras"], out["num_free_cameras"] = cameras_out, int(summary[10])
        return _call.raise_with_outputs(host_status.tolist(), out, "image", IMAGE_STATUS)      # every other image is complete: the error carries the call's outputs

    forward = adjust
