"""Global poses on the device, on the kernels of `csrc/lg_posegraph.hip` behind `lg_posegraph_solve` (include/lightglue_amd.h holds the definition).  It
reads what `RelativePoseEstimator` returns — `R [P, 3, 3]`, `t [P, 3]`, `num_inliers [P]` over a pair list — in place and returns one pose (R | t),
X_cam = R X_world + t, per image: rotation averaging over the view graph, then position averaging along the pairs' translation directions, both robust to
wrong pairs, fp64, dense Cholesky.  The poses are what `Triangulator` and `BundleAdjuster` take.  ONE call with ONE host synchronisation.
`solver="pcg"` (`lg_posegraph_solve_pcg`) solves both stages by matrix-free preconditioned conjugate gradients instead, for up to 4 096 images."""
from __future__ import annotations

import torch
from torch import nn

from . import _cabi, _call
from ._readers import as_relative

SOLVERS = ("cholesky", "pcg")
PAIR_STATES = ("used", "bad_index", "no_model", "outside_component", "rotation_outlier", "no_position")      # pair_state 0 .. 5
IMAGE_STATES = ("posed", "rotation_only", "not_connected")                                                  # image_state 0 .. 2


class GlobalPoseEstimator(nn.Module):
    """num_iterations: the fixed budget of EACH of the two solvers, in [6, 100].  rotation_scale, direction_scale: the robust scales (degrees) the two
    reweightings end at (they start wide and halve down to these).  max_rotation_error: a pair further than this (degrees) from the solved rotations is a
    rotation outlier and is not used for positions.  min_inliers: with `RelativePoseEstimator`'s dict, a pair with fewer inliers is not used.
    solver: "cholesky" (the default: both systems dense, up to 256 images) or "pcg": both systems solved by preconditioned conjugate gradients over the
    images' adjacency lists, up to 4 096 images, with rotation_cg_iterations / position_cg_iterations (each in [1, 1000]) the budget of ONE solve of
    either stage and cg_tolerance in (0, 1) the relative residual a solve stops at; num_iterations x (rotation_cg_iterations + position_cg_iterations)
    must not exceed 20 000 (that many solver iterations are enqueued).  The three are read with "pcg" only.  What "pcg" does NOT report: a view graph
    whose position system the dense solver calls singular by its pivot floor.  positions_ok is False only for a missing baseline, a singular 3 x 3
    block of one image (collinear cameras) and a failed recurrence.  On 1 100 images with 3 300 pairs (3 per image) the dense definition returns
    positions_ok = False; "pcg" converges (up to 918 solver iterations in one solve) to centres 4.35 x the scene's extent off.  With 8 pairs per
    image both agree.  The caller's signals are `direction_error`, `rotation_cg_unconverged` and `position_cg_unconverged`."""

    def __init__(self, num_iterations: int = 12, rotation_scale: float = 5.0, max_rotation_error: float = 15.0, direction_scale: float = 5.0,
                 min_inliers: int = 15, solver: str = "cholesky", rotation_cg_iterations: int = 64, position_cg_iterations: int = 800,
                 cg_tolerance: float = 1e-6):
        super().__init__()
        if solver not in SOLVERS:
            raise ValueError(f"solver must be one of {SOLVERS}, got {solver!r}")
        self.solver = solver
        self.num_iterations = _call.int_in("num_iterations", num_iterations, _cabi.LG_PG_MIN_ITERATIONS, _cabi.LG_BA_MAX_ITERATIONS, refuse_bool=True)
        self.rotation_scale, self.max_rotation_error, self.direction_scale = (_call.positive(name, v, " degrees") for name, v in (
            ("rotation_scale", rotation_scale), ("max_rotation_error", max_rotation_error), ("direction_scale", direction_scale)))
        self.min_inliers = _call.int_in("min_inliers", min_inliers, 0, 2 ** 31 - 1, True, "must be an integer >= 0")
        self.rotation_cg_iterations = self.position_cg_iterations = self.cg_tolerance = None
        if solver == "pcg":
            self.rotation_cg_iterations, self.position_cg_iterations = (
                _call.int_in(name, v, 1, _cabi.LG_BA_PCG_MAX_CG_ITERATIONS, refuse_bool=True)
                for name, v in (("rotation_cg_iterations", rotation_cg_iterations), ("position_cg_iterations", position_cg_iterations)))
            if isinstance(cg_tolerance, (bool, str)) or cg_tolerance is None or not 0.0 < float(cg_tolerance) < 1.0:
                raise ValueError(f"cg_tolerance must lie in (0, 1), got {cg_tolerance!r}")
            self.cg_tolerance = float(cg_tolerance)
            enqueued = self.num_iterations * (self.rotation_cg_iterations + self.position_cg_iterations)
            if enqueued > _cabi.LG_BA_PCG_MAX_SOLVER_ITERATIONS:
                raise ValueError(f"num_iterations x (rotation_cg_iterations + position_cg_iterations) must not exceed "
                                 f"{_cabi.LG_BA_PCG_MAX_SOLVER_ITERATIONS} (the call enqueues that many solver iterations), got {enqueued}")

    @torch.no_grad()
    def estimate(self, pairs, relative, num_images: int, origin: int = 0, baseline=None, weights=None) -> dict:
        """pairs [P, 2] (a, b), indices outside [0, num_images) and a == b allowed (pair_state says so); relative: `RelativePoseEstimator`'s dict (R, t,
        num_inliers are read) or (R [P, 3, 3], t [P, 3]) with X_b = R X_a + t; weights [P] (default: num_inliers, or 1); origin: the image whose pose is the
        identity; baseline: the image at distance 1 from it (None: the origin's neighbour over its heaviest usable pair).  Returns poses [K, 3, 4] (NaN where
        an image has none), image_state [K] uint8 (`IMAGE_STATES`), pair_state [P] uint8 (`PAIR_STATES`), rotation_error [P], direction_error [P] (degrees,
        NaN where not evaluated), origin, baseline (None if no pair fixed the scale), num_posed, rotation_iterations, position_iterations, positions_ok;
        with solver="pcg" also rotation_cg_iterations, position_cg_iterations (solver iterations run over the call), rotation_cg_unconverged,
        position_cg_unconverged (solves that ended on their budget) and cg_failures (solves whose recurrence, or whose 3 x 3 blocks, failed).  num_images: up
        to 256 with "cholesky", up to 4 096 with "pcg".  ONE host synchronisation."""
        pairs = torch.as_tensor(pairs)
        if pairs.dim() != 2 or pairs.shape[1] != 2 or pairs.dtype.is_floating_point or pairs.dtype is torch.bool:
            raise ValueError(f"pairs must be [P, 2] integers, got {tuple(pairs.shape)} {pairs.dtype}")
        P = int(pairs.shape[0])
        pcg = self.solver == "pcg"
        K = _call.int_in("num_images", num_images, 2, _cabi.LG_BA_PCG_MAX_IMAGES if pcg else _cabi.LG_BA_MAX_IMAGES, refuse_bool=True)
        if not 1 <= P <= _cabi.LG_PG_MAX_PAIRS:
            raise ValueError(f"the pair list must hold between 1 and {_cabi.LG_PG_MAX_PAIRS} pairs, got {P}")
        origin, other = _call.int_in("origin", origin, 0, K - 1, True, f"must name an image in [0, {K})"), f"must be None or an image in [0, {K}) other than origin"
        if baseline is not None and _call.int_in("baseline", baseline, 0, K - 1, True, other) == origin:
            raise ValueError(f"baseline {other}, got {baseline!r}")
        R, t, inl = as_relative(relative, P)
        if weights is not None:
            weights = torch.as_tensor(weights)
            if tuple(weights.shape) != (P,) or not weights.dtype.is_floating_point:
                raise ValueError(f"weights must be a [{P}] float tensor, got {tuple(weights.shape)} {weights.dtype}")
        device = R.device
        _call.require_gpu(device, "R")                  # behind every shape check: those need no device
        f32 = lambda x: x.detach().to(device=device, dtype=torch.float32).contiguous()
        R, t = f32(R), f32(t)
        pairs = pairs.detach().to(device=device, dtype=torch.int64).contiguous()
        inl = None if inl is None else inl.detach().to(device=device, dtype=torch.int32).contiguous()
        w = f32(weights) if weights is not None else (inl.to(torch.float32) if inl is not None else torch.ones(P, device=device, dtype=torch.float32))
        poses = torch.empty((K, 3, 4), device=device, dtype=torch.float32)
        image_state = torch.empty((K,), device=device, dtype=torch.uint8)
        pair_state = torch.empty((P,), device=device, dtype=torch.uint8)
        errors = torch.empty((2, P), device=device, dtype=torch.float32)
        summary = torch.zeros((12 if pcg else 8,), device=device, dtype=torch.float64)
        p = _call._ptr
        io = lambda ws, nbytes: _cabi.LgPosegraphIO(
            images=K, pairs=P, flags=0, num_iterations=self.num_iterations, origin=origin, baseline=-1 if baseline is None else int(baseline),
            min_inliers=self.min_inliers, rotation_scale=self.rotation_scale, max_rotation_error=self.max_rotation_error,
            direction_scale=self.direction_scale, pair_index=p(pairs), rotations=p(R), translations=p(t), weights=p(w), num_inliers=p(inl),
            workspace=ws, workspace_bytes=nbytes, poses=p(poses), image_state=p(image_state), pair_state=p(pair_state),
            rotation_error=p(errors[0]), direction_error=p(errors[1]), summary=p(summary))
        if pcg:
            pcg_io = lambda ws, nbytes: _cabi.LgPosegraphPcgIO(base=io(ws, nbytes), rotation_cg_iterations=self.rotation_cg_iterations,
                                                               position_cg_iterations=self.position_cg_iterations, cg_tolerance=self.cg_tolerance)
            _call.device_call(device, "lg_posegraph_solve_pcg", "lg_posegraph_pcg_workspace_bytes", (K, P, 0), pcg_io)
        else:
            _call.device_call(device, "lg_posegraph_solve", "lg_posegraph_workspace_bytes", (K, P, 0), io)
        host = summary.cpu().numpy()                  # THE host sync of the call
        out = {"poses": poses, "image_state": image_state, "pair_state": pair_state, "rotation_error": errors[0], "direction_error": errors[1],
               "origin": int(host[0]), "baseline": None if host[1] < 0 else int(host[1]), "num_posed": int(host[2]), "rotation_iterations": int(host[3]),
               "position_iterations": int(host[4]), "positions_ok": bool(host[5])}
        if pcg:
            out.update(rotation_cg_iterations=int(host[8]), position_cg_iterations=int(host[9]), rotation_cg_unconverged=int(host[10]),
                       position_cg_unconverged=int(host[11]), cg_failures=int(host[6]))
        return out

    forward = estimate

