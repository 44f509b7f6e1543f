"""Global poses on the device, on the kernels of `csrc/lg_posegraph.hip` behind `lg_posegraph_solve` (include/lightglue_amd.h holds the definition).  It
reads what `RelativePoseEstimator` returns — `R [P, 3, 3]`, `t [P, 3]`, `num_inliers [P]` over a pair list — in place and returns one pose (R | t),
X_cam = R X_world + t, per image: rotation averaging over the view graph, then position averaging along the pairs' translation directions, both robust to
wrong pairs, fp64, dense Cholesky.  The poses are what `Triangulator` and `BundleAdjuster` take.  ONE call with ONE host synchronisation."""
from __future__ import annotations

import ctypes as C

import torch
from torch import nn

from . import _cabi, _call

PAIR_STATES = ("used", "bad_index", "no_model", "outside_component", "rotation_outlier", "no_position")      # pair_state 0 .. 5
IMAGE_STATES = ("posed", "rotation_only", "not_connected")                                                  # image_state 0 .. 2


def as_relative(relative, P: int):
    """(R [P, 3, 3], t [P, 3], num_inliers [P] or None) from `RelativePoseEstimator`'s dict or a tuple (R, t); shapes checked, nothing moved"""
    inl = None
    if isinstance(relative, dict):
        for k in ("R", "t", "num_inliers"):
            if k not in relative:
                raise ValueError(f"relative is a dict without {k!r}: pass RelativePoseEstimator's dict or a tuple (R [P, 3, 3], t [P, 3])")
        R, t, inl = relative["R"], relative["t"], torch.as_tensor(relative["num_inliers"])
    elif isinstance(relative, (tuple, list)) and len(relative) == 2:
        R, t = relative
    else:
        raise ValueError("relative must be RelativePoseEstimator's dict or a tuple (R [P, 3, 3], t [P, 3])")
    R, t = torch.as_tensor(R), torch.as_tensor(t)
    if tuple(R.shape) != (P, 3, 3):
        raise ValueError(f"R must have shape [{P}, 3, 3], got {tuple(R.shape)}")
    if tuple(t.shape) != (P, 3):
        raise ValueError(f"t must have shape [{P}, 3], got {tuple(t.shape)}")
    if inl is not None and (tuple(inl.shape) != (P,) or inl.dtype.is_floating_point or inl.dtype is torch.bool):
        raise ValueError(f"num_inliers must hold [{P}] integers, got {tuple(inl.shape)} {inl.dtype}")
    return R, t, inl


class GlobalPoseEstimator(nn.Module):
    """num_iterations: the fixed budget of EACH of the two solvers, in [6, 100].  rotation_scale, direction_scale: the robust scales (degrees) the two
    reweightings end at (they start wide and halve down to these).  max_rotation_error: a pair further than this (degrees) from the solved rotations is a
    rotation outlier and is not used for positions.  min_inliers: with `RelativePoseEstimator`'s dict, a pair with fewer inliers is not used."""

    def __init__(self, num_iterations: int = 12, rotation_scale: float = 5.0, max_rotation_error: float = 15.0, direction_scale: float = 5.0,
                 min_inliers: int = 15):
        super().__init__()
        lo, hi = _cabi.LG_PG_MIN_ITERATIONS, _cabi.LG_BA_MAX_ITERATIONS
        if isinstance(num_iterations, bool) or int(num_iterations) != num_iterations or not lo <= int(num_iterations) <= hi:
            raise ValueError(f"num_iterations must be an integer in [{lo}, {hi}], got {num_iterations!r}")
        for name, v in (("rotation_scale", rotation_scale), ("max_rotation_error", max_rotation_error), ("direction_scale", direction_scale)):
            if not 0.0 < float(v) < float("inf"):
                raise ValueError(f"{name} must be > 0 degrees, got {v!r}")
        if isinstance(min_inliers, bool) or int(min_inliers) != min_inliers or not 0 <= int(min_inliers) < 2 ** 31:
            raise ValueError(f"min_inliers must be an integer >= 0, got {min_inliers!r}")
        self.num_iterations, self.min_inliers = int(num_iterations), int(min_inliers)
        self.rotation_scale, self.max_rotation_error, self.direction_scale = float(rotation_scale), float(max_rotation_error), float(direction_scale)

    @torch.no_grad()
    def estimate(self, pairs, relative, num_images: int, origin: int = 0, baseline=None, weights=None) -> dict:
        """pairs [P, 2] (a, b), indices outside [0, num_images) and a == b allowed (pair_state says so); relative: `RelativePoseEstimator`'s dict (R, t,
        num_inliers are read) or (R [P, 3, 3], t [P, 3]) with X_b = R X_a + t; weights [P] (default: num_inliers, or 1); origin: the image whose pose is the
        identity; baseline: the image at distance 1 from it (None: the origin's neighbour over its heaviest usable pair).  Returns poses [K, 3, 4] (NaN where
        an image has none), image_state [K] uint8 (`IMAGE_STATES`), pair_state [P] uint8 (`PAIR_STATES`), rotation_error [P], direction_error [P] (degrees,
        NaN where not evaluated), origin, baseline (None if no pair fixed the scale), num_posed, rotation_iterations, position_iterations, positions_ok.
        ONE host synchronisation."""
        pairs = torch.as_tensor(pairs)
        if pairs.dim() != 2 or pairs.shape[1] != 2 or pairs.dtype.is_floating_point or pairs.dtype is torch.bool:
            raise ValueError(f"pairs must be [P, 2] integers, got {tuple(pairs.shape)} {pairs.dtype}")
        P = int(pairs.shape[0])
        if isinstance(num_images, bool) or int(num_images) != num_images or not 2 <= int(num_images) <= _cabi.LG_BA_MAX_IMAGES:
            raise ValueError(f"num_images must be an integer in [2, {_cabi.LG_BA_MAX_IMAGES}], got {num_images!r}")
        K = int(num_images)
        if not 1 <= P <= _cabi.LG_PG_MAX_PAIRS:
            raise ValueError(f"the pair list must hold between 1 and {_cabi.LG_PG_MAX_PAIRS} pairs, got {P}")
        if isinstance(origin, bool) or int(origin) != origin or not 0 <= int(origin) < K:
            raise ValueError(f"origin must name an image in [0, {K}), got {origin!r}")
        if baseline is not None and (isinstance(baseline, bool) or int(baseline) != baseline or not 0 <= int(baseline) < K or int(baseline) == int(origin)):
            raise ValueError(f"baseline must be None or an image in [0, {K}) other than origin, got {baseline!r}")
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
        summary = torch.zeros((8,), device=device, dtype=torch.float64)
        with torch.cuda.device(device):
            stream = torch.cuda.current_stream(device)
            lib = _cabi.load()
            nbytes = lib.lg_posegraph_workspace_bytes(K, P, 0)
            ws = torch.empty((max(nbytes, 256),), device=device, dtype=torch.uint8)
            p = _call._ptr
            io = _cabi.LgPosegraphIO(
                images=K, pairs=P, flags=0, num_iterations=self.num_iterations, origin=int(origin), baseline=-1 if baseline is None else int(baseline),
                min_inliers=self.min_inliers, rotation_scale=self.rotation_scale, max_rotation_error=self.max_rotation_error,
                direction_scale=self.direction_scale, pair_index=p(pairs), rotations=p(R), translations=p(t), weights=p(w), num_inliers=p(inl),
                workspace=p(ws), workspace_bytes=max(nbytes, 0), poses=p(poses), image_state=p(image_state), pair_state=p(pair_state),
                rotation_error=p(errors[0]), direction_error=p(errors[1]), summary=p(summary))
            _cabi.check(lib.lg_posegraph_solve(C.byref(io), C.c_void_p(stream.cuda_stream)))
            host = summary.cpu().numpy()              # THE host sync of the call
        return {"poses": poses, "image_state": image_state, "pair_state": pair_state, "rotation_error": errors[0], "direction_error": errors[1],
                "origin": int(host[0]), "baseline": None if host[1] < 0 else int(host[1]), "num_posed": int(host[2]), "rotation_iterations": int(host[3]),
                "position_iterations": int(host[4]), "positions_ok": bool(host[5])}

    forward = estimate

