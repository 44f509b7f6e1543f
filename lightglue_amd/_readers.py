"""THE readers of what the geometry classes take beside a feature store (`_call.build_side` reads that, `_call.as_matches0` the matches): cameras, poses, tracks,
labels, the held images and relative poses -> tensors as the C ABI reads them, or the ValueError.  Each is written once here and imported by every class that
takes its input; none is exported from the package.  Plain tensor code: nothing here launches a kernel of the library's."""
from __future__ import annotations

import torch


def as_cameras(cameras, K: int, device, what: str = "cameras") -> torch.Tensor:
    """[K, 4] float32 (fx, fy, cx, cy) on `device` from a [K, 4] tensor or from [K, 3, 3] calibration matrices (zero skew, last row (0, 0, 1): checked on
    the host, so matrices that live on the device cost a copy of their own; the [K, 4] form is read as it stands)"""
    cam = torch.as_tensor(cameras)
    if cam.dim() == 3 and tuple(cam.shape[1:]) == (3, 3):
        flat = cam.detach().to(torch.float64).reshape(-1, 9)
        zero, one = flat[:, [1, 3, 6, 7]], flat[:, 8]
        if bool((zero != 0).any()) or bool((one != 1).any()):
            raise ValueError(f"{what}: calibration matrices must have zero skew and a last row of (0, 0, 1)")
        cam = flat[:, [0, 4, 2, 5]]
    if cam.dim() != 2 or tuple(cam.shape) != (K, 4):
        raise ValueError(f"{what} must have shape [{K}, 4] (fx, fy, cx, cy) or [{K}, 3, 3], got {tuple(cam.shape)}")
    return cam.detach().to(device=device, dtype=torch.float32).contiguous()


def as_poses(poses, K: int, device) -> torch.Tensor:
    """[K, 3, 4] float32 (R | t) on `device` from a [K, 3, 4] tensor or a tuple (R [K, 3, 3], t [K, 3])"""
    if isinstance(poses, (tuple, list)) and len(poses) == 2:
        R, t = torch.as_tensor(poses[0]), torch.as_tensor(poses[1])
        if tuple(R.shape) != (K, 3, 3) or tuple(t.shape) != (K, 3):
            raise ValueError(f"poses (R, t) must have shapes [{K}, 3, 3] and [{K}, 3], got {tuple(R.shape)} and {tuple(t.shape)}")
        poses = torch.cat([R.to(device=device, dtype=torch.float32), t.to(device=device, dtype=torch.float32)[:, :, None]], 2)
    poses = torch.as_tensor(poses)
    if tuple(poses.shape) != (K, 3, 4):
        raise ValueError(f"poses must have shape [{K}, 3, 4] (R | t) or be a tuple (R [{K}, 3, 3], t [{K}, 3]), got {tuple(poses.shape)}")
    return poses.detach().to(device=device, dtype=torch.float32).contiguous()


def as_track_id(track_id, K: int, N: int, device) -> torch.Tensor:
    """track_id [K, N] int64 on `device`: THE check of the labels `BundleAdjuster` and `GlobalPositioner` read"""
    tid = torch.as_tensor(track_id)
    if tuple(tid.shape) != (K, N):
        raise ValueError(f"track_id must have shape [{K}, {N}], got {tuple(tid.shape)}")
    if tid.dtype.is_floating_point or tid.dtype is torch.bool:
        raise ValueError(f"track_id must hold integers, got {tid.dtype}")
    return tid.detach().to(device=device, dtype=torch.int64).contiguous()


def as_tracks(tracks, K: int, N: int, device):
    """(track_id [K, N] int64, xyz [T, 3] float32) on `device` from `Triangulator`'s dict or a tuple (track_id, xyz)"""
    if isinstance(tracks, dict):
        tracks = (tracks["track_id"], tracks["xyz"])
    if not isinstance(tracks, (tuple, list)) or len(tracks) != 2:
        raise ValueError("tracks must be the Triangulator's dict or a tuple (track_id [K, N], xyz [T, 3])")
    tid, xyz = as_track_id(tracks[0], K, N, device), torch.as_tensor(tracks[1])
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError(f"xyz must have shape [T, 3], got {tuple(xyz.shape)}")
    if xyz.shape[0] > K * N // 2:
        raise ValueError(f"xyz holds {xyz.shape[0]} tracks: more than K N / 2 = {K * N // 2} (a track has at least two observations)")
    return tid, xyz.detach().to(device=device, dtype=torch.float32).contiguous()


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


def as_constant(constant_pose, K: int, name: str = "constant_pose") -> torch.Tensor:
    """[K] bool on the host from a [K] mask or a sequence of image indices; at least one pose must be constant (no camera need be: name = "constant_camera")"""
    c = torch.as_tensor(constant_pose).detach().cpu()
    if c.numel() == 0 and c.dtype is not torch.bool:       # an empty index list (torch reads [] as float)
        c = c.reshape(0).long()
    if c.dtype is not torch.bool:
        if c.dtype.is_floating_point or c.dim() != 1:
            raise ValueError(f"{name} must be a [K] bool mask or a sequence of image indices")
        if c.numel() and (int(c.min()) < 0 or int(c.max()) >= K):
            raise ValueError(f"{name} names an image outside [0, {K})")
        mask = torch.zeros(K, dtype=torch.bool)
        mask[c.long()] = True
        c = mask
    if tuple(c.shape) != (K,):
        raise ValueError(f"{name} must have shape [{K}], got {tuple(c.shape)}")
    if name == "constant_pose" and not bool(c.any()):
        raise ValueError("constant_pose holds no image: nothing fixes the gauge (hold at least one pose; two fix scale as well)")
    return c


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
