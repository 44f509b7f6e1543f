"""What the Python layer over the geometry kernels answers before it reaches the device, pinned as tables: every constructor setting of `NearestNeighborMatcher`
and the seven geometry classes (accepted values with their types, or the exact ValueError), `GlobalPoseEstimator.estimate`'s own arguments, and every reader of
cameras, poses, tracks, labels, held images and relative poses, good forms and refusals.  The tables hold the answers of the tree BEFORE the wrappers were
written over shared helpers (they pass there with the readers taken from the class modules); the last section tests those helpers of `_call` directly.
Plain host code on CPU tensors: no GPU, no library."""
import ctypes

import numpy as np
import pytest
import torch

from lightglue_amd import (AbsolutePoseEstimator, BundleAdjuster, GlobalPoseEstimator, GlobalPositioner, NearestNeighborMatcher, RelativePoseEstimator,
                           Triangulator, TwoViewVerifier, _cabi, _call)
from lightglue_amd import _readers as readers      # the readers' one home

NAN, INF = float("nan"), float("inf")
RANSAC = (TwoViewVerifier, RelativePoseEstimator, AbsolutePoseEstimator)
NO_GPU = "lightglue_amd runs on MI355X (ROCm device type 'cuda') only; there is no CPU fallback. Got R on cpu."


def rows(classes, table):
    return [pytest.param(cls, kwargs, want, id=f"{cls.__name__}-{kwargs}") for cls in classes for kwargs, want in table]


# (kwargs, the attributes an accepted constructor holds | the ValueError's text)
SETTINGS = rows(RANSAC, [
    (dict(threshold=INF), dict(threshold=INF)),                                        # only > 0 is asked of it
    (dict(threshold=True), dict(threshold=1.0)),
    (dict(threshold=1e-300), dict(threshold=1e-300)),
    (dict(num_hypotheses=256), dict(num_hypotheses=256)),
    (dict(num_hypotheses=65536), dict(num_hypotheses=65536)),
    (dict(num_hypotheses=512.0), dict(num_hypotheses=512)),
    (dict(num_hypotheses="512"), dict(num_hypotheses=512)),
    (dict(num_hypotheses=True), "num_hypotheses must be a multiple of 256 in [256, 65536], got True"),
    (dict(num_hypotheses=1.0), "num_hypotheses must be a multiple of 256 in [256, 65536], got 1.0"),
    (dict(num_hypotheses="3"), "num_hypotheses must be a multiple of 256 in [256, 65536], got '3'"),
    (dict(seed=True), dict(seed=1)),
    (dict(seed=1.0), dict(seed=1)),
    (dict(seed="3"), dict(seed=3)),
    (dict(seed=2 ** 32 - 1), dict(seed=2 ** 32 - 1)),
    (dict(refine=0), dict(refine=False)),
    (dict(threshold=0, num_hypotheses=1), "threshold must be > 0, got 0"),
    (dict(num_hypotheses=1, seed=-1), "num_hypotheses must be a multiple of 256 in [256, 65536], got 1"),
]) + rows((TwoViewVerifier,), [
    (dict(model="homography"), dict(model="homography")),
    (dict(model="affine"), "model must be one of ['fundamental', 'homography'], got 'affine'"),
    (dict(model="affine", threshold=0), "model must be one of ['fundamental', 'homography'], got 'affine'"),
]) + rows((NearestNeighborMatcher,), [
    (dict(), dict(mutual=True, ratio_threshold=None, distance_threshold=None)),
    (dict(mutual=0, ratio_threshold=1, distance_threshold=INF), dict(mutual=False, ratio_threshold=1.0, distance_threshold=INF)),
    (dict(ratio_threshold=True, distance_threshold=True), dict(ratio_threshold=1.0, distance_threshold=1.0)),
    (dict(ratio_threshold=1e-300), dict(ratio_threshold=1e-300)),
    (dict(ratio_threshold=0.0), "ratio_threshold must lie in (0, 1] or be None, got 0.0"),
    (dict(ratio_threshold=1.0000001), "ratio_threshold must lie in (0, 1] or be None, got 1.0000001"),
    (dict(ratio_threshold=NAN), "ratio_threshold must lie in (0, 1] or be None, got nan"),
    (dict(ratio_threshold=INF), "ratio_threshold must lie in (0, 1] or be None, got inf"),
    (dict(distance_threshold=0.0), "distance_threshold must be > 0 or None, got 0.0"),
    (dict(distance_threshold=-1), "distance_threshold must be > 0 or None, got -1"),
    (dict(distance_threshold=NAN), "distance_threshold must be > 0 or None, got nan"),
    (dict(ratio_threshold=2, distance_threshold=0), "ratio_threshold must lie in (0, 1] or be None, got 2"),
]) + rows((Triangulator,), [
    (dict(num_hypotheses=1, max_tracks=1, max_track_length=2), dict(num_hypotheses=1, max_tracks=1, max_track_length=2)),
    (dict(num_hypotheses=4096, max_tracks=4, max_track_length=1024), dict(num_hypotheses=4096, max_tracks=4, max_track_length=1024)),
    (dict(num_hypotheses=True, max_tracks=True), dict(num_hypotheses=1, max_tracks=1)),          # these integers take a bool
    (dict(num_hypotheses=1.0, max_tracks=2.0, max_track_length=2.0), dict(num_hypotheses=1, max_tracks=2, max_track_length=2)),
    (dict(num_hypotheses=0), "num_hypotheses must be an integer in [1, 4096], got 0"),
    (dict(num_hypotheses=4097), "num_hypotheses must be an integer in [1, 4096], got 4097"),
    (dict(num_hypotheses=1.5), "num_hypotheses must be an integer in [1, 4096], got 1.5"),
    (dict(num_hypotheses="3"), "num_hypotheses must be an integer in [1, 4096], got '3'"),
    (dict(max_tracks=0), "max_tracks must be an integer in [1, 4], got 0"),
    (dict(max_tracks=5), "max_tracks must be an integer in [1, 4], got 5"),
    (dict(max_tracks="3"), "max_tracks must be an integer in [1, 4], got '3'"),
    (dict(max_track_length=1), "max_track_length must be an integer in [2, 1024], got 1"),
    (dict(max_track_length=1025), "max_track_length must be an integer in [2, 1024], got 1025"),
    (dict(max_track_length=True), "max_track_length must be an integer in [2, 1024], got True"),   # as 1, below the range
    (dict(max_track_length="3"), "max_track_length must be an integer in [2, 1024], got '3'"),
    (dict(max_reproj_error=True, min_angle=0, refine=0, robust=1), dict(max_reproj_error=1.0, min_angle=0.0, refine=False, robust=True)),
    (dict(max_reproj_error=1e-300, min_angle=179.9), dict(max_reproj_error=1e-300, min_angle=179.9)),
    (dict(max_reproj_error=0.0), "max_reproj_error must be > 0, got 0.0"),
    (dict(max_reproj_error=NAN), "max_reproj_error must be > 0, got nan"),
    (dict(max_reproj_error=INF), "max_reproj_error must be > 0, got inf"),
    (dict(min_angle=180), "min_angle must lie in [0, 180), got 180"),
    (dict(min_angle=-0.1), "min_angle must lie in [0, 180), got -0.1"),
    (dict(min_angle=NAN), "min_angle must lie in [0, 180), got nan"),
    (dict(num_hypotheses=0, max_tracks=0), "num_hypotheses must be an integer in [1, 4096], got 0"),
    (dict(max_tracks=0, max_reproj_error=0), "max_tracks must be an integer in [1, 4], got 0"),
    (dict(max_reproj_error=0, min_angle=180), "max_reproj_error must be > 0, got 0"),
    (dict(min_angle=180, max_track_length=1), "min_angle must lie in [0, 180), got 180"),
]) + rows((BundleAdjuster,), [
    (dict(), dict(num_iterations=10, initial_damping=1e-4, function_tolerance=1e-6, loss="squared", loss_scale=2.0, filter_rounds=0, max_reproj_error=4.0,
                  refine_focal=False, robust_entry=False)),
    (dict(num_iterations=1), dict(num_iterations=1)),
    (dict(num_iterations=100), dict(num_iterations=100)),
    (dict(num_iterations=True), dict(num_iterations=1)),                                           # this one takes a bool, filter_rounds does not
    (dict(num_iterations=3.0, initial_damping=True, function_tolerance=1), dict(num_iterations=3, initial_damping=1.0, function_tolerance=1.0)),
    (dict(num_iterations=0), "num_iterations must be an integer in [1, 100], got 0"),
    (dict(num_iterations=101), "num_iterations must be an integer in [1, 100], got 101"),
    (dict(num_iterations="3"), "num_iterations must be an integer in [1, 100], got '3'"),
    (dict(initial_damping=0), "initial_damping must be > 0, got 0"),
    (dict(initial_damping=NAN), "initial_damping must be > 0, got nan"),
    (dict(initial_damping=INF), "initial_damping must be > 0, got inf"),
    (dict(function_tolerance=0.0), "function_tolerance must be > 0, got 0.0"),
    (dict(function_tolerance=NAN), "function_tolerance must be > 0, got nan"),
    (dict(function_tolerance=INF), "function_tolerance must be > 0, got inf"),
    (dict(loss_scale=-1, max_reproj_error=0), dict(loss_scale=-1.0, max_reproj_error=0.0, robust_entry=False)),     # the defaults' path reads neither
    (dict(filter_rounds=0.0, max_reproj_error=0), dict(filter_rounds=0, max_reproj_error=0.0, robust_entry=False)),
    (dict(loss="cauchy", loss_scale=True), dict(loss="cauchy", loss_scale=1.0, filter_rounds=0, robust_entry=True)),
    (dict(loss="huber", max_reproj_error=-1), dict(loss="huber", max_reproj_error=-1.0, robust_entry=True)),        # no filter: not read
    (dict(filter_rounds=4, loss_scale=0), dict(filter_rounds=4, loss_scale=0.0, robust_entry=True)),               # squared: not read
    (dict(filter_rounds=1.0), dict(filter_rounds=1, robust_entry=True)),
    (dict(loss="l1"), "loss must be one of ['cauchy', 'huber', 'squared'], got 'l1'"),
    (dict(filter_rounds=5), "filter_rounds must be an integer in [0, 4], got 5"),
    (dict(filter_rounds=-1), "filter_rounds must be an integer in [0, 4], got -1"),
    (dict(filter_rounds=True), "filter_rounds must be an integer in [0, 4], got True"),
    (dict(filter_rounds="3"), "filter_rounds must be an integer in [0, 4], got '3'"),
    (dict(loss="huber", loss_scale=0), "loss_scale must be > 0 with a robust loss, got 0"),
    (dict(loss="huber", loss_scale=NAN), "loss_scale must be > 0 with a robust loss, got nan"),
    (dict(loss="cauchy", loss_scale=INF), "loss_scale must be > 0 with a robust loss, got inf"),
    (dict(filter_rounds=2, max_reproj_error=0), "max_reproj_error must be > 0 with filter_rounds > 0, got 0"),
    (dict(filter_rounds=2, max_reproj_error=NAN), "max_reproj_error must be > 0 with filter_rounds > 0, got nan"),
    (dict(filter_rounds=2, max_reproj_error=INF), "max_reproj_error must be > 0 with filter_rounds > 0, got inf"),
    (dict(refine_focal=np.bool_(True)), dict(refine_focal=True)),
    (dict(refine_focal=1), "refine_focal must be a bool, got 1"),
    (dict(refine_focal=1, loss="l1"), "refine_focal must be a bool, got 1"),
    (dict(loss="l1", filter_rounds=5), "loss must be one of ['cauchy', 'huber', 'squared'], got 'l1'"),
    (dict(loss="huber", filter_rounds=5, loss_scale=0), "filter_rounds must be an integer in [0, 4], got 5"),
    (dict(loss="huber", filter_rounds=1, loss_scale=0, max_reproj_error=0), "loss_scale must be > 0 with a robust loss, got 0"),
    (dict(filter_rounds=1, max_reproj_error=0, num_iterations=0), "max_reproj_error must be > 0 with filter_rounds > 0, got 0"),
    (dict(num_iterations=0, initial_damping=0), "num_iterations must be an integer in [1, 100], got 0"),
    (dict(initial_damping=0, function_tolerance=0), "initial_damping must be > 0, got 0"),
]) + rows((GlobalPoseEstimator, GlobalPositioner), [
    (dict(num_iterations=6), dict(num_iterations=6)),
    (dict(num_iterations=100), dict(num_iterations=100)),
    (dict(num_iterations=7.0), dict(num_iterations=7)),
    (dict(num_iterations=5), "num_iterations must be an integer in [6, 100], got 5"),
    (dict(num_iterations=101), "num_iterations must be an integer in [6, 100], got 101"),
    (dict(num_iterations=True), "num_iterations must be an integer in [6, 100], got True"),
    (dict(num_iterations="7"), "num_iterations must be an integer in [6, 100], got '7'"),
]) + rows((GlobalPoseEstimator,), [
    (dict(), dict(num_iterations=12, rotation_scale=5.0, max_rotation_error=15.0, direction_scale=5.0, min_inliers=15)),
    (dict(rotation_scale=True, max_rotation_error=1, direction_scale=1e-300), dict(rotation_scale=1.0, max_rotation_error=1.0, direction_scale=1e-300)),
    (dict(min_inliers=0), dict(min_inliers=0)),
    (dict(min_inliers=2 ** 31 - 1), dict(min_inliers=2 ** 31 - 1)),
    (dict(min_inliers=3.0), dict(min_inliers=3)),
    (dict(rotation_scale=0), "rotation_scale must be > 0 degrees, got 0"),
    (dict(rotation_scale=NAN), "rotation_scale must be > 0 degrees, got nan"),
    (dict(max_rotation_error=INF), "max_rotation_error must be > 0 degrees, got inf"),
    (dict(max_rotation_error=-1.0), "max_rotation_error must be > 0 degrees, got -1.0"),
    (dict(direction_scale=0.0), "direction_scale must be > 0 degrees, got 0.0"),
    (dict(direction_scale=NAN), "direction_scale must be > 0 degrees, got nan"),
    (dict(min_inliers=-1), "min_inliers must be an integer >= 0, got -1"),
    (dict(min_inliers=2 ** 31), "min_inliers must be an integer >= 0, got 2147483648"),
    (dict(min_inliers=True), "min_inliers must be an integer >= 0, got True"),
    (dict(min_inliers="3"), "min_inliers must be an integer >= 0, got '3'"),
    (dict(min_inliers=1.5), "min_inliers must be an integer >= 0, got 1.5"),
    (dict(num_iterations=5, rotation_scale=0), "num_iterations must be an integer in [6, 100], got 5"),
    (dict(rotation_scale=0, max_rotation_error=0), "rotation_scale must be > 0 degrees, got 0"),
    (dict(max_rotation_error=0, direction_scale=0), "max_rotation_error must be > 0 degrees, got 0"),
    (dict(direction_scale=0, min_inliers=-1), "direction_scale must be > 0 degrees, got 0"),
]) + rows((GlobalPositioner,), [
    (dict(), dict(num_iterations=12, angle_scale=1.0, max_angle_error=2.0)),
    (dict(angle_scale=True, max_angle_error=1e-300), dict(angle_scale=1.0, max_angle_error=1e-300)),
    (dict(angle_scale=0), "angle_scale must be > 0 degrees, got 0"),
    (dict(angle_scale=NAN), "angle_scale must be > 0 degrees, got nan"),
    (dict(angle_scale=INF), "angle_scale must be > 0 degrees, got inf"),
    (dict(max_angle_error=0.0), "max_angle_error must be > 0 degrees, got 0.0"),
    (dict(max_angle_error=NAN), "max_angle_error must be > 0 degrees, got nan"),
    (dict(max_angle_error=INF), "max_angle_error must be > 0 degrees, got inf"),
    (dict(num_iterations=5, angle_scale=0), "num_iterations must be an integer in [6, 100], got 5"),
    (dict(angle_scale=0, max_angle_error=0), "angle_scale must be > 0 degrees, got 0"),
])


@pytest.mark.parametrize("cls, kwargs, want", SETTINGS)
def test_constructor_settings(cls, kwargs, want):
    if isinstance(want, str):
        with pytest.raises(ValueError) as err:
            cls(**kwargs)
        assert str(err.value) == want
    else:
        obj = cls(**kwargs)
        got = {k: getattr(obj, k) for k in want}
        assert got == want and {k: type(v) for k, v in got.items()} == {k: type(v) for k, v in want.items()}


# ---------------------------------------------------------------------- GlobalPoseEstimator.estimate: its own arguments, refused before the device is asked for
def _estimate(**kwargs):
    args = dict(pairs=[[0, 1], [1, 2]], relative=(torch.eye(3).expand(2, 3, 3), torch.ones(2, 3)), num_images=3)
    return GlobalPoseEstimator().estimate(**{**args, **kwargs})


@pytest.mark.parametrize("kwargs, want", [
    (dict(), NO_GPU),                                                       # everything accepted: the next refusal is the device's
    (dict(num_images=2, pairs=[[0, 1]], relative=(torch.eye(3)[None], torch.ones(1, 3))), NO_GPU),
    (dict(num_images=256, origin=255, baseline=0), NO_GPU),
    (dict(num_images=3.0, origin=1.0, baseline=2.0), NO_GPU),
    (dict(origin=2, baseline=None, weights=torch.ones(2, dtype=torch.float64)), NO_GPU),
    (dict(pairs=[0, 1]), "pairs must be [P, 2] integers, got (2,) torch.int64"),
    (dict(pairs=[[0.0, 1.0]]), "pairs must be [P, 2] integers, got (1, 2) torch.float32"),
    (dict(pairs=torch.zeros(1, 2, dtype=torch.bool)), "pairs must be [P, 2] integers, got (1, 2) torch.bool"),
    (dict(num_images=1), "num_images must be an integer in [2, 256], got 1"),
    (dict(num_images=257), "num_images must be an integer in [2, 256], got 257"),
    (dict(num_images=True), "num_images must be an integer in [2, 256], got True"),
    (dict(num_images=2.5), "num_images must be an integer in [2, 256], got 2.5"),
    (dict(num_images="3"), "num_images must be an integer in [2, 256], got '3'"),
    (dict(pairs=torch.zeros(0, 2, dtype=torch.int64)), "the pair list must hold between 1 and 1048576 pairs, got 0"),
    (dict(origin=-1), "origin must name an image in [0, 3), got -1"),
    (dict(origin=3), "origin must name an image in [0, 3), got 3"),
    (dict(origin=True), "origin must name an image in [0, 3), got True"),
    (dict(origin=0.5), "origin must name an image in [0, 3), got 0.5"),
    (dict(origin="1"), "origin must name an image in [0, 3), got '1'"),
    (dict(baseline=0), "baseline must be None or an image in [0, 3) other than origin, got 0"),
    (dict(origin=1.0, baseline=1), "baseline must be None or an image in [0, 3) other than origin, got 1"),
    (dict(baseline=3), "baseline must be None or an image in [0, 3) other than origin, got 3"),
    (dict(baseline=-1), "baseline must be None or an image in [0, 3) other than origin, got -1"),
    (dict(baseline=True), "baseline must be None or an image in [0, 3) other than origin, got True"),
    (dict(baseline="1"), "baseline must be None or an image in [0, 3) other than origin, got '1'"),
    (dict(weights=torch.ones(3)), "weights must be a [2] float tensor, got (3,) torch.float32"),
    (dict(weights=[1, 2]), "weights must be a [2] float tensor, got (2,) torch.int64"),
    (dict(pairs=[0, 1], num_images=1), "pairs must be [P, 2] integers, got (2,) torch.int64"),                      # the order of the refusals
    (dict(num_images=1, pairs=torch.zeros(0, 2, dtype=torch.int64)), "num_images must be an integer in [2, 256], got 1"),
    (dict(pairs=torch.zeros(0, 2, dtype=torch.int64), origin=9), "the pair list must hold between 1 and 1048576 pairs, got 0"),
    (dict(origin=9, baseline=9), "origin must name an image in [0, 3), got 9"),
    (dict(baseline=9, relative=None), "baseline must be None or an image in [0, 3) other than origin, got 9"),
    (dict(relative=None, weights=[1, 2]), "relative must be RelativePoseEstimator's dict or a tuple (R [P, 3, 3], t [P, 3])"),
])
def test_estimate_arguments(kwargs, want):
    with pytest.raises(RuntimeError if want is NO_GPU else ValueError) as err:
        _estimate(**kwargs)
    assert str(err.value) == want


# ---------------------------------------------------------------------- the readers
K3 = torch.tensor([[[500.0, 0, 320], [0, 510, 240], [0, 0, 1]]])
R2, T2 = torch.eye(3).expand(2, 3, 3), torch.tensor([[1.0, 2, 3], [4, 5, 6]])
TID = torch.tensor([[0, -1, 1, 1], [0, 1, -1, -1]])
XYZ = torch.zeros(2, 3, dtype=torch.float64)


def same(want):
    """a good form's check: the same values, dtype and shape, contiguous"""
    want = torch.as_tensor(want)
    return lambda got: torch.equal(got, want) and got.dtype is want.dtype and got.is_contiguous()


def each(*checks):
    return lambda got: len(got) == len(checks) and all(c(g) if callable(c) else (g == c and type(g) is type(c)) for c, g in zip(checks, got))


READERS = [
    ("as_cameras", (K3, 1, "cpu"), same(torch.tensor([[500.0, 510, 320, 240]]))),
    ("as_cameras", ([[500, 510, 320, 240]], 1, "cpu"), same(torch.tensor([[500.0, 510, 320, 240]]))),
    ("as_cameras", (torch.ones(2, 4, dtype=torch.float64).t().contiguous().t(), 2, "cpu"), same(torch.ones(2, 4))),
    ("as_cameras", (K3 + torch.tensor([[[0.0, 1e-9, 0], [0, 0, 0], [0, 0, 0]]]).double(), 1, "cpu"), "cameras: calibration matrices must have zero skew and a last row of (0, 0, 1)"),
    ("as_cameras", (K3 * 2, 1, "cpu", "cameras1"), "cameras1: calibration matrices must have zero skew and a last row of (0, 0, 1)"),
    ("as_cameras", (K3, 2, "cpu"), "cameras must have shape [2, 4] (fx, fy, cx, cy) or [2, 3, 3], got (1, 4)"),
    ("as_cameras", (torch.ones(2, 5), 2, "cpu", "cameras0"), "cameras0 must have shape [2, 4] (fx, fy, cx, cy) or [2, 3, 3], got (2, 5)"),
    ("as_cameras", (torch.ones(4), 1, "cpu"), "cameras must have shape [1, 4] (fx, fy, cx, cy) or [1, 3, 3], got (4,)"),
    ("as_poses", ((R2, T2), 2, "cpu"), same(torch.cat([R2, T2[:, :, None]], 2))),
    ("as_poses", ([R2.double(), T2.tolist()], 2, "cpu"), same(torch.cat([R2, T2[:, :, None]], 2))),
    ("as_poses", (torch.ones(2, 4, 3, dtype=torch.float64).transpose(1, 2), 2, "cpu"), same(torch.ones(2, 3, 4))),
    ("as_poses", ((R2, T2[:1]), 2, "cpu"), "poses (R, t) must have shapes [2, 3, 3] and [2, 3], got (2, 3, 3) and (1, 3)"),
    ("as_poses", ((R2[:, :2], T2), 2, "cpu"), "poses (R, t) must have shapes [2, 3, 3] and [2, 3], got (2, 2, 3) and (2, 3)"),
    ("as_poses", (torch.ones(2, 4, 4), 2, "cpu"), "poses must have shape [2, 3, 4] (R | t) or be a tuple (R [2, 3, 3], t [2, 3]), got (2, 4, 4)"),
    ("as_poses", (torch.ones(3, 3, 4), 2, "cpu"), "poses must have shape [2, 3, 4] (R | t) or be a tuple (R [2, 3, 3], t [2, 3]), got (3, 3, 4)"),
    ("as_track_id", (TID, 2, 4, "cpu"), same(TID)),
    ("as_track_id", (TID.to(torch.int16).tolist(), 2, 4, "cpu"), same(TID)),
    ("as_track_id", (TID.to(torch.uint8), 2, 4, "cpu"), same(TID.to(torch.uint8).long())),
    ("as_track_id", (TID, 4, 2, "cpu"), "track_id must have shape [4, 2], got (2, 4)"),
    ("as_track_id", (TID.float(), 2, 4, "cpu"), "track_id must hold integers, got torch.float32"),
    ("as_track_id", (TID > 0, 2, 4, "cpu"), "track_id must hold integers, got torch.bool"),
    ("as_tracks", ({"track_id": TID, "xyz": XYZ, "more": 1}, 2, 4, "cpu"), each(same(TID), same(XYZ.float()))),
    ("as_tracks", ([TID.int(), XYZ.tolist()], 2, 4, "cpu"), each(same(TID), same(XYZ.float()))),
    ("as_tracks", ((TID, torch.zeros(4, 3)), 2, 4, "cpu"), each(same(TID), same(torch.zeros(4, 3)))),          # K N / 2 tracks: the most
    ("as_tracks", (TID, 2, 4, "cpu"), "tracks must be the Triangulator's dict or a tuple (track_id [K, N], xyz [T, 3])"),
    ("as_tracks", ((TID, XYZ, XYZ), 2, 4, "cpu"), "tracks must be the Triangulator's dict or a tuple (track_id [K, N], xyz [T, 3])"),
    ("as_tracks", ((TID.float(), torch.zeros(3)), 2, 4, "cpu"), "track_id must hold integers, got torch.float32"),      # the labels' refusal comes first
    ("as_tracks", ((TID, torch.zeros(3)), 2, 4, "cpu"), "xyz must have shape [T, 3], got (3,)"),
    ("as_tracks", ((TID, torch.zeros(2, 4)), 2, 4, "cpu"), "xyz must have shape [T, 3], got (2, 4)"),
    ("as_tracks", ((TID, torch.zeros(5, 3)), 2, 4, "cpu"), "xyz holds 5 tracks: more than K N / 2 = 4 (a track has at least two observations)"),
    ("as_labels", ({"track_id": TID, "num_tracks": 2}, 2, 4, "cpu"), each(same(TID), 2)),
    ("as_labels", ([TID.tolist(), 4.0], 2, 4, "cpu"), each(same(TID), 4)),
    ("as_labels", ((TID, 0), 2, 4, "cpu"), each(same(TID), 0)),
    ("as_labels", ((TID, np.int64(3)), 2, 4, "cpu"), each(same(TID), 3)),
    ("as_labels", ({"track_id": TID}, 2, 4, "cpu"), "tracks is a dict without 'num_tracks': pass the Triangulator's dict or a tuple (track_id [K, N], T)"),
    ("as_labels", ({"num_tracks": 2}, 2, 4, "cpu"), "tracks is a dict without 'track_id': pass the Triangulator's dict or a tuple (track_id [K, N], T)"),
    ("as_labels", (TID, 2, 4, "cpu"), "tracks must be the Triangulator's dict or a tuple (track_id [K, N], T)"),
    ("as_labels", ((TID[:1], 2), 2, 4, "cpu"), "track_id must have shape [2, 4], got (1, 4)"),
    ("as_labels", ((TID, 5), 2, 4, "cpu"), "the number of tracks must be an integer in [0, K N / 2 = 4] (a track has at least two observations), got 5"),
    ("as_labels", ((TID, -1), 2, 4, "cpu"), "the number of tracks must be an integer in [0, K N / 2 = 4] (a track has at least two observations), got -1"),
    ("as_labels", ((TID, True), 2, 4, "cpu"), "the number of tracks must be an integer in [0, K N / 2 = 4] (a track has at least two observations), got True"),
    ("as_labels", ((TID, 1.5), 2, 4, "cpu"), "the number of tracks must be an integer in [0, K N / 2 = 4] (a track has at least two observations), got 1.5"),
    ("as_labels", ((TID, torch.tensor(2)), 2, 4, "cpu"), "the number of tracks must be an integer in [0, K N / 2 = 4] (a track has at least two observations), got tensor(2)"),
    ("as_constant", ([True, False, True], 3), same(torch.tensor([True, False, True]))),
    ("as_constant", ([2, 0, 2], 3), same(torch.tensor([True, False, True]))),
    ("as_constant", (torch.tensor([1], dtype=torch.int32), 3), same(torch.tensor([False, True, False]))),
    ("as_constant", ([], 3, "constant_camera"), same(torch.zeros(3, dtype=torch.bool))),
    ("as_constant", (torch.zeros(3, dtype=torch.bool), 3, "constant_camera"), same(torch.zeros(3, dtype=torch.bool))),
    ("as_constant", ([], 3), "constant_pose holds no image: nothing fixes the gauge (hold at least one pose; two fix scale as well)"),
    ("as_constant", ([False] * 3, 3), "constant_pose holds no image: nothing fixes the gauge (hold at least one pose; two fix scale as well)"),
    ("as_constant", ([0.0, 1.0], 3), "constant_pose must be a [K] bool mask or a sequence of image indices"),
    ("as_constant", ([[0, 1]], 3, "constant_camera"), "constant_camera must be a [K] bool mask or a sequence of image indices"),
    ("as_constant", ([0, 3], 3), "constant_pose names an image outside [0, 3)"),
    ("as_constant", ([-1], 3, "constant_camera"), "constant_camera names an image outside [0, 3)"),
    ("as_constant", ([True, False], 3), "constant_pose must have shape [3], got (2,)"),
    ("as_constant", ([[True, False, True]], 3, "constant_camera"), "constant_camera must have shape [3], got (1, 3)"),
    ("as_relative", ((R2, T2), 2), each(lambda g: g is R2, lambda g: g is T2, lambda g: g is None)),                # nothing moved
    ("as_relative", ([R2.tolist(), T2.tolist()], 2), each(same(R2), same(T2), lambda g: g is None)),
    ("as_relative", ({"R": R2, "t": T2, "num_inliers": [5, 0], "E": None}, 2), each(lambda g: g is R2, lambda g: g is T2, same(torch.tensor([5, 0])))),
    ("as_relative", ({"R": R2, "t": T2}, 2), "relative is a dict without 'num_inliers': pass RelativePoseEstimator's dict or a tuple (R [P, 3, 3], t [P, 3])"),
    ("as_relative", ({"t": T2, "num_inliers": [5, 0]}, 2), "relative is a dict without 'R': pass RelativePoseEstimator's dict or a tuple (R [P, 3, 3], t [P, 3])"),
    ("as_relative", ((R2, T2, None), 2), "relative must be RelativePoseEstimator's dict or a tuple (R [P, 3, 3], t [P, 3])"),
    ("as_relative", (R2, 2), "relative must be RelativePoseEstimator's dict or a tuple (R [P, 3, 3], t [P, 3])"),
    ("as_relative", ((R2, T2), 3), "R must have shape [3, 3, 3], got (2, 3, 3)"),
    ("as_relative", ((R2, T2[:, :2]), 2), "t must have shape [2, 3], got (2, 2)"),
    ("as_relative", ({"R": R2, "t": T2, "num_inliers": [5]}, 2), "num_inliers must hold [2] integers, got (1,) torch.int64"),
    ("as_relative", ({"R": R2, "t": T2, "num_inliers": [5.0, 1.0]}, 2), "num_inliers must hold [2] integers, got (2,) torch.float32"),
    ("as_relative", ({"R": R2, "t": T2, "num_inliers": [True, False]}, 2), "num_inliers must hold [2] integers, got (2,) torch.bool"),
]


@pytest.mark.parametrize("name, args, want", [pytest.param(*row, id=f"{row[0]}-{i}") for i, row in enumerate(READERS)])
def test_readers(name, args, want):
    reader = getattr(readers, name)
    if isinstance(want, str):
        with pytest.raises(ValueError) as err:
            reader(*args)
        assert str(err.value) == want
    else:
        assert want(reader(*args))


# ---------------------------------------------------------------------- the helpers of `_call` the wrappers are written over
def test_helper_int_in():
    assert _call.int_in("n", 3, 3, 5) == 3 and _call.int_in("n", 5.0, 3, 5) == 5 and type(_call.int_in("n", 5.0, 3, 5)) is int
    assert _call.int_in("n", True, 1, 5) == 1 and type(_call.int_in("n", True, 1, 5)) is int and _call.int_in("n", np.int32(4), 3, 5, True) == 4
    for value, refuse_bool, shown in ((2, False, "2"), (6, False, "6"), (3.5, False, "3.5"), ("3", False, "'3'"), (True, True, "True"), (True, False, "True")):
        with pytest.raises(ValueError) as err:
            _call.int_in("n", value, 3, 5, refuse_bool)
        assert str(err.value) == f"n must be an integer in [3, 5], got {shown}"
    with pytest.raises(ValueError) as err:
        _call.int_in("origin", 7, 0, 2, True, "must name an image in [0, 3)")
    assert str(err.value) == "origin must name an image in [0, 3), got 7"
    for value, error in ((NAN, ValueError), (INF, OverflowError), (None, TypeError), ("x", ValueError)):      # what int() itself says is not rewritten
        with pytest.raises(error):
            _call.int_in("n", value, 3, 5)


def test_helper_positive():
    assert _call.positive("x", 1e-300) == 1e-300 and _call.positive("x", "2.5") == 2.5
    assert _call.positive("x", True) == 1.0 and type(_call.positive("x", True)) is float and type(_call.positive("x", 3)) is float
    for value, shown in ((0, "0"), (-0.0, "-0.0"), (-1.5, "-1.5"), (NAN, "nan"), (INF, "inf"), (-INF, "-inf")):
        with pytest.raises(ValueError) as err:
            _call.positive("x", value)
        assert str(err.value) == f"x must be > 0, got {shown}"
    with pytest.raises(ValueError) as err:
        _call.positive("angle_scale", 0, " degrees")
    assert str(err.value) == "angle_scale must be > 0 degrees, got 0"


def test_helper_status_error_of_images():
    from lightglue_amd.bundle import IMAGE_STATUS
    out = {"poses": torch.zeros(3, 3, 4)}
    ok = np.zeros(3, np.int32)
    assert _call.raise_with_outputs(ok.tolist(), out, "image", IMAGE_STATUS) is out
    with pytest.raises(_cabi.LightGlueAmdError) as err:
        _call.raise_with_outputs([_cabi.LG_OK, _cabi.LG_ERR_CAMERA, _cabi.LG_OK, _cabi.LG_ERR_CAMERA], out, "image", IMAGE_STATUS)
    assert err.value.outputs is out
    assert str(err.value) == ("image 1: a camera whose focal length is not finite and > 0, whose principal point is not finite, or a non-finite pose (LG_ERR_CAMERA): "
                              "its observations were left out; "
                              "image 3: a camera whose focal length is not finite and > 0, whose principal point is not finite, or a non-finite pose (LG_ERR_CAMERA): "
                              "its observations were left out")
    with pytest.raises(_cabi.LightGlueAmdError) as err:
        _call.raise_on_status([_cabi.LG_ERR_CAMERA] * 9, "image", IMAGE_STATUS)
    assert str(err.value).count("image ") == 8 and not hasattr(err.value, "outputs")                        # the first eight are named
    with pytest.raises(_cabi.LightGlueAmdError) as err:
        _call.raise_on_status([_cabi.LG_ERR_CAMERA])                                                        # the default is the pair's table
    assert str(err.value) == "pair 0: a camera whose focal length is not finite and > 0, or whose principal point is not finite (LG_ERR_CAMERA)"


def test_helper_index_ptrs_and_device_index():
    assert _call.index_ptrs(None) == (None, None)
    index = torch.arange(6, dtype=torch.int32).reshape(2, 3)
    assert _call.index_ptrs(index) == (index.data_ptr(), index.data_ptr() + 12)
    pt = torch.tensor([[0, 1], [2, 3], [4, 5]])
    got = _call.device_index(pt, torch.device("cpu"))
    assert got.dtype is torch.int32 and got.is_contiguous() and got.tolist() == [[0, 2, 4], [1, 3, 5]]
    assert _call.device_index(pt[:0], torch.device("cpu")) is None
    same_store, P, index = _call.store_pairs({"keypoints": torch.zeros(6, 4, 2)}, pt, None, True)          # store_pairs hands out the same index
    assert same_store and P == 3 and torch.equal(index, got)


def test_helper_summary_status():
    status, summary_ptr, status_ptr, read = _call.summary_status(12, 5, torch.device("cpu"))
    assert status.dtype is torch.int32 and tuple(status.shape) == (5,) and status_ptr == status.data_ptr() == summary_ptr + 96 and summary_ptr % 8 == 0
    summary, host_status = read()
    assert summary.dtype == np.float64 and summary.shape == (12,) and not summary.any() and host_status.dtype == np.int32 and host_status.tolist() == [0] * 5
    ctypes.c_double.from_address(summary_ptr + 8).value = 2.5                        # what a call writes through the two addresses
    ctypes.c_int32.from_address(status_ptr + 12).value = _cabi.LG_ERR_CAMERA
    summary, host_status = read()
    assert summary.tolist() == [0, 2.5] + [0] * 10 and host_status.tolist() == [0, 0, 0, _cabi.LG_ERR_CAMERA, 0] and status.tolist() == host_status.tolist()
    empty, summary_ptr, status_ptr, _ = _call.summary_status(8, 0, torch.device("cpu"))                    # the positioner's eight doubles
    assert status_ptr - summary_ptr == 64 and empty.numel() == 0
