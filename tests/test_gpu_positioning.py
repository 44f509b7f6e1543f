"""GlobalPositioner on the GPU against the float64 definition (tests/positioning_oracle.py), against itself, and in the chain it exists for.

Bars and where they come from (those of tests/test_gpu_posegraph.py and tests/test_gpu_bundle.py):
  Node states, image states, statuses, the returned labels, the counts and `positions_ok` are integers: they equal the oracle's exactly.  The iteration count
  is compared wherever the oracle does not mark the stop test as decided by fp64 rounding (`near`: the tested step is rounding, it changes when the oracle
  swaps its solver, and lies within 100 x of the bar 1e-12; tests/posegraph_oracle.py has the reasoning).
  R comes back as the bits that went in.  A translation entry may differ from the oracle's fp64 value by ONE float32 ulp of the scale (the largest coordinate
  magnitude among t and the image's centre), a point coordinate by one float32 ulp of the point's largest coordinate magnitude: both sides are fp64, each
  value is rounded to float32 once, and the two differ in the order of their sums only.  points3d holds the bits of xyz.
  angle_error: one float32 ulp of the error, plus what the oracle itself cannot hold: ANGLE_FLOOR = 1e-12 degrees (an angle between two fp64 directions carries
  their rounding) and OWN_MARGIN x the largest amount by which the error moves when the oracle solves its systems by LU in place of the Cholesky.
The scenes are those of tests/positioning_oracle.py: cameras on an arc around a box, planted tracks with 0.5 px of noise, the first and the last image held,
every free image's rotation turned by up to 0.3 degrees (what rotation averaging leaves)."""
import numpy as np
import pytest
import torch

import positioning_oracle as P
import posegraph_oracle as G
import triangulate_oracle as O
import lightglue_amd
from lightglue_amd import BundleAdjuster, GlobalPoseEstimator, GlobalPositioner, RelativePoseEstimator, Triangulator

ANGLE_FLOOR, OWN_MARGIN = 1e-12, 100.0
INT_KEYS = ("num_posed", "num_points", "num_outliers", "num_degenerate", "iterations", "positions_ok")
BIT_KEYS = ("poses", "xyz", "points3d", "track_id", "node_state", "image_state", "angle_error", "status") + INT_KEYS
# the chain: final cost per observation of the adjusted reconstruction started from the positioner's (track_id, xyz) and poses over that of the existing chain
# (Triangulator(max_reproj_error=64) on the estimator's poses, then the adjuster), both with origin and baseline held at the SAME two poses.  The two minimise
# one cost from two starts, so the ratio is 1 where both keep the same observations and both get there in 20 iterations.  Measured on the first run: 1.0000
# (1477.44 over 499 observations of 110 tracks on either side; the positioner's start costs 1773.4, the triangulated one 28547.2; profiles/global_positioning.md).
# Asserted with 5 %: what a side may still be short of the minimum when the adjuster stops at function_tolerance, and an observation either side may drop
CHAIN_MARGIN = 1.05

pytestmark = pytest.mark.gpu


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(inp, **kw):
    feats = {"keypoints": cuda(inp["kpts"])}
    if inp.get("num") is not None:
        feats["num_keypoints"] = cuda(np.asarray(inp["num"], np.int32))
    out = GlobalPositioner(**kw).solve(feats, (cuda(inp["track_id"]), inp["T"]), cuda(inp["cams"]), cuda(inp["poses"]), torch.from_numpy(np.asarray(inp["held"])))
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}


def check(got, want, inp, what, max_iterations=12):
    for k in INT_KEYS:
        if k == "num_degenerate":
            assert got[k] == int((np.unique(inp["track_id"][want["node_state"] == P.DEGENERATE])).size), (what, k)
        elif k == "iterations" and want["near"]:
            assert 1 <= got[k] <= max_iterations, (what, k, got[k])
        else:
            assert got[k] == want[k], (what, k, got[k], want[k])
    for k in ("node_state", "image_state", "status", "track_id"):
        assert (got[k] == want[k]).all(), (what, k, np.flatnonzero((got[k] != want[k]).ravel())[:8])
    P64 = want["poses64"]
    assert (np.isnan(got["poses"]) == np.isnan(P64)).all(), what
    ok = want["status"] == 0
    assert np.array_equal(got["poses"][ok, :, :3], np.asarray(inp["poses"], np.float32)[ok, :, :3]), what              # R: the bits that went in
    held = want["image_state"] == P.HELD
    assert np.array_equal(got["poses"][held], np.asarray(inp["poses"], np.float32)[held]), what
    posed = want["image_state"] == P.POSED
    scale = np.maximum(abs(P64[posed, :, 3]).max(1), abs(want["centres64"][posed]).max(1)) if posed.any() else np.ones(0)
    tu = np.array([O.ulp32(s) for s in scale])
    dt = abs(got["poses"][posed, :, 3] - P64[posed, :, 3]).max(1) if posed.any() else np.zeros(0)
    X64 = want["xyz64"]
    assert (np.isnan(got["xyz"]) == np.isnan(X64)).all(), what
    has = ~np.isnan(X64[:, 0])
    xu = np.array([O.ulp32(s) for s in abs(X64[has]).max(1)])
    dx = abs(got["xyz"][has] - X64[has]).max(1) if has.any() else np.zeros(0)
    inl = got["node_state"] == P.INLIER
    assert np.array_equal(got["points3d"][inl], got["xyz"][got["track_id"][inl]]) and np.isnan(got["points3d"][~inl]).all(), what
    w64 = want["angle_error64"]
    assert (np.isnan(got["angle_error"]) == np.isnan(w64)).all(), what
    m = ~np.isnan(w64)
    bar = np.array([O.ulp32(e) for e in w64[m]]) + ANGLE_FLOOR + OWN_MARGIN * want["own"]
    da = abs(got["angle_error"][m].astype(np.float64) - w64[m]) / bar if m.any() else np.zeros(1)
    print("%s: worst / bar: t %.3f, xyz %.3f, angle_error %.3f; %d posed, %d points, %d outliers, %d iterations (oracle %d, near %s)" % (
        what, float((dt / tu).max()) if posed.any() else 0.0, float((dx / xu).max()) if has.any() else 0.0, float(da.max()), got["num_posed"], got["num_points"],
        got["num_outliers"], got["iterations"], want["iterations"], want["near"]))
    assert (dt <= tu).all() and (dx <= xu).all() and da.max() <= 1.0, what


def same_bits(a, b, what, keys=BIT_KEYS):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True) if isinstance(a[k], np.ndarray) else a[k] == b[k], (what, k)


def sized(K, N, tracks):
    sc = P.scene(K, N, tracks)
    return dict(P.oracle_input(sc), poses=P.noisy_rotations(sc["poses"], 0.3, 17 + K, sc["held"]))


def chain_input():
    sc = G.chain_scene()
    tr = O.triangulate(dict(kpts=sc["kpts"], num=None, pairs=sc["pairs"], matches0=sc["matches0"], cams=sc["cams"], poses=sc["poses"]), tracks_only=True)
    held = np.zeros(6, bool)
    held[[0, 5]] = True
    return dict(kpts=sc["kpts"], num=None, track_id=tr["track_id"], T=tr["num_tracks"], cams=sc["cams"], poses=P.noisy_rotations(sc["poses"], 0.3, 23, held), held=held)


# ---------------------------------------------------------------------- 1. sizes: one Cholesky panel, two with a ragged last one, four and several row tiles
@pytest.mark.parametrize("K", [6, 17, 49])
def test_sizes_match_the_definition(K):
    inp = chain_input() if K == 6 else sized(K, 32, {17: 100, 49: 300}[K])
    want = P.solve(inp)
    assert want["num_posed"] == K and want["positions_ok"] and want["num_points"] == inp["T"]
    check(run(inp), want, inp, "K = %d" % K)


def test_the_envelope_256_images():
    inp = sized(256, 16, 900)
    want = P.solve(inp, num_iterations=6)
    assert want["num_posed"] == 256 and want["positions_ok"]
    check(run(inp, num_iterations=6), want, inp, "K = 256", 6)


def test_more_tracks_than_scan_threads():
    """1030 two-view tracks over 6 x 400 nodes (400 rows per image: 352 would run the planting out of rows): each of the scan's 1024 threads owns
    ceil(1030 / 1024) = 2 consecutive tracks (the last 509 own none), and tracks 500 and 1027 lose one observation each, so two unlisted tracks sit between
    listed ones and their offsets must not move"""
    sc = P.scene(6, 400, 1030, seed=3, lo=2, hi=2)
    tid, left = sc["track_id"].copy(), []
    for j in (500, 1027):
        (k, i), other = sorted(sc["planted"]["rows"][j].items())
        tid[k, i] = -1
        left.append(other)
    inp = dict(P.oracle_input(sc), track_id=tid)
    want = P.solve(inp, num_iterations=6)
    assert inp["T"] == 1030 > 1024 and all(want["node_state"][k, i] == P.PEELED for k, i in left)                # on the definition, before the GPU is read
    assert want["num_posed"] == 6 and want["num_points"] == 1028 and (want["node_state"] == P.PEELED).sum() == 2 and want["positions_ok"]
    check(run(inp, num_iterations=6), want, inp, "1030 tracks", 6)


# ---------------------------------------------------------------------- 2. every edge
def extras_scene():
    """scene(8, 32, 48) with ragged num_keypoints (dead rows that carry labels), four tracks with a second row in one of their images (0.3 px beside the first)
    and rotations turned by up to 0.3 degrees"""
    sc = P.scene(8, 32, 48, seed=1)
    kpts, tid = sc["kpts"].copy(), sc["track_id"].copy()
    num = np.asarray([32, 30, 32, 29, 32, 32, 31, 32])
    rng = np.random.default_rng(5)
    for j in (3, 11, 27, 40):
        k = int(rng.choice(list(sc["planted"]["rows"][j])))
        free = [r for r in range(num[k]) if tid[k, r] < 0]
        kpts[k, free[0]] = kpts[k, sc["planted"]["rows"][j][k]] + np.float32(0.3)
        tid[k, free[0]] = j
    return dict(P.oracle_input(sc), kpts=kpts, track_id=tid, num=num, poses=P.noisy_rotations(sc["poses"], 0.3, 3, sc["held"])), sc


def test_two_rows_in_one_image_and_ragged_keypoint_counts():
    inp, sc = extras_scene()
    want = P.solve(inp)
    dead = np.arange(32)[None, :] >= inp["num"][:, None]
    assert (want["node_state"][dead] == P.NONE).all() and (inp["track_id"][dead] >= 0).any() and want["positions_ok"]
    assert (want["node_state"] == P.INLIER).sum() > (sc["track_id"] >= 0).sum() - dead.sum()          # the second rows are observations
    check(run(inp), want, inp, "two rows in one image, ragged counts")


def test_edge_inputs_follow_the_definition():
    e = P.edge_scene()
    inp = P.oracle_input(e)
    want = P.solve(inp)
    got = run(inp)
    check(got, want, inp, "edge")
    assert set(np.unique(got["node_state"]).tolist()) == {P.NONE, P.INLIER, P.PEELED, P.NOT_CONNECTED, P.DEGENERATE} and got["num_degenerate"] == 1
    assert got["image_state"].tolist() == [P.HELD, P.POSED, P.POSED, P.POSED, P.HELD, P.TOO_FEW_TRACKS, 3, 3, 3]
    bad, clean, planted, _ = P.stray_scene()
    want = P.solve(bad)
    got = run(bad)
    check(got, want, bad, "stray observations")
    assert ((got["node_state"] == P.OUTLIER) == planted).all()


def test_bad_images_leave_everything_else_bit_for_bit():
    inp, _ = extras_scene()
    cams, poses, tid = inp["cams"].copy(), inp["poses"].copy(), inp["track_id"].copy()
    cams[2, 0], poses[5, 1, 1] = 0.0, np.nan
    tid[[2, 5]] = -1
    bad = dict(inp, cams=cams, poses=poses)
    got, ref = run(bad), run(dict(inp, track_id=tid))
    check(got, P.solve(bad), bad, "a bad camera and a NaN rotation")
    assert got["status"].tolist() == [0, 0, 7, 0, 0, 7, 0, 0] and (got["image_state"][[2, 5]] == P.IMG_BAD).all() and np.isnan(got["poses"][[2, 5]]).all()
    rest = [0, 1, 3, 4, 6, 7]
    for k in ("poses", "points3d", "track_id", "node_state", "angle_error", "image_state"):
        assert np.array_equal(got[k][rest], ref[k][rest], equal_nan=True), k
    same_bits(got, ref, "without the two images' labels", ("xyz", "num_points", "num_outliers", "iterations", "positions_ok"))
    # held images at one centre, poses on the device: refused behind the call
    poses = inp["poses"].copy()
    poses[7] = poses[0]
    with pytest.raises(ValueError, match="distinct centres"):
        run(dict(inp, poses=poses))


# ---------------------------------------------------------------------- 3. invariance
def test_outputs_are_the_same_bits():
    inp = sized(17, 32, 100)
    first = run(inp)
    same_bits(first, run(inp), "the same call again")
    perm = np.random.default_rng(9).permutation(inp["T"])
    moved = run(dict(inp, track_id=np.where(inp["track_id"] >= 0, perm[np.clip(inp["track_id"], 0, None)], -1)))
    same_bits(first, moved, "tracks relabelled", ("poses", "points3d", "node_state", "image_state", "angle_error", "status") + INT_KEYS)
    assert np.array_equal(first["xyz"], moved["xyz"][perm], equal_nan=True)
    assert np.array_equal(np.where(first["track_id"] >= 0, perm[np.clip(first["track_id"], 0, None)], -1), moved["track_id"])


# ---------------------------------------------------------------------- 4. the chain this feature exists for
def test_positions_from_tracks_in_the_chain():
    """chain_scene -> RelativePoseEstimator -> GlobalPoseEstimator -> GlobalPositioner -> BundleAdjuster, no Triangulator.triangulate in between, against the
    existing chain run here too.  First run on the device: 32 of 110 tracks within 8 px from the estimator's poses, 110 from the positioner's; 0 outliers; both chains end at 1477.44 over 499
    observations"""
    sc = G.chain_scene()
    K = len(sc["poses"])
    feats, cams, pairs = {"keypoints": cuda(sc["kpts"])}, torch.from_numpy(sc["cams"]), sc["pairs"].tolist()
    rel = RelativePoseEstimator(threshold=3.0, num_hypotheses=512, refine=True, seed=0).estimate_pairs(feats, pairs, cuda(sc["matches0"]), cams)
    est = lightglue_amd.estimate_global_poses(GlobalPoseEstimator(), rel, pairs, K)
    assert est["num_posed"] == K and est["positions_ok"]
    held = [est["origin"], est["baseline"]]
    tracks = Triangulator().build_tracks(feats, pairs, rel)
    pos = lightglue_amd.position_from_tracks(GlobalPositioner(), tracks, feats, cams, est)
    assert pos["poses"].is_cuda and pos["num_posed"] == K and pos["positions_ok"] and pos["image_state"].tolist().count(P.HELD) == 2
    assert torch.equal(pos["poses"][held], est["poses"][held]) and torch.equal(pos["poses"][:, :, :3], est["poses"][:, :, :3])
    kept = {name: Triangulator(max_reproj_error=8.0).triangulate(feats, pairs, rel, cams, poses)["num_tracks"] for name, poses in (("estimated", est["poses"]), ("positioned", pos["poses"]))}
    old = Triangulator(max_reproj_error=64.0).triangulate(feats, pairs, rel, cams, est["poses"])
    before = lightglue_amd.bundle_adjust(BundleAdjuster(num_iterations=20), old, feats, cams, est["poses"], held)
    after = lightglue_amd.bundle_adjust(BundleAdjuster(num_iterations=20), (pos["track_id"], pos["xyz"]), feats, cams, pos["poses"], held)
    per = {"estimated": before["final_cost"] / before["num_observations"], "positioned": after["final_cost"] / after["num_observations"]}
    print("chain: tracks within 8 px: %d from the estimator's poses, %d from the positioner's (%d tracks, %d points, %d outliers); final cost %.6g over %d "
          "observations (start %.6g) from the positioner, %.6g over %d (start %.6g) from the existing chain: per observation %.4f against %.4f, ratio %.4f" % (
              kept["estimated"], kept["positioned"], tracks["num_tracks"], pos["num_points"], pos["num_outliers"], after["final_cost"], after["num_observations"],
              after["initial_cost"], before["final_cost"], before["num_observations"], before["initial_cost"], per["positioned"], per["estimated"],
              per["positioned"] / per["estimated"]))
    assert kept["positioned"] >= kept["estimated"]
    assert per["positioned"] <= CHAIN_MARGIN * per["estimated"]
