"""BundleAdjuster on the GPU against the float64 definition (tests/bundle_oracle.py) and against itself.

Bars and where they come from (tests/test_bundle_cpu.py derives every figure without a GPU, from the oracle alone on the inputs of this file):
  Observations, node states, iterations run, steps accepted, `converged` and the per-image status are integers: they equal the oracle's exactly.
  A pose entry, a point and a row of points3d may differ from the oracle's fp64 value by ONE float32 ulp of the scale: for a point the largest coordinate
  magnitude among the point and the centres of the cameras that see it (the triangulator's scale, about 100 here: 7.6e-6), for t the same over the image's
  centre and t, for R 1.  Both sides are fp64 and each value is rounded to float32 once; the oracle itself moves by at most
  Q_POINT    3.54e-08  of that ulp on points
  Q_T        2.82e-07  on t
  Q_R        1.69e-07  on R
  between its Schur + Cholesky solver and ONE np.linalg.solve on the full damped system and between ascending and descending accumulation, on every scene of
  this file; the CPU test asserts all three are below 1e-3: the precondition of the one-ulp bar.
  Costs agree within 1e-9 relative; observation_error within one float32 ulp of the error.
  A call whose oracle run places a decision (accept / reject, convergence, a pivot, pz = 0) within a relative 1e-9 of its bar could be excluded; the CPU test
  asserts the oracle marks NONE on these scenes, so none is.
The scenes are those of tests/bundle_oracle.py: the triangulator's recipe (640 x 480 images, camera (500, 500, 320, 240), cameras about 6 units from a box
centred at (100, -50, 20), pixel noise 0.5), free poses off by about 0.01 rad and 0.03 units, points by 0.03 units."""
import numpy as np
import pytest
import torch

import bundle_oracle as B
import triangulate_oracle as O
import lightglue_amd
from lightglue_amd import AbsolutePoseEstimator, BundleAdjuster, Triangulator
from lightglue_amd._cabi import LightGlueAmdError

Q_POINT, Q_T, Q_R = 3.54e-8, 2.82e-7, 1.69e-7
INT_KEYS = ("num_observations", "num_iterations", "num_accepted", "converged")
BIT_KEYS = ("poses", "xyz", "points3d", "node_state", "observation_error", "initial_cost", "final_cost") + INT_KEYS

pytestmark = pytest.mark.gpu


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(inp, expect=None, **conf):
    """one call -> host outputs; expect: the words the call's error must hold (then the error's outputs come back)"""
    feats = {"keypoints": cuda(inp["kpts"])}
    if inp.get("num") is not None:
        feats["num_keypoints"] = torch.as_tensor(np.asarray(inp["num"]), dtype=torch.int32)
    call = lambda: BundleAdjuster(**conf).adjust(feats, (cuda(inp["track_id"]), cuda(inp["xyz"])), torch.from_numpy(inp["cams"]), cuda(inp["poses"]),
                                                 torch.from_numpy(inp["constant"]))
    if expect is None:
        out = call()
    else:
        with pytest.raises(LightGlueAmdError) as err:
            call()
        for word in expect:
            assert word in str(err.value), (word, str(err.value))
        out = err.value.outputs
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}


def check(got, want, inp, what):
    assert want["near"] == [], (what, want["near"])
    for k in INT_KEYS:
        assert got[k] == want[k], (what, k, got[k], want[k])
    assert (got["node_state"] == want["node_state"]).all(), (what, np.argwhere(got["node_state"] != want["node_state"])[:8])
    assert (got["status"] == want["status"]).all(), (what, got["status"])
    for k in ("initial_cost", "final_cost"):
        assert abs(got[k] - want[k]) <= 1e-9 * want[k], (what, k, got[k], want[k])
    track, image = B.scales(inp, want)
    pu, tu = np.array([O.ulp32(s) for s in track]), np.array([O.ulp32(s) for s in image])
    adj = want["adjusted"]
    dx = abs(got["xyz"].astype(np.float64) - want["xyz64"]).max(1)
    dt = abs(got["poses"][:, :, 3].astype(np.float64) - want["poses64"][:, :, 3]).max(1)
    dr = abs(got["poses"][:, :, :3].astype(np.float64) - want["poses64"][:, :, :3]).max()
    print("%s: worst / ulp: points %.3f, t %.3f, R %.3f; cost %.9g -> %.9g in %d iterations" % (
        what, float((dx[adj] / pu[adj]).max()), float((dt / tu).max()), dr / O.ulp32(1.0), got["initial_cost"], got["final_cost"], got["num_iterations"]))
    assert (dx[adj] <= pu[adj]).all() and (dt <= tu).all() and dr <= O.ulp32(1.0), what
    # what is not adjusted / not free comes back as the bits that went in
    assert np.array_equal(got["xyz"][~adj], inp["xyz"][~adj], equal_nan=True) and np.array_equal(got["poses"][~want["free"]], inp["poses"][~want["free"]], equal_nan=True)
    active = want["node_state"] == B.ACTIVE
    tid = np.asarray(inp["track_id"])
    dp = abs(got["points3d"][active].astype(np.float64) - want["points3d64"][active]).max(1)
    assert (dp <= pu[tid[active]]).all() and np.isnan(got["points3d"][~active]).all(), what
    assert (got["points3d"][active] == got["xyz"][tid[active]]).all(), what
    de = abs(got["observation_error"][active].astype(np.float64) - want["error64"][active])
    assert (de <= np.array([O.ulp32(e) for e in want["error64"][active]])).all() and np.isnan(got["observation_error"][~active]).all(), what


def same_bits(a, b, what, keys=BIT_KEYS):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True) if isinstance(a[k], np.ndarray) else a[k] == b[k], (what, k)


@pytest.fixture(scope="module")
def main():
    return run(B.GPU_SCENES["main"]())


# ---------------------------------------------------------------------- 1. the main scene
def test_main_scene_matches_the_definition(main):
    want = B.answer("main")
    check(main, want, B.GPU_SCENES["main"](), "main")
    assert main["num_observations"] == 212 and main["converged"] and main["final_cost"] < 0.05 * main["initial_cost"]


# ---------------------------------------------------------------------- 2. every edge in one scene
def test_edge_inputs_leave_everything_else_untouched():
    bad, clean, what = B.edge_scene()
    got = run(bad, expect=("LG_ERR_CAMERA", "image %d" % what["bad_image"]))
    check(got, B.answer("edge"), bad, "edge")
    assert got["status"].tolist() == [0, 0, 0, B.LG_ERR_CAMERA, 0, 0, 0]
    assert set(np.unique(got["node_state"]).tolist()) == {B.NONE, B.ACTIVE, B.BAD_IMAGE, B.NON_FINITE, B.BEHIND, B.SHORT}
    alone = run(clean)                                                   # the same call without the bad entries: no status, no error
    check(alone, B.answer("edge clean"), clean, "edge clean")
    same_bits(got, alone, "edge against clean", ("poses", "xyz", "initial_cost", "final_cost") + INT_KEYS)
    for k in ("points3d", "observation_error"):
        assert np.array_equal(got[k], alone[k], equal_nan=True), k
    assert ((got["node_state"] == B.ACTIVE) == (alone["node_state"] == B.ACTIVE)).all()


# ---------------------------------------------------------------------- 3. systems that cross the Cholesky's panels (48 columns = 8 images)
@pytest.mark.parametrize("count", [9, 24])
def test_cholesky_across_panels(count):
    name = "K = %d" % count
    inp = B.GPU_SCENES[name]()
    want = B.answer(name)
    assert want["free"].sum() == count - 2 and 6 * count > lightglue_amd._cabi.LG_BA_CHOLESKY_BLOCK
    check(run(inp), want, inp, name)


# ---------------------------------------------------------------------- 3b. rejected steps; a track beyond the longest taken on, two rows of one image in a track
def test_rejected_steps_follow_the_definition():
    inp, want = B.GPU_SCENES["far"](), B.answer("far")
    assert want["num_accepted"] <= want["num_iterations"] - 2 and want["converged"]          # at least two trials are rejected on the way
    check(run(inp), want, inp, "far start")


def test_too_long_track_and_shared_labels():
    inp, clean = B.long_scene()
    want = B.answer("long")
    T = len(inp["xyz"]) - 2
    assert (want["node_state"] == B.TOO_LONG).sum() == 1148 > lightglue_amd._cabi.LG_BA_MAX_TRACK_LENGTH and not want["adjusted"][T] and want["adjusted"][T + 1]
    assert (want["node_state"][2, 100:102] == B.ACTIVE).all() and (inp["track_id"][2, 100:102] == T + 1).all()
    got = run(inp)
    check(got, want, inp, "long")
    alone = run(clean)                                                   # without the long track's labels: the same bits everywhere else
    same_bits(got, alone, "long against clean", tuple(k for k in BIT_KEYS if k != "node_state"))
    assert ((got["node_state"] == B.ACTIVE) == (alone["node_state"] == B.ACTIVE)).all()


# ---------------------------------------------------------------------- 3c. more tracks than the scan's workgroup has threads
def test_more_tracks_than_scan_threads():
    """1030 two-view tracks over 6 x 400 nodes: each of the scan's 1024 threads owns ceil(1030 / 1024) = 2 consecutive tracks (the last 509 own none), and
    tracks 500 and 1027 lose one observation each, so two unlisted tracks sit between listed ones and their offsets must not move.  Two iterations."""
    sc = B.scene(6, 400, 1030, 201, hi=2)
    tid, left = sc["track_id"].copy(), []
    for j in (500, 1027):
        (k, i), other = sorted(sc["planted"]["rows"][j].items())
        tid[k, i] = -1
        left.append(other)
    inp = dict(B.oracle_input(sc), track_id=tid)
    want = B.adjust(inp, num_iterations=2)
    assert len(inp["xyz"]) == 1030 > 1024 and all(want["node_state"][k, i] == B.SHORT for k, i in left)          # on the definition, before the GPU is read
    assert want["num_observations"] == 2056 and (want["node_state"] == B.SHORT).sum() == 2 and want["num_accepted"] == 2
    check(run(inp, num_iterations=2), want, inp, "1030 tracks")


# ---------------------------------------------------------------------- 4. invariance
def test_outputs_are_the_same_bits(main):
    inp = B.GPU_SCENES["main"]()
    same_bits(main, run(inp), "the same call again")
    moved, perm = B.relabel(inp, 5)
    other = run(moved)
    same_bits(main, dict(other, xyz=other["xyz"][perm]), "tracks relabelled")
    assert (main["poses"][:2] == inp["poses"][:2]).all() and (main["poses"][2:] != inp["poses"][2:]).any()
    one = run(inp, num_iterations=1)
    check(one, B.answer("main", num_iterations=1), inp, "one iteration")
    assert one["num_iterations"] == 1 and one["num_accepted"] == 1 and not one["converged"] and one["final_cost"] > main["final_cost"]
    # a heavily damped start: the budget runs out before the call converges, lambda falling all the way
    slow = run(inp, initial_damping=B.SLOW_DAMPING)
    check(slow, B.adjust(inp, initial_damping=B.SLOW_DAMPING), inp, "damped start")
    assert slow["num_iterations"] == 10 and slow["num_accepted"] == 10 and not slow["converged"]


# ---------------------------------------------------------------------- 5. the chain this feature exists for
def test_triangulate_adjust_localise_on_the_device():
    sc = B.chain_scene()
    feats, cams, poses = {"keypoints": cuda(sc["kpts"])}, torch.from_numpy(sc["cams"]), cuda(sc["poses"])
    tri = Triangulator(max_reproj_error=8.0).triangulate(feats, sc["pairs"].tolist(), cuda(sc["matches0"]), cams, poses)
    assert tri["num_tracks"] == 80
    out = lightglue_amd.bundle_adjust(BundleAdjuster(), tri, feats, cams, poses, [0, 1])
    assert out["final_cost"] < 0.5 * out["initial_cost"] and out["num_observations"] == int((tri["track_id"] >= 0).sum()) and out["converged"]
    assert out["points3d"].is_cuda and tuple(out["points3d"].shape) == tuple(tri["points3d"].shape)
    assert torch.equal(out["poses"][:2], poses[:2]) and torch.equal(out["poses"][5], poses[5])      # constant, and an image without observations
    # the oracle on the device's tracks
    inp = dict(kpts=sc["kpts"], num=None, track_id=tri["track_id"].cpu().numpy(), xyz=tri["xyz"].cpu().numpy(), cams=sc["cams"], poses=sc["poses"], constant=sc["constant"])
    want = B.adjust(inp)
    if not want["near"]:
        check({k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}, want, inp, "chain")
    est = AbsolutePoseEstimator(threshold=3.0, num_hypotheses=512, refine=True, seed=0)
    qm0 = cuda(sc["query_matches0"])
    a = est.estimate_pairs(feats, sc["query_pairs"].tolist(), qm0, cams, out["points3d"], pool=True)
    b = est.estimate_pairs(feats, sc["query_pairs"].tolist(), qm0, cams, tri["points3d"], pool=True)
    print("inliers of image 5: %d with the adjusted points, %d with the triangulated ones" % (int(a["num_inliers"][0]), int(b["num_inliers"][0])))
    assert a["queries"].tolist() == [5] and int(a["num_inliers"][0]) >= int(b["num_inliers"][0]) >= 100
