"""BundleAdjuster's robust mode on the GPU against the float64 definition (tests/bundle_robust_oracle.py), against lg_bundle_adjust and against itself.

The bars are those of tests/test_gpu_bundle.py, unchanged: node states, the counters (now also num_filtered and num_filter_stages), `converged` and the
per-image status equal the oracle's exactly; a pose entry, a point and a row of points3d may differ from the oracle's fp64 value by ONE float32 ulp of the
scale (for a point the largest coordinate magnitude among the point and the centres of the cameras that see it, for t the same over the image's centre and
t, for R 1); costs agree within 1e-9 relative; observation_error within one float32 ulp of the error.  The scale of a track is taken over its observations
of the FIRST stage, so that a track the filter took out of the adjustment is still measured.  What comes back as input bits is what never moved: a track
never adjusted, an image never free.
tests/test_bundle_robust_cpu.py asserts that the oracle places no decision within a relative 1e-9 of its bar on these inputs, with one exception it names:
Huber with one filter round on the planted scene accepts its last step on a cost decrease of 5.9e-10 of the cost (3e-8 absolute, five orders above the
fp64 noise of a sum of 200 terms).  That call is NOT excluded here: its decisions are asserted equal like all others.
The scenes are those of tests/bundle_oracle.py and tests/bundle_robust_oracle.py (K = 6 .. 9, N = 32 .. 96)."""
import numpy as np
import pytest
import torch

import bundle_oracle as B
import bundle_robust_oracle as R
import triangulate_oracle as O
import lightglue_amd
from lightglue_amd import AbsolutePoseEstimator, BundleAdjuster, Triangulator
from lightglue_amd._cabi import LightGlueAmdError
from test_gpu_bundle import BIT_KEYS, INT_KEYS, cuda, same_bits

pytestmark = pytest.mark.gpu

COUNTS = INT_KEYS + ("num_filtered", "num_filter_stages")
ALL_BITS = BIT_KEYS + ("num_filtered", "num_filter_stages")


def run(inp, expect=None, entry=None, **conf):
    """one call -> host outputs; entry: True forces lg_bundle_adjust_robust, False lg_bundle_adjust; expect: the words the call's error must hold"""
    feats = {"keypoints": cuda(inp["kpts"])}
    if inp.get("num") is not None:
        feats["num_keypoints"] = torch.as_tensor(np.asarray(inp["num"]), dtype=torch.int32)
    ba = BundleAdjuster(**conf)
    if entry is not None:
        ba.robust_entry = entry
    call = lambda: ba.adjust(feats, (cuda(inp["track_id"]), cuda(inp["xyz"])), torch.from_numpy(inp["cams"]), cuda(inp["poses"]), torch.from_numpy(inp["constant"]))
    if expect is None:
        out = call()
    else:
        with pytest.raises(LightGlueAmdError) as err:
            call()
        for word in expect:
            assert word in str(err.value), (word, str(err.value))
        out = err.value.outputs
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}


def check(got, want, inp, what, near=()):
    """tests/test_gpu_bundle.py check with the robust mode's counters, its scale and its rule for what comes back as input bits"""
    assert want["near"] == list(near), (what, want["near"])
    for k in COUNTS:
        assert got[k] == want[k], (what, k, got[k], want[k])
    assert (got["node_state"] == want["node_state"]).all(), (what, np.argwhere(got["node_state"] != want["node_state"])[:8])
    assert (got["status"] == want["status"]).all(), (what, got["status"])
    for k in ("initial_cost", "final_cost"):
        assert abs(got[k] - want[k]) <= 1e-9 * want[k], (what, k, got[k], want[k])
    track, image = R.scales(inp, want)
    pu, tu = np.array([O.ulp32(s) for s in track]), np.array([O.ulp32(s) for s in image])
    adj = want["adjusted"]
    dx = abs(got["xyz"].astype(np.float64) - want["xyz64"]).max(1)
    dt = abs(got["poses"][:, :, 3].astype(np.float64) - want["poses64"][:, :, 3]).max(1)
    dr = abs(got["poses"][:, :, :3].astype(np.float64) - want["poses64"][:, :, :3]).max()
    print("%s: worst / ulp: points %.3f, t %.3f, R %.3f; cost %.9g -> %.9g in %d iterations, %d filtered" % (
        what, float((dx[adj] / pu[adj]).max()), float((dt / tu).max()), dr / O.ulp32(1.0), got["initial_cost"], got["final_cost"], got["num_iterations"],
        got["num_filtered"]))
    assert (dx[adj] <= pu[adj]).all() and (dt <= tu).all() and dr <= O.ulp32(1.0), what
    assert np.array_equal(got["xyz"][~adj], inp["xyz"][~adj], equal_nan=True) and np.array_equal(got["poses"][~want["free"]], inp["poses"][~want["free"]], equal_nan=True)
    active = want["node_state"] == B.ACTIVE
    tid = np.asarray(inp["track_id"])
    dp = abs(got["points3d"][active].astype(np.float64) - want["points3d64"][active]).max(1)
    assert (dp <= pu[tid[active]]).all() and np.isnan(got["points3d"][~active]).all(), what
    assert (got["points3d"][active] == got["xyz"][tid[active]]).all(), what
    de = abs(got["observation_error"][active].astype(np.float64) - want["error64"][active])
    assert (de <= np.array([O.ulp32(e) for e in want["error64"][active]])).all() and np.isnan(got["observation_error"][~active]).all(), what


def filtered(got):
    return sorted(map(tuple, np.argwhere(got["node_state"] == R.FILTERED).tolist()))


@pytest.fixture(scope="module")
def planted_run():
    return run(R.planted_scene()[0], **R.CAUCHY, **R.ONE_ROUND)


# ---------------------------------------------------------------------- 1. the planted scene: both losses, without and with a filter round
def test_cauchy_with_one_round_matches_the_definition(planted_run):
    inp, planted, truth = R.planted_scene()
    check(planted_run, R.answer("planted", **R.CAUCHY, **R.ONE_ROUND), inp, "planted, cauchy, one round")
    assert filtered(planted_run) == planted and planted_run["num_filtered"] == 12 and planted_run["num_filter_stages"] == 1 and planted_run["num_observations"] == 200
    plain = run(inp)                                                     # the squared loss on the same input, through lg_bundle_adjust
    check(plain, R.answer("planted"), inp, "planted, squared")
    adj = R.answer("planted")["adjusted"]
    error = lambda out: np.median(np.linalg.norm(out["xyz"].astype(np.float64) - truth, axis=1)[adj])
    print("median point error: %.4f robust, %.4f squared" % (error(planted_run), error(plain)))
    assert error(planted_run) < 0.1 * error(plain) and plain["num_filtered"] == 0


@pytest.mark.parametrize("loss,rounds,near", [("cauchy", 0, ()), ("huber", 0, ()), ("huber", 1, ("accept",))])
def test_losses_match_the_definition_on_the_planted_scene(loss, rounds, near):
    inp, planted, _ = R.planted_scene()
    conf = dict(R.CAUCHY if loss == "cauchy" else R.HUBER, **(R.ONE_ROUND if rounds else {}))
    got = run(inp, **conf)
    check(got, R.answer("planted", **conf), inp, "planted, %s, %d rounds" % (loss, rounds), near)
    assert filtered(got) == (planted if rounds else []) and got["num_observations"] == 212 - 12 * rounds


# ---------------------------------------------------------------------- 2. the filter's edges; two Cholesky panels
def test_filter_shortens_a_track_to_one_observation():
    inp, moved, alone, j = R.short_scene()
    got = run(inp, **R.CAUCHY, **R.ONE_ROUND)
    check(got, R.answer("short", **R.CAUCHY, **R.ONE_ROUND), inp, "short")
    assert filtered(got) == [moved] and got["node_state"][alone] == B.SHORT and np.isnan(got["points3d"][alone]).all()
    assert not np.array_equal(got["xyz"][j], inp["xyz"][j])              # the last accepted point, not the bits that went in


def test_filter_takes_the_last_observations_of_a_free_image():
    inp, nodes = R.last_observation_scene()
    got = run(inp, **R.LAST)
    check(got, R.answer("last", **R.LAST), inp, "last")
    assert filtered(got) == nodes and not np.array_equal(got["poses"][R.LAST_IMAGE], inp["poses"][R.LAST_IMAGE])
    one = run(inp, **R.CAUCHY, num_iterations=1)                         # the pose it had reached when it stopped being free
    assert np.array_equal(got["poses"][R.LAST_IMAGE], one["poses"][R.LAST_IMAGE])


def test_cholesky_across_panels_under_cauchy():
    inp, want = R.SCENES["K = 9"](), R.answer("K = 9", **R.CAUCHY)
    assert want["free"].sum() == 7 and 6 * 9 > lightglue_amd._cabi.LG_BA_CHOLESKY_BLOCK
    check(run(inp, **R.CAUCHY), want, inp, "K = 9, cauchy")


def test_two_observations_of_one_image_carry_their_own_weights():
    inp, want = R.SCENES["long"](), R.answer("long", **R.CAUCHY)
    T = len(inp["xyz"]) - 1
    assert (want["node_state"][2, 100:102] == B.ACTIVE).all() and (inp["track_id"][2, 100:102] == T).all()          # the reduce kernel's per-observation W
    err = want["error64"][2, 100:102]
    assert abs(err[0] - err[1]) > 1e-3                                    # two different weights
    check(run(inp, **R.CAUCHY), want, inp, "long, cauchy")


# ---------------------------------------------------------------------- 3. identities with lg_bundle_adjust and between the stages
def test_plain_settings_through_the_robust_entry_are_the_plain_bytes():
    for name in ("main", "long"):
        inp = B.GPU_SCENES[name]()
        old = run(inp, entry=False)
        same_bits(old, run(inp, entry=True), name + ": squared, no round, through lg_bundle_adjust_robust", ALL_BITS)
        same_bits(old, run(inp, loss="huber", loss_scale=1e6), name + ": huber with c = 1e6", ALL_BITS)        # every weight is exactly 1
    inp = R.planted_scene()[0]
    same_bits(run(inp, **R.ONE_ROUND), run(inp, loss="huber", loss_scale=1e6, **R.ONE_ROUND), "planted, one round: squared against huber with c = 1e6", ALL_BITS)


def test_a_filter_that_removes_nothing_is_the_longer_single_stage_call():
    inp = B.GPU_SCENES["main"]()
    for conf, iterations, rounds in ((R.CAUCHY, 3, 1), (R.CAUCHY, 2, 2), (dict(loss="squared"), 1, 3)):
        staged = run(inp, **conf, filter_rounds=rounds, max_reproj_error=50.0, num_iterations=iterations)
        single = run(inp, entry=True, **conf, num_iterations=iterations * (rounds + 1))
        assert staged["num_filtered"] == 0 and staged["num_filter_stages"] == 0
        same_bits(staged, single, (conf, iterations, rounds), ALL_BITS)
    assert run(inp, **R.CAUCHY, num_iterations=6)["num_iterations"] == 6          # (cauchy, 3, 1) crosses its stage boundary before it converges


# ---------------------------------------------------------------------- 4. invariance
def test_outputs_are_the_same_bits(planted_run):
    inp = R.planted_scene()[0]
    same_bits(planted_run, run(inp, **R.CAUCHY, **R.ONE_ROUND), "the same call again", ALL_BITS)
    moved, perm = B.relabel(inp, 5)
    other = run(moved, **R.CAUCHY, **R.ONE_ROUND)
    same_bits(planted_run, dict(other, xyz=other["xyz"][perm]), "tracks relabelled", ALL_BITS)


def test_bad_camera_leaves_everything_else_untouched():
    bad, clean, what = B.edge_scene()
    got = run(bad, expect=("LG_ERR_CAMERA", "image %d" % what["bad_image"]), **R.CAUCHY, **R.ONE_ROUND)
    check(got, R.answer("edge", **R.CAUCHY, **R.ONE_ROUND), bad, "edge, cauchy")
    assert got["status"].tolist() == [0, 0, 0, B.LG_ERR_CAMERA, 0, 0, 0]
    alone = run(clean, **R.CAUCHY, **R.ONE_ROUND)
    same_bits(got, alone, "edge against clean", ("poses", "xyz", "points3d", "observation_error", "initial_cost", "final_cost") + COUNTS)
    assert ((got["node_state"] == B.ACTIVE) == (alone["node_state"] == B.ACTIVE)).all()


# ---------------------------------------------------------------------- 5. the chain: contaminated matches, a generous triangulation, the robust adjustment
def test_triangulate_adjust_robustly_localise_on_the_device():
    sc = R.chain_scene()
    feats, cams, poses = {"keypoints": cuda(sc["kpts"])}, torch.from_numpy(sc["cams"]), cuda(sc["poses"])
    tri = Triangulator(max_reproj_error=R.CHAIN_MAX_REPROJ_ERROR).triangulate(feats, sc["pairs"].tolist(), cuda(sc["matches0"]), cams, poses)
    assert tri["num_tracks"] == 80                                       # the generous bar keeps every contaminated track
    out = lightglue_amd.bundle_adjust(BundleAdjuster(**R.CAUCHY, **R.ONE_ROUND), tri, feats, cams, poses, [0, 1])
    host = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}
    inp = dict(kpts=sc["kpts"], num=None, track_id=tri["track_id"].cpu().numpy(), xyz=tri["xyz"].cpu().numpy(), cams=sc["cams"], poses=sc["poses"], constant=sc["constant"])
    want = R.adjust(inp, **R.CAUCHY, **R.ONE_ROUND)
    if not want["near"]:
        check(host, want, inp, "chain")
    assert set(sc["moved"]) <= set(filtered(host)) and out["num_filtered"] <= len(sc["moved"]) + 2 and out["converged"]
    assert float(np.nanmax(host["observation_error"])) < 4.0
    plain = lightglue_amd.bundle_adjust(BundleAdjuster(), tri, feats, cams, poses, [0, 1])
    assert float(np.nanmax(plain["observation_error"].cpu().numpy())) > 20.0          # the squared loss keeps them and bends the rest
    est = AbsolutePoseEstimator(threshold=3.0, num_hypotheses=512, refine=True, seed=0)
    qm0 = cuda(sc["query_matches0"])
    a = est.estimate_pairs(feats, sc["query_pairs"].tolist(), qm0, cams, out["points3d"], pool=True)
    b = est.estimate_pairs(feats, sc["query_pairs"].tolist(), qm0, cams, plain["points3d"], pool=True)
    print("inliers of image 5: %d with the robustly adjusted points, %d with the squared loss" % (int(a["num_inliers"][0]), int(b["num_inliers"][0])))
    assert a["queries"].tolist() == [5] and int(a["num_inliers"][0]) >= 100
