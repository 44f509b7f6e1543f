"""BundleAdjuster(refine_focal=True) on the GPU against the float64 definition (tests/bundle_focal_oracle.py), against lg_bundle_adjust_robust and against
itself.

The bars are those of tests/test_gpu_bundle.py and tests/test_gpu_bundle_robust.py, imported (`check`) and not redefined: node states, the counters,
`converged` and the per-image status equal the oracle's exactly; a pose entry, a point and a row of points3d may differ from the oracle's fp64 value by ONE
float32 ulp of the scale; costs agree within 1e-9 relative; observation_error within one float32 ulp of the error.  For `cameras`: fx and fy within one
float32 ulp of the oracle's fp64 value (both sides are fp64 and round to float32 once), cx, cy and every row that never moved are the input's bits, and
num_free_cameras equals the oracle's.
tests/test_bundle_focal_cpu.py asserts that the oracle places no decision within a relative 1e-9 of its bar on these inputs, with the exceptions it names:
on "main", "K = 9", "camera held" and "all held" the last accepted step lowers the cost by 1.4e-10 .. 7.5e-10 of it (6e-9 .. 6e-8 absolute, five orders
above the fp64 noise of a sum of 200 terms).  Those calls are NOT excluded: their decisions are asserted equal like all others.
The scenes are those of tests/bundle_oracle.py and tests/bundle_robust_oracle.py (K = 6 .. 9, N = 32 .. 288) with every focal length multiplied by a
factor of its own in [0.92, 1.08]."""
import numpy as np
import pytest
import torch

import bundle_focal_oracle as F
import bundle_oracle as B
import bundle_robust_oracle as R
import triangulate_oracle as O
import lightglue_amd
from lightglue_amd import AbsolutePoseEstimator, BundleAdjuster, RelativePoseEstimator, Triangulator
from lightglue_amd._cabi import LightGlueAmdError
from test_bundle_focal_cpu import NEAR
from test_gpu_bundle import cuda, same_bits
from test_gpu_bundle_robust import ALL_BITS, COUNTS, check, filtered

pytestmark = pytest.mark.gpu

FOCAL_BITS = ALL_BITS + ("cameras", "num_free_cameras")


def run(inp, expect=None, refine_focal=True, **conf):
    """one call -> host outputs; inp may hold constant_camera; expect: the words the call's error must hold (then the error's outputs come back)"""
    feats = {"keypoints": cuda(inp["kpts"])}
    if inp.get("num") is not None:
        feats["num_keypoints"] = torch.as_tensor(np.asarray(inp["num"]), dtype=torch.int32)
    ba = BundleAdjuster(refine_focal=refine_focal, **conf)
    if not refine_focal:
        ba.robust_entry = True
    held = {} if inp.get("constant_camera") is None or not refine_focal else {"constant_camera": torch.from_numpy(inp["constant_camera"])}
    call = lambda: ba.adjust(feats, (cuda(inp["track_id"]), cuda(inp["xyz"])), torch.from_numpy(inp["cams"]), cuda(inp["poses"]), torch.from_numpy(inp["constant"]), **held)
    if expect is None:
        out = call()
    else:
        with pytest.raises(LightGlueAmdError) as err:
            call()
        for word in expect:
            assert word in str(err.value), (word, str(err.value))
        out = err.value.outputs
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}


def check_focal(got, want, inp, what, near=()):
    """the imported check, then the cameras"""
    check(got, want, inp, what, near)
    cams = np.asarray(inp["cams"], np.float32)
    assert got["cameras"].dtype == np.float32 and got["cameras"].shape == cams.shape and got["num_free_cameras"] == want["num_free_cameras"], what
    moved = want["free_camera"]
    df = abs(got["cameras"][:, :2].astype(np.float64) - want["cameras64"][:, :2])
    ulp = np.array([[O.ulp32(v) for v in row] for row in want["cameras64"][:, :2]])
    print("%s: cameras worst / ulp %.3f, %d free" % (what, float((df[moved] / ulp[moved]).max()) if moved.any() else 0.0, got["num_free_cameras"]))
    assert (df[moved] <= ulp[moved]).all(), what
    assert np.array_equal(got["cameras"][:, 2:], cams[:, 2:]) and np.array_equal(got["cameras"][~moved], cams[~moved]), what
    assert (got["cameras"][moved, :2] != cams[moved, :2]).all(), what                  # a free camera did move


def answer(name):
    return F.SCENES[name](), F.answer(name), NEAR.get(name, ())


@pytest.fixture(scope="module")
def main_run():
    return run(F.SCENES["main"]())


# ---------------------------------------------------------------------- 1 - 3. the squared loss: the main scene; one column past the first panel; more rows below it
def test_main_scene_matches_the_definition(main_run):
    inp, want, near = answer("main")
    check_focal(main_run, want, inp, "main", near)
    assert want["num_free_cameras"] == 6 and want["free"].sum() == 4
    # 6. a pose-held image with a free camera: images 0 and 1 — the pose back bit for bit, the focal length refined
    assert np.array_equal(main_run["poses"][:2], inp["poses"][:2]) and (main_run["cameras"][:2, :2] != inp["cams"][:2, :2]).all()
    fixed = run(inp, refine_focal=False)
    assert main_run["final_cost"] < fixed["final_cost"] and "cameras" not in fixed and "num_free_cameras" not in fixed


def test_forty_nine_columns_cross_the_panel_by_one():
    inp, want, near = answer("K = 7")
    assert len(inp["cams"]) == 7 and 7 * 7 == lightglue_amd._cabi.LG_BA_CHOLESKY_BLOCK + 1 and want["num_free_cameras"] == 5
    check_focal(run(inp), want, inp, "K = 7", near)


def test_several_rows_below_the_first_panel():
    inp, want, near = answer("K = 9")
    assert want["free"].sum() == 7 and want["num_free_cameras"] == 9
    check_focal(run(inp), want, inp, "K = 9", near)


# ---------------------------------------------------------------------- 4, 5. the robust mode's settings mean what they mean without refine_focal
@pytest.fixture(scope="module")
def planted_run():
    return run(F.SCENES["planted"](), **F.CONF["planted"])


def test_cauchy_and_one_round_filter_exactly_the_planted_observations(planted_run):
    inp, want, near = answer("planted")
    check_focal(planted_run, want, inp, "planted, cauchy, one round", near)
    assert filtered(planted_run) == R.planted_scene()[1] and planted_run["num_filtered"] == 12 and planted_run["num_filter_stages"] == 1


def test_two_observations_of_one_image_weigh_the_focal_column_separately():
    inp, want, near = answer("long")
    T = len(inp["xyz"]) - 1
    assert (want["node_state"][2, 100:102] == B.ACTIVE).all() and (inp["track_id"][2, 100:102] == T).all()
    assert abs(want["error64"][2, 100] - want["error64"][2, 101]) > 1e-3               # two different weights
    check_focal(run(inp, **F.CONF["long"]), want, inp, "long, cauchy", near)


# ---------------------------------------------------------------------- 6. constant_camera
def test_a_pose_free_image_with_a_held_camera():
    inp, want, near = answer("camera held")
    got = run(inp)
    check_focal(got, want, inp, "cameras 3 and 4 held", near)
    assert got["num_free_cameras"] == 4 and np.array_equal(got["cameras"][3:5], inp["cams"][3:5])
    assert (got["poses"][3:5] != inp["poses"][3:5]).any(axis=(1, 2)).all()             # their poses moved
    # indices and a mask are one argument
    by_index = run(dict(inp, constant_camera=np.array([3, 4])))
    same_bits(got, by_index, "held by index", FOCAL_BITS)


def test_all_cameras_held_is_the_robust_entry_on_the_same_call():
    inp, want, near = answer("all held")
    got = run(inp)
    check_focal(got, want, inp, "all held", near)
    other = run(inp, refine_focal=False)                                               # lg_bundle_adjust_robust
    assert got["num_free_cameras"] == 0 and np.array_equal(got["cameras"], inp["cams"])
    for k in COUNTS:
        assert got[k] == other[k], k
    assert (got["node_state"] == other["node_state"]).all() and (got["status"] == other["status"]).all()
    check(other, dict(want, near=[]), inp, "all held, through lg_bundle_adjust_robust")     # both within the ulp bars of one fp64 answer
    # the columns are interleaved per image, so the 42 x 42 system sits inside the 49 x 49 one at other positions: other panels and other partial sums in the
    # substitution.  Bit equality does not follow from the layout; it is reported
    equal = {k: bool(np.array_equal(got[k], other[k], equal_nan=True)) for k in ("poses", "xyz", "points3d", "observation_error", "final_cost")}
    print("all held against lg_bundle_adjust_robust, equal bits:", equal)


# ---------------------------------------------------------------------- 7. invariance
def test_outputs_are_the_same_bits(main_run, planted_run):
    inp = F.SCENES["main"]()
    same_bits(main_run, run(inp), "the same call again", FOCAL_BITS)
    moved, perm = B.relabel(inp, 5)
    other = run(moved)
    same_bits(main_run, dict(other, xyz=other["xyz"][perm]), "tracks relabelled", FOCAL_BITS)
    inp = F.SCENES["planted"]()
    moved, perm = B.relabel(inp, 7)
    other = run(moved, **F.CONF["planted"])
    same_bits(planted_run, dict(other, xyz=other["xyz"][perm]), "planted, tracks relabelled", FOCAL_BITS)


# ---------------------------------------------------------------------- 8. the bad camera
def test_bad_camera_leaves_everything_else_untouched():
    what = B.edge_scene()[2]
    bad, clean = F.SCENES["edge"](), F.SCENES["edge clean"]()
    got = run(bad, expect=("LG_ERR_CAMERA", "image %d" % what["bad_image"]))
    check(got, F.answer("edge"), bad, "edge")
    assert got["status"].tolist() == [0, 0, 0, B.LG_ERR_CAMERA, 0, 0, 0]
    alone = run(clean)
    same_bits(got, alone, "edge against clean", ("poses", "xyz", "points3d", "observation_error", "initial_cost", "final_cost", "num_free_cameras") + COUNTS)
    k = what["bad_image"]
    assert np.array_equal(got["cameras"][k], bad["cams"][k]) and np.array_equal(np.delete(got["cameras"], k, 0), np.delete(alone["cameras"], k, 0))
    assert np.array_equal(got["cameras"][what["empty_image"]], bad["cams"][what["empty_image"]])        # no active observation: both kept


# ---------------------------------------------------------------------- 9. the chain
CHAIN_FACTORS = (0.92, 1.08, 0.92, 1.08, 0.92, 1.08)


def test_refined_cameras_feed_the_other_estimators():
    """contaminated matches (tests/bundle_robust_oracle.py's chain scene) with every focal length 8 % off, the sign alternating from image to image (one
    common factor is absorbed by the points' depths and costs no track): generous triangulation -> Cauchy, one filter round, focal lengths refined ->
    out["cameras"] as it is into Triangulator, AbsolutePoseEstimator and RelativePoseEstimator"""
    sc = R.chain_scene()
    wrong = sc["cams"].copy()
    wrong[:, :2] = (wrong[:, :2] * np.array(CHAIN_FACTORS)[:, None]).astype(np.float32)
    feats, cams, poses = {"keypoints": cuda(sc["kpts"])}, torch.from_numpy(wrong), cuda(sc["poses"])
    pairs, m0 = sc["pairs"].tolist(), cuda(sc["matches0"])
    tri = Triangulator(max_reproj_error=R.CHAIN_MAX_REPROJ_ERROR).triangulate(feats, pairs, m0, cams, poses)
    assert tri["num_tracks"] == 80
    out = lightglue_amd.bundle_adjust(BundleAdjuster(refine_focal=True, **R.CAUCHY, **R.ONE_ROUND), tri, feats, cams, poses, [0, 1])
    host = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}
    inp = dict(kpts=sc["kpts"], num=None, track_id=tri["track_id"].cpu().numpy(), xyz=tri["xyz"].cpu().numpy(), cams=wrong, poses=sc["poses"], constant=sc["constant"])
    want = F.adjust(inp, **R.CAUCHY, **R.ONE_ROUND)
    if not want["near"]:
        check_focal(host, want, inp, "chain")
    assert set(sc["moved"]) <= set(filtered(host)) and out["converged"] and out["num_free_cameras"] == 5
    assert out["cameras"].dtype == torch.float32 and tuple(out["cameras"].shape) == (O.K, 4) and out["cameras"].is_cuda
    before = abs(wrong[:5, 0] / sc["cams"][:5, 0] - 1.0)
    after = abs(host["cameras"][:5, 0] / sc["cams"][:5, 0] - 1.0)
    print("focal error before %s after %s" % (before.round(4), after.round(4)))
    assert (after < before).all()
    strict = Triangulator(max_reproj_error=4.0)
    a = strict.triangulate(feats, pairs, m0, out["cameras"], out["poses"])
    b = strict.triangulate(feats, pairs, m0, cams, poses)
    print("tracks within 4 pixels: %d with the refined cameras and poses, %d with the input's" % (a["num_tracks"], b["num_tracks"]))
    assert a["num_tracks"] > b["num_tracks"] and a["num_tracks"] >= 70
    est = AbsolutePoseEstimator(threshold=3.0, num_hypotheses=512, refine=True, seed=0)
    loc = est.estimate_pairs(feats, sc["query_pairs"].tolist(), cuda(sc["query_matches0"]), out["cameras"], out["points3d"], pool=True)
    assert loc["queries"].tolist() == [5]
    rel = RelativePoseEstimator(seed=0).estimate_pairs(feats, pairs, m0, out["cameras"])
    assert len(rel["R"]) == len(pairs)
