"""GlobalPoseEstimator on the GPU against the float64 definition (tests/posegraph_oracle.py) and against itself.

Bars and where they come from:
  Pair states, image states, the baseline, the images posed, the iterations either solver ran and `positions_ok` are integers: they equal the oracle's exactly.
  One exception, the bundle adjuster's rule for a decision that lies on its bar: where the oracle marks a stage's convergence test as decided by fp64 rounding
  (`near`: the step is rounding, it changes when the oracle swaps its solver, and lies within 100 x of the bar; tests/posegraph_oracle.py has the figures) that stage's iteration count is not compared.  First run on the device:
  K = 16 stopped after 8 position iterations, the oracle after 7, its steps there 5.8e-14, 2.8e-13, 1.1e-13, 4.3e-14 against the bar 1e-12.  Everything
  else of such a call is compared as usual: steps of that size are six orders below a float32 ulp.
  A pose entry may differ from the oracle's fp64 value by ONE float32 ulp of the scale: 1 for R; for t the largest coordinate magnitude among t and the
  image's centre.  Both sides are fp64 and each value is rounded to float32 once; the two differ in the order of their sums only.
  rotation_error and direction_error: one float32 ulp of the error (the bar tests/test_gpu_bundle.py sets for observation_error), plus what the oracle
  itself cannot hold, which matters only for errors near zero: 1e-12 degrees (an angle between two fp64 directions carries their rounding, 2.2e-16 of
  the vectors' length over a few operations times 57.3 degrees per radian; the baseline's own pair has error 0 by construction and a float32 ulp of 0 is
  1e-45), and OWN_MARGIN x the largest amount by which the error moves when the oracle solves its systems by LU in place of the Cholesky (`own`: the
  centres carry the rounding of the solve, about 1e-11, which is 6e-10 degrees of a direction; one float32 ulp of an error below 0.01 degrees is smaller).
  OWN_MARGIN = 100 is the spread of that rounding from one sample to the next (tests/posegraph_oracle.py: 70 x).  First run on the device, exact scenes
  (errors of 1e-5 degrees, all of them rounding of the float32 inputs): K = 49 and K = 256 were 5.7 and 4.0 float32 ulps of the error off, K <= 17 below 0.66.
  The size scenes carry 0.3 degrees of noise per pair since: the errors are then what a caller sees, not residue.
The scenes are those of tests/posegraph_oracle.py: cameras on an arc around a box (tests/triangulate_oracle.py), a ring plus random chords, weights 40 .. 400."""
import numpy as np
import pytest
import torch

import posegraph_oracle as G
import triangulate_oracle as O
import lightglue_amd
from lightglue_amd import BundleAdjuster, GlobalPoseEstimator, RelativePoseEstimator, Triangulator

INT_KEYS = ("origin", "baseline", "num_posed", "rotation_iterations", "position_iterations", "positions_ok")
BIT_KEYS = ("poses", "image_state", "pair_state", "rotation_error", "direction_error") + INT_KEYS
ANGLE_FLOOR, OWN_MARGIN = 1e-12, 100.0
# the chain: final cost per observation of the adjusted reconstruction started from the estimated poses over that started from the true poses in the same
# gauge.  Measured on the first run: 9.21 (1477.4 against 160.3 over the same 499 observations of 110 tracks; profiles/global_poses.md) — the origin and
# the baseline are held, so the error of the baseline's estimated pose stays in the reconstruction.  Asserted with a 2 x margin
CHAIN_COST_RATIO = 2.0 * 9.2149

pytestmark = pytest.mark.gpu


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(inp, **kw):
    conf = {k: kw.pop(k) for k in list(kw) if k in ("num_iterations", "rotation_scale", "max_rotation_error", "direction_scale", "min_inliers")}
    out = GlobalPoseEstimator(**conf).estimate(cuda(inp["pairs"]), (cuda(inp["R"]), cuda(inp["t"])), inp["K"], origin=inp.get("origin", 0),
                                               weights=cuda(inp["weights"]), **kw)
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}


def want_of(inp, **kw):
    return G.estimate(inp["pairs"], inp["R"], inp["t"], inp["K"], origin=inp.get("origin", 0), weights=inp["weights"], **kw)


def check(got, want, what, max_iterations=12):
    for k in INT_KEYS:
        g = -1 if got[k] is None else got[k]
        if k.split("_")[0] in want["near"]:
            assert k.endswith("_iterations") and 1 <= g <= max_iterations, (what, k, g)
            continue
        assert g == want[k], (what, k, got[k], want[k])
    assert (got["pair_state"] == want["pair_state"]).all(), (what, np.flatnonzero(got["pair_state"] != want["pair_state"])[:8])
    assert (got["image_state"] == want["image_state"]).all(), (what, got["image_state"], want["image_state"])
    P64 = want["poses64"]
    assert (np.isnan(got["poses"]) == np.isnan(P64)).all(), what
    dr = np.nan_to_num(abs(got["poses"][:, :, :3] - P64[:, :, :3])).max()
    posed = want["image_state"] == G.POSED
    scale = np.maximum(abs(P64[posed, :, 3]).max(1), abs(want["centres64"][posed]).max(1)) if posed.any() else np.ones(0)
    tu = np.array([O.ulp32(s) for s in scale])
    dt = abs(got["poses"][posed, :, 3] - P64[posed, :, 3]).max(1) if posed.any() else np.zeros(0)
    worst = {}
    for k in ("rotation_error", "direction_error"):
        w64 = want[k + "64"]
        assert (np.isnan(got[k]) == np.isnan(w64)).all(), (what, k)
        m = ~np.isnan(w64)
        d = abs(got[k][m].astype(np.float64) - w64[m])
        bar = np.array([O.ulp32(e) for e in w64[m]]) + ANGLE_FLOOR + OWN_MARGIN * want["own"][k + "64"]
        worst[k] = float((d / bar).max()) if m.any() else 0.0
    print("%s: worst / bar: R %.3f, t %.3f, rotation_error %.3f, direction_error %.3f; %d posed, iterations %d + %d" % (
        what, dr / O.ulp32(1.0), float((dt / tu).max()) if posed.any() else 0.0, worst["rotation_error"], worst["direction_error"], got["num_posed"],
        got["rotation_iterations"], got["position_iterations"]))
    assert dr <= O.ulp32(1.0) and (dt <= tu).all() and worst["rotation_error"] <= 1.0 and worst["direction_error"] <= 1.0, what


def same_bits(a, b, what, keys=BIT_KEYS):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True) if isinstance(a[k], np.ndarray) else a[k] == b[k], (what, k)


# ---------------------------------------------------------------------- 1. sizes: the smallest system, one panel, a panel and a short one, across panels
@pytest.mark.parametrize("K", [3, 16, 17, 49])
def test_sizes_match_the_definition(K):
    sc = G.scene(K, noise=0.3)
    want = G.run(sc)
    assert want["num_posed"] == K and want["positions_ok"] and (want["pair_state"] == G.USED).all()
    got = run(sc)
    check(got, want, "K = %d" % K)
    rot, centre = G.against_truth(dict(want, poses64=got["poses"].astype(np.float64),
                                       centres64=-np.einsum("kji,kj->ki", got["poses"][:, :, :3], got["poses"][:, :, 3]).astype(np.float64)), sc)
    assert rot < 1.0 and centre < 0.01, (rot, centre)               # 0.3 degrees per pair: tests/test_posegraph_cpu.py has the oracle's figures


def test_the_envelope_256_images():
    sc = G.scene(256, chords=768, noise=0.3)
    assert len(sc["pairs"]) == 1024
    want = G.run(sc)
    assert want["num_posed"] == 256
    check(run(sc), want, "K = 256")


# ---------------------------------------------------------------------- 2. noise and replaced chords
def test_noise_and_outliers_follow_the_definition():
    sc = G.scene(20, seed=0, noise=0.5, outliers=0.25)
    want = G.run(sc)
    assert sc["planted"].sum() == 15 and (want["pair_state"][sc["planted"]] == G.ROTATION_OUTLIER).all() and want["num_posed"] == 20
    got = run(sc)
    check(got, want, "noise + outliers")
    assert (got["pair_state"] == G.ROTATION_OUTLIER).sum() == 15


# ---------------------------------------------------------------------- 3. every edge in one scene
def test_edge_inputs_leave_everything_else_untouched():
    bad, clean, what = G.edge_scene()
    got, alone = run(bad), run(clean)
    check(got, want_of(bad), "edge")
    check(alone, want_of(clean), "edge clean")
    for p, st in enumerate(what["states"]):
        assert st is None or got["pair_state"][p] == st, (p, st, got["pair_state"][p])
    mid = slice(what["front"], what["front"] + what["clean"])
    assert set(np.unique(got["pair_state"]).tolist()) == {G.USED, G.BAD_INDEX, G.NO_MODEL, G.OUTSIDE, G.NO_POSITION}
    assert got["image_state"][what["hanging"]] == G.ROTATION_ONLY and (got["image_state"][list(what["second"])] == G.NOT_CONNECTED).all()
    assert got["image_state"][what["alone"]] == G.NOT_CONNECTED and np.isnan(got["poses"][what["alone"]]).all()
    assert np.isfinite(got["poses"][what["hanging"], :, :3]).all() and np.isnan(got["poses"][what["hanging"], :, 3]).all()
    # the same call without the entries that contribute nothing: the same bits
    same_bits(got, alone, "edge against clean", ("poses", "image_state") + INT_KEYS)
    for k in ("pair_state", "rotation_error", "direction_error"):
        assert np.array_equal(got[k][mid], alone[k], equal_nan=True), k


def test_collinear_centres_have_rotations_only():
    sc = G.collinear_scene()
    want = want_of(sc)
    assert not want["positions_ok"] and (want["image_state"] == G.ROTATION_ONLY).all()
    got = run(sc)
    check(got, want, "collinear")
    assert not got["positions_ok"] and got["num_posed"] == 0 and np.isnan(got["poses"][:, :, 3]).all() and np.isfinite(got["poses"][:, :, :3]).all()


def test_given_baseline_and_origin():
    sc = G.scene(16, origin=5)
    other = int(sc["pairs"][[5 in p for p in sc["pairs"].tolist()]].sum(1).max() - 5)          # a neighbour of image 5
    want = G.estimate(sc["pairs"], sc["R"], sc["t"], 16, origin=5, baseline=other, weights=sc["weights"])
    got = run(sc, baseline=other)
    check(got, want, "origin 5, a given baseline")
    assert got["origin"] == 5 and got["baseline"] == other
    assert np.array_equal(got["poses"][5], np.eye(3, 4, dtype=np.float32))
    c = -got["poses"][other, :, :3].T @ got["poses"][other, :, 3]
    assert abs(np.linalg.norm(c) - 1.0) < 1e-6
    # a baseline no usable pair joins to the origin: no positions
    far = next(k for k in range(16) if k != 5 and not any({5, k} == set(p) for p in sc["pairs"].tolist()))
    none = run(sc, baseline=far)
    check(none, G.estimate(sc["pairs"], sc["R"], sc["t"], 16, origin=5, baseline=far, weights=sc["weights"]), "no pair to the baseline")
    assert none["baseline"] is None and not none["positions_ok"] and none["position_iterations"] == 0


# ---------------------------------------------------------------------- 4. invariance
def test_outputs_are_the_same_bits():
    sc = G.scene(17, seed=1, noise=0.3)
    first = run(sc)
    same_bits(first, run(sc), "the same call again")
    order = np.random.default_rng(5).permutation(len(sc["pairs"]))
    moved = dict(sc, pairs=sc["pairs"][order], R=sc["R"][order], t=sc["t"][order], weights=sc["weights"][order])
    other = run(moved)
    same_bits(first, other, "pairs permuted", ("poses", "image_state") + INT_KEYS)
    for k in ("pair_state", "rotation_error", "direction_error"):
        assert np.array_equal(first[k][order], other[k], equal_nan=True), k
    short = run(sc, num_iterations=6)
    check(short, G.run(sc, num_iterations=6), "six iterations")
    assert short["rotation_iterations"] <= 6 and short["position_iterations"] <= 6


# ---------------------------------------------------------------------- 5. the chain this feature exists for
def test_relative_poses_to_adjusted_reconstruction_on_the_device():
    sc = G.chain_scene()
    K = len(sc["poses"])
    feats, cams, pairs = {"keypoints": cuda(sc["kpts"])}, torch.from_numpy(sc["cams"]), sc["pairs"].tolist()
    rel = RelativePoseEstimator(threshold=3.0, num_hypotheses=512, refine=True, seed=0).estimate_pairs(feats, pairs, cuda(sc["matches0"]), cams)
    est = lightglue_amd.estimate_global_poses(GlobalPoseEstimator(), rel, pairs, K)
    assert est["poses"].is_cuda and est["num_posed"] == K and est["positions_ok"]
    want = G.estimate(sc["pairs"], rel["R"].cpu().numpy(), rel["t"].cpu().numpy(), K, num_inliers=rel["num_inliers"].cpu().numpy())
    check({k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in est.items()}, want, "chain")
    held = [est["origin"], est["baseline"]]
    cost = {}
    for name, poses in (("estimated", est["poses"]), ("true", cuda(G.gauge_poses(sc["poses"], *held)))):
        tri = Triangulator(max_reproj_error=64.0).triangulate(feats, pairs, rel, cams, poses)
        out = lightglue_amd.bundle_adjust(BundleAdjuster(num_iterations=20), tri, feats, cams, poses, held)
        cost[name] = (out["final_cost"], out["num_observations"], tri["num_tracks"])
    print("chain: final cost %.6g over %d observations of %d tracks from the estimated poses, %.6g over %d of %d from the true ones: ratio %.4f" % (
        cost["estimated"] + cost["true"] + (cost["estimated"][0] / cost["true"][0],)))
    assert cost["estimated"][2] >= 0.9 * cost["true"][2]
    assert cost["estimated"][0] <= CHAIN_COST_RATIO * cost["true"][0] * cost["estimated"][1] / cost["true"][1]
