"""GlobalPoseEstimator(solver="pcg") on the GPU against the float64 definitions and against itself.

Bars: those of tests/test_gpu_posegraph.py (its `check`): integers and states equal the oracle's (a stage's iteration count is not compared where the oracle
marks its convergence test as decided by fp64 rounding, `near`); R and t within ONE float32 ulp of the scale; the two error outputs within one float32 ulp of
the error + 1e-12 degrees + OWN_MARGIN x what the oracle itself moves by when it changes its accumulation order (`own`).  The oracle is
tests/posegraph_pcg_oracle.py, which follows the header's order of operations; the calls at cg_tolerance = 1e-13 are compared with the dense definition
(tests/posegraph_oracle.py) too.  The four solver counters equal the iterative oracle's for a stage that ran the oracle's number of iterations and has no
solve whose count moves with the accumulation order (`moving`); otherwise they are printed.

What makes the one-ulp bar against the dense definition meaningful (tests/test_posegraph_pcg_cpu.py asserts all of it without a GPU): at 1e-13 the two
definitions take the same decisions and differ by at most 1e-3 of a float32 ulp of the scale; measured there: K = 3: R 1.9e-9, t 2.9e-7; K = 16: 1.9e-9,
1.7e-7; K = 49: 2.8e-9, 1.1e-4; the hub scene (K = 300): 2.8e-9, 2.7e-6.  `moving` covers 0, 0, 1 and 3 of their 18 .. 22 solves and none at the default
tolerance; no decision of any call lies within 1e-9 of its bar (the closest: the solver's stop at 6.2e-3, p.q at 1.1e-4 of |p| |q| with budgets of one);
the largest solver-iteration counts are 30 / 130 (K = 49 at 1e-13), 27 / 255 (hub), 18 / 401 (K = 1 100 under its budget of 600), 18 / 121 (K = 49)."""
import functools

import numpy as np
import pytest
import torch

import bundle_pcg_oracle as BP
import posegraph_oracle as G
import posegraph_pcg_oracle as P
import triangulate_oracle as O
from lightglue_amd import BundleAdjuster, GlobalPoseEstimator, Triangulator, _cabi
from test_gpu_posegraph import BIT_KEYS, INT_KEYS, check as check_poses, cuda, same_bits

pytestmark = pytest.mark.gpu

CG_KEYS = ("rotation_cg_iterations", "position_cg_iterations", "rotation_cg_unconverged", "position_cg_unconverged", "cg_failures")
# the chain above 256 images: final cost of the adjusted reconstruction started from the estimated poses over that started from the true poses in the same
# gauge, per observation.  Measured on the first run: 1.0000 (744.472 against 744.472 over the same 4 171 observations of 1 200 tracks;
# profiles/global_poses_pcg.md) — the relative poses are exact, so the estimated poses are the true ones to float32.  Asserted with a 2 x margin
CHAIN_COST_RATIO = 2.0 * 1.0000


def run(inp, solver="pcg", **kw):
    conf = {k: kw.pop(k) for k in list(kw) if k in ("num_iterations", "rotation_cg_iterations", "position_cg_iterations", "cg_tolerance")}
    if solver is not None:
        conf["solver"] = solver
    out = GlobalPoseEstimator(**conf).estimate(cuda(inp["pairs"]), (cuda(inp["R"]), cuda(inp["t"])), inp["K"], origin=inp.get("origin", 0),
                                               weights=cuda(inp["weights"]), **kw)
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def call(name):
    """the device's answer to a call of tests/posegraph_pcg_oracle.py's list, once per session"""
    make, conf = P.CALLS[name]
    return run(make(), **conf)


def check(got, want, what):
    check_poses(got, want, what)
    for stage in ("rotation", "position"):
        comparable = got[stage + "_iterations"] == want[stage + "_iterations"] and not any(s == stage for s, _ in want["moving"])
        for k in (stage + "_cg_iterations", stage + "_cg_unconverged"):
            print("%s: %s %d, the oracle's %d%s" % (what, k, got[k], want[k], "" if comparable else " (not compared: %s, moving %s)" % (want["near"], want["moving"])))
            assert not comparable or got[k] == want[k], (what, k, got[k], want[k])
    assert got["cg_failures"] == want["cg_failures"], (what, got["cg_failures"], want["cg_failures"])


# ---------------------------------------------------------------------- 1. against the dense definition: the smallest system, 16, 49
@pytest.mark.parametrize("K", [3, 16, 49])
def test_tight_tolerance_matches_both_definitions(K):
    name = "K%d tight" % K
    got = call(name)
    assert set(got) == set(BIT_KEYS) | set(CG_KEYS)
    check(got, P.answer(name), name)
    check_poses(got, P.dense_answer(name), name + " against the dense definition")
    assert got["rotation_cg_unconverged"] == 0 and got["position_cg_unconverged"] == 0 and got["cg_failures"] == 0 and got["num_posed"] == K


# ---------------------------------------------------------------------- 2. the default tolerance, and a budget of one
def test_default_tolerance_and_a_budget_of_one():
    got = call("K16 default")
    check(got, P.answer("K16 default"), "K = 16, default tolerance")
    assert got["rotation_cg_unconverged"] == 0 and got["position_cg_unconverged"] == 0
    one, want = call("K16 one"), P.answer("K16 one")
    check(one, want, "K = 16, budgets of one")
    assert one["rotation_iterations"] == one["position_iterations"] == 12
    assert one["rotation_cg_iterations"] == one["rotation_cg_unconverged"] == one["rotation_iterations"]
    assert one["position_cg_iterations"] == one["position_cg_unconverged"] == one["position_iterations"]
    assert np.isfinite(one["poses"]).all() and np.isfinite(one["rotation_error"]).all() and np.isfinite(one["direction_error"]).all()


# ---------------------------------------------------------------------- 3. a hub (a list of 300 entries: past one wave's stride and past 256) and a double pair
def test_hub_and_double_pair_cross_the_folds():
    sc = P.hub_scene()
    assert np.bincount(sc["pairs"].ravel())[sc["hub"]] == 300 and sc["K"] > _cabi.LG_BA_MAX_IMAGES
    with pytest.raises(ValueError, match=r"num_images must be an integer in \[2, %d\], got 300" % _cabi.LG_BA_MAX_IMAGES):      # LG_BA_MAX_IMAGES by its value:
        run(sc, solver="cholesky")                                                                                            # the dense refusal keeps its words
    got = call("hub tight")
    check(got, P.answer("hub tight"), "hub")
    check_poses(got, P.dense_answer("hub tight"), "hub against the dense definition")
    assert got["num_posed"] == 300 and got["position_cg_unconverged"] == 0


# ---------------------------------------------------------------------- 4. beyond one workgroup's lanes
def test_1100_images_follow_the_definition_and_the_truth():
    sc = P.CALLS["big"][0]()
    assert len(sc["pairs"]) == 8800
    got, want = call("big"), P.answer("big")
    check(got, want, "K = 1100")
    assert got["num_posed"] == 1100 and got["positions_ok"]
    rot, centre = G.against_truth(dict(want, poses64=got["poses"].astype(np.float64),
                                       centres64=-np.einsum("kji,kj->ki", got["poses"][:, :, :3], got["poses"][:, :, 3]).astype(np.float64)), sc)
    print("K = 1100: rotation %.3f degrees, centres %.4f of the extent off the truth" % (rot, centre))        # the oracle: 0.17 degrees, 0.25 %
    assert rot < 1.0 and centre < 0.01, (rot, centre)


# ---------------------------------------------------------------------- 5. edges
def test_edge_inputs_leave_everything_else_untouched():
    bad, clean, what = G.edge_scene()
    got, alone = call("edge"), call("edge clean")
    check(got, P.answer("edge"), "edge")
    check(alone, P.answer("edge clean"), "edge clean")
    for p, st in enumerate(what["states"]):
        assert st is None or got["pair_state"][p] == st, (p, st, got["pair_state"][p])
    mid = slice(what["front"], what["front"] + what["clean"])
    assert set(np.unique(got["pair_state"]).tolist()) == {G.USED, G.BAD_INDEX, G.NO_MODEL, G.OUTSIDE, G.NO_POSITION}
    assert got["image_state"][what["hanging"]] == G.ROTATION_ONLY and (got["image_state"][list(what["second"])] == G.NOT_CONNECTED).all()
    assert got["image_state"][what["alone"]] == G.NOT_CONNECTED and np.isnan(got["poses"][what["alone"]]).all()
    same_bits(got, alone, "edge against clean", ("poses", "image_state") + INT_KEYS + CG_KEYS)
    for k in ("pair_state", "rotation_error", "direction_error"):
        assert np.array_equal(got[k][mid], alone[k], equal_nan=True), k


def test_collinear_centres_have_rotations_only():
    got, want = call("collinear"), P.answer("collinear")
    assert not want["positions_ok"] and (want["image_state"] == G.ROTATION_ONLY).all()
    check(got, want, "collinear")
    assert got["positions_ok"] is False and got["num_posed"] == 0 and (got["image_state"] == G.ROTATION_ONLY).all()
    assert np.isnan(got["poses"][:, :, 3]).all() and np.isfinite(got["poses"][:, :, :3]).all() and got["cg_failures"] == 1


def test_no_usable_pair_at_the_origin():
    got, want = call("no baseline"), P.answer("no baseline")
    check(got, want, "no usable pair at the origin")
    assert got["baseline"] is None and not got["positions_ok"] and got["position_iterations"] == 0 and got["position_cg_iterations"] == 0
    assert got["position_cg_unconverged"] == 0 and got["num_posed"] == 0


# ---------------------------------------------------------------------- 6. the same bits
@pytest.mark.parametrize("name", ["hub tight", "big"])
def test_the_same_call_again_gives_the_same_bits(name):
    make, conf = P.CALLS[name]
    same_bits(call(name), run(make(), **conf), name + " again", BIT_KEYS + CG_KEYS)


def test_a_permuted_pair_list_gives_the_same_bits():
    first, other, moved = call("K49 default"), call("K49 permuted"), P.CALLS["K49 permuted"][0]()
    check(first, P.answer("K49 default"), "K = 49, default tolerance")
    same_bits(first, other, "pairs permuted", ("poses", "image_state") + INT_KEYS + CG_KEYS)
    for k in ("pair_state", "rotation_error", "direction_error"):
        assert np.array_equal(first[k][moved["order"]], other[k], equal_nan=True), k


# ---------------------------------------------------------------------- 7. the default solver is the call without the argument
def test_cholesky_is_the_call_without_the_argument():
    for inp in (G.scene(16, noise=0.3), G.edge_scene()[0]):
        plain, chol = run(inp, solver=None), run(inp, solver="cholesky")
        assert set(plain) == set(chol) == set(BIT_KEYS) and not any("cg" in k for k in plain)
        same_bits(plain, chol, "solver=\"cholesky\"")


# ---------------------------------------------------------------------- 8. the envelope
def test_the_envelope_4096_images():
    K = _cabi.LG_BA_PCG_MAX_IMAGES
    sc = G.scene(K, chords=7 * K)                           # exact relative poses: the scene is built in a second
    assert len(sc["pairs"]) == 8 * K
    conf = dict(num_iterations=6, rotation_cg_iterations=20, position_cg_iterations=60)
    got = run(sc, **conf)
    assert 1 <= got["rotation_iterations"] <= 6 and 1 <= got["position_iterations"] <= 6 and got["cg_failures"] == 0 and got["positions_ok"]
    posed = got["image_state"] == G.POSED
    assert got["num_posed"] == posed.sum() > 0.99 * K and np.isfinite(got["poses"][posed]).all() and np.isfinite(got["poses"][:, :, :3]).all()
    print("K = 4096: %d posed, solver iterations %d / %d, on the budget %d / %d" % (got["num_posed"], got["rotation_cg_iterations"], got["position_cg_iterations"],
                                                                                   got["rotation_cg_unconverged"], got["position_cg_unconverged"]))
    same_bits(got, run(sc, **conf), "K = 4096 again", BIT_KEYS + CG_KEYS)
    with pytest.raises(ValueError, match=r"\[2, %d\], got %d" % (K, K + 1)):        # before the GPU is touched: the inputs are host tensors
        GlobalPoseEstimator(solver="pcg").estimate(torch.from_numpy(sc["pairs"]), (torch.from_numpy(sc["R"]), torch.from_numpy(sc["t"])), K + 1)


# ---------------------------------------------------------------------- 9. the chain above 256 images
def test_the_chain_above_256_images():
    """exact relative poses between the images of the bundle adjuster's 300-image scene that share tracks -> global poses -> triangulation -> adjustment"""
    inp = BP.big_scene()
    K, N = inp["kpts"].shape[:2]
    true_poses, _ = O.cameras(K, BP.BIG_SEED)
    tid = inp["track_id"]
    rows = [dict() for _ in range(int(tid.max()) + 1)]
    for k, i in zip(*np.nonzero(tid >= 0)):
        rows[tid[k, i]][int(k)] = int(i)
    shared = {}
    for at in rows:
        seen = sorted(at)
        for x, a in enumerate(seen):
            for b in seen[x + 1:]:
                shared.setdefault((a, b), []).append((at[a], at[b]))
    pairs = np.asarray(sorted(shared), np.int64)
    m0 = np.full((len(pairs), N), -1, np.int64)
    for p, key in enumerate(sorted(shared)):
        for ra, rb in shared[key]:
            m0[p, ra] = rb
    Rw = true_poses[:, :, :3].astype(np.float64)
    cw = -np.einsum("kji,kj->ki", Rw, true_poses[:, :, 3].astype(np.float64))
    Rab, t = G.relative(Rw, cw, pairs)
    weights = np.asarray([len(shared[tuple(p)]) for p in pairs.tolist()], np.float32)
    est = GlobalPoseEstimator(solver="pcg").estimate(cuda(pairs), (cuda(Rab.astype(np.float32)), cuda(t.astype(np.float32))), K, weights=cuda(weights))
    assert est["num_posed"] == K and est["positions_ok"] and est["position_cg_unconverged"] == 0 and est["rotation_cg_unconverged"] == 0
    held = [est["origin"], est["baseline"]]
    feats, cams = {"keypoints": cuda(inp["kpts"])}, torch.from_numpy(inp["cams"])
    cost = {}
    for name, poses in (("estimated", est["poses"]), ("true", cuda(G.gauge_poses(true_poses, *held)))):
        tri = Triangulator(max_reproj_error=64.0).triangulate(feats, pairs.tolist(), cuda(m0), cams, poses)
        out = BundleAdjuster(solver="pcg", num_iterations=BP.BIG_ITERATIONS, max_cg_iterations=120).adjust(feats, tri, cams, poses, held)
        cost[name] = (out["final_cost"], out["num_observations"], tri["num_tracks"])
    print("chain: final cost %.6g over %d observations of %d tracks from the estimated poses, %.6g over %d of %d from the true ones: ratio %.4f" % (
        cost["estimated"] + cost["true"] + (cost["estimated"][0] / cost["true"][0],)))
    assert cost["estimated"][2] == cost["true"][2] == len(rows)
    assert cost["estimated"][0] <= CHAIN_COST_RATIO * cost["true"][0] * cost["estimated"][1] / cost["true"][1]
