"""RelativePoseEstimator on the GPU against the float64 definition (tests/relpose_oracle.py), against the two-view verifier and against itself.

Bars and where they come from (tests/test_relpose_cpu.py derives every figure without a GPU, from the oracle alone on the inputs of this file, over the
hypotheses whose sample is all planted inliers, and asserts that the constants below are those figures):
  Q_RESIDUAL 6.15e-04  the largest |d32 - d64| / t of a Sampson distance among the correspondences within 2 t, between the oracle's float64 run and its run
                       with the bearings formed in float32, the candidate rounded to float32 and the test evaluated in float32
  Q_MODEL    1.25e-04  the largest entry difference between the two runs' unit-norm pixel-space F
  Q_POSE_R   3.82e-08  the largest change of an entry of the oracle's R when one entry of the float32 E moves by one float32 ulp (either way)
  Q_POSE_T   3.54e-08  the same for t
  MARGIN = 8 Q_RESIDUAL, MODEL_MARGIN = 8 Q_MODEL, POSE_MARGIN_R / _T = 8 Q_POSE_R / _T.  A correspondence whose float64 residual lies within MARGIN t of t
  may fall on either side and is excluded from mask comparisons; which ones are excluded is decided by the float64 definition alone, and at most 2 % of a
  pair's correspondences may be (the CPU test asserts that for the oracle's own models on every input of this file).
The inputs are the cases of tests/relpose_oracle.py (640 x 480 scenes, noise 0.5, t = 3, 50 % planted; S = 5 and 8 fully planted; camera (500, 500, 320, 240) on
side 0, the same or (400, 400, 300, 250) on side 1), built without a GPU."""
import numpy as np
import pytest
import torch

import relpose_oracle as P
import lightglue_amd
from lightglue_amd import NearestNeighborMatcher, RelativePoseEstimator, TwoViewVerifier
from lightglue_amd import _cabi
from lightglue_amd._cabi import LightGlueAmdError

Q_RESIDUAL, Q_MODEL = 6.15e-4, 1.25e-4
Q_POSE_R, Q_POSE_T = 3.82e-8, 3.54e-8
MARGIN, MODEL_MARGIN, MAX_EXCLUDED = 8 * Q_RESIDUAL, 8 * Q_MODEL, 0.02
POSE_MARGIN_R, POSE_MARGIN_T = 8 * Q_POSE_R, 8 * Q_POSE_T
MAX_SOLVER_HYPS = 64            # all-inlier hypotheses compared per case in the solver test (S = 5, 8: every hypothesis is one)
KEYS = ("R", "t", "E", "models", "inliers0", "num_inliers", "num_in_front", "matches0", "best_hypothesis")

pytestmark = pytest.mark.gpu


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def pad(k):
    return np.concatenate([k, np.zeros((P.N0 - len(k), 2), np.float32)])


def list_inputs():
    """every case as one indexed list: store 0 holds the 7 image-0 sides, store 1 an unrelated image at index 0 (with a camera nothing may use), then the
    image-1 sides of the `same` and of the `other` cases; -> (feats0, feats1, cameras0, cameras1, pairs, matches0 [14, N0])"""
    same, other = [P.case(S, "same") for S in P.SIZES], [P.case(S, "other") for S in P.SIZES]
    rng = np.random.default_rng(77)
    # image-0 sides differ between the variants only where their scene seeds differ: keep one store image per case
    feats0 = {"keypoints": cuda(np.stack([c["kpts0"] for c in same + other]))}
    junk = rng.uniform(0, 480, (P.N0, 2)).astype(np.float32)
    feats1 = {"keypoints": cuda(np.stack([junk] + [pad(c["kpts1"]) for c in same + other])), "num_keypoints": torch.tensor([P.N0] + [P.N1] * 14, dtype=torch.int32)}
    cameras0 = torch.tensor([P.CAM0] * 14, dtype=torch.float32)
    cameras1 = torch.tensor([(123.0, 456.0, 7.0, 8.0)] + [P.CAMS1["same"]] * 7 + [P.CAMS1["other"]] * 7, dtype=torch.float32)
    pairs = [(i, i + 1) for i in range(14)]
    m0 = cuda(np.stack([c["matches0"] for c in same + other]))
    return feats0, feats1, cameras0, cameras1, pairs, m0


def run(hyps, refine, **kw):
    feats0, feats1, cameras0, cameras1, pairs, m0 = list_inputs()
    est = RelativePoseEstimator(threshold=P.T, num_hypotheses=hyps, refine=refine, seed=P.SEED)
    return est.estimate_pairs(feats0, pairs, {"matches0": m0}, cameras0, feats1, cameras1, **kw)


@pytest.fixture(scope="module")
def outputs():
    """the four configurations of the end-to-end tests, each run once"""
    return {(hyps, refine): run(hyps, refine) for hyps in P.HYPS for refine in (False, True)}


def host(out, b):
    return {k: out[k][b].cpu().numpy() for k in KEYS}


def same(a, b, what=""):
    for k in KEYS:
        assert torch.equal(a[k], b[k]), (what, k)
    assert len(a["matches"]) == len(b["matches"]) and all(torch.equal(x, y) for x, y in zip(a["matches"], b["matches"])), what


def check_consistent(got, c, what):
    """the returned mask is the float64 mask of the RETURNED F outside the margin; count, matches0 and the rows off the correspondence list agree with it"""
    corr, rows = c["corr"], c["rows"]
    model = got["models"].reshape(9).astype(np.float64)
    assert np.isfinite(model).all() and abs(np.linalg.norm(model) - 1) < 1e-5 and model[np.argmax(abs(model))] > 0, what
    want = P.inlier_mask(P.KIND, model, corr, P.T)
    d = P.distances(P.KIND, model, corr)
    near = abs(d - P.T) <= MARGIN * P.T
    assert near.mean() <= MAX_EXCLUDED, (what, near.mean())
    mask = got["inliers0"]
    assert (mask[rows] == want)[~near].all(), (what, int((mask[rows] != want)[~near].sum()))
    assert mask.sum() == mask[rows].sum() == got["num_inliers"], what
    assert (got["matches0"] == np.where(mask, c["matches0"], -1)).all(), what
    return d


def check_empty(got, what):
    assert got["num_inliers"] == 0 and not got["inliers0"].any() and (got["matches0"] == -1).all() and got["best_hypothesis"] == -1 and got["num_in_front"] == 0, what
    for k in ("R", "t", "E", "models"):
        assert (got[k] == 0).all(), (what, k)


# ---------------------------------------------------------------------- 1. the solver stage
def test_solver_candidates_hold_every_oracle_solution():
    hyps = max(P.HYPS)
    cand = run(hyps, False, return_candidates=True)["candidates"].cpu().numpy().reshape(14, hyps, P.ROOTS, 9)
    assert np.isfinite(cand).all()
    nz = (cand != 0).any(-1)
    flat = cand[nz].astype(np.float64)
    assert (abs(np.linalg.norm(flat, axis=1) - 1) < 1e-5).all() and (flat[np.arange(len(flat)), np.argmax(abs(flat), 1)] > 0).all()
    checked = skipped = 0
    for b, (S, variant) in enumerate(P.CASES):
        r64 = P.case_oracle(S, variant, hyps, False)
        sep = P.separation(r64["models"], r64["valid"])
        allin = np.nonzero(P.all_inlier(S, variant, hyps))[0][:MAX_SOLVER_HYPS]
        assert len(allin) >= 5
        for h in allin:
            for r in np.nonzero(r64["valid"][h])[0]:
                if sep[h, r] < 10 * MODEL_MARGIN:
                    skipped += 1
                    continue
                checked += 1
                diff = abs(cand[b, h].astype(np.float64) - r64["models"][h, r]).max(-1)
                assert diff.min() <= MODEL_MARGIN, (S, variant, h, r, diff.min())
    print("oracle solutions compared %d, skipped for a neighbour within 10 MODEL_MARGIN %d (%.1f %%)" % (checked, skipped, 100.0 * skipped / (checked + skipped)))
    assert checked >= 300


# ---------------------------------------------------------------------- 2. the exact tie to the verifier's scoring
def test_scoring_is_the_verifiers_scoring(outputs):
    feats0, feats1, _, _, pairs, m0 = list_inputs()
    for (hyps, refine), out in outputs.items():
        models = out["models"][:, None].expand(-1, 256, -1, -1).contiguous()
        ref = TwoViewVerifier(model="fundamental", threshold=P.T, num_hypotheses=256, refine=False).score_models(feats0, pairs, m0, models, feats1)
        for k in ("inliers0", "num_inliers", "matches0"):
            assert torch.equal(ref[k], out[k]), (hyps, refine, k)
        assert torch.equal(ref["models"], out["models"])          # already in output form


# ---------------------------------------------------------------------- 3. end to end
@pytest.mark.parametrize("hyps", P.HYPS)
def test_end_to_end(outputs, hyps):
    for b, (S, variant) in enumerate(P.CASES):
        c = P.case(S, variant)
        plain, refined = host(outputs[hyps, False], b), host(outputs[hyps, True], b)
        allin = P.all_inlier(S, variant, hyps)
        shrunk = P.verify(c["corr"], c["cam0"], c["cam1"], P.T * (1 - MARGIN), hyps, P.SEED, False)
        bound = int(shrunk["counts"][allin].max()) if allin.any() else 0
        for refine, got in ((False, plain), (True, refined)):
            what = (S, variant, hyps, refine)
            print(what, "count", int(got["num_inliers"]), "oracle", P.case_oracle(S, variant, hyps, refine)["count"], "bound", bound, "hypothesis", int(got["best_hypothesis"]))
            d = check_consistent(got, c, what)
            assert got["num_inliers"] >= bound, (what, got["num_inliers"], bound)
            assert (d[c["planted"]] <= P.T).mean() >= 0.95, (what, (d[c["planted"]] <= P.T).mean())
            assert (outputs[hyps, refine]["matches"][b].cpu().numpy() == np.stack([np.nonzero(got["inliers0"])[0], got["matches0"][got["inliers0"]]], -1)).all(), what
        assert refined["num_inliers"] >= plain["num_inliers"], (S, variant, hyps)
        assert refined["best_hypothesis"] == plain["best_hypothesis"]


# ---------------------------------------------------------------------- 4. pose consistency
def test_pose_is_the_definitions_pose_of_the_returned_essential_matrix(outputs):
    for (hyps, refine), out in outputs.items():
        for b, (S, variant) in enumerate(P.CASES):
            c, got, what = P.case(S, variant), host(out, b), (S, variant, hyps, refine)
            R, t, E = got["R"].astype(np.float64), got["t"].astype(np.float64), got["E"].reshape(9)
            assert abs(R @ R.T - np.eye(3)).max() < 1e-6 and abs(np.linalg.det(R) - 1) < 1e-6 and abs(np.linalg.norm(t) - 1) < 1e-6, what
            wantR, wantt, nif, counts = P.pose(E, c["corr"], got["inliers0"][c["rows"]], c["cam0"], c["cam1"])
            assert counts[-1] > counts[-2], (what, counts)                 # nothing rests on a tie between decompositions
            assert abs(R - wantR).max() <= POSE_MARGIN_R and abs(t - wantt).max() <= POSE_MARGIN_T, (what, abs(R - wantR).max(), abs(t - wantt).max())
            assert got["num_in_front"] == nif and 0 < nif <= got["num_inliers"], (what, got["num_in_front"], nif)
            back = P.essential_of(got["models"].reshape(9), c["cam0"], c["cam1"])
            assert abs(np.linalg.norm(E.astype(np.float64)) - 1) < 1e-5 and E[np.argmax(abs(E))] > 0 and abs(E - back).max() <= MODEL_MARGIN, what


# ---------------------------------------------------------------------- 5. position independence
def test_a_pair_is_independent_of_its_list():
    feats0, feats1, cameras0, cameras1, pairs, m0 = list_inputs()
    est = RelativePoseEstimator(threshold=P.T, num_hypotheses=512, refine=True, seed=3)
    pick = [2, 9, 13, 6, 10]                                            # S = 65 same, 65 other, 1000 other, 1000 same, 255 other
    sub, res = [pairs[p] for p in pick], m0[pick]
    whole = est.estimate_pairs(feats0, sub, res, cameras0, feats1, cameras1)
    assert int((whole["num_inliers"] > 0).sum()) == 5
    for at in range(5):
        alone = est.estimate_pairs(feats0, sub[at:at + 1], res[at:at + 1], cameras0, feats1, cameras1)
        for k in KEYS:
            assert torch.equal(alone[k][0], whole[k][at]), (at, k)
        assert torch.equal(alone["matches"][0], whole["matches"][at])
    perm = [4, 2, 0, 3, 1, 0]                                           # the front pair to the back, the back pair to the front, and a duplicate
    shuffled = est.estimate_pairs(feats0, [sub[p] for p in perm], res[perm], cameras0, feats1, cameras1)
    for at, p in enumerate(perm):
        for k in KEYS:
            assert torch.equal(shuffled[k][at], whole[k][p]), (p, k)
    same(est.estimate_pairs(feats0, sub, res, cameras0, feats1, cameras1), whole, "two calls with one seed")
    same(est.estimate_pairs(feats0, torch.tensor(sub, device="cuda"), res, cameras0, feats1, cameras1, validate=False), whole, "a device pair list")
    K1 = torch.zeros(15, 3, 3)
    K1[:, 0, 0], K1[:, 1, 1], K1[:, 0, 2], K1[:, 1, 2], K1[:, 2, 2] = cameras1[:, 0], cameras1[:, 1], cameras1[:, 2], cameras1[:, 3], 1.0
    same(est.estimate_pairs(feats0, sub, res, cameras0, feats1, K1), whole, "calibration matrices")
    reseeded = RelativePoseEstimator(threshold=P.T, num_hypotheses=512, refine=True, seed=4).estimate_pairs(feats0, sub, res, cameras0, feats1, cameras1)
    assert not torch.equal(reseeded["best_hypothesis"], whole["best_hypothesis"])
    # a pair of the list is the forward call on its own images and cameras
    i0, i1 = [p[0] for p in sub], [p[1] for p in sub]
    data = {"image0": {"keypoints": feats0["keypoints"][i0]}, "image1": {"keypoints": feats1["keypoints"][i1], "num_keypoints": feats1["num_keypoints"][i1]}}
    fwd = est(data, res, cameras0[i0], cameras1[i1])
    for k in KEYS:
        assert torch.equal(fwd[k], whole[k]), k


# ---------------------------------------------------------------------- 6. edges
def test_empty_results_and_statuses():
    feats0, feats1, cameras0, cameras1, pairs, m0 = list_inputs()
    est = RelativePoseEstimator(threshold=P.T, num_hypotheses=256, refine=True)
    good = est.estimate_pairs(feats0, pairs[:3], m0[:3], cameras0, feats1, cameras1)
    # four matches and none
    few = m0[:3].clone()
    few[1] = -1
    few[2] = -1
    rows = torch.nonzero(m0[2] >= 0)[:4, 0]
    few[2, rows] = m0[2, rows]
    out = est.estimate_pairs(feats0, pairs[:3], few, cameras0, feats1, cameras1)
    check_empty(host(out, 1), "no match")
    check_empty(host(out, 2), "four matches")
    for k in KEYS:
        assert torch.equal(out[k][0], good[k][0]), k
        assert torch.isfinite(out[k].float()).all(), k
    # an index outside its store
    with pytest.raises(ValueError, match=r"pairs \[1\] index outside the feature stores of 14 and 15 images"):
        est.estimate_pairs(feats0, [(0, 1), (1, 15), (2, 3)], m0[:3], cameras0, feats1, cameras1)
    with pytest.raises(LightGlueAmdError, match=r"pair 1: an image index outside its feature store") as err:
        est.estimate_pairs(feats0, torch.tensor([(0, 1), (1, 15), (2, 3)], device="cuda"), m0[:3], cameras0, feats1, cameras1, validate=False)
    check_empty(host(err.value.outputs, 1), "index")
    for p in (0, 2):
        for k in KEYS:
            assert torch.equal(err.value.outputs[k][p], good[k][p]), (p, k)
    # a camera without a focal length: that pair only, with its own status
    bad = cameras1.clone()
    bad[2, 0] = 0.0
    with pytest.raises(LightGlueAmdError, match=r"pair 1: a camera whose focal length") as err:
        est.estimate_pairs(feats0, pairs[:3], m0[:3], cameras0, feats1, bad)
    check_empty(host(err.value.outputs, 1), "camera")
    for p in (0, 2):
        for k in KEYS:
            assert torch.equal(err.value.outputs[k][p], good[k][p]), (p, k)
    for value in (float("nan"), float("inf"), -500.0):
        bad[2, 0] = value
        with pytest.raises(LightGlueAmdError, match=r"pair 1: a camera"):
            est.estimate_pairs(feats0, pairs[:3], m0[:3], cameras0, feats1, bad)
    with pytest.raises(ValueError, match="zero skew"):
        est.estimate_pairs(feats0, pairs[:3], m0[:3], torch.eye(3).repeat(14, 1, 1) + torch.tensor([[0.0, 0.1, 0], [0, 0, 0], [0, 0, 0]]), feats1, cameras1)
    with pytest.raises(ValueError, match=r"cameras1 must have shape \[15, 4\]"):
        est.estimate_pairs(feats0, pairs[:3], m0[:3], cameras0, feats1)             # cameras1 = cameras0 does not cover store 1
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        est.estimate_pairs({"keypoints": feats0["keypoints"].cpu()}, pairs[:1], m0[:1].cpu(), cameras0, {"keypoints": feats1["keypoints"].cpu()}, cameras1)


EDGE_N0 = 300                               # not a multiple of 256
EDGE_SIZES = (4, 5, 7, 8, 257)              # below the sample, the sample, below and at the refit threshold, one past the 256-row tile


@pytest.mark.parametrize("S", EDGE_SIZES)
def test_list_lengths_at_the_thresholds(S):
    """the S = 1000 scene (K0 != K1) cut to its first EDGE_N0 image-0 rows and thinned to the first S correspondences among them"""
    c = P.case(1000, "other")
    rows = c["rows"][c["rows"] < EDGE_N0][:S]
    assert len(rows) == S
    m0 = np.full(EDGE_N0, -1, np.int64)
    m0[rows] = c["matches0"][rows]
    c = dict(c, matches0=m0, rows=rows, corr=c["corr"][:S], planted=c["planted"][:S])
    data = {"image0": {"keypoints": cuda(c["kpts0"][None, :EDGE_N0])}, "image1": {"keypoints": cuda(c["kpts1"][None])}}
    cams = torch.tensor([P.CAM0]), torch.tensor([P.CAMS1["other"]])
    outs = {refine: RelativePoseEstimator(threshold=P.T, num_hypotheses=256, refine=refine, seed=P.SEED)(data, cuda(m0[None]), *cams) for refine in (False, True)}
    plain, refined = host(outs[False], 0), host(outs[True], 0)          # status LG_OK: nothing was raised
    if S < P.SAMPLE:
        check_empty(plain, S)
        check_empty(refined, S)
        return
    allin = c["planted"][P.sample(P.SEED, 256, S, P.SAMPLE)].all(1)
    shrunk = P.verify(c["corr"], c["cam0"], c["cam1"], P.T * (1 - MARGIN), 256, P.SEED, False)
    bound = int(shrunk["counts"][allin].max()) if allin.any() else 0
    for refine, got in ((False, plain), (True, refined)):
        what = (S, refine)
        if got["num_inliers"] == 0:
            check_empty(got, what)
            continue
        d = check_consistent(got, c, what)
        print(what, "count", int(got["num_inliers"]), "bound", bound, "within the margin %.4f (at most %.2f)" % ((abs(d - P.T) <= MARGIN * P.T).mean(), MAX_EXCLUDED))
        assert got["num_inliers"] >= bound, (what, got["num_inliers"], bound)
        assert (outs[refine]["matches"][0].cpu().numpy() == np.stack([np.nonzero(got["inliers0"])[0], got["matches0"][got["inliers0"]]], -1)).all(), what
        # the scoring is the verifier's, at these lengths too
        models = outs[refine]["models"][:, None].expand(-1, 256, -1, -1).contiguous()
        ref = TwoViewVerifier(model="fundamental", threshold=P.T, num_hypotheses=256, refine=False).score_models(data["image0"], [(0, 0)], cuda(m0[None]), models, data["image1"])
        for k in ("inliers0", "num_inliers", "matches0", "models"):
            assert torch.equal(ref[k], outs[refine][k]), (what, k)
    assert refined["num_inliers"] >= plain["num_inliers"] and refined["best_hypothesis"] == plain["best_hypothesis"], S
    if plain["num_inliers"] < P.REFIT_MIN:                              # no refit below 8 inliers: at S = 5 and 7 never
        same(outs[True], outs[False], (S, "no refit"))
    assert S >= P.REFIT_MIN or plain["num_inliers"] < P.REFIT_MIN


def test_num_keypoints_is_honoured():
    c = P.case(65, "same")
    num0, num1 = 1000, 1040
    junk = c["matches0"].copy()
    free = np.nonzero(junk < 0)[0]
    junk[free[:40]] = [P.N1 + 5, 10 ** 12, P.N0, 2 ** 31, 2 ** 32 + 3] * 8              # >= n1 (the store holds N0 rows per image)
    junk[free[40:60]] = np.arange(num1, num1 + 20)                                      # >= num_keypoints1
    junk[num0:] = np.arange(P.N0 - num0)                                                # rows >= num_keypoints0
    clean = np.where((np.arange(P.N0) < num0) & (junk >= 0) & (junk < num1), junk, -1)
    assert (clean >= 0).sum() >= 50 and (junk != clean).sum() >= 100
    tail = np.concatenate([c["kpts1"], np.full((P.N0 - P.N1, 2), np.nan, np.float32)])   # rows nothing may read
    feats = {"keypoints": cuda(np.stack([c["kpts0"], tail])), "num_keypoints": torch.tensor([num0, num1])}
    cams = torch.tensor([P.CAM0, P.CAMS1["same"]])
    est = RelativePoseEstimator(threshold=P.T, num_hypotheses=256, refine=True)
    a, b = est.estimate_pairs(feats, [(0, 1)], cuda(junk[None]), cams), est.estimate_pairs(feats, [(0, 1)], cuda(clean[None]), cams)
    same(a, b, "junk against clean")
    assert int(a["num_inliers"][0]) > 0
    rows, _ = P.correspondences(c["kpts0"], tail, junk, num0, num1)
    got = host(a, 0)
    assert got["inliers0"].sum() == got["inliers0"][rows].sum()


def test_behind_the_nn_matcher_deferred_or_not():
    c = P.case(P.TV.TILE + 1, "same")
    rng = np.random.default_rng(21)
    d0, d1 = rng.standard_normal((P.N0, 64)), rng.standard_normal((P.N0, 64))
    d1[c["matches0"][c["rows"]]] = d0[c["rows"]] + 0.05 * rng.standard_normal((len(c["rows"]), 64))      # descriptors follow the scene's correspondences
    store = {"keypoints": cuda(np.stack([c["kpts0"], pad(c["kpts1"])])), "descriptors": cuda(np.stack([d0, d1]).astype(np.float32)), "num_keypoints": torch.tensor([P.N0, P.N1])}
    pairs = [(0, 1), (1, 0)]
    matcher = NearestNeighborMatcher(mutual=True, distance_threshold=0.5)
    result = matcher.match_pairs(store, pairs)
    assert (result["matches0"][0].cpu().numpy() == c["matches0"]).all()                # exactly the scene's correspondences: the case's oracle applies
    cams = torch.tensor([P.CAM0, P.CAMS1["same"]])
    est = RelativePoseEstimator(threshold=P.T, num_hypotheses=512, refine=True, seed=P.SEED)
    out = lightglue_amd.estimate_poses(est, result, store, pairs, cams)
    same(out, est.estimate_pairs(store, pairs, result, cams), "glue.estimate_poses")
    same(out, est.estimate_pairs(store, pairs, result["matches0"], cams), "matches0 itself")
    same(lightglue_amd.estimate_poses(est, matcher.match_pairs(store, pairs, deferred=True), store, pairs, cams), out, "a deferred result")
    d = check_consistent(host(out, 0), c, "nn")
    assert (d[c["planted"]] <= P.T).mean() >= 0.95
    # the reverse pair is the reverse motion: R^T and -R^T t, as far as two separate minimal-sample searches agree
    R01, R10 = out["R"][0].double().cpu().numpy(), out["R"][1].double().cpu().numpy()
    assert int(out["num_inliers"][1]) > 0 and np.degrees(np.arccos(np.clip((np.trace(R01 @ R10) - 1) / 2, -1, 1))) < 10.0
