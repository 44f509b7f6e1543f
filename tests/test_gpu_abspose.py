"""AbsolutePoseEstimator on the GPU against the float64 definition (tests/abspose_oracle.py) and against itself.

Bars and where they come from (tests/test_abspose_cpu.py derives every figure without a GPU, from the oracle alone on the inputs of this file, over the
hypotheses whose sample is all planted, and asserts that the constants below are those figures):
  Q_RESIDUAL 3.42e-04  the largest |d32 - d64| / t of a reprojection distance among the correspondences within 2 t, between the oracle's float64 run and its
                       run with float32 centring, bearings, candidates and test
  Q_POSE_R   2.45e-06  the largest entry difference between the two runs' candidate rotations (world frame)
  Q_POSE_T   2.34e-04  the same for the translations: |c| ~ 113 carries a rotation difference into t = t' - R c
  Q_REFINE_R 1.20e-07  the largest change of an entry of the refined R when one entry of the float32 starting pose moves by one float32 ulp (either way), plus
                       half a float32 ulp: the rounding of the output
  Q_REFINE_T 1.02e-05  the same for t
  MARGIN = 8 Q_RESIDUAL, POSE_MARGIN_R / _T = 8 Q_POSE_R / _T, REFINE_MARGIN_R / _T = 8 Q_REFINE_R / _T: the factor the two earlier rows use for accumulation
  order and fmaf placement.  A correspondence whose float64 reprojection error lies within MARGIN t of t may fall on either side and is excluded from mask
  comparisons; which ones are excluded is decided by the float64 definition alone, and at most 2 % of a problem's correspondences may be (the CPU test
  asserts that for the oracle's own poses on every input of this file).  SOLVER_FLOOR is the oracle's own count of the candidates the solver test compares.
The inputs are the cases of tests/abspose_oracle.py (640 x 480 scenes, camera (500, 500, 320, 240) about 5 units from a box of world points centred at
(100, -50, 20), noise 0.5, t = 3, 50 % planted; S = 3 and 6 fully planted; NaN rows in points3d1, some of them matched), built without a GPU: seven pairs posed
one by one and five queries pooled over nine database images."""
import numpy as np
import pytest
import torch

import abspose_oracle as A
import lightglue_amd
from lightglue_amd import AbsolutePoseEstimator, NearestNeighborMatcher
from lightglue_amd._cabi import LightGlueAmdError

Q_RESIDUAL, Q_POSE_R, Q_POSE_T = 3.42e-4, 2.45e-6, 2.34e-4
Q_REFINE_R, Q_REFINE_T = 1.20e-7, 1.02e-5
MARGIN, MAX_EXCLUDED = 8 * Q_RESIDUAL, 0.02
POSE_MARGIN_R, POSE_MARGIN_T = 8 * Q_POSE_R, 8 * Q_POSE_T
REFINE_MARGIN_R, REFINE_MARGIN_T = 8 * Q_REFINE_R, 8 * Q_REFINE_T
SOLVER_FLOOR = 1255
PROBLEM_KEYS = ("R", "t", "num_inliers", "best_hypothesis")
PAIR_KEYS = ("inliers0", "pair_num_inliers", "matches0")
KEYS = PROBLEM_KEYS + PAIR_KEYS
NQ = len(A.SIZES)                                        # the per-pair cases: query q against database image q + 1

pytestmark = pytest.mark.gpu


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def stores():
    """query store: the 7 per-pair cases, then the 5 pooled queries; database store: an unrelated image at index 0 (all its points NaN), the 7 cases' images,
    then the 9 pooled ones; -> (feats0, feats1, cameras [12, 4], points [17, N1, 3])"""
    cases, pr = [A.case(S) for S in A.SIZES], A.pooled()
    feats0 = {"keypoints": cuda(np.concatenate([np.stack([c["kpts0"] for c in cases]), pr["kpts0"]]))}
    points = np.concatenate([np.full((1, A.N1, 3), np.nan, np.float32), np.stack([c["points"] for c in cases]), pr["points"]])
    feats1 = {"num_keypoints": torch.full((len(points),), A.N1, dtype=torch.int32)}
    cameras = torch.tensor(np.concatenate([np.stack([c["cam"] for c in cases]), pr["cams"]]))
    return feats0, feats1, cameras, cuda(points)


def pair_list():
    """(pairs [7], matches0 [7, N0]) of the per-pair cases"""
    return [(i, i + 1) for i in range(NQ)], cuda(np.stack([A.case(S)["matches0"] for S in A.SIZES]))


def pool_list():
    """(pairs [9, 2] on the device, one of them with a database index outside the store, matches0 [9, N0]) of the pooled cases"""
    pr = A.pooled()
    pairs = pr["pairs"] + np.array([NQ, NQ + 1])
    pairs[pr["bad"], 1] = 1 + NQ + 9
    return torch.from_numpy(pairs).cuda(), cuda(pr["matches0"])


def run(hyps, refine, seed=A.SEED, **kw):
    feats0, feats1, cameras, points = stores()
    pairs, m0 = pair_list()
    return AbsolutePoseEstimator(threshold=A.T, num_hypotheses=hyps, refine=refine, seed=seed).estimate_pairs(feats0, pairs, {"matches0": m0}, cameras, points, feats1, **kw)


def run_pool(hyps, refine, **kw):
    """the pooled list always ends in an error that names the pair with the bad index and the pair of the query with the bad camera: -> (outputs, message)"""
    feats0, feats1, cameras, points = stores()
    pairs, m0 = pool_list()
    with pytest.raises(LightGlueAmdError) as err:
        AbsolutePoseEstimator(threshold=A.T, num_hypotheses=hyps, refine=refine, seed=A.SEED).estimate_pairs(feats0, pairs, m0, cameras, points, feats1, pool=True, validate=False, **kw)
    return err.value.outputs, str(err.value)


@pytest.fixture(scope="module")
def outputs():
    """the four configurations of the end-to-end tests, each run once: (per pair, pooled)"""
    return {(hyps, refine): (run(hyps, refine), run_pool(hyps, refine)[0]) for hyps in A.HYPS for refine in (False, True)}


def views(outs):
    """every problem of `outs` = (per pair, pooled) as the oracle numbers it: {name: dict(R, t, num_inliers, best_hypothesis, mask [S] in the problem's order,
    consistent: masks, counts, matches0 and the ragged lists of its pairs agree)}"""
    plain, pool = outs
    pr = A.pooled()
    out = {}
    for b, S in enumerate(A.SIZES):
        c = A.case(S)
        inl, m0 = plain["inliers0"][b].cpu().numpy(), plain["matches0"][b].cpu().numpy()
        ok = (m0 == np.where(inl, c["matches0"], -1)).all() and inl.sum() == inl[c["rows"]].sum() == int(plain["pair_num_inliers"][b])
        ok = ok and (plain["matches"][b].cpu().numpy() == np.stack([np.nonzero(inl)[0], m0[inl]], -1)).all()
        out["pair", S] = dict({k: plain[k][b].cpu().numpy() for k in PROBLEM_KEYS}, mask=inl[c["rows"]], consistent=bool(ok))
    queries = pool["queries"].tolist()
    inl, m0 = pool["inliers0"].cpu().numpy(), pool["matches0"].cpu().numpy()
    for q, p in pr["problems"].items():
        g = queries.index(NQ + q)
        members = [i for i in range(len(pr["pairs"])) if pr["pairs"][i, 0] == q and not pr["bad"][i]]
        assert all(int(pool["group_of_pair"][i]) == g for i in members)
        at = np.asarray(members, int)[p["place"]] if len(p["place"]) else np.zeros(0, int)
        mask = inl[at, p["rows"]]
        ok = all((m0[i] == np.where(inl[i], pr["matches0"][i], -1)).all() and inl[i].sum() == int(pool["pair_num_inliers"][i]) for i in range(len(pr["pairs"])) if pr["pairs"][i, 0] == q)
        ok = ok and mask.sum() == sum(inl[i].sum() for i in range(len(pr["pairs"])) if pr["pairs"][i, 0] == q)
        out["pool", q] = dict({k: pool[k][g].cpu().numpy() for k in PROBLEM_KEYS}, mask=mask, consistent=bool(ok))
    return out


def world_pose(v):
    return np.concatenate([v["R"].astype(np.float64), v["t"].astype(np.float64)[:, None]], 1).reshape(12)


def check_consistent(v, corr, cam, what):
    """the returned mask is the float64 mask of the RETURNED pose outside the margin; counts, matches0 and the ragged lists agree with it"""
    R = v["R"].astype(np.float64)
    assert np.isfinite(world_pose(v)).all() and abs(R @ R.T - np.eye(3)).max() < 1e-6 and abs(np.linalg.det(R) - 1) < 1e-6, what
    d = A.distances(world_pose(v), corr, cam)
    near = abs(d - A.T) <= MARGIN * A.T
    assert near.mean() <= MAX_EXCLUDED, (what, near.mean())
    assert (v["mask"] == (d <= A.T))[~near].all(), (what, int((v["mask"] != (d <= A.T))[~near].sum()))
    assert v["consistent"] and v["mask"].sum() == v["num_inliers"], what
    return d


def check_empty(v, what):
    assert v["num_inliers"] == 0 and not v["mask"].any() and v["best_hypothesis"] == -1 and (v["R"] == 0).all() and (v["t"] == 0).all() and v["consistent"], what


# ---------------------------------------------------------------------- 1. the solver stage
def test_solver_candidates_hold_every_oracle_root():
    hyps = max(A.HYPS)
    cand = np.concatenate([run(hyps, False, return_candidates=True)["candidates"].cpu().numpy(), run_pool(hyps, False, return_candidates=True)[0]["candidates"].cpu().numpy()])
    assert cand.shape == (NQ + 5, hyps, A.ROOTS, 3, 4) and np.isfinite(cand).all()
    nz = (cand != 0).any((-1, -2))
    R = cand[nz][:, :, :3].astype(np.float64)
    assert abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-6 and (np.linalg.det(R) > 0).all() and nz[:NQ].any(-1).mean() > 0.9
    cand = cand.reshape(NQ + 5, hyps, A.ROOTS, 12).astype(np.float64)
    checked = skipped = 0
    for name, corr, cam, planted, oracle in A.problems():
        g = A.SIZES.index(name[1]) if name[0] == "pair" else NQ + name[1]
        allin = A.all_inlier_of(planted, len(corr), hyps)
        todo, n, skip = A.solver_roots_to_compare(oracle(hyps, False), allin, 10 * POSE_MARGIN_R)
        for h, r, want in todo:
            dR, dt = A.pose_difference(cand[g, h], want)
            assert ((dR <= POSE_MARGIN_R) & (dt <= POSE_MARGIN_T)).any(), (name, h, r, dR.min(), dt.min())
        checked, skipped = checked + n, skipped + skip
    print("oracle candidates compared %d, skipped for a neighbour within 10 POSE_MARGIN_R %d (%.1f %%)" % (checked, skipped, 100.0 * skipped / (checked + skipped)))
    assert checked >= SOLVER_FLOOR > 0


# ---------------------------------------------------------------------- 2. the scoring stage on its own
def test_scoring_the_returned_poses_gives_the_same_bits(outputs):
    feats0, feats1, cameras, points = stores()
    pairs, m0 = pair_list()
    ppairs, pm0 = pool_list()
    scorer = AbsolutePoseEstimator(threshold=A.T, num_hypotheses=256, refine=False)
    for (hyps, refine), (plain, pool) in outputs.items():
        poses = torch.cat([plain["R"], plain["t"][:, :, None]], 2)[:, None].expand(-1, 256, -1, -1).contiguous()
        ref = scorer.score_poses(feats0, pairs, m0, cameras, points, poses, feats1)
        for k in KEYS:
            want = torch.where(plain[k] < 0, plain[k], torch.zeros_like(plain[k])) if k == "best_hypothesis" else plain[k]      # the winner is hypothesis 0 now
            assert torch.equal(ref[k], want), (hyps, refine, k)
        poses = torch.cat([pool["R"], pool["t"][:, :, None]], 2)[:, None].expand(-1, 256, -1, -1).contiguous()
        with pytest.raises(LightGlueAmdError) as err:
            scorer.score_poses(feats0, ppairs, pm0, cameras, points, poses, feats1, pool=True, validate=False)
        for k in ("R", "t", "num_inliers") + PAIR_KEYS:
            assert torch.equal(err.value.outputs[k], pool[k]), (hyps, refine, k)


def test_given_poses_are_scored_as_the_definition_scores_them():
    """random poses, the planted pose at 5 and its copy at 9 (the lower index wins), an all-zero and a non-finite one: the oracle's float32 run of the same"""
    feats0, feats1, cameras, points = stores()
    pairs, m0 = pair_list()
    rng = np.random.default_rng(11)
    given = np.zeros((NQ, 256, 12), np.float32)
    for b, S in enumerate(A.SIZES):
        c = A.case(S)
        g = rng.standard_normal((256, 12))
        g[5] = g[9] = np.concatenate([c["R"], c["t"][:, None]], 1).reshape(12)
        g[0], g[1, 3] = 0.0, np.nan
        given[b] = g
    out = AbsolutePoseEstimator(threshold=A.T, num_hypotheses=256, refine=False).score_poses(feats0, pairs, m0, cameras, points, cuda(given.reshape(NQ, 256, 3, 4)), feats1)
    for b, S in enumerate(A.SIZES):
        c = A.case(S)
        want = A.verify(c["corr"], c["cam"], A.T, 256, given=given[b], dtype=np.float32)
        assert int(out["best_hypothesis"][b]) == want["best_hypothesis"] == 5, S
        d = A.distances(given[b, 5], c["corr"], c["cam"])
        near = abs(d - A.T) <= MARGIN * A.T
        got = out["inliers0"][b].cpu().numpy()[c["rows"]]
        assert (got == want["mask"])[~near].all() and abs(int(out["num_inliers"][b]) - want["count"]) <= near.sum() and want["count"] >= 0.45 * S, S
        assert (out["R"][b].cpu().numpy().reshape(9) == given[b, 5].reshape(3, 4)[:, :3].reshape(9)).all() and (out["t"][b].cpu().numpy() == given[b, 5].reshape(3, 4)[:, 3]).all()


# ---------------------------------------------------------------------- 3. end to end
@pytest.mark.parametrize("hyps", A.HYPS)
def test_end_to_end(outputs, hyps):
    plain_all, refined_all = views(outputs[hyps, False]), views(outputs[hyps, True])
    for name, corr, cam, planted, oracle in A.problems():
        allin = A.all_inlier_of(planted, len(corr), hyps)
        shrunk = A.verify(corr, cam, A.T * (1 - MARGIN), hyps, A.SEED, False)
        bound = int(shrunk["counts"][allin].max()) if allin.any() else 0
        for refine, got in ((False, plain_all[name]), (True, refined_all[name])):
            what = (name, hyps, refine)
            print(what, "count", int(got["num_inliers"]), "oracle", oracle(hyps, refine)["count"], "bound", bound, "hypothesis", int(got["best_hypothesis"]))
            d = check_consistent(got, corr, cam, what)
            assert got["num_inliers"] >= bound, (what, got["num_inliers"], bound)
            assert (d[planted] <= A.T).mean() >= 0.95, (what, (d[planted] <= A.T).mean())
        assert refined_all[name]["num_inliers"] >= plain_all[name]["num_inliers"], (name, hyps)
        assert refined_all[name]["best_hypothesis"] == plain_all[name]["best_hypothesis"]
    for refined in (plain_all, refined_all):
        check_empty(refined["pool", 2], "a query without a correspondence")
        check_empty(refined["pool", 4], "a query with a bad camera")


# ---------------------------------------------------------------------- 4. the refinement is the definition's, from the GPU's own winner
def test_refined_pose_is_the_definitions_refinement_of_the_winner(outputs):
    compared = 0
    for hyps in A.HYPS:
        plain_all, refined_all = views(outputs[hyps, False]), views(outputs[hyps, True])
        for name, corr, cam, planted, oracle in A.problems():
            plain, refined = plain_all[name], refined_all[name]
            if plain["num_inliers"] < A.REFINE_MIN or (world_pose(plain) == world_pose(refined)).all():
                continue                                             # nothing refined, or the refinement was dropped
            c, cc = A.centre(corr, np.float32)
            start = A.to_centred(world_pose(plain), c, np.float32)   # the winner's candidate up to one ulp of t': what Q_REFINE_* measure
            want = A.to_world(A.refine(cc, plain["mask"], start, cam), c)
            dR, dt = A.pose_difference(world_pose(refined), want)
            print(name, hyps, "refined against the definition: dR %.2e dt %.2e" % (dR, dt))
            assert dR <= REFINE_MARGIN_R and dt <= REFINE_MARGIN_T, (name, hyps, dR, dt)
            compared += 1
    assert compared >= 12


# ---------------------------------------------------------------------- 5. position independence, and pooling is concatenation
def test_a_problem_is_independent_of_its_list():
    feats0, feats1, cameras, points = stores()
    pairs, m0 = pair_list()
    est = AbsolutePoseEstimator(threshold=A.T, num_hypotheses=512, refine=True, seed=3)
    pick = [2, 6, 3, 5, 1]                                              # S = 65, 1000, 255, 257, 6
    sub, res = [pairs[p] for p in pick], m0[pick]
    whole = est.estimate_pairs(feats0, sub, res, cameras, points, feats1)
    assert int((whole["num_inliers"] > 0).sum()) == 5 and whole["queries"].tolist() == [p[0] for p in sub]
    for at in range(5):
        alone = est.estimate_pairs(feats0, sub[at:at + 1], res[at:at + 1], cameras, points, feats1)
        for k in KEYS:
            assert torch.equal(alone[k][0], whole[k][at]), (at, k)
        assert torch.equal(alone["matches"][0], whole["matches"][at])
    perm = [4, 2, 0, 3, 1, 0]                                           # the front pair to the back, the back pair to the front, and a duplicate
    shuffled = est.estimate_pairs(feats0, [sub[p] for p in perm], res[perm], cameras, points, feats1)
    for at, p in enumerate(perm):
        for k in KEYS:
            assert torch.equal(shuffled[k][at], whole[k][p]), (p, k)
    again = est.estimate_pairs(feats0, torch.tensor(sub, device="cuda"), res, cameras, points, feats1, validate=False)
    for k in KEYS:
        assert torch.equal(again[k], whole[k]), k
    # pooled over distinct queries: the same problems, in ascending query order
    pooled = est.estimate_pairs(feats0, sub, res, cameras, points, feats1, pool=True)
    order = sorted(range(5), key=lambda i: sub[i][0])
    assert pooled["queries"].tolist() == [sub[i][0] for i in order] and pooled["group_of_pair"].tolist() == [order.index(i) for i in range(5)]
    for k in PROBLEM_KEYS:
        assert torch.equal(pooled[k], whole[k][order]), k
    for k in PAIR_KEYS:
        assert torch.equal(pooled[k], whole[k]), k
    reseeded = AbsolutePoseEstimator(threshold=A.T, num_hypotheses=512, refine=True, seed=4).estimate_pairs(feats0, sub, res, cameras, points, feats1)
    assert not torch.equal(reseeded["best_hypothesis"], whole["best_hypothesis"])
    # a pair of the list is the forward call on its own images, cameras and points
    i0, i1 = [p[0] for p in sub], [p[1] for p in sub]
    fwd = est({"image0": {"keypoints": feats0["keypoints"][i0]}, "image1": {"num_keypoints": feats1["num_keypoints"][i1]}}, res, cameras[i0], points[i1])
    for k in KEYS:
        assert torch.equal(fwd[k], whole[k]), k
    K = torch.zeros(len(cameras), 3, 3)
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = cameras[:, 0], cameras[:, 1], cameras[:, 2], cameras[:, 3], 1.0
    mats = est.estimate_pairs(feats0, sub, res, K, points, feats1)
    for k in KEYS:
        assert torch.equal(mats[k], whole[k]), k


def test_pooling_is_the_concatenation_of_the_pairs_lists():
    """query 0's three pairs sit on ascending blocks of its rows, so their pooled list IS the list of one pair against a database image that holds all three
    images' points: the same bits, and the pooled mask is that pair's mask cut into the three pairs' rows"""
    pr = A.pooled()
    feats0, feats1, cameras, points = stores()
    members = [i for i in range(len(pr["pairs"])) if pr["pairs"][i, 0] == 0]
    merged_pts, merged_m0, at = np.full((A.N1, 3), np.nan, np.float32), np.full(A.N0, -1, np.int64), 0
    for i in members:
        rows = np.nonzero(pr["matches0"][i] >= 0)[0]
        merged_pts[at:at + len(rows)] = pr["points"][pr["pairs"][i, 1]][pr["matches0"][i][rows]]
        merged_m0[rows] = np.arange(at, at + len(rows))
        at += len(rows)
    assert at == 300
    est = AbsolutePoseEstimator(threshold=A.T, num_hypotheses=512, refine=True, seed=A.SEED)
    one = est.estimate_pairs(feats0, [(NQ, 0)], cuda(merged_m0[None]), cameras, cuda(merged_pts[None]))
    pairs = [(NQ, 1 + NQ + int(pr["pairs"][i, 1])) for i in members]
    pool = est.estimate_pairs(feats0, pairs, cuda(pr["matches0"][members]), cameras, points, feats1, pool=True)
    assert int(one["num_inliers"][0]) >= 140 and pool["R"].shape == (1, 3, 3) and pool["queries"].tolist() == [NQ]
    for k in PROBLEM_KEYS:
        assert torch.equal(pool[k], one[k]), k
    assert torch.equal(pool["inliers0"].any(0), one["inliers0"][0]) and int(pool["inliers0"].sum()) == int(one["num_inliers"][0]) == int(pool["pair_num_inliers"].sum())
    # pairs of the problem in another order: another numbering of the list, so other samples — but the same scene
    other = est.estimate_pairs(feats0, pairs[::-1], cuda(pr["matches0"][members[::-1]]), cameras, points, feats1, pool=True)
    assert int(other["num_inliers"][0]) >= 140 and abs(other["R"][0] - pool["R"][0]).max() < 1e-2


# ---------------------------------------------------------------------- 6. edges
def test_empty_results_and_statuses():
    feats0, feats1, cameras, points = stores()
    pairs, m0 = pair_list()
    est = AbsolutePoseEstimator(threshold=A.T, num_hypotheses=256, refine=True)
    good = est.estimate_pairs(feats0, pairs[2:5], m0[2:5], cameras, points, feats1)

    def empty(out, b, what):
        assert int(out["num_inliers"][b]) == 0 and int(out["pair_num_inliers"][b]) == 0 and not bool(out["inliers0"][b].any()) and bool((out["matches0"][b] == -1).all()), what
        assert int(out["best_hypothesis"][b]) == -1 and bool((out["R"][b] == 0).all()) and bool((out["t"][b] == 0).all()) and len(out["matches"][b]) == 0, what

    def unchanged(out, ps):
        for p in ps:
            for k in KEYS:
                assert torch.equal(out[k][p], good[k][p]), (p, k)
    # two matches and none
    few = m0[2:5].clone()
    few[1] = -1
    few[2] = -1
    rows = torch.nonzero(m0[4] >= 0)[:2, 0]
    few[2, rows] = m0[4, rows]
    out = est.estimate_pairs(feats0, pairs[2:5], few, cameras, points, feats1)
    empty(out, 1, "no match")
    empty(out, 2, "two matches")
    unchanged(out, (0,))
    assert all(bool(torch.isfinite(out[k].float()).all()) for k in KEYS)
    # matches onto rows without a point count for nothing
    clean = m0[2:5].clone()
    clean[~torch.isfinite(points[torch.arange(3, 6, device="cuda")[:, None], clean.clamp(min=0)]).all(-1)] = -1
    assert int((clean != m0[2:5]).sum()) == 24
    unchanged(est.estimate_pairs(feats0, pairs[2:5], clean, cameras, points, feats1), (0, 1, 2))
    # an index outside its store
    with pytest.raises(ValueError, match=r"pairs \[1\] index outside the feature stores of 12 and 17 images"):
        est.estimate_pairs(feats0, [(2, 3), (3, 17), (4, 5)], m0[2:5], cameras, points, feats1)
    with pytest.raises(LightGlueAmdError, match=r"pair 1: an image index outside its feature store") as err:
        est.estimate_pairs(feats0, torch.tensor([(2, 3), (3, 17), (4, 5)], device="cuda"), m0[2:5], cameras, points, feats1, validate=False)
    empty(err.value.outputs, 1, "index")
    unchanged(err.value.outputs, (0, 2))
    # a camera without a focal length: that problem only, with its own status
    bad = cameras.clone()
    for value in (0.0, float("nan"), float("inf"), -500.0):
        bad[3, 0] = value
        with pytest.raises(LightGlueAmdError, match=r"pair 1: a camera") as err:
            est.estimate_pairs(feats0, pairs[2:5], m0[2:5], bad, points, feats1)
        empty(err.value.outputs, 1, "camera")
        unchanged(err.value.outputs, (0, 2))
    with pytest.raises(ValueError, match="zero skew"):
        est.estimate_pairs(feats0, pairs[2:5], m0[2:5], torch.eye(3).repeat(12, 1, 1) + torch.tensor([[0.0, 0.1, 0], [0, 0, 0], [0, 0, 0]]), points, feats1)
    with pytest.raises(ValueError, match=r"points3d1 must have shape"):
        est.estimate_pairs(feats0, pairs[2:5], m0[2:5], cameras, points[0], feats1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        est.estimate_pairs({"keypoints": feats0["keypoints"].cpu()}, pairs[:1], m0[:1].cpu(), cameras, points.cpu(), feats1)


EDGE_N0 = 300                               # not a multiple of 256
EDGE_SIZES = (2, 3, 4, 257)                 # below the sample, the sample, the refinement threshold, one past the 256-row tile


@pytest.mark.parametrize("S", EDGE_SIZES)
def test_list_lengths_at_the_thresholds(S):
    """the S = 1000 scene cut to its first EDGE_N0 image-0 rows and thinned to the first S correspondences among them: as one pair, and pooled from two pairs
    (the first 200 rows of the list at most, then the rest: at S = 257 the list passes 256 only as their concatenation) — the same list, so the same bits"""
    c = A.case(1000)
    rows = c["rows"][c["rows"] < EDGE_N0][:S]
    assert len(rows) == S
    m0 = np.full(EDGE_N0, -1, np.int64)
    m0[rows] = c["matches0"][rows]
    corr, planted, cam = c["corr"][:S], c["planted"][:S], c["cam"]
    first = min(200, S // 2)
    halves = np.stack([np.where(np.isin(np.arange(EDGE_N0), rows[:first]), m0, -1), np.where(np.isin(np.arange(EDGE_N0), rows[first:]), m0, -1)])
    feats0, cams, points = {"keypoints": cuda(c["kpts0"][None, :EDGE_N0])}, torch.tensor([A.CAM]), cuda(c["points"][None])
    views_of = {}
    for refine in (False, True):
        est = AbsolutePoseEstimator(threshold=A.T, num_hypotheses=256, refine=refine, seed=A.SEED)
        one = est.estimate_pairs(feats0, [(0, 0)], cuda(m0[None]), cams, points)       # status LG_OK: nothing was raised
        pool = est.estimate_pairs(feats0, [(0, 0), (0, 0)], cuda(halves), cams, points, pool=True)
        assert pool["R"].shape == (1, 3, 3) and pool["pair_num_inliers"].tolist() == [int(pool["inliers0"][0].sum()), int(pool["inliers0"][1].sum())]
        for k in PROBLEM_KEYS:
            assert torch.equal(pool[k], one[k]), (S, refine, k)
        assert torch.equal(pool["inliers0"].any(0), one["inliers0"][0]) and not bool(pool["inliers0"].all(0).any()), (S, refine)
        assert torch.equal(pool["matches0"].max(0)[0], one["matches0"][0]), (S, refine)
        inl, got0 = one["inliers0"][0].cpu().numpy(), one["matches0"][0].cpu().numpy()
        ok = (got0 == np.where(inl, m0, -1)).all() and inl.sum() == inl[rows].sum() == int(one["pair_num_inliers"][0])
        ok = ok and (one["matches"][0].cpu().numpy() == np.stack([np.nonzero(inl)[0], got0[inl]], -1)).all()
        views_of[refine] = dict({k: one[k][0].cpu().numpy() for k in PROBLEM_KEYS}, mask=inl[rows], consistent=bool(ok))
    plain, refined = views_of[False], views_of[True]
    if S < A.SAMPLE:
        check_empty(plain, S)
        check_empty(refined, S)
        return
    allin = A.all_inlier_of(planted, S, 256)
    shrunk = A.verify(corr, cam, A.T * (1 - MARGIN), 256, A.SEED, False)
    bound = int(shrunk["counts"][allin].max()) if allin.any() else 0
    for refine, got in ((False, plain), (True, refined)):
        what = (S, refine)
        if got["num_inliers"] == 0:
            check_empty(got, what)
            continue
        d = check_consistent(got, corr, cam, what)
        print(what, "count", int(got["num_inliers"]), "bound", bound, "within the margin %.4f (at most %.2f)" % ((abs(d - A.T) <= MARGIN * A.T).mean(), MAX_EXCLUDED))
        assert got["num_inliers"] >= bound, (what, got["num_inliers"], bound)
    assert refined["num_inliers"] >= plain["num_inliers"] and refined["best_hypothesis"] == plain["best_hypothesis"], S
    if plain["num_inliers"] < A.REFINE_MIN:                             # no refinement below 4 inliers: at S = 3 never
        assert (world_pose(refined) == world_pose(plain)).all() and (refined["mask"] == plain["mask"]).all(), S
    assert S >= A.REFINE_MIN or plain["num_inliers"] < A.REFINE_MIN


def test_pooled_statuses_and_a_problem_that_goes_on_without_a_pair():
    pr = A.pooled()
    out, message = run_pool(256, True)
    at = {q: [i for i in range(9) if pr["pairs"][i, 0] == q] for q in range(5)}
    bad = int(np.nonzero(pr["bad"])[0][0])
    parts = {bad: "an image index outside its feature store (LG_ERR_INDEX): the pair was not matched",
             at[4][0]: "a camera whose focal length is not finite and > 0, or whose principal point is not finite (LG_ERR_CAMERA)"}
    assert message == "; ".join("pair %d: %s" % (i, parts[i]) for i in sorted(parts))
    assert out["queries"].tolist() == [NQ + q for q in range(5)] and out["group_of_pair"].tolist() == [int(q) for q in pr["pairs"][:, 0]]
    assert int(out["pair_num_inliers"][bad]) == 0 and not bool(out["inliers0"][bad].any()) and int(out["num_inliers"][3]) >= 25
    assert out["num_inliers"].tolist() == [int(out["pair_num_inliers"][at[q]].sum()) for q in range(5)]
    # the problem with the bad pair is the problem without it; and with the bad pair FIRST the camera is still found
    feats0, feats1, cameras, points = stores()
    pairs, m0 = pool_list()
    keep = [i for i in at[3] if i != bad]
    est = AbsolutePoseEstimator(threshold=A.T, num_hypotheses=256, refine=True, seed=A.SEED)
    alone = est.estimate_pairs(feats0, pairs[keep], m0[keep], cameras, points, feats1, pool=True, validate=False)
    with pytest.raises(LightGlueAmdError, match=r"^pair 0: an image index outside its feature store \(LG_ERR_INDEX\): the pair was not matched$") as err:
        est.estimate_pairs(feats0, pairs[[bad] + keep], m0[[bad] + keep], cameras, points, feats1, pool=True, validate=False)
    for k in PROBLEM_KEYS:
        assert torch.equal(alone[k][0], out[k][3]) and torch.equal(err.value.outputs[k][0], out[k][3]), k
    for k in PAIR_KEYS:
        assert torch.equal(alone[k][0], out[k][keep[0]]) and torch.equal(err.value.outputs[k][1], out[k][keep[0]]), k


def test_num_keypoints_is_honoured():
    c = A.case(65)
    num0, num1 = 1000, 1040
    junk = c["matches0"].copy()
    free = np.nonzero(junk < 0)[0]
    junk[free[:40]] = [A.N1 + 5, 10 ** 12, A.N0, 2 ** 31, 2 ** 32 + 3] * 8               # >= n1
    junk[free[40:50]] = np.arange(num1, num1 + 10)                                       # >= num_keypoints1, inside the store
    junk[num0:] = np.arange(A.N0 - num0)                                                 # rows >= num_keypoints0
    pts = c["points"].copy()
    pts[num1:] = 1.0                                                                     # finite junk behind num_keypoints1: rows nothing may read
    ok = (np.arange(A.N0) < num0) & (junk >= 0) & (junk < num1)
    clean = np.where(ok, junk, -1)
    assert (clean >= 0).sum() >= 50 and (junk != clean).sum() >= 100
    feats0 = {"keypoints": cuda(c["kpts0"][None]), "num_keypoints": torch.tensor([num0])}
    feats1 = {"num_keypoints": torch.tensor([num1])}
    cams = torch.tensor([A.CAM])
    est = AbsolutePoseEstimator(threshold=A.T, num_hypotheses=256, refine=True)
    a = est.estimate_pairs(feats0, [(0, 0)], cuda(junk[None]), cams, cuda(pts[None]), feats1)
    b = est.estimate_pairs(feats0, [(0, 0)], cuda(clean[None]), cams, cuda(pts[None]), feats1)
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k
    rows, corr = A.correspondences(c["kpts0"], pts, junk, num0, num1)
    assert int(a["num_inliers"][0]) >= 20 and int(a["inliers0"][0].sum()) == int(a["inliers0"][0][cuda(rows)].sum())


def test_behind_the_nn_matcher_deferred_or_not():
    c = A.case(A.TILE + 1)
    rng = np.random.default_rng(21)
    rows = c["rows"]
    d0, d1 = rng.standard_normal((A.N0, 64)), rng.standard_normal((A.N0, 64))
    d1[c["matches0"][rows]] = d0[rows] + 0.05 * rng.standard_normal((len(rows), 64))          # descriptors follow the scene's correspondences
    k1 = rng.uniform(0, 480, (A.N0, 2)).astype(np.float32)                                    # the database keypoints themselves are never read by the estimator
    store = {"keypoints": cuda(np.stack([c["kpts0"], k1])), "descriptors": cuda(np.stack([d0, d1]).astype(np.float32)), "num_keypoints": torch.tensor([A.N0, A.N1])}
    pts = np.full((2, A.N0, 3), np.nan, np.float32)
    pts[1, :A.N1] = c["points"]
    pairs = [(0, 1)]
    matcher = NearestNeighborMatcher(mutual=True, distance_threshold=0.5)
    result = matcher.match_pairs(store, pairs)
    want = np.where(np.isin(np.arange(A.N0), rows), c["matches0"], -1)
    assert (result["matches0"][0].cpu().numpy() == want).all()                                # exactly the scene's correspondences: the case's oracle applies
    cams = torch.tensor([A.CAM, A.CAM])
    est = AbsolutePoseEstimator(threshold=A.T, num_hypotheses=512, refine=True, seed=A.SEED)
    out = lightglue_amd.estimate_absolute_poses(est, result, store, pairs, cams, cuda(pts))

    def same(a, b, what):
        for k in KEYS:
            assert torch.equal(a[k], b[k]), (what, k)
    same(out, est.estimate_pairs(store, pairs, result, cams, cuda(pts), pool=True), "glue.estimate_absolute_poses")
    same(out, est.estimate_pairs(store, pairs, result["matches0"], cams, cuda(pts)), "matches0 itself, not pooled")
    same(lightglue_amd.estimate_absolute_poses(est, matcher.match_pairs(store, pairs, deferred=True), store, pairs, cams, cuda(pts)), out, "a deferred result")
    inl = out["inliers0"][0].cpu().numpy()
    v = dict(R=out["R"][0].cpu().numpy(), t=out["t"][0].cpu().numpy(), num_inliers=int(out["num_inliers"][0]), mask=inl[rows], consistent=inl.sum() == inl[rows].sum())
    d = check_consistent(v, c["corr"], c["cam"], "nn")
    assert (d[c["planted"]] <= A.T).mean() >= 0.95
