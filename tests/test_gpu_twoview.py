"""TwoViewVerifier on the GPU against the float64 definition (tests/twoview_oracle.py) and against itself.

Bars and where they come from (tests/test_twoview_cpu.py derives both figures without a GPU, from the oracle's float32 run against its float64 run on the
inputs of this file, over the hypotheses whose sample is all planted inliers, and asserts that the constants below are those figures):
  Q_RESIDUAL 9.30e-03  the largest |d32 - d64| / t of a residual (reprojection error / Sampson distance) among the correspondences within 2 t
  Q_MODEL    2.53e-04  the largest entry difference between the two runs' unit-norm models
  MARGIN = 8 Q_RESIDUAL, MODEL_MARGIN = 8 Q_MODEL: the fp32 kernels may order and fuse their operations differently from numpy.  A correspondence whose
  float64 residual lies within MARGIN t of t may fall on either side and is excluded from mask comparisons; which ones are excluded is decided by the float64
  definition alone, and at most 2 % of a pair's correspondences may be (the CPU test asserts that for the oracle's own models on every input of this file).
The inputs are the cases of tests/twoview_oracle.py (640 x 480 scenes, noise 0.5, t = 3, 30 % / 50 % planted inliers for H / F), built without a GPU."""
import numpy as np
import pytest
import torch

import twoview_oracle as O
import lightglue_amd
from lightglue_amd import NearestNeighborMatcher, TwoViewVerifier
from lightglue_amd._cabi import LightGlueAmdError

Q_RESIDUAL, Q_MODEL = 9.30e-3, 2.53e-4
MARGIN, MODEL_MARGIN, MAX_EXCLUDED = 8 * Q_RESIDUAL, 8 * Q_MODEL, 0.02
KINDS = ("homography", "fundamental")
KEYS = ("models", "inliers0", "num_inliers", "matches0", "best_hypothesis")

pytestmark = pytest.mark.gpu


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def batch_of(cases):
    """the cases as B pairs of one forward call: ({"image0", "image1"}, matches0 [B, N0])"""
    pad = lambda k: np.concatenate([k, np.zeros((O.N0 - len(k), 2), np.float32)])
    data = {"image0": {"keypoints": cuda(np.stack([c["kpts0"] for c in cases]))},
            "image1": {"keypoints": cuda(np.stack([pad(c["kpts1"]) for c in cases])), "num_keypoints": torch.full((len(cases),), O.N1, dtype=torch.int32)}}
    return data, cuda(np.stack([c["matches0"] for c in cases]))


def host(out, b):
    return {k: out[k][b].cpu().numpy() for k in KEYS}


def same(a, b, what=""):
    for k in KEYS:
        assert torch.equal(a[k], b[k]), (what, k)
    assert len(a["matches"]) == len(b["matches"]) and all(torch.equal(x, y) for x, y in zip(a["matches"], b["matches"])), what


def check_consistent(kind, got, c, what):
    """the returned mask is the float64 mask of the RETURNED model outside the margin; count, matches0 and the rows off the correspondence list agree with it"""
    corr, rows = c["corr"], c["rows"]
    model = got["models"].reshape(9).astype(np.float64)
    assert np.isfinite(model).all() and abs(np.linalg.norm(model) - 1) < 1e-5 and model[np.argmax(abs(model))] > 0, what
    want = O.inlier_mask(kind, model, corr, O.T)
    d = O.distances(kind, model, corr)
    near = abs(d - O.T) <= MARGIN * O.T
    assert near.mean() <= MAX_EXCLUDED, (what, near.mean())
    mask = got["inliers0"]
    assert (mask[rows] == want)[~near].all(), (what, int((mask[rows] != want)[~near].sum()))
    assert mask.sum() == mask[rows].sum() == got["num_inliers"], what
    assert (got["matches0"] == np.where(mask, c["matches0"], -1)).all(), what
    return d


def check_empty(got, what):
    assert got["num_inliers"] == 0 and not got["inliers0"].any() and (got["models"] == 0).all() and (got["matches0"] == -1).all() and got["best_hypothesis"] == -1, what


# ---------------------------------------------------------------------- 1. scoring alone
@pytest.mark.parametrize("kind", KINDS)
def test_scoring_given_models(kind):
    sizes = (65, 1000)
    cases = [O.case(kind, S) for S in sizes]
    data, m0 = batch_of(cases)
    feats0, feats1 = data["image0"], data["image1"]
    models = cuda(np.stack([O.scoring_models(kind, S) for S in sizes]).reshape(len(sizes), O.GIVEN, 3, 3))
    v = TwoViewVerifier(model=kind, threshold=O.T, num_hypotheses=256, refine=False)
    out = v.score_models(feats0, [(b, b) for b in range(len(sizes))], m0, models, feats1)
    for b, (S, c) in enumerate(zip(sizes, cases)):
        got = host(out, b)
        assert got["best_hypothesis"] == O.PLANTED_AT, (S, got["best_hypothesis"])          # the planted model, and of its two identical copies the lower index
        check_consistent(kind, got, c, (kind, S))
        want = O.output_form(O.scoring_models(kind, S)[O.PLANTED_AT])
        assert (got["models"].reshape(9) == want).all(), S                                  # a given model comes back as it stands, in output form
    # the same candidates behind 256 random ones: the winner sits in the second workgroup of its pair and reaches the pair's key through the atomic
    filler = lambda S: np.tile(O.scoring_models(kind, S)[48:], (2, 1))[:O.GIVEN]
    wide = cuda(np.stack([np.concatenate([filler(S), O.scoring_models(kind, S)]) for S in sizes]).reshape(len(sizes), 2 * O.GIVEN, 3, 3))
    out2 = v.score_models(feats0, [(b, b) for b in range(len(sizes))], m0, wide, feats1)
    assert out2["best_hypothesis"].tolist() == [O.GIVEN + O.PLANTED_AT] * len(sizes)
    for k in ("models", "inliers0", "num_inliers", "matches0"):
        assert torch.equal(out2[k], out[k]), k


# ---------------------------------------------------------------------- 2. end to end
@pytest.mark.parametrize("hyps", O.HYPS)
@pytest.mark.parametrize("kind", KINDS)
def test_end_to_end(kind, hyps):
    sizes = O.case_sizes(kind)
    cases = [O.case(kind, S) for S in sizes]
    data, m0 = batch_of(cases)
    outs = {refine: TwoViewVerifier(model=kind, threshold=O.T, num_hypotheses=hyps, refine=refine, seed=O.SEED)(data, {"matches0": m0}) for refine in (False, True)}
    for b, (S, c) in enumerate(zip(sizes, cases)):
        plain, refined = host(outs[False], b), host(outs[True], b)
        allin = O.all_inlier(kind, S, hyps)
        shrunk = O.verify(kind, c["corr"], O.T * (1 - MARGIN), hyps, O.SEED, False)
        bound = int(shrunk["counts"][allin].max()) if allin.any() else 0
        for refine, got in ((False, plain), (True, refined)):
            what = (kind, S, hyps, refine)
            print(what, "count", int(got["num_inliers"]), "oracle", O.case_oracle(kind, S, hyps, refine)["count"], "bound", bound, "hypothesis", int(got["best_hypothesis"]))
            d = check_consistent(kind, got, c, what)
            assert got["num_inliers"] >= bound, (what, got["num_inliers"], bound)
            assert (d[c["planted"]] <= O.T).mean() >= 0.95, (what, (d[c["planted"]] <= O.T).mean())
            assert (outs[refine]["matches"][b].cpu().numpy() == np.stack([np.nonzero(got["inliers0"])[0], got["matches0"][got["inliers0"]]], -1)).all(), what
        assert refined["num_inliers"] >= plain["num_inliers"], (kind, S, hyps)
        assert refined["best_hypothesis"] == plain["best_hypothesis"]
        h = int(plain["best_hypothesis"])
        if h >= 0 and allin[h]:                    # the winner's model is the definition's model of that hypothesis (one of its roots) within the model margin
            r64 = O.case_oracle(kind, S, hyps, False)
            diff = [abs(O.output_form(r64["models"][h, r]) - plain["models"].reshape(9)).max() for r in range(3) if r64["valid"][h, r]]
            assert diff and min(diff) <= MODEL_MARGIN, (kind, S, hyps, diff)


# ---------------------------------------------------------------------- 3. independence
def independence_store(kind):
    """4 images of N0 rows (ragged num_keypoints) and 6 pairs with their matches0: two scenes, a pair of unrelated random matches, a self pair, a repeated pair"""
    a, b = O.case(kind, 65), O.case(kind, O.TILE + 1)
    pad = lambda k: np.concatenate([k, np.full((O.N0 - len(k), 2), 7.0, np.float32)])
    kpts = np.stack([a["kpts0"], pad(a["kpts1"]), b["kpts0"], pad(b["kpts1"])])
    num = np.array([O.N0, O.N1, 1000, 900], np.int32)
    rng = np.random.default_rng(5)
    rand = np.where(rng.random(O.N0) < 0.3, rng.integers(0, O.N0, O.N0), -1)
    ident = np.where(rng.random(O.N0) < 0.2, np.arange(O.N0), -1)
    pairs = [(0, 1), (2, 3), (0, 3), (1, 1), (2, 3), (3, 0)]
    m0 = np.stack([a["matches0"], b["matches0"], rand, ident, b["matches0"], rand[::-1].copy()]).astype(np.int64)
    return kpts, num, pairs, m0


@pytest.mark.parametrize("kind", KINDS)
def test_a_pair_is_independent_of_its_list(kind):
    kpts, num, pairs, m0 = independence_store(kind)
    feats = {"keypoints": cuda(kpts), "num_keypoints": torch.from_numpy(num)}
    res = cuda(m0)
    v = TwoViewVerifier(model=kind, threshold=O.T, num_hypotheses=512, refine=True, seed=3)
    whole = v.verify_pairs(feats, pairs, {"matches0": res})
    assert int((whole["num_inliers"] > 0).sum()) >= 5      # nothing trivial is compared (the self pair has no fundamental matrix: x1 = x0)
    for p in range(len(pairs)):
        alone = v.verify_pairs(feats, pairs[p:p + 1], res[p:p + 1])
        for k in KEYS:
            assert torch.equal(alone[k][0], whole[k][p]), (p, k)
        assert torch.equal(alone["matches"][0], whole["matches"][p])
    perm = [4, 2, 0, 5, 1, 3]
    shuffled = v.verify_pairs(feats, [pairs[p] for p in perm], res[perm])
    for at, p in enumerate(perm):
        for k in KEYS:
            assert torch.equal(shuffled[k][at], whole[k][p]), (p, k)
    for k in KEYS:                                                      # the repeated pair
        assert torch.equal(whole[k][1], whole[k][4]), k
    same(v.verify_pairs(feats, pairs, res), whole, "two calls with one seed")
    other = {"keypoints": feats["keypoints"].clone(), "num_keypoints": torch.from_numpy(num.copy())}
    same(v.verify_pairs(feats, pairs, res, other), whole, "feats1 given")
    same(v.verify_pairs(feats, torch.tensor(pairs, device="cuda"), res, validate=False), whole, "a device pair list")
    reseeded = TwoViewVerifier(model=kind, threshold=O.T, num_hypotheses=512, refine=True, seed=4).verify_pairs(feats, pairs, res)
    assert not torch.equal(reseeded["best_hypothesis"], whole["best_hypothesis"])
    # a pair of the list is the forward call on its own images
    data = {"image0": {"keypoints": feats["keypoints"][[0, 2]], "num_keypoints": torch.from_numpy(num[[0, 2]])},
            "image1": {"keypoints": feats["keypoints"][[1, 3]], "num_keypoints": torch.from_numpy(num[[1, 3]])}}
    fwd = v(data, res[:2])
    for k in KEYS:
        assert torch.equal(fwd[k], whole[k][:2]), k


# ---------------------------------------------------------------------- 4. edge cases
@pytest.mark.parametrize("kind", KINDS)
def test_empty_results(kind):
    rng = np.random.default_rng(9)
    n = 200                                 # not a multiple of 64
    need = O.SAMPLE[kind]
    kp0, kp1 = rng.uniform(0, 480, (5, n, 2)).astype(np.float32), rng.uniform(0, 480, (5, n, 2)).astype(np.float32)
    m0 = np.full((5, n), -1, np.int64)
    m0[1, rng.permutation(n)[:need - 1]] = rng.permutation(n)[:need - 1]              # one short of a sample
    rows = rng.permutation(n)[:30]
    m0[2, rows] = rows                                                                   # all correspondences identical
    kp0[2, rows], kp1[2, rows] = (100.5, 200.25), (300.0, 50.75)
    m0[3, rows] = rows                                                                   # all collinear (on both sides)
    s = rng.uniform(0, 400, 30).astype(np.float32)
    kp0[3, rows], kp1[3, rows] = np.stack([s, 0.5 * s + 10], 1), np.stack([1.5 * s + 3, s], 1)
    m0[4, rows] = rows                                                                   # a pair that does have a model, so that the call is not all empty
    data = {"image0": {"keypoints": cuda(kp0)}, "image1": {"keypoints": cuda(kp1)}}
    for refine in (False, True):
        out = TwoViewVerifier(model=kind, threshold=O.T, num_hypotheses=256, refine=refine)(data, cuda(m0))
        for b in (0, 1, 2) + ((3,) if kind == "homography" else ()):
            check_empty(host(out, b), (kind, refine, b))
        for k in KEYS:
            assert torch.isfinite(out[k].float()).all(), k
        assert int(out["num_inliers"][4]) > 0 and all(len(out["matches"][b]) == int(out["num_inliers"][b]) for b in range(5))


@pytest.mark.parametrize("kind", KINDS)
def test_entries_outside_the_images_are_unmatched(kind):
    c = O.case(kind, 65)
    num0, num1 = 1000, 1040
    junk = c["matches0"].copy()
    free = np.nonzero(junk < 0)[0]
    junk[free[:40]] = [O.N1 + 5, 10 ** 12, O.N0, 2 ** 31, 2 ** 32 + 3] * 8              # >= n1 (the store holds N0 rows per image)
    junk[free[40:60]] = np.arange(num1, num1 + 20)                                      # >= num_keypoints1
    junk[num0:] = np.arange(O.N0 - num0)                                                # rows >= num_keypoints0
    clean = np.where((np.arange(O.N0) < num0) & (junk >= 0) & (junk < num1), junk, -1)
    assert (clean >= 0).sum() >= 50 and (junk != clean).sum() >= 100
    pad = np.concatenate([c["kpts1"], np.full((O.N0 - O.N1, 2), np.nan, np.float32)])  # rows nothing may read
    feats = {"keypoints": cuda(np.stack([c["kpts0"], pad])), "num_keypoints": torch.tensor([num0, num1])}
    v = TwoViewVerifier(model=kind, threshold=O.T, num_hypotheses=256, refine=True)
    a, b = v.verify_pairs(feats, [(0, 1)], cuda(junk[None])), v.verify_pairs(feats, [(0, 1)], cuda(clean[None]))
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k
    assert int(a["num_inliers"][0]) > 0
    rows, corr = O.correspondences(c["kpts0"], pad, junk, num0, num1)
    got = host(a, 0)
    assert got["inliers0"].sum() == got["inliers0"][rows].sum()


@pytest.mark.parametrize("kind", KINDS)
def test_an_index_outside_the_store_empties_that_pair_only(kind):
    kpts, num, pairs, m0 = independence_store(kind)
    feats = {"keypoints": cuda(kpts), "num_keypoints": torch.from_numpy(num)}
    v = TwoViewVerifier(model=kind, threshold=O.T, num_hypotheses=256, refine=True)
    good = v.verify_pairs(feats, pairs[:3], cuda(m0[:3]))
    with pytest.raises(ValueError, match=r"pairs \[1\] index outside the feature stores of 4 and 4 images"):
        v.verify_pairs(feats, [(0, 1), (2, 4), (0, 3)], cuda(m0[:3]))
    with pytest.raises(LightGlueAmdError, match=r"pair 1: an image index outside its feature store") as err:
        v.verify_pairs(feats, torch.tensor([(0, 1), (2, 4), (0, 3)], device="cuda"), cuda(m0[:3]), validate=False)
    out = err.value.outputs
    check_empty(host(out, 1), kind)
    for p in (0, 2):
        for k in KEYS:
            assert torch.equal(out[k][p], good[k][p]), (p, k)
    with pytest.raises(LightGlueAmdError, match=r"pair 0: an image index"):
        v.verify_pairs(feats, torch.tensor([(-1, 1)], device="cuda"), cuda(m0[:1]), validate=False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        v.verify_pairs({"keypoints": torch.from_numpy(kpts)}, pairs[:1], torch.from_numpy(m0[:1]))


# ---------------------------------------------------------------------- 4b. list lengths around the sample size, the refit threshold and the 256-row tile
EDGE_N0 = 300                               # not a multiple of 256
EDGE_SIZES = {"homography": (3, 4, 255, 256, 257), "fundamental": (6, 7, 8, 257)}


# the window of image-0 rows a case is cut from: the first of 0, 100, 200, ... on which the float64 definition's own models (refined or not) keep at most 2 % of
# the correspondences within the margin — the rule behind twoview_oracle.SCENE_SEED, decided by the definition alone; the test asserts it before it reads the GPU.
# The finding behind the one entry: homography, S = 255 cut from rows 0 - 299 leaves 7 of the 255 correspondences (0.0275) within the margin of the returned model, on
# the library before the shared steps exactly as on this one, and the float64 definition's own unrefined model has the same 0.0275 there (it does not recover the
# plane: count 51 against 80 refined); rows 200 - 499 give 0.0078 / 0.0.  The kernels are not at fault at rows 0 - 299 and nothing was changed in them for it
EDGE_START = {("homography", 255): 200}


def thinned(c, S, n0=EDGE_N0, start=0):
    """the S = 1000 scene cut to the n0 image-0 rows from `start` on and thinned to the first S correspondences among them (the oracle's order is ascending in the row)"""
    first = int(np.searchsorted(c["rows"], start))
    rows = c["rows"][first:first + S]
    assert len(rows) == S and rows[-1] < start + n0
    m0 = np.full(n0, -1, np.int64)
    m0[rows - start] = c["matches0"][rows]
    return dict(kpts0=c["kpts0"][start:start + n0], kpts1=c["kpts1"], matches0=m0, rows=rows - start, corr=c["corr"][first:first + S], planted=c["planted"][first:first + S])


@pytest.mark.parametrize("kind, S", [(kind, S) for kind in KINDS for S in EDGE_SIZES[kind]])
def test_list_lengths_at_the_thresholds(kind, S):
    c = thinned(O.case(kind, 1000), S, start=EDGE_START.get((kind, S), 0))
    if S >= O.SAMPLE[kind]:
        for refine in (False, True):                                    # the input is one the definition itself can be compared on
            r64 = O.verify(kind, c["corr"], O.T, 256, O.SEED, refine)
            if r64["count"]:
                assert (abs(O.distances(kind, np.asarray(r64["model"], np.float64).reshape(9), c["corr"]) - O.T) <= MARGIN * O.T).mean() <= MAX_EXCLUDED, (kind, S, refine)
    data = {"image0": {"keypoints": cuda(c["kpts0"][None])}, "image1": {"keypoints": cuda(c["kpts1"][None])}}
    outs = {refine: TwoViewVerifier(model=kind, threshold=O.T, num_hypotheses=256, refine=refine, seed=O.SEED)(data, cuda(c["matches0"][None])) for refine in (False, True)}
    plain, refined = host(outs[False], 0), host(outs[True], 0)          # status LG_OK: nothing was raised
    if S < O.SAMPLE[kind]:
        check_empty(plain, (kind, S))
        check_empty(refined, (kind, S))
        return
    allin = c["planted"][O.sample(O.SEED, 256, S, O.SAMPLE[kind])].all(1)
    shrunk = O.verify(kind, c["corr"], O.T * (1 - MARGIN), 256, O.SEED, False)
    bound = int(shrunk["counts"][allin].max()) if allin.any() else 0
    for refine, got in ((False, plain), (True, refined)):
        what = (kind, S, refine)
        if got["num_inliers"] == 0:
            check_empty(got, what)
        else:
            d = check_consistent(kind, got, c, what)
            print(what, "count", int(got["num_inliers"]), "bound", bound, "within the margin %.4f (at most %.2f)" % ((abs(d - O.T) <= MARGIN * O.T).mean(), MAX_EXCLUDED))
        assert got["num_inliers"] >= bound, (what, got["num_inliers"], bound)
        assert (outs[refine]["matches"][0].cpu().numpy() == np.stack([np.nonzero(got["inliers0"])[0], got["matches0"][got["inliers0"]]], -1)).all(), what
    assert refined["num_inliers"] >= plain["num_inliers"] and refined["best_hypothesis"] == plain["best_hypothesis"], (kind, S)
    if plain["num_inliers"] < O.REFIT_MIN[kind]:                        # no refit below 4 (H) / 8 (F) inliers: at S = 7 never
        same(outs[True], outs[False], (kind, S, "no refit"))
    assert S != 7 or plain["num_inliers"] < O.REFIT_MIN[kind]


# ---------------------------------------------------------------------- 5. behind the nearest-neighbour matcher
@pytest.mark.parametrize("kind", KINDS)
def test_verify_pairs_behind_the_nn_matcher(kind):
    c = O.case(kind, O.TILE + 1)
    rng = np.random.default_rng(21)
    d0, d1 = rng.standard_normal((O.N0, 64)), rng.standard_normal((O.N0, 64))
    d1[c["matches0"][c["rows"]]] = d0[c["rows"]] + 0.05 * rng.standard_normal((len(c["rows"]), 64))      # descriptors follow the scene's correspondences
    pad = np.concatenate([c["kpts1"], np.zeros((O.N0 - O.N1, 2), np.float32)])
    store = {"keypoints": cuda(np.stack([c["kpts0"], pad])), "descriptors": cuda(np.stack([d0, d1]).astype(np.float32)), "num_keypoints": torch.tensor([O.N0, O.N1])}
    pairs = [(0, 1), (1, 0)]
    matcher = NearestNeighborMatcher(mutual=True, distance_threshold=0.5)            # planted rows lie at distance ~0.07, unrelated rows near sqrt(2)
    result = matcher.match_pairs(store, pairs)
    assert (result["matches0"][0].cpu().numpy() == c["matches0"]).all()                # exactly the scene's correspondences: the case's oracle applies
    v = TwoViewVerifier(model=kind, threshold=O.T, num_hypotheses=512, refine=True, seed=O.SEED)
    out = lightglue_amd.verify_pairs(v, result, store, pairs)
    same(out, v.verify_pairs(store, pairs, result), "glue.verify_pairs")
    same(lightglue_amd.verify_pairs(v, matcher.match_pairs(store, pairs, deferred=True), store, pairs), out, "a deferred result")
    got = host(out, 0)
    d = check_consistent(kind, got, c, kind)
    assert (d[c["planted"]] <= O.T).mean() >= 0.95
    assert int(out["num_inliers"][1]) > 0
