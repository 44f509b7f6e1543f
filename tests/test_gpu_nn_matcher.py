"""NearestNeighborMatcher on the GPU against the float64 definition (tests/nn_oracle.py) and against itself.

Bars and where they come from:
  scores 1e-5   worst-case fp32 bound of a normalised dot product of depth D <= 256, |d sim| <= (D + 8) 2^-24 ~ 1.6e-5, halved by (s + 1) / 2
  margin 1e-4   six times that bound: a row whose every decision (arg-max gap, ratio test, distance test, and with the mutual check those of its partner's
                column) lies at least 1e-4 from its boundary in the float64 definition must come out EQUAL; rows nearer than that are excluded, and at most 1 %
                of the rows of a comparison may be.  tests/test_nn_matcher_cpu.py asserts, without a GPU, that on the inputs of this file the cap is respected.
                Which rows are excluded is a property of the float64 definition alone, never of what the GPU returned.  On the store of test 1 (seed 1) the
                definition excludes 0.05 % .. 0.35 % of the rows, depending on the configuration (2 .. 14 of 3996): 30 % of the generator's rows are outliers
                whose two best columns are unrelated random rows, and a few of those lie within 1e-4 of each other under any seed (smallest gap 4e-6).  The
                seam and duplicate inputs are small images of unrelated random rows, where one near-tied row weighs up to 1.5 %: their cap is SMALL_CAP, and
                the rows those tests are about (the planted ones) are asserted not to be among the excluded.
The inputs are built by functions of this module (`oracle_case`, `seam_case`, `duplicates_case`) that need no GPU, so that the CPU test sees the same arrays."""
import functools
import itertools

import numpy as np
import pytest
import torch

import nn_oracle as O
from lightglue_amd import NearestNeighborMatcher, _cabi, glue, sift_to_rootsift
from lightglue_amd._cabi import LightGlueAmdError

SCORE_TOL, MARGIN, MAX_EXCLUDED = 1e-5, 1e-4, 0.01
SMALL_CAP = 0.02           # tests 2 and 8 (see above)
T, ROWS = _cabi.LG_NN_TILE, _cabi.LG_NN_ROWS_PER_WORKGROUP     # the kernel's image-1 tile and the rows a workgroup owns


def store(seed, K, N, D, sigma=0.45, outlier=0.3, dtype="f32"):
    rng = np.random.Generator(np.random.PCG64(seed)); base = rng.standard_normal((N, D)); out = []
    for _ in range(K):
        x = base[rng.permutation(N)] + sigma * rng.standard_normal((N, D))
        rep = rng.random(N) < outlier; x[rep] = rng.standard_normal((int(rep.sum()), D))
        if dtype == "u8":
            x = np.abs(x); x = np.clip(np.round(x / np.linalg.norm(x, axis=1, keepdims=True) * 512), 0, 255).astype(np.uint8)
        else:
            x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float16 if dtype == "f16" else np.float32)
        out.append(x)
    return np.stack(out)


# ---------------------------------------------------------------------- test 1: the inputs and their oracle
CONFIGS = [(256, "f32", None), (128, "f16", None), (128, "u8", None), (128, "u8", "rootsift"), (64, "f32", None)]
THRESHOLDS = [(None, None), (0.8, None), (0.9, 0.7)]
PAIRS = [(0, 1), (1, 0), (2, 1), (1, 2), (0, 0), (0, 1)]      # ragged counts, an n below one MFMA tile, a self pair, a repeated pair
NUM = [333, 200, 5]
SEED = 1


@functools.lru_cache(maxsize=None)
def oracle_store(D, dtype, seed=SEED):
    return store(seed, 3, 333, D, dtype=dtype)


@functools.lru_cache(maxsize=None)
def oracle_sims(D, dtype, transform):
    s = oracle_store(D, dtype)
    return [O.similarity(s[i, :NUM[i]], s[j, :NUM[j]], transform, transform) for i, j in PAIRS]


@functools.lru_cache(maxsize=None)
def oracle_case(D, dtype, transform, ratio, distance, mutual):
    """the float64 answer for every pair of PAIRS, padded to the store's N like the matcher's outputs"""
    N, out = 333, []
    for (i, j), sim in zip(PAIRS, oracle_sims(D, dtype, transform)):
        out.append(pad_ref(O.match(sim, mutual=mutual, ratio=ratio, distance=distance), N, N))
    return out


def pad_ref(r, N0, N1):
    for side, N in ((0, N0), (1, N1)):
        for key, fill in ((f"matches{side}", -1), (f"matching_scores{side}", 0.0), (f"margin{side}", np.inf)):
            r[key] = np.concatenate([r[key], np.full(N - len(r[key]), fill, r[key].dtype)])
    return r


def excluded_fraction(refs):
    bad = sum(int((r["margin0"] < MARGIN).sum() + (r["margin1"] < MARGIN).sum()) for r in refs)
    return bad / max(1, sum(len(r["margin0"]) + len(r["margin1"]) for r in refs))


def feats_of(arr, num=None, transform=None, keypoints=False):
    f = {"descriptors": torch.from_numpy(np.ascontiguousarray(arr)).cuda()}
    if num is not None:
        f["num_keypoints"] = torch.tensor(num, dtype=torch.int32)
    if transform is not None:
        f["descriptor_transform"] = transform
    if keypoints:
        f["keypoints"] = torch.zeros(arr.shape[:-1] + (2,), device="cuda")
    return f


def compare(out, refs, what="", cap=MAX_EXCLUDED):
    """matches0 / matches1 / the list equal to the oracle on every row whose margins are all >= MARGIN, scores within SCORE_TOL there; at most MAX_EXCLUDED
    of the rows excluded.  Returns (max |d score|, excluded fraction) and prints them before asserting."""
    worst, mism = 0.0, []
    for p, r in enumerate(refs):
        for side in (0, 1):
            good = r[f"margin{side}"] >= MARGIN
            got_m = out[f"matches{side}"][p].cpu().numpy()
            got_s = out[f"matching_scores{side}"][p].cpu().numpy().astype(np.float64)
            if (got_m[good] != r[f"matches{side}"][good]).any():
                mism.append((p, side, np.where(good & (got_m != r[f"matches{side}"]))[0][:8].tolist()))
            same = good & (got_m == r[f"matches{side}"])
            if same.any():
                worst = max(worst, float(np.abs(got_s[same] - r[f"matching_scores{side}"][same]).max()))
        good0 = r["margin0"] >= MARGIN
        lst, lsc = out["matches"][p].cpu().numpy(), out["scores"][p].cpu().numpy()
        m0 = out["matches0"][p].cpu().numpy()
        idx = np.where(m0 > -1)[0]                   # the list is exactly the matched rows of matches0, ascending, with their scores
        assert lst.shape == (len(idx), 2) and (lst[:, 0] == idx).all() and (lst[:, 1] == m0[idx]).all(), (what, p, "match list")
        assert (lsc == out["matching_scores0"][p].cpu().numpy()[idx]).all(), (what, p, "score list")
        keep = good0[r["matches"][:, 0]] if len(r["matches"]) else np.zeros(0, bool)
        keep_got = good0[lst[:, 0]] if len(lst) else np.zeros(0, bool)
        if not np.array_equal(lst[keep_got], r["matches"][keep]):
            mism.append((p, "list"))
    frac = excluded_fraction(refs)
    print(f"nn {what}: max |d score| {worst:.3e} (bar {SCORE_TOL:g}), rows excluded {frac:.4%} (cap {cap:.0%})")
    assert frac <= cap, (what, frac)
    assert not mism, (what, mism[:6])
    assert worst <= SCORE_TOL, (what, worst)
    return worst, frac


def assert_same(a, b, what=""):
    """two output dicts equal in every bit"""
    for k in ("matches0", "matches1", "matching_scores0", "matching_scores1", "prune0", "prune1"):
        assert torch.equal(a[k], b[k]), (what, k)
    assert len(a["matches"]) == len(b["matches"])
    for x, y in zip(a["matches"] + a["scores"], b["matches"] + b["scores"]):
        assert torch.equal(x, y), (what, "lists")
    sa, sb = a["stop"], b["stop"]
    assert (torch.equal(sa, sb) if torch.is_tensor(sa) else sa == sb), (what, "stop")


@pytest.mark.gpu
@pytest.mark.parametrize("mutual", [True, False])
@pytest.mark.parametrize("ratio,distance", THRESHOLDS)
@pytest.mark.parametrize("D,dtype,transform", CONFIGS)
def test_against_oracle(D, dtype, transform, ratio, distance, mutual):
    m = NearestNeighborMatcher(mutual=mutual, ratio_threshold=ratio, distance_threshold=distance)
    out = m.match_pairs(feats_of(oracle_store(D, dtype), NUM, transform), PAIRS)
    assert out["matches0"].dtype == torch.int64 and out["matches0"].shape == (len(PAIRS), 333) and out["matching_scores1"].dtype == torch.float32
    assert out["stop"].dtype == torch.int64 and not out["stop"].any() and out["prune0"].dtype == torch.float32 and not out["prune0"].any() and not out["prune1"].any()
    compare(out, oracle_case(D, dtype, transform, ratio, distance, mutual), f"D{D} {dtype} {transform} r{ratio} d{distance} mutual{mutual}")
    for p, (i, j) in enumerate(PAIRS):               # rows at or beyond num_keypoints: -1 / 0
        assert (out["matches0"][p, NUM[i]:] == -1).all() and (out["matching_scores0"][p, NUM[i]:] == 0).all()
        assert (out["matches1"][p, NUM[j]:] == -1).all() and (out["matching_scores1"][p, NUM[j]:] == 0).all()


# ---------------------------------------------------------------------- test 2: tile seams
SEAM_N1 = [1, 15, 16, 17, T, T + 1, 2 * T + 3]
SEAM_N0 = [1, 17, ROWS + 1]
SEAM_D, SEAM_RATIO = 256, 0.8


@functools.lru_cache(maxsize=None)
def seam_case(n0, n1):
    """image 0: n0 random rows.  One image 1 per combination (best, second) of the positions {0, T - 1, T, n1 - 1} inside the image: random rows, an exact copy of
    row a_i at `best` and a sigma = 0.1 noised copy at `second` (none when the image has one row) — i walks through image 0, its last row included.
    -> (image 0 [1, n0, D], images 1 [C, n1, D], planted [(i, best, second)], the oracle per pair (ratio 0.8, one direction each, no mutual check))"""
    rng = np.random.Generator(np.random.PCG64(1000 * n0 + n1))
    a = rng.standard_normal((1, n0, SEAM_D)).astype(np.float32)
    pos = sorted({q for q in (0, T - 1, T, n1 - 1) if 0 <= q < n1})
    combos = [(b, s) for b, s in itertools.permutations(pos, 2)] or [(pos[0], None)]
    imgs, planted = [], []
    for c, (b, s) in enumerate(combos):
        i = (n0 - 1 - c) % n0
        x = rng.standard_normal((n1, SEAM_D)).astype(np.float32)
        x[b] = a[0, i]
        if s is not None:
            x[s] = a[0, i] + (0.1 * rng.standard_normal(SEAM_D)).astype(np.float32)
        imgs.append(x); planted.append((i, b, s))
    imgs = np.stack(imgs)
    refs = [O.match(O.similarity(a[0], imgs[c]), mutual=False, ratio=SEAM_RATIO) for c in range(len(combos))]
    return a, imgs, planted, refs


@pytest.mark.gpu
@pytest.mark.parametrize("n0", SEAM_N0)
@pytest.mark.parametrize("n1", SEAM_N1)
def test_tile_seams(n0, n1):
    a, imgs, planted, refs = seam_case(n0, n1)
    m = NearestNeighborMatcher(mutual=False, ratio_threshold=SEAM_RATIO)
    out = m.match_pairs(feats_of(a), [(0, c) for c in range(len(imgs))], feats_of(imgs))
    compare(out, refs, f"seams n0 {n0} n1 {n1}", cap=SMALL_CAP)
    for c, (i, b, s) in enumerate(planted):
        assert refs[c]["margin0"][i] >= MARGIN                                   # (the planted rows are never among the excluded ones)
        assert int(out["matches0"][c, i]) == b == int(refs[c]["matches0"][i]), (c, i, b, s)
        assert abs(2.0 * float(out["matching_scores0"][c, i]) - 2.0) <= 1e-6     # s1 = 1


# ---------------------------------------------------------------------- test 3: the storage format changes nothing
@pytest.mark.gpu
@pytest.mark.parametrize("dtype,transform", [("f16", None), ("u8", None), ("u8", "rootsift")])
@pytest.mark.parametrize("mutual,ratio,distance", [(True, 0.8, None), (False, 0.9, 0.7)])
def test_format_independence_bit_for_bit(dtype, transform, mutual, ratio, distance):
    m = NearestNeighborMatcher(mutual=mutual, ratio_threshold=ratio, distance_threshold=distance)
    stored = torch.from_numpy(oracle_store(128, dtype)).cuda()
    got = m.match_pairs({"descriptors": stored, "num_keypoints": NUM, "descriptor_transform": transform}, PAIRS)
    wide = sift_to_rootsift(stored) if transform else stored.float()
    assert wide.dtype == torch.float32
    assert_same(got, m.match_pairs({"descriptors": wide, "num_keypoints": NUM}, PAIRS), f"{dtype} {transform}")


# ---------------------------------------------------------------------- test 4: one fp32 sim in both directions
@pytest.mark.gpu
@pytest.mark.parametrize("mutual,ratio,distance", [(False, None, None), (False, 0.9, 0.7), (True, 0.8, None)])
@pytest.mark.parametrize("D,dtype", [(256, "f32"), (128, "f16")])
def test_symmetry(D, dtype, mutual, ratio, distance):
    m = NearestNeighborMatcher(mutual=mutual, ratio_threshold=ratio, distance_threshold=distance)
    A, B = feats_of(oracle_store(D, dtype), NUM), feats_of(store(2, 3, 301, D, dtype=dtype), [301, 64, 129])
    ab = m.match_pairs(A, PAIRS, B)
    ba = m.match_pairs(B, [(j, i) for i, j in PAIRS], A)
    for x, y in (("matches1", "matches0"), ("matching_scores1", "matching_scores0"), ("matches0", "matches1"), ("matching_scores0", "matching_scores1")):
        assert torch.equal(ab[x], ba[y]), (x, y)


# ---------------------------------------------------------------------- test 5: the pair list against forward on stacked tensors
@pytest.mark.gpu
@pytest.mark.parametrize("D,dtype", [(256, "f32"), (128, "f16")])
def test_pair_list_equals_stacked_forward(D, dtype):
    m = NearestNeighborMatcher(ratio_threshold=0.9)
    desc = torch.from_numpy(oracle_store(D, dtype)).cuda()
    num = torch.tensor(NUM, dtype=torch.int32, device="cuda")
    listed = m.match_pairs({"descriptors": desc, "num_keypoints": num}, PAIRS)
    i0, i1 = (torch.tensor([p[s] for p in PAIRS], device="cuda") for s in (0, 1))
    stacked = m({"image0": {"descriptors": desc[i0], "num_keypoints": num[i0]}, "image1": {"descriptors": desc[i1], "num_keypoints": num[i1]}})
    assert_same(listed, stacked, "stacked")
    poisoned = desc.clone()
    for k, n in enumerate(NUM):
        poisoned[k, n:] = float("nan")               # padding rows may hold anything
    assert_same(listed, m.match_pairs({"descriptors": poisoned, "num_keypoints": num}, PAIRS), "NaN padding")
    compare(listed, oracle_case(D, dtype, None, 0.9, None, True), "pair list")


# ---------------------------------------------------------------------- test 6: edges
@pytest.mark.gpu
def test_edges():
    m = NearestNeighborMatcher(ratio_threshold=0.8)
    s = oracle_store(64, "f32")
    # an image without keypoints on either side, by count and by shape
    out = m.match_pairs(feats_of(s, [0, 200, 5]), [(0, 1), (1, 0), (1, 2)])
    assert (out["matches0"][0] == -1).all() and (out["matches1"][0] == -1).all() and (out["matching_scores1"][0] == 0).all() and out["matches"][0].shape == (0, 2)
    assert (out["matches0"][1] == -1).all() and (out["matches1"][1] == -1).all() and out["scores"][1].shape == (0,)
    assert (out["matches0"][2] > -1).any()
    empty = feats_of(s[:, :0])
    for f0, f1, shape0, shape1 in ((empty, feats_of(s), (2, 0), (2, 333)), (feats_of(s), empty, (2, 333), (2, 0))):
        out = m.match_pairs(f0, [(0, 1), (2, 2)], f1)
        assert out["matches0"].shape == shape0 and out["matches1"].shape == shape1 and (out["matches0"] == -1).all() and (out["matches1"] == -1).all()
        assert [tuple(x.shape) for x in out["matches"]] == [(0, 2), (0, 2)]
    # no pairs
    out = m.match_pairs(feats_of(s), [])
    assert out["matches0"].shape == (0, 333) and out["matches"] == [] and out["scores"] == []
    # an index outside the store: named on the host, or through the status word
    with pytest.raises(ValueError, match=r"pairs \[1\] index outside the feature stores of 3 and 3 images"):
        m.match_pairs(feats_of(s), [(0, 1), (0, 3), (1, 2)])
    with pytest.raises(LightGlueAmdError, match=r"pair 1: an image index outside its feature store"):
        m.match_pairs(feats_of(s), torch.tensor([(0, 1), (0, 3), (1, 2)], device="cuda"), validate=False)
    # deferred
    f = feats_of(s, NUM)
    handle = m.match_pairs(f, PAIRS, deferred=True)
    assert_same(handle.result(), m.match_pairs(f, PAIRS), "deferred")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.match_pairs({"descriptors": torch.from_numpy(s)}, PAIRS)
    with pytest.raises(AssertionError, match="dim must be a multiple of 16"):
        m.match_pairs(feats_of(s[:, :, :20]), PAIRS)
    with pytest.raises(ValueError, match="descriptor_transform"):
        m.match_pairs(feats_of(s, transform="hellinger"), PAIRS)


# ---------------------------------------------------------------------- test 7: drop-in for the glue helpers
@pytest.mark.gpu
def test_drop_in_for_glue_helpers():
    m = NearestNeighborMatcher(ratio_threshold=0.9)
    s = oracle_store(128, "f16")
    per_image = [{"keypoints": torch.zeros(n, 2, device="cuda"), "descriptors": torch.from_numpy(s[k, :n]).cuda()} for k, n in enumerate(NUM)]
    refs = oracle_case(128, "f16", None, 0.9, None, True)
    res = glue.match_pairs(m, per_image, PAIRS)
    batch = glue.match_batch(m, [per_image[i] for i, _ in PAIRS], [per_image[j] for _, j in PAIRS])
    for got in (res, batch):
        assert len(got) == len(PAIRS)
        for p, ((i, j), r) in enumerate(zip(PAIRS, got)):
            assert r["matches0"].shape == (NUM[i],) and r["matches1"].shape == (NUM[j],) and r["prune0"].shape == (NUM[i],) and r["stop"] == 0
            assert r["matches"].shape[1] == 2 and r["scores"].shape == (r["matches"].shape[0],)
        stacked = {k: [r[k] for r in got] for k in ("matches0", "matches1", "matching_scores0", "matching_scores1", "matches", "scores")}
        compare(stacked, [{k: (v[:NUM[i]] if k.endswith("0") and k != "matches" else v[:NUM[j]] if k.endswith("1") else v) for k, v in r.items()}
                          for (i, j), r in zip(PAIRS, refs)], "glue")
    # the reference's two-image helper shape: a matcher call on batch-1 feature dicts
    one = m({"image0": {"descriptors": per_image[0]["descriptors"][None]}, "image1": {"descriptors": per_image[1]["descriptors"][None]}})
    assert one["stop"] == 0 and torch.equal(glue.rbd(one)["matches0"], res[0]["matches0"])


# ---------------------------------------------------------------------- test 8: exact duplicates among the columns
DUP_D = 64


@functools.lru_cache(maxsize=None)
def duplicates_case():
    """image 1: 150 random rows; rows 3, 70, 140 are one row r (three tiles), rows 7 and 100 the unit vector e_0.  image 0: random rows, row 0 a noised r (its
    nearest neighbours are the three copies, all at the same distance d1 > 0), row 1 = e_0 (d1 == 0 exactly in any precision)."""
    rng = np.random.Generator(np.random.PCG64(8))
    b = rng.standard_normal((1, 150, DUP_D)).astype(np.float32)
    a = rng.standard_normal((1, 40, DUP_D)).astype(np.float32)
    b[0, [70, 140]] = b[0, 3]
    b[0, [7, 100]] = np.eye(DUP_D, dtype=np.float32)[0]
    a[0, 0] = b[0, 3] + (0.1 * rng.standard_normal(DUP_D)).astype(np.float32)
    a[0, 1] = b[0, 7]
    sim = O.similarity(a[0], b[0])
    return a, b, {ratio: [O.match(sim, mutual=False, ratio=ratio, duplicates_ok=True)] for ratio in (None, 0.8)}


@pytest.mark.gpu
@pytest.mark.parametrize("ratio", [None, 0.8])
def test_duplicate_rows_lowest_index_and_ratio(ratio):
    a, b, refs = duplicates_case()
    out = NearestNeighborMatcher(mutual=False, ratio_threshold=ratio).match_pairs(feats_of(a), [(0, 0)], feats_of(b))
    compare(out, refs[ratio], f"duplicates ratio {ratio}", cap=SMALL_CAP)
    m0 = out["matches0"][0]
    assert int(m0[0]) == (3 if ratio is None else -1)          # equal distances: the lowest index — and d1 <= 0.64 d1 fails for d1 > 0
    assert int(m0[1]) == 7 and float(out["matching_scores0"][0, 1]) == 1.0      # d1 == 0 passes the ratio test
    # the copies themselves, seen from image 1: each has row 0 of image 0 as its neighbour, at identical similarities
    assert out["matching_scores1"][0, 3] == out["matching_scores1"][0, 70] == out["matching_scores1"][0, 140]
