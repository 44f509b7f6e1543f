"""oracle/aliked_oracle.py (numpy; float64 wherever the operation is continuous) against the reference's OWN DKD and SDDH modules, run by
`tools/make_golden_aliked.py --stages` on seeded crafted inputs (tests/golden/aliked_stages/*.npz).  The GPU stage tests
(test_gpu_detect_stages.py, test_gpu_aliked_stages.py) compare the kernels with this oracle, so it is pinned here first.

Discrete outputs — which pixels DKD keeps, and in which order — must agree exactly, except inside groups of equal scores, whose order (and,
at the cut, whose members) torch.sort / topk leave open.  Continuous outputs are compared within T_ref, the largest deviation of the
reference's fp32 results from the float64 oracle over all stage fixtures, per quantity.  Measured (`AO.T_REF` holds these figures, this
module asserts them with a margin of 2x, the GPU tests allow the kernels 4x):

    knorm (normalised keypoints, [-1, 1])      1.65e-07   (dkd_many_*: 272 x 96, r = 1)        T_REF 1.7e-07
    keypoints (pixels)                         4.54e-05   (dkd_wide_*: 24 x 600)               T_REF 4.6e-05
    keypoint_scores                            3.57e-05   (dkd_wide_*)                         T_REF 3.6e-05
    descriptors (unit norm, 128-d)             1.01e-06   (sddh_n16_b2_40x56_n33_clamped)      T_REF 1.1e-06

knorm: x / wh * 2 - 1 is rounded three times near +-1 (ulp 6e-8) after an fp32 soft-argmax.  Pixel keypoints carry that error times
(w - 1) / 2 = 300 on the 600-wide map.  The bilinear score inherits the position error times the map's slope, which on these noise maps is
close to one score unit per pixel (on a network's smooth score map it is 1e-5, test_gpu_aliked.py).  Descriptors: three fp32 contractions
(1152, 128 and up to 4096 deep); the largest error is where the clamped offsets put samples on the map's edge."""
import json
from pathlib import Path

import numpy as np
import pytest

import make_golden_aliked as G
from oracle import aliked_oracle as AO

STAGES = Path(__file__).resolve().parent / "golden" / "aliked_stages"
GENS = {"score_maps": G.score_maps, "quantised_maps": G.quantised_maps}


def load(name):
    z = np.load(STAGES / f"{name}.npz")
    return json.loads(str(z["meta"])), {k: z[k] for k in z.files if k != "meta"}


def assert_same_selection(idx, ref_idx, score_flat, candidates, ordered):
    """idx == ref_idx, except where scores tie: within a group of equal scores the order is open, and the group the cut splits (the lowest
    score of a limited selection) may hold any candidates of that score (the idea of test_superpoint_head.assert_same_detections)."""
    assert len(idx) == len(ref_idx)
    sc, ref_sc = score_flat[idx], score_flat[ref_idx]
    np.testing.assert_array_equal(sc, ref_sc)            # the same scores in the same places: only tie groups can differ
    if not ordered:                                      # raster order is defined
        np.testing.assert_array_equal(idx, ref_idx)
        return
    cand = set(candidates.tolist())
    for v in np.unique(sc):
        mine, theirs = set(idx[sc == v].tolist()), set(ref_idx[ref_sc == v].tolist())
        if v == sc.min():
            assert mine <= cand and theirs <= cand and len(mine) == len(theirs)
        else:
            assert mine == theirs


def dkd_case(name):
    meta, gold = load(name)
    smap = GENS[meta["gen"]](*meta["args"])
    sel = AO.dkd_select(smap, meta["radius"], meta["top_k"], meta["scores_th"], meta["n_limit"], meta["image_size"])
    everything = AO.dkd_select(smap, meta["radius"], -1, 1e-30 if meta["top_k"] > 0 else meta["scores_th"], smap[0].size, meta["image_size"])
    return meta, gold, smap, sel, everything


@pytest.mark.parametrize("name", sorted(G.DKD_STAGES))
def test_dkd_select_matches_reference(name):
    meta, gold, smap, sel, everything = dkd_case(name)
    ends = np.cumsum(gold["counts"])
    for b in range(smap.shape[0]):
        ref_idx = gold["indices"][ends[b] - gold["counts"][b]:ends[b]].astype(np.int64)
        ordered = meta["top_k"] > 0 or len(everything[b]) > meta["n_limit"]
        assert_same_selection(sel[b], ref_idx, smap[b].reshape(-1), everything[b], ordered)


def dkd_deviation(name):
    """per quantity: the largest |reference fp32 - oracle float64| of a DKD fixture, refined at the REFERENCE's indices"""
    meta, gold = load(name)
    smap = GENS[meta["gen"]](*meta["args"])
    ends = np.cumsum(gold["counts"])
    dev = {"knorm": 0.0, "keypoints": 0.0, "keypoint_scores": 0.0}
    for b in range(smap.shape[0]):
        sl = slice(ends[b] - gold["counts"][b], ends[b])
        kn, kp, ks = AO.dkd_refine(smap[b], gold["indices"][sl], meta["radius"])
        for key, val in (("knorm", kn), ("keypoints", kp), ("keypoint_scores", ks)):
            dev[key] = max(dev[key], float(np.abs(gold[key][sl] - val).max(initial=0)))
    return dev


def sddh_deviation(name):
    meta, gold = load(name)
    sd = G.scaled_offset_weights(G.aliked_state_dict(meta["wseed"], meta["model"]), meta["gain"])
    levels = G.crafted_levels(meta["lseed"], meta["b"], meta["h"], meta["w"])
    kn = G.stage_knorm(meta["kseed"], meta["b"], meta["n"], meta["h"], meta["w"])
    d = AO.sddh(levels, (meta["h"], meta["w"]), kn, {k: v.numpy() for k, v in sd.items() if k.startswith("desc_head.")}, 32 if meta["model"].endswith("32") else 16)
    assert np.isfinite(gold["descriptors"]).all()
    return float(np.abs(gold["descriptors"] - np.stack(d)).max())


@pytest.mark.parametrize("name", sorted(G.DKD_STAGES))
def test_dkd_refine_matches_reference(name):
    dev = dkd_deviation(name)
    print(name, dev)
    for key, v in dev.items():
        assert v <= 2 * AO.T_REF[key], (key, v)


@pytest.mark.parametrize("name", sorted(G.SDDH_STAGES))
def test_sddh_matches_reference(name):
    dev = sddh_deviation(name)
    print(name, dev)
    assert dev <= 2 * AO.T_REF["descriptors"]


def test_t_ref_is_the_measured_deviation():
    """T_REF is what the fixtures measure, not a bar picked above it: the largest deviation over all stage fixtures lies in (T_REF / 2, T_REF]."""
    worst = {"descriptors": max(sddh_deviation(n) for n in G.SDDH_STAGES)}
    for n in G.DKD_STAGES:
        for key, v in dkd_deviation(n).items():
            worst[key] = max(worst.get(key, 0.0), v)
    print(worst)
    for key, v in worst.items():
        assert AO.T_REF[key] / 2 < v <= AO.T_REF[key], (key, v, AO.T_REF[key])


def test_fixture_files_match_the_case_tables():
    assert sorted(p.stem for p in STAGES.glob("*.npz")) == sorted([*G.DKD_STAGES, *G.SDDH_STAGES])


# --------------------------------------------------------------------------- the oracle's own rules, on inputs small enough to read
def test_tie_rule_and_cut_inside_a_tie_group():
    """constant map: every interior pixel ties; a limit keeps the first ones in raster order (top-k and n_limit alike)"""
    m = np.full((1, 12, 10), 0.5, np.float32)
    interior = np.array([y * 10 + x for y in range(2, 10) for x in range(2, 8)])
    assert AO.dkd_select(m, 2, -1, 0.2, 20000)[0].tolist() == interior.tolist()
    assert AO.dkd_select(m, 2, -1, 0.2, 7)[0].tolist() == interior[:7].tolist()
    assert AO.dkd_select(m, 2, 7, -1.0, 20000)[0].tolist() == interior[:7].tolist()
    m[0, 6:] = 0.75     # the better group first, then the first of the worse one
    got = AO.dkd_select(m, 2, -1, 0.2, 30)[0]
    upper = np.array([y * 10 + x for y in range(6, 10) for x in range(2, 8)])
    assert got.tolist() == upper.tolist() + interior[:6].tolist()


def test_batch_rule_mean_mode_image_size_and_top_k_shortfall():
    m = G.score_maps(30, 3, 20, 24)
    means = AO.image_mean(m)
    per_image = [np.nonzero(AO.dkd_nms(m, 2)[b].reshape(-1) > means[b])[0] for b in range(3)]
    for got, want in zip(AO.dkd_select(m, 2, -1, 0.99, 20000), per_image):       # nothing above 0.99 anywhere: three means
        assert got.tolist() == want.tolist() and len(got) > 0
    for got, want in zip(AO.dkd_select(m, 2, -1, -1.0, 20000), per_image):       # the mean mode
        assert got.tolist() == want.tolist()
    m[1, 10, 10] = 0.995                                                         # one pixel of ONE image passes: no fallback anywhere
    got = AO.dkd_select(m, 2, -1, 0.99, 20000)
    assert [g.tolist() for g in got] == [[], [10 * 24 + 10], []]
    full = AO.dkd_select(m, 2, -1, 0.2, 20000)
    part = AO.dkd_select(m, 2, -1, 0.2, 20000, image_size=[[17.9, 15.2]] * 3)    # (w, h), truncated to 17 x 15
    for f, p in zip(full, part):
        y, x = np.divmod(f, 24)
        assert p.tolist() == f[(x < 17 - 2) & (y < 15 - 2)].tolist()
    z = np.zeros((1, 9, 9), np.float32)
    z[0, 4, 4] = 0.3
    assert AO.dkd_select(z, 2, 5, -1.0, 20000)[0].tolist() == [40]               # top-k: positive maxima only
    assert AO.dkd_select(np.zeros((1, 9, 9), np.float32), 2, -1, 0.2, 20000)[0].tolist() == []


def test_refine_on_a_symmetric_peak_and_keypoint_pixels():
    s = np.full((9, 11), 0.1, np.float32)
    s[4, 5] = 0.9
    kn, kp, ks = AO.dkd_refine(s, np.array([4 * 11 + 5]), 2)
    np.testing.assert_allclose(kp, [[5.0, 4.0]], atol=1e-12)
    np.testing.assert_allclose(kn, [[0.0, 0.0]], atol=1e-12)
    np.testing.assert_allclose(ks, [0.9], atol=1e-6)
    kwh, corner = AO.keypoint_pixels(np.array([[-1, -1], [1, 1], [0, 0]], np.float32), 8, 8)
    assert kwh.tolist() == [[0, 0], [7, 7], [3.5, 3.5]] and corner.tolist() == [[0, 0], [4, 4], [2, 2]]   # the corner clamp at w - 1 - 3
