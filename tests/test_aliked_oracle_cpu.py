"""oracle/aliked_oracle.py (numpy; float64 wherever the operation is continuous) against the reference's OWN DKD and SDDH modules and its whole
encoder, run by `tools/make_golden_aliked.py --stages` on seeded crafted inputs (tests/golden/aliked_stages/*.npz).  The GPU stage tests
(test_gpu_detect_stages.py, test_gpu_aliked_stages.py, test_gpu_aliked_encoder.py) compare the kernels with this oracle, so it is pinned here first.

Discrete outputs — which pixels DKD keeps, and in which order — must agree exactly, except inside groups of equal scores, whose order (and,
at the cut, whose members) torch.sort / topk leave open.  Continuous outputs are compared within T_ref, the largest deviation of the
reference's fp32 results from the float64 oracle over all stage fixtures, per quantity.  Measured (`AO.T_REF` holds these figures, this
module asserts them with a margin of 2x, the GPU tests allow the kernels 4x):

    knorm (normalised keypoints, [-1, 1])      1.65e-07   (dkd_many_*: 272 x 96, r = 1)        T_REF 1.7e-07
    keypoints (pixels)                         4.54e-05   (dkd_wide_*: 24 x 600)               T_REF 4.6e-05
    keypoint_scores                            3.57e-05   (dkd_wide_*)                         T_REF 3.6e-05
    descriptors (unit norm, 128-d)             1.01e-06   (sddh_n16_b2_40x56_n33_clamped)      T_REF 1.1e-06
    x1 (level maps: rms about 1, max 3 .. 5)   1.52e-06   (enc_24x17_b2_rgb_noise_g4)          T_REF 1.6e-06
    x2                                         2.12e-06   (enc_8x8_b1_rgb_noise_g1)            T_REF 2.2e-06
    x3                                         3.17e-06   (enc_40x56_b1_rgb_image_g4)          T_REF 3.2e-06
    x4                                         1.59e-06   (enc_72x90_b1_rgb_noise_g1)          T_REF 1.6e-06
    encoder_scores                             7.18e-06   (enc_40x300_b1_rgb_noise_g4)         T_REF 7.2e-06

The encoder rows compare `AO.encoder` with the reference's whole ALIKED module on the `ENC_STAGES` images (x1, x2 on the five fixtures that store
them).  x3 is the deepest fp32 chain in front of a 576-deep contraction on clamped, partly-outside samples; the scores' figure comes from the one
case whose logits reach +-7, where the sigmoid's argument carries the four levels' errors through three more convolutions.

knorm: x / wh * 2 - 1 is rounded three times near +-1 (ulp 6e-8) after an fp32 soft-argmax.  Pixel keypoints carry that error times
(w - 1) / 2 = 300 on the 600-wide map.  The bilinear score inherits the position error times the map's slope, which on these noise maps is
close to one score unit per pixel (on a network's smooth score map it is 1e-5, test_gpu_aliked.py).  Descriptors: three fp32 contractions
(1152, 128 and up to 4096 deep); the largest error is where the clamped offsets put samples on the map's edge."""
import functools
import json
from pathlib import Path

import numpy as np
import pytest
import torch

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


@functools.lru_cache(maxsize=None)
def encoder_case(name, eps=AO.BN_EPS):
    """(meta, fixture, oracle levels, oracle scores, offset trace) of an encoder fixture; computed once, shared, never modified"""
    meta, gold = load(name)
    sd, image = G.encoder_inputs(name)
    assert meta == dict(zip(("wseed", "gen", "iseed", "b", "c", "h", "w", "gain", "small_variance"), G.ENC_STAGES[name][:9]))
    trace = {}
    levels, scores = AO.encoder(image.numpy(), {k: v.numpy() for k, v in sd.items()}, trace=trace, eps=eps)
    return meta, gold, levels, scores, trace["offsets"]


def encoder_deviation(name):
    """per quantity the fixture stores: the largest |reference fp32 - oracle float64|"""
    meta, gold, levels, scores, _ = encoder_case(name)
    hp, wp, _, _ = AO.padded_dims(meta["h"], meta["w"])
    dev = {}
    for i, s in enumerate((0, 1, 3, 5)):
        assert levels[i].shape == (meta["b"], hp >> s, wp >> s, 32) and np.isfinite(levels[i]).all()
        if f"x{i + 1}" in gold:
            assert gold[f"x{i + 1}"].shape == levels[i].shape and np.isfinite(gold[f"x{i + 1}"]).all()
            dev[f"x{i + 1}"] = float(np.abs(gold[f"x{i + 1}"] - levels[i]).max())
    assert gold["scores"].shape == scores.shape == (meta["b"], meta["h"], meta["w"])
    dev["encoder_scores"] = float(np.abs(gold["scores"] - scores).max())
    return dev


@pytest.mark.parametrize("name", sorted(G.ENC_STAGES))
def test_encoder_matches_reference(name):
    dev = encoder_deviation(name)
    print(name, dev)
    stored = {"x3", "x4", "encoder_scores"} | ({"x1", "x2"} if G.ENC_STAGES[name][9] else set())
    assert set(dev) == stored
    for key, v in dev.items():
        assert v <= 2 * AO.T_REF[key], (key, v)


def test_t_ref_is_the_measured_deviation():
    """T_REF is what the fixtures measure, not a bar picked above it: the largest deviation over all stage fixtures lies in (T_REF / 2, T_REF]."""
    worst = {"descriptors": max(sddh_deviation(n) for n in G.SDDH_STAGES)}
    for n in G.DKD_STAGES:
        for key, v in dkd_deviation(n).items():
            worst[key] = max(worst.get(key, 0.0), v)
    for n in G.ENC_STAGES:
        for key, v in encoder_deviation(n).items():
            worst[key] = max(worst.get(key, 0.0), v)
    print(worst)
    assert set(worst) == set(AO.T_REF)
    for key, v in worst.items():
        assert AO.T_REF[key] / 2 < v <= AO.T_REF[key], (key, v, AO.T_REF[key])


def test_fixture_files_match_the_case_tables():
    assert sorted(p.stem for p in STAGES.glob("*.npz")) == sorted([*G.DKD_STAGES, *G.SDDH_STAGES, *G.ENC_STAGES])


# --------------------------------------------------------------------------- what the encoder cases cover, from the oracle's offset trace alone
def offset_coverage(off):
    """(share of offsets at the clamp, share of samples inside / partly outside / outside) of one clamped offset tensor [B, h, w, 18]"""
    h, w = off.shape[1:3]
    assert np.abs(off).max() <= max(h, w) / 4.0
    inside, partly, outside = AO.sample_classes(*AO.deform_positions(off), h, w)
    assert ((inside.astype(int) + partly + outside) == 1).all()
    return float((np.abs(off) == max(h, w) / 4.0).mean()), float(inside.mean()), float(partly.mean()), float(outside.mean())


@pytest.mark.parametrize("name", sorted(n for n, c in G.ENC_STAGES.items() if c[7] == 4.0))
def test_gain_4_cases_put_block3_samples_everywhere(name):
    """so that the GPU comparison cannot pass emptily: in both deformable convs of block3 the clamp acts (on most offsets where the level is at most
    8 x 8, its clamp at most 2 px) and the samples fall inside the map, on cells that straddle its border, and outside it"""
    offsets = encoder_case(name)[4]
    assert len(offsets) == 4
    for off in offsets[:2]:
        clamped, inside, partly, outside = offset_coverage(off)
        print(name, off.shape[1:3], f"clamped {clamped:.0%} inside {inside:.0%} partly {partly:.0%} outside {outside:.0%}")
        if max(off.shape[1:3]) <= 8:
            assert clamped >= 0.5
        assert inside >= 0.05 and partly >= 0.05 and outside >= 0.05


@pytest.mark.parametrize("name", sorted(n for n, c in G.ENC_STAGES.items() if AO.padded_dims(c[5], c[6])[:2] == (32, 32)))
def test_one_by_one_level_has_partly_outside_and_outside_samples(name):
    """block4 on a 1 x 1 map: no sample's cell lies on the map; both other classes occur, in both convs"""
    for off in encoder_case(name)[4][2:]:
        assert off.shape[1:3] == (1, 1) and np.abs(off).max() <= 0.25
        _, inside, partly, outside = offset_coverage(off)
        assert inside == 0
        assert partly > 0 and outside > 0


def test_small_variance_case_sees_the_epsilon():
    """with BatchNorm's 1e-5 replaced by 0 the oracle moves some level map by more than 100 x T_REF: a kernel-side fold with another epsilon cannot
    hide in this case (under the seeded variances of [0.5, 1.5] it moves the maps by about 1e-5 relative)"""
    name = "enc_8x8_b1_rgb_noise_g4_smallvar"
    levels, levels0 = encoder_case(name)[2], encoder_case(name, 0.0)[2]
    moved = {f"x{i + 1}": float(np.abs(a - b).max()) / AO.T_REF[f"x{i + 1}"] for i, (a, b) in enumerate(zip(levels, levels0))}
    print(moved)
    assert max(moved.values()) > 100
    var = np.concatenate([v.numpy().ravel() for k, v in G.encoder_inputs(name)[0].items() if k.endswith("running_var")])
    assert 1e-6 <= var.min() and var.max() <= 1e-3


def test_encoder_input_generators():
    sd = G.aliked_state_dict(30)
    up = G.scaled_encoder_offsets(sd, 4.0)
    changed = sorted(k for k in sd if not torch.equal(sd[k], up[k]))
    assert changed == sorted(f"{n}.{p}" for n in G.ENCODER_OFFSET_CONVS for p in ("bias", "weight")) and len(changed) == 8
    assert all(torch.equal(up[k], sd[k] * 4.0) for k in changed)
    sv = G.small_variance(sd, 1)
    for k in sd:
        if k.endswith("running_var"):
            w = k[:-len("running_var")] + "weight"
            assert torch.equal(sv[w], sd[w] * torch.sqrt(sv[k] + 1e-5)) and not torch.equal(sv[k], sd[k])
        elif not (".bn" in k and k.endswith("weight")):
            assert torch.equal(sv[k], sd[k])
    img = G.noise_image(1, 2, 9, 11, 3)
    assert img.shape == (2, 3, 9, 11) and img.dtype == torch.float32 and 0 <= float(img.min()) and float(img.max()) < 1
    assert torch.equal(img, G.noise_image(1, 2, 9, 11, 3)) and not torch.equal(img[0], img[1])


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


# --------------------------------------------------------------------------- the encoder's own rules, on inputs small enough to read
def test_deform_conv_at_zero_offsets_is_the_plain_conv_and_integer_offsets_shift_it():
    rng = np.random.Generator(np.random.PCG64(1))
    x, w = rng.standard_normal((2, 5, 7, 3)), rng.standard_normal((4, 3, 3, 3))
    zero = np.zeros((2, 5, 7, 18))
    plain = AO.conv2d(x, w)
    np.testing.assert_allclose(AO.deform_conv2d(x, zero, w), plain, atol=1e-13)
    # every tap moved by (dy, dx) = (1, -2): the plain conv of the map shifted up by one and right by two, zeros moving in.  (Not in the first row
    # and the last column: there a moved tap lands ON the map where the plain conv of the shifted map reads its zero padding.)
    off = zero.copy()
    off[..., 0::2], off[..., 1::2] = 1.0, -2.0
    shifted = np.zeros_like(x)
    shifted[:, :-1, 2:] = x[:, 1:, :-2]
    np.testing.assert_allclose(AO.deform_conv2d(x, off, w)[:, 1:, :-1], AO.conv2d(shifted, w)[:, 1:, :-1], atol=1e-13)
    # ONE tap moved: only that tap's term changes.  Tap k = 3 i + j = 5 is (i, j) = (1, 2), the pixel to the right; dy in channel 10, dx in channel 11
    off = zero.copy()
    off[..., 10], off[..., 11] = 2.0, -1.0                    # it now reads the pixel two rows below the centre
    below = np.zeros_like(x)
    below[:, :-2] = x[:, 2:]
    right = np.zeros_like(x)
    right[:, :, :-1] = x[:, :, 1:]
    np.testing.assert_allclose(AO.deform_conv2d(x, off, w), plain + (below - right) @ w[:, :, 1, 2].T, atol=1e-13)


def test_deform_sample_border_rules():
    """a 2 x 3 map of ones and a filter that reads the centre tap only: the output IS the sample.  Half a pixel off the map keeps half the weight, each
    corner dropped on its own; at one pixel off the sample is zero; between h - 1 and h the far row is dropped."""
    x, w = np.ones((1, 2, 3, 1)), np.zeros((1, 1, 3, 3))
    w[0, 0, 1, 1] = 1.0

    def centre(dy, dx):
        off = np.zeros((1, 2, 3, 18))
        off[..., 8], off[..., 9] = dy, dx
        return AO.deform_conv2d(x, off, w)[0, :, :, 0]

    np.testing.assert_allclose(centre(-0.5, 0.0), [[0.5, 0.5, 0.5], [1, 1, 1]])
    np.testing.assert_allclose(centre(-0.5, -0.5), [[0.25, 0.5, 0.5], [0.5, 1, 1]])
    np.testing.assert_allclose(centre(-1.0, 0.0), [[0, 0, 0], [1, 1, 1]])
    np.testing.assert_allclose(centre(0.75, 0.0), [[1, 1, 1], [0.25, 0.25, 0.25]])         # row 1 + 0.75 lies in (h - 1, h)
    np.testing.assert_allclose(centre(1.0, 0.25), [[1, 1, 0.75], [0, 0, 0]])               # row 1 + 1 = h: zero; column 2.25: the far corner dropped
    py, px = AO.deform_positions(np.zeros((1, 2, 3, 18)))
    assert py[0, 0, 0].tolist() == [-1, -1, -1, 0, 0, 0, 1, 1, 1] and px[0, 0, 2].tolist() == [1, 2, 3] * 3
    inside, partly, outside = AO.sample_classes(np.array([0.0, 1.0, -0.5, 1.5, -1.0, 2.0]), np.array([0.0, 2.0, 1.0, 1.0, 1.0, 1.0]), 2, 3)
    assert inside.tolist() == [True, True, False, False, False, False] and partly.tolist() == [False, False, True, True, False, False]
    assert outside.tolist() == [False, False, False, False, True, True]


def test_padding_geometry_for_odd_pads():
    """InputPadder(32): the odd pixel of an odd pad goes to the FAR side (left / top get pad // 2), replicated from the border pixel"""
    assert AO.padded_dims(24, 17) == (32, 32, 4, 7) and AO.padded_dims(31, 33) == (32, 64, 0, 15) and AO.padded_dims(64, 32) == (64, 32, 0, 0)
    x = np.arange(24 * 17, dtype=np.float64).reshape(1, 24, 17, 1)
    p = AO.replicate_pad(x)
    assert p.shape == (1, 32, 32, 1)
    np.testing.assert_array_equal(p[0, 4:28, 7:24, 0], x[0, :, :, 0])
    np.testing.assert_array_equal(p[0, :4, 7:24, 0], np.broadcast_to(x[0, 0, :, 0], (4, 17)))
    np.testing.assert_array_equal(p[0, 4:28, 24:, 0], np.broadcast_to(x[0, :, 16:, 0], (24, 8)))
    assert p[0, 0, 0, 0] == x[0, 0, 0, 0] and p[0, 31, 31, 0] == x[0, 23, 16, 0]
    q = AO.replicate_pad(np.arange(31 * 33, dtype=np.float64).reshape(1, 31, 33, 1))
    assert q.shape == (1, 32, 64, 1) and q[0, 0, 15, 0] == 0 and q[0, 31, 15, 0] == q[0, 30, 15, 0] == 30 * 33 and q[0, 0, 47, 0] == q[0, 0, 63, 0] == 32
    # batch norm as written, average pooling
    sd = {"bn.weight": np.array([2.0]), "bn.bias": np.array([0.5]), "bn.running_mean": np.array([1.0]), "bn.running_var": np.array([4.0 - 1e-5])}
    np.testing.assert_allclose(AO.batch_norm(np.array([[[[3.0]]]]), sd, "bn"), [[[[2.5]]]], atol=1e-15)
    np.testing.assert_allclose(AO.avg_pool(np.arange(16.0).reshape(1, 4, 4, 1), 2)[0, :, :, 0], [[2.5, 4.5], [10.5, 12.5]])
