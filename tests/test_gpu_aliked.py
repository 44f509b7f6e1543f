"""ALIKED on the MI355X against fixtures produced by the REAL reference class (tools/make_golden_aliked.py: aliked.py executed unmodified
with seeded weights; torchvision's deform_conv2d restated in plain torch, checked in test_aliked_cpu.py).

Bars: the network is exact fp32, so the score map agrees with the reference's torch convolutions to summation-order round-off (1e-5 abs).
DKD thresholds and NMS-compares those scores, so a keypoint may differ from the reference's only where the fixture's recorded margin
(threshold or NMS near-tie) lies within that round-off; at most 1 % may differ.  On the common keypoints: coordinates 1e-3 px (soft-argmax
sums in another order), scores 1e-5, descriptors 2e-4 (two 128-deep and one 1152-deep fp32 contraction after a per-keypoint normalisation)."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

import make_golden_aliked as G
from conftest import require_gpu

GOLD = Path(__file__).resolve().parent / "golden" / "aliked"
NAMES = sorted(p.stem for p in GOLD.glob("*.npz"))
ROUNDOFF = 1e-5


def _load(name):
    z = np.load(GOLD / f"{name}.npz")
    meta = json.loads(str(z["meta"]))
    return meta, {k: z[k] for k in z.files if k != "meta"}


def _model(meta):
    from lightglue_amd import ALIKED
    sd = G.aliked_state_dict(meta["wseed"], meta["model"])
    return ALIKED(weights=sd, model_name=meta["model"], **meta["conf"]).eval().cuda()


def _images(meta):
    seeds = meta["iseeds"]
    if len(seeds) == 1:
        return G.aliked_image(seeds[0], meta["b"], meta["h"], meta["w"], meta["c"])
    return torch.cat([G.aliked_image(s, 1, meta["h"], meta["w"], meta["c"]) for s in seeds], 0)


def _match(ref_k, got_k, tol=1e-2):
    """index pairs (i_ref, j_got) of keypoints at the same position"""
    if len(ref_k) == 0 or len(got_k) == 0:
        return np.zeros(0, int), np.zeros(0, int)
    d = np.linalg.norm(ref_k[:, None, :] - got_k[None, :, :], axis=-1)
    j = d.argmin(1)
    ok = d[np.arange(len(ref_k)), j] < tol
    return np.nonzero(ok)[0], j[ok]


def _compare(meta, gold, out):
    counts = out["num_keypoints"].cpu().numpy()
    kp, ks, ds = (out[k].cpu().numpy() for k in ("keypoints", "keypoint_scores", "descriptors"))
    margin = min(meta["threshold_margin"], meta["nms_tie_margin"])
    for b in range(meta["b"]):
        n_ref, n_got = int(gold["counts"][b]), int(counts[b])
        rk, gk = gold["keypoints"][b, :n_ref], kp[b, :n_got]
        i, j = _match(rk, gk)
        differ = max(n_ref, n_got) - len(i)
        if differ:
            assert margin < ROUNDOFF, f"image {b}: {differ} keypoints differ although the fixture has no tie within round-off (margin {margin:.2e})"
            assert differ <= 0.01 * max(n_ref, 1), f"image {b}: {differ} of {n_ref} keypoints differ"
        assert np.abs(rk[i] - gk[j]).max(initial=0) <= 1e-3, "keypoint coordinates"
        assert np.abs(gold["keypoint_scores"][b, i] - ks[b, j]).max(initial=0) <= 1e-5, "keypoint scores"
        assert np.abs(gold["descriptors"][b, i] - ds[b, j]).max(initial=0) <= 2e-4, "descriptors"
        if meta["conf"].get("max_num_keypoints", -1) > 0 and not differ and (j != np.arange(len(j))).any():
            # sorted outputs: the reference's order, except among scores tied within round-off (torch's sort leaves their order open)
            assert margin < ROUNDOFF, "order of the best-by-score keypoints"
        assert not ds[b, n_got:].any() and not kp[b, n_got:].any(), "padding rows are zero"


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_aliked_matches_reference(name):
    require_gpu()
    meta, gold = _load(name)
    model = _model(meta)
    img = _images(meta).cuda()
    scores, _ = model.encode(img)
    torch.cuda.synchronize()
    err = float(np.abs(scores.cpu().numpy() - gold["scores"]).max())
    assert err <= ROUNDOFF, f"score map differs by {err:.2e}"
    out = model({"image": img})
    torch.cuda.synchronize()
    _compare(meta, gold, out)


@pytest.mark.gpu
def test_ragged_batch_equals_per_image_calls():
    require_gpu()
    meta, _ = _load("n16_rgb_ragged_2x80x104")
    model = _model(meta)
    img = _images(meta).cuda()
    out = model({"image": img})
    counts = out["num_keypoints"].cpu().numpy()
    assert counts[0] != counts[1]
    for b in range(2):
        one = model({"image": img[b:b + 1]})
        n = int(counts[b])
        assert int(one["num_keypoints"][0]) == n
        for k in ("keypoints", "keypoint_scores", "descriptors"):
            torch.testing.assert_close(out[k][b, :n], one[k][0, :n], rtol=0, atol=0)


@pytest.mark.gpu
def test_gray_equals_rgb_broadcast():
    require_gpu()
    meta, _ = _load("n16_gray_b1_96x128_fallback")
    model = _model(meta)
    gray = _images(meta).cuda()
    a, b = model({"image": gray}), model({"image": gray.expand(-1, 3, -1, -1).contiguous()})
    for k in ("keypoints", "keypoint_scores", "descriptors", "num_keypoints"):
        torch.testing.assert_close(a[k], b[k], rtol=0, atol=0)


@pytest.mark.gpu
def test_image_size_borders_and_extract():
    """image_size moves the far borders (ref :162-166); extract() attaches image_size and keeps the pixel frame."""
    require_gpu()
    meta, _ = _load("n16_rgb_b1_120x160_th")
    model = _model(meta)
    img = _images(meta).cuda()
    out = model({"image": img, "image_size": torch.tensor([[100.0, 90.0]], device="cuda")})
    n = int(out["num_keypoints"][0])
    k = out["keypoints"][0, :n]
    assert n > 0 and float(k[:, 0].max()) < 100 - 2 + 1 and float(k[:, 1].max()) < 90 - 2 + 1
    feats = model.extract(img[0])
    assert feats["image_size"].tolist() == [[160.0, 120.0]]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model({"image": img.cpu()})


@pytest.mark.gpu
def test_workspace_is_not_a_dense_feature_map():
    """1024 x 768: encode workspace + level maps stay well below the B H W 128 fp32 map the reference materialises."""
    require_gpu()
    from lightglue_amd import _cabi
    lib = _cabi.load()
    b, h, w = 2, 768, 1024
    total = lib.lg_aliked_workspace_bytes(b, h, w, 16) + lib.lg_aliked_levels_bytes(b, h, w)
    assert 0 < total < b * h * w * 128 * 4


@pytest.mark.gpu
def test_end_to_end_with_lightglue():
    """ALIKED -> a 128-d LightGlue (the features="aliked" configuration, seeded weights) through glue.match_pair gives the matches of the matcher fed the reference's features."""
    require_gpu()
    from lightglue_amd import LightGlue, match_pair
    from lightglue_amd import synthetic as synth
    meta, gold = _load("n16_rgb_ragged_2x80x104")
    extractor = _model(meta)
    sd = synth.make_state_dict(0, input_dim=128, recipe="A")
    matcher = LightGlue(features=None, input_dim=128, depth_confidence=-1, width_confidence=-1).eval()
    matcher.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    matcher = matcher.cuda()
    img = _images(meta).cuda()
    f0, f1, m01 = match_pair(extractor, matcher, img[0], img[1])
    ref = {}
    for b in range(2):
        n = int(gold["counts"][b])
        ref[f"image{b}"] = {"keypoints": torch.from_numpy(gold["keypoints"][b:b + 1, :n]).cuda(),
                            "descriptors": torch.from_numpy(gold["descriptors"][b:b + 1, :n]).cuda(),
                            "image_size": torch.tensor([[meta["w"], meta["h"]]], dtype=torch.float32, device="cuda")}
    r01 = matcher(ref)
    got, exp = m01["matches0"].cpu().numpy(), r01["matches0"][0].cpu().numpy()
    assert got.shape == exp.shape
    assert (got != exp).sum() <= max(1, int(0.01 * len(exp))), f"{int((got != exp).sum())} of {len(exp)} matches differ"
    assert (exp > -1).sum() > 0
