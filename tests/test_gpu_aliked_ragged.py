"""ALIKED on a ragged batch: images of different sizes in the top-left corners of one canvas (`valid_size`), each with its own padding to a multiple of 32.
The yardstick is the uniform B = 1 call on the crop (itself pinned to the reference by tests/test_gpu_aliked.py), and the comparison is `torch.equal`: inside an
image every output of every stage is bit-identical, whatever lies outside it — NaN in the canvas padding, unwritten workspace rows, the other images."""
import functools
import json
from pathlib import Path

import numpy as np
import pytest
import torch

import make_golden_aliked as G
from conftest import require_gpu

GOLD = Path(__file__).resolve().parent / "golden" / "aliked"
# (h, w): centred pads 12 / 12; pads 15 + 16 and 0 + 1; no pad; one 32-pixel tile.  1/32-level maps of 2 x 3, 2 x 1, 2 x 3 and 1 x 1, three conv tiles across
SIZES = [(40, 72), (33, 31), (64, 96), (8, 8)]
CANVASES = [(64, 96), (70, 100)]      # the second pads to 96 x 128: tiles outside every image
MODES = {"threshold": {"detection_threshold": 0.2}, "topk": {"detection_threshold": 0.0, "max_num_keypoints": 64},
         "mean": {"detection_threshold": 0.0, "max_num_keypoints": -1}}
DTYPES = {"f32": torch.float32, "f16": torch.float16}
SHIFTS = (0, 1, 3, 5)


def _padded(h, w):
    return h + ((h // 32 + 1) * 32 - h) % 32, w + ((w // 32 + 1) * 32 - w) % 32


@functools.lru_cache(maxsize=None)
def _model(name, mode, dtype):
    from lightglue_amd import ALIKED
    return ALIKED(weights=G.aliked_state_dict(3, name), model_name=name, descriptor_dtype=DTYPES[dtype], **MODES[mode]).eval().cuda()


@functools.lru_cache(maxsize=None)
def _image(i, h, w, c):
    return G.aliked_image(40 + i, 1, h, w, c).cuda()


def _canvas(images, hc, wc, fill=float("nan")):
    canvas = torch.full((len(images), images[0].shape[1], hc, wc), fill, device="cuda")
    for b, img in enumerate(images):
        canvas[b, :, : img.shape[-2], : img.shape[-1]] = img[0]
    return canvas


@functools.lru_cache(maxsize=None)
def _crop_results(name, mode, dtype, c, sizes):
    """the yardstick, computed once per configuration: (scores, level maps, forward) of the uniform B = 1 call on every crop"""
    model, out = _model(name, mode, dtype), []
    for i, (h, w) in enumerate(sizes):
        img = _image(i, h, w, c)
        scores, levels = model.encode(img)
        out.append((scores, [m.clone() for m in model.level_maps(levels, (1, h, w))], model({"image": img})))
    torch.cuda.synchronize()
    return out


def _check_against_crops(model, sizes, c, canvas_hw, crops):
    hc, wc = canvas_hw
    canvas = _canvas([_image(i, h, w, c) for i, (h, w) in enumerate(sizes)], hc, wc)
    valid = [[w, h] for h, w in sizes]
    scores, levels = model.encode(canvas, valid_size=valid)
    maps = model.level_maps(levels, (len(sizes), hc, wc))
    out = model({"image": canvas, "valid_size": valid})
    torch.cuda.synchronize()
    counts = out["num_keypoints"].cpu().tolist()
    for b, (h, w) in enumerate(sizes):
        ref_scores, ref_maps, ref = crops[b]
        assert torch.equal(scores[b, :h, :w], ref_scores[0]), f"image {b}: scores inside {h} x {w}"
        outside = scores[b].clone()
        outside[:h, :w] = 0
        assert not outside.any(), f"image {b}: the scores outside the image must be 0"      # (NaN is truthy: a leak from the canvas padding fails here too)
        hp, wp = _padded(h, w)
        for lvl, s in enumerate(SHIFTS):
            assert torch.equal(maps[lvl][b, : hp >> s, : wp >> s], ref_maps[lvl][0]), f"image {b}: level map {lvl}"
        n = int(ref["num_keypoints"][0])
        assert counts[b] == n, f"image {b}: {counts[b]} keypoints, the crop gives {n}"
        for key in ("keypoints", "keypoint_scores", "descriptors"):
            assert out[key].dtype == ref[key].dtype
            assert torch.equal(out[key][b, :n], ref[key][0, :n]), f"image {b}: {key}"
            assert not out[key][b, n:].any(), f"image {b}: {key} rows beyond the count must be zero"
    return counts


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("name", ["aliked-n16", "aliked-n32"])
def test_canvas_of_four_equals_the_crops(name, c, mode, dtype):
    require_gpu()
    model = _model(name, mode, dtype)
    crops = _crop_results(name, mode, dtype, c, tuple(SIZES))
    for canvas_hw in CANVASES:
        counts = _check_against_crops(model, SIZES, c, canvas_hw, crops)
    assert max(counts) > 0      # the test has keypoints to compare


@pytest.mark.gpu
def test_portrait_plus_landscape():
    """more than one workgroup row and column partly outside an image"""
    require_gpu()
    sizes = ((120, 200), (200, 120))
    model = _model("aliked-n16", "threshold", "f32")
    counts = _check_against_crops(model, sizes, 3, (200, 200), _crop_results("aliked-n16", "threshold", "f32", 3, sizes))
    assert max(counts) > 0


@pytest.mark.gpu
def test_threshold_fallback_is_per_image():
    """DKD's "no pixel passes scores_th -> the image's mean score" is asked of each image of a ragged batch alone: image 1 lies entirely below 0.5 and must
    return what its own B = 1 detect returns, the mean-threshold set (under the whole-batch rule image 0's maxima would leave it empty); the 1.0 in the canvas
    padding is neither a maximum, nor part of a mean, nor a neighbour in any window."""
    require_gpu()
    from lightglue_amd import ALIKED
    model = ALIKED(weights=G.aliked_state_dict(3), detection_threshold=0.5, max_num_keypoints=-1).eval().cuda()
    sizes = [(40, 56), (32, 48)]
    maps = [torch.from_numpy(G.score_maps(1, 1, 40, 56)).cuda(), torch.from_numpy(G.score_maps(2, 1, 32, 48)).cuda() * 0.5]
    assert float(maps[0].max()) > 0.5 and float(maps[1].max()) < 0.5
    canvas = torch.full((2, 48, 64), 1.0, device="cuda")
    for b, m in enumerate(maps):
        canvas[b, : m.shape[1], : m.shape[2]] = m[0]
    got = model.detect(canvas, valid_size=[[w, h] for h, w in sizes])
    torch.cuda.synchronize()
    for b, m in enumerate(maps):
        ref = model.detect(m)
        n = int(ref[3][0])
        assert n > 0 and int(got[3][b]) == n, f"image {b}: {int(got[3][b])} keypoints, its own detect gives {n}"
        for g, r, what in zip(got[:3], ref[:3], ("keypoints", "scores", "normalised keypoints")):
            assert torch.equal(g[b, :n], r[0, :n]), f"image {b}: {what}"
            assert not g[b, n:].any()
    assert float(got[1][1].max()) < 0.5      # image 1's set is the mean-threshold one: nothing in it reaches scores_th


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["size", "input"])
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_extract_batch_equals_the_extract_loop(dtype, order):
    require_gpu()
    from lightglue_amd import collate_features
    model = _model("aliked-n16", "threshold", dtype)
    shapes = [(96, 128, 3), (128, 96, 3), (80, 80, 3), (96, 128, 1), (80, 80, 3), (128, 96, 3)]      # resize=64: 48 x 64, 64 x 48, 64 x 64
    images = [G.aliked_image(60 + i, 1, h, w, c)[0].cuda() for i, (h, w, c) in enumerate(shapes)]
    images[2] = (images[2] * 255).round().to(torch.uint8)
    store = model.extract_batch(images, batch_size=4, resize=64, order=order)
    loop = collate_features([model.extract(i, resize=64) for i in images])
    torch.cuda.synchronize()
    assert set(store) == set(loop)
    for key in loop:
        assert store[key].dtype == loop[key].dtype and store[key].shape == loop[key].shape, key
        assert torch.equal(store[key], loop[key]), key
    assert store["descriptors"].dtype == DTYPES[dtype] and int(store["num_keypoints"].max()) > 0


# ---- the uniform path is untouched: one fixture of the reference class, by the bars of tests/test_gpu_aliked.py (restated)
def _match(ref_k, got_k, tol=1e-2):
    if len(ref_k) == 0 or len(got_k) == 0:
        return np.zeros(0, int), np.zeros(0, int)
    d = np.linalg.norm(ref_k[:, None, :] - got_k[None, :, :], axis=-1)
    j = d.argmin(1)
    ok = d[np.arange(len(ref_k)), j] < tol
    return np.nonzero(ok)[0], j[ok]


@pytest.mark.gpu
def test_uniform_forward_still_matches_the_reference():
    require_gpu()
    from lightglue_amd import ALIKED
    z = np.load(GOLD / "n16_rgb_b2_64x96_top60.npz")
    meta = json.loads(str(z["meta"]))
    model = ALIKED(weights=G.aliked_state_dict(meta["wseed"], meta["model"]), model_name=meta["model"], **meta["conf"]).eval().cuda()
    seeds = meta["iseeds"]
    img = (G.aliked_image(seeds[0], meta["b"], meta["h"], meta["w"], meta["c"]) if len(seeds) == 1
           else torch.cat([G.aliked_image(s, 1, meta["h"], meta["w"], meta["c"]) for s in seeds], 0)).cuda()
    scores, _ = model.encode(img)
    out = model({"image": img})
    torch.cuda.synchronize()
    assert float(np.abs(scores.cpu().numpy() - z["scores"]).max()) <= 1e-5
    counts = out["num_keypoints"].cpu().numpy()
    kp, ks, ds = (out[k].cpu().numpy() for k in ("keypoints", "keypoint_scores", "descriptors"))
    margin = min(meta["threshold_margin"], meta["nms_tie_margin"])
    for b in range(meta["b"]):
        n_ref, n_got = int(z["counts"][b]), int(counts[b])
        rk, gk = z["keypoints"][b, :n_ref], kp[b, :n_got]
        i, j = _match(rk, gk)
        differ = max(n_ref, n_got) - len(i)
        if differ:
            assert margin < 1e-5 and differ <= 0.01 * max(n_ref, 1), f"image {b}: {differ} of {n_ref} keypoints differ"
        assert np.abs(rk[i] - gk[j]).max(initial=0) <= 1e-3, "keypoint coordinates"
        assert np.abs(z["keypoint_scores"][b, i] - ks[b, j]).max(initial=0) <= 1e-5, "keypoint scores"
        assert np.abs(z["descriptors"][b, i] - ds[b, j]).max(initial=0) <= 2e-4, "descriptors"
        assert not ds[b, n_got:].any() and not kp[b, n_got:].any(), "padding rows are zero"
