"""Ragged-batch SuperPoint extraction on the MI355X: images of DIFFERENT sizes in the top-left corners of one canvas, one call.

The bar is bit identity: for every image, everything the ragged call returns inside that image's extents — scores, the descriptor map, and rows
< num_keypoints of keypoints / scores / descriptors — equals (torch.equal) what the B = 1 call on the h x w crop returns, whatever the canvas padding
holds (NaN, 1e30).  Sizes: the canvas itself, sizes odd at every pool level, edges exactly on / one past the 8-row x 32-pixel conv tile and the 64-pixel
NMS tile, an image smaller than one NMS tile, and the single-cell minimum 8 x 8."""
from pathlib import Path

import numpy as np
import pytest
import torch

import make_golden_superpoint as G
from conftest import require_gpu

GOLD = Path(__file__).resolve().parent / "golden"
CANVAS = (96, 160)
SIZES = [(96, 160), (75, 109), (67, 91), (40, 64), (41, 65), (17, 33), (8, 8)]      # (h, w)
_cache = {}


def _images():
    """one seeded image per size (host, [1, h, w]); computed once, never modified"""
    if "images" not in _cache:
        _cache["images"] = [torch.from_numpy(G.encoder_image(20 + i, 1, h, w))[0] for i, (h, w) in enumerate(SIZES)]
    return _cache["images"]


def _canvas(images, canvas_hw, fill):
    c = torch.full((len(images), 1) + tuple(canvas_hw), fill, dtype=torch.float32)
    for i, im in enumerate(images):
        c[i, :, : im.shape[-2], : im.shape[-1]] = im
    return c.cuda(), [[im.shape[-1], im.shape[-2]] for im in images]


def _model(**conf):
    from lightglue_amd import SuperPoint
    return SuperPoint(weights=G.encoder_state_dict(0), **conf).cuda().eval()


def _crop_results(model, key):
    """forward + encode of every crop alone (the B = 1 reference), shared by the parametrisations with the same configuration"""
    if key not in _cache:
        out = []
        for im in _images():
            x = im[None].cuda()
            out.append((model({"image": x}), model.encode(x)))
        _cache[key] = out
    return _cache[key]


def _assert_rows_equal(got, b, ref):
    n = int(ref["num_keypoints"][0])
    assert int(got["num_keypoints"][b]) == n
    for k in ("keypoints", "keypoint_scores", "descriptors"):
        assert got[k].dtype == ref[k].dtype
        assert torch.equal(got[k][b, :n], ref[k][0, :n]), (k, b)
        assert not got[k][b, n:].any(), (k, b)                      # rows >= count are zero
    return n


@pytest.mark.gpu
@pytest.mark.parametrize("fill", [float("nan"), 1e30])
@pytest.mark.parametrize("topk", [None, 50])
@pytest.mark.parametrize("conv_precision", ["fp32", "f16x3"])
def test_ragged_forward_is_bit_identical_to_the_crops(conv_precision, topk, fill):
    require_gpu()
    model = _model(conv_precision=conv_precision, max_num_keypoints=topk)
    canvas, sizes = _canvas(_images(), CANVAS, fill)
    got = model({"image": canvas, "valid_size": torch.tensor(sizes)})
    scores, dense = model.encode(canvas, valid_size=sizes)
    refs = _crop_results(model, (conv_precision, topk))
    counts = []
    for b, ((h, w), (ref, (rs, rd))) in enumerate(zip(SIZES, refs)):
        hs, ws = h // 8 * 8, w // 8 * 8
        assert torch.equal(scores[b, :hs, :ws], rs[0]), b
        assert torch.equal(dense[b, :, : h // 8, : w // 8], rd[0]), b
        outside = scores[b].clone()
        outside[:hs, :ws] = 0
        assert not outside.any(), b                                 # the score canvas is defined everywhere: 0 outside the image
        counts.append(_assert_rows_equal(got, b, ref))
    assert counts[-1] == 0 and max(counts) > 0                      # 8 x 8 at remove_borders = 4: no keypoint
    if topk is not None:
        assert max(counts) == topk and 0 < sorted(counts)[1] < topk  # the limit binds for some images and not for others
    again = model({"image": canvas, "valid_size": sizes})
    assert all(torch.equal(got[k], again[k]) for k in got)          # deterministic


@pytest.mark.gpu
def test_ragged_forward_float16_descriptors():
    require_gpu()
    model = _model(max_num_keypoints=50, descriptor_dtype=torch.float16)
    canvas, sizes = _canvas(_images(), CANVAS, float("nan"))
    got = model({"image": canvas, "valid_size": sizes})
    assert got["descriptors"].dtype == torch.float16
    for b, (ref, _) in enumerate(_crop_results(model, "f16")):
        _assert_rows_equal(got, b, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("topk", [None, 50])
@pytest.mark.parametrize("remove_borders", [0, 4])
def test_ragged_detection_on_crafted_ties(remove_borders, topk):
    """The detection stage alone on plateaus and exact ties, the outside filled with 1.0 (above every score): a zero- or anything-filled outside that took
    part in the NMS would produce maxima of its own and suppress real ones next to the far border, and with remove_borders = 0 would leak keypoints."""
    require_gpu()
    from lightglue_amd.superpoint_head import detect_keypoints
    maps = [torch.from_numpy(G.score_map(3, 1, 67, 91))[0], torch.from_numpy(G.score_map(4, 1, 64, 64))[0]]
    canvas = torch.full((2, 80, 128), 1.0)
    for i, m in enumerate(maps):
        canvas[i, : m.shape[0], : m.shape[1]] = m
    sizes = [[m.shape[1], m.shape[0]] for m in maps]
    kp, sc, cnt = detect_keypoints(canvas.cuda(), 4, remove_borders, 0.0005, topk, sizes=sizes)
    for b, m in enumerate(maps):
        rkp, rsc, rcnt = detect_keypoints(m[None].cuda(), 4, remove_borders, 0.0005, topk)
        n = int(rcnt[0])
        assert n > 0 and int(cnt[b]) == n
        assert torch.equal(kp[b, :n], rkp[0, :n]) and torch.equal(sc[b, :n], rsc[0, :n])


@pytest.mark.gpu
@pytest.mark.parametrize("resize,as_uint8", [(None, False), (64, False), (None, True), (64, True)])
def test_extract_batch_equals_the_extract_loop(resize, as_uint8):
    require_gpu()
    import gpu_util
    from lightglue_amd import collate_features
    from lightglue_amd import synthetic as synth
    model = _model(max_num_keypoints=64)
    images = [im.cuda() for im in _images()[:6]]
    if as_uint8:
        images = [(im.clamp(0, 1) * 255).round().to(torch.uint8) for im in images]
    images[1] = images[1][None]                                    # [1, C, H, W] is accepted like [C, H, W]
    conf = {} if resize is None else {"resize": resize}
    want = collate_features([model.extract(im, **conf) for im in images])
    got = model.extract_batch(images, batch_size=4, **conf)
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert torch.equal(got[k], want[k]), k
    assert got["image_size"].tolist() == [[float(w), float(h)] for h, w in SIZES[:6]]
    if not as_uint8:
        matcher = gpu_util.make_model(synth.make_state_dict(0, recipe="A"), "f16x3", depth_confidence=-1, width_confidence=-1)
        res = matcher.match_pairs(got, [[0, 1], [2, 3]])
        assert res["matches0"].shape == (2, got["keypoints"].shape[1])


@pytest.mark.gpu
@pytest.mark.parametrize("conv_precision", ["fp32", "f16x3"])
def test_ragged_row_meets_the_reference_fixture(conv_precision):
    """The criteria of test_full_extractor_matches_reference, on the fixture's 75 x 109 image placed in a 120 x 160 canvas next to a 120 x 160 image."""
    require_gpu()
    from lightglue_amd import SuperPoint
    z = np.load(GOLD / "superpoint_full_b1_75x109_top40.npz")
    wseed, iseed, b, h, w, topk = (int(v) for v in z["case"])
    assert (b, h, w, topk) == (1, 75, 109, 40)
    model = SuperPoint(weights=G.encoder_state_dict(wseed), max_num_keypoints=topk, conv_precision=conv_precision).cuda().eval()
    images = [torch.from_numpy(G.encoder_image(iseed, 1, h, w))[0], torch.from_numpy(G.encoder_image(10, 1, 120, 160))[0]]
    canvas, sizes = _canvas(images, (120, 160), float("nan"))
    out = model({"image": canvas, "valid_size": sizes})
    kp, sc, desc, cnt = (out[k].cpu().numpy() for k in ("keypoints", "keypoint_scores", "descriptors", "num_keypoints"))
    ref_kp, ref_sc, ref_desc = z["keypoints"][0], z["keypoint_scores"][0], z["descriptors"][0]
    n = int(cnt[0])
    got = {(int(x), int(y)): i for i, (x, y) in enumerate(kp[0, :n])}
    ref = {(int(x), int(y)): i for i, (x, y) in enumerate(ref_kp)}
    common = sorted(set(got) & set(ref))
    assert len(common) >= 0.99 * len(ref) and abs(n - len(ref)) <= max(1, len(ref) // 100), (n, len(ref), len(common))
    gi = np.array([got[c] for c in common]); ri = np.array([ref[c] for c in common])
    np.testing.assert_allclose(sc[0][gi], ref_sc[ri], atol=2e-6, rtol=2e-5)
    np.testing.assert_allclose(desc[0][gi], ref_desc[ri], atol=2e-5, rtol=0)


@pytest.mark.gpu
def test_uniform_path_equals_ragged_with_full_sizes():
    require_gpu()
    model = _model(max_num_keypoints=50)
    img = torch.from_numpy(G.encoder_image(11, 2, 64, 96)).cuda()
    uniform = model({"image": img})
    ragged = model({"image": img, "valid_size": [[96, 64], [96, 64]]})
    assert sorted(uniform) == sorted(ragged)
    for k in uniform:
        assert torch.equal(uniform[k], ragged[k]), k
    su, du = model.encode(img)
    sr, dr = model.encode(img, valid_size=[[96, 64], [96, 64]])
    assert torch.equal(su, sr) and torch.equal(du, dr)
