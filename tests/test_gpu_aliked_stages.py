"""SDDH (`ALIKED.describe`: ak_patch_kernel, the offset GEMM, ak_offsets_kernel, ak_sample_kernel, the sf / agg GEMMs, ak_desc_norm_kernel) on
CRAFTED level maps written through `ALIKED.level_maps`, against `aliked_oracle.sddh` (float64; pinned to the reference's own SDDH module in
test_aliked_oracle_cpu.py).  End to end (test_gpu_aliked.py) these pieces hide behind a smooth encoder output and a 2e-4 bar; here the level maps
are independent noise, the keypoints sit on corners, edges and pixel centres, and the bar is 4 x T_ref.

Bar: descriptors within 4 x aliked_oracle.T_REF["descriptors"] (the reference's own fp32 distance from the float64 oracle; x 2 because the
kernels sum in another order than torch's CPU kernels, x 2 for expf / division implementations).  Zero rows are exactly zero."""
import numpy as np
import pytest
import torch

import make_golden_aliked as G
from conftest import require_gpu
from oracle import aliked_oracle as AO

TOL = 4 * AO.T_REF["descriptors"]
MODELS = {"aliked-n16": 20, "aliked-n32": 21}     # model -> weight seed (those of the stage fixtures)
_models = {}


def model_and_weights(name, gain):
    """one ALIKED per (model, offset gain), shared by the tests (weights are never modified)"""
    if (name, gain) not in _models:
        from lightglue_amd import ALIKED
        sd = G.scaled_offset_weights(G.aliked_state_dict(MODELS[name], name), gain)
        head = {k: v.numpy() for k, v in sd.items() if k.startswith("desc_head.")}
        _models[(name, gain)] = (ALIKED(weights=sd, model_name=name).eval().cuda(), head)
    return _models[(name, gain)]


def describe(model, levels, shape, knorm, counts):
    """write the crafted levels through level_maps, run describe"""
    from lightglue_amd import _cabi
    buf = torch.zeros(_cabi.load().lg_aliked_levels_bytes(*shape), dtype=torch.uint8, device="cuda")
    for view, lvl in zip(model.level_maps(buf, shape), levels):
        view.copy_(torch.from_numpy(lvl))
    out = model.describe(buf, shape, torch.from_numpy(knorm).cuda(), torch.tensor(counts, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def check(name, gain, levels, shape, knorm, counts):
    model, head = model_and_weights(name, gain)
    b, h, w = shape
    got = describe(model, levels, shape, knorm, counts)
    ref = AO.sddh(levels, (h, w), [knorm[i, :counts[i]] for i in range(b)], head, model.n_pos)
    assert got.shape == (b, knorm.shape[1], 128) and np.isfinite(got).all()
    for i in range(b):
        err = float(np.abs(got[i, :counts[i]] - ref[i]).max(initial=0))
        print(f"{name} gain {gain} image {i}: {counts[i]} rows, descriptors off by {err:.2e} (bar {TOL:.2e})")
        assert err <= TOL, f"image {i}: descriptors off by {err:.2e}"
        assert not got[i, counts[i]:].any(), "rows at and beyond counts[b] are zero"
    return got, ref


CASES = [(m, g) for m in MODELS for g in (1.0, G.OFFSET_GAIN)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,gain", CASES)
def test_describe_ragged_batch_with_live_pad_rows(name, gain):
    """40 x 56 (pads to 64 x 64 with offsets 12 / 4, a 2 x 2 fourth level), B = 2, N = 33, counts [33, 5].  66 rows: describe_layout rounds them
    to 96, so the GEMM PAD ROWS are live (zeroed patch / feat rows that must stay finite and must not leak into row 65).  Keypoints: the four
    corners, where the PATCH-CORNER CLAMP to [0, W - 4] x [0, H - 4] acts, edge midpoints, exact pixel centres, random ones.  gain 1: fractional
    offsets inside the map.  gain 40: offset_conv.2 scaled so that about 70 % of the offsets sit on the OFFSET CLAMP +-max(h, w) / 4 = 14 px
    and many sample positions leave the map (zero samples, partly-outside bilinear cells)."""
    require_gpu()
    shape = (2, 40, 56)
    levels = G.crafted_levels(1, *shape)
    knorm = G.stage_knorm(1, 2, 33, 40, 56)
    got, ref = check(name, gain, levels, shape, knorm, [33, 5])
    assert np.abs(np.linalg.norm(ref[0], axis=1) - 1).max() < 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize("name,gain", CASES)
def test_describe_all_zero_levels_image(name, gain):
    """B = 2, N = 33, image 1 with all-zero level maps: x1234 / max(||x1234||, 1e-12) and the final max(||d||, 1e-12) must give exact zeros,
    not NaN, and must not disturb image 0."""
    require_gpu()
    shape = (2, 40, 56)
    levels = [l.copy() for l in G.crafted_levels(1, *shape)]
    for l in levels:
        l[1] = 0
    got, _ = check(name, gain, levels, shape, G.stage_knorm(1, 2, 33, 40, 56), [33, 33])
    assert not got[1].any() and np.isfinite(got).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name,gain", CASES)
def test_describe_one_keypoint_per_image(name, gain):
    """B = 3, N = 1: three rows padded to 32; row -> image is `row / N` with N = 1, each image samples ITS OWN level maps."""
    require_gpu()
    shape = (3, 40, 56)
    k = G.stage_knorm(2, 3, 33, 40, 56)
    knorm = np.stack([k[0, 3], k[1, 20], k[2, 5]])[:, None, :]   # a corner, a random position, an edge midpoint
    got, _ = check(name, gain, G.crafted_levels(2, *shape), shape, knorm, [1, 1, 1])
    assert len({got[i, 0].tobytes() for i in range(3)}) == 3


@pytest.mark.gpu
@pytest.mark.parametrize("name,gain", CASES)
def test_describe_8x8_one_by_one_fourth_level(name, gain):
    """8 x 8 (the ABI's minimum; pads to 32 x 32 with offsets 12 / 12): a 1 x 1 FOURTH LEVEL (up_coord with in = 1: both taps the same pixel),
    the patch-corner clamp at W - 4 = 4 for every keypoint right of pixel 5, offset clamp at 2 px."""
    require_gpu()
    shape = (1, 8, 8)
    knorm = G.stage_knorm(3, 1, 20, 8, 8)
    check(name, gain, G.crafted_levels(3, *shape), shape, knorm, [20])
    _, corner = AO.keypoint_pixels(knorm[0], 8, 8)
    assert (corner.max(0) == 4).all() and (corner.min(0) == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(MODELS))
def test_encoder_levels_through_level_maps_reproduce_forward(name):
    """The loop between the helper and the real path: the encoder's level maps, READ through level_maps and written into a fresh buffer, fed back
    into describe with the knorm detect returned, give forward's descriptors bit for bit."""
    require_gpu()
    from lightglue_amd import _cabi
    model, _ = model_and_weights(name, 1.0)
    img = G.aliked_image(12, 2, 40, 56, 3).cuda()
    shape = (2, 40, 56)
    out = model({"image": img})
    scores, levels = model.encode(img)
    kpts, ks, knorm, counts = model.detect(scores)
    nmax = int(counts.max())
    assert nmax > 0 and torch.equal(counts, out["num_keypoints"])
    views = model.level_maps(levels, shape)
    assert [tuple(v.shape) for v in views] == [(2, 64, 64, 32), (2, 32, 32, 32), (2, 8, 8, 32), (2, 2, 2, 32)]
    assert all(bool(torch.isfinite(v).all()) and bool(v.any()) for v in views)
    fresh = torch.zeros(_cabi.load().lg_aliked_levels_bytes(*shape), dtype=torch.uint8, device="cuda")
    for dst, src in zip(model.level_maps(fresh, shape), views):
        dst.copy_(src)
    again = model.describe(fresh, shape, knorm[:, :nmax].contiguous(), counts)
    torch.cuda.synchronize()
    assert torch.equal(again, out["descriptors"])
    ref = AO.sddh([v.cpu().numpy() for v in views], (40, 56), [knorm[i, :int(counts[i])].cpu().numpy() for i in range(2)],
                  {k: v.numpy() for k, v in G.aliked_state_dict(MODELS[name], name).items() if k.startswith("desc_head.")}, model.n_pos)
    for i in range(2):
        assert np.abs(again[i, :int(counts[i])].cpu().numpy() - ref[i]).max(initial=0) <= TOL
