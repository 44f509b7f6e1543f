"""The ALIKED encoder (`ALIKED.encode`: ak_conv_first_kernel, ak_pool_kernel, ak_deform_gather_kernel, ak_score_head0_kernel, the three
ak_small_conv_kernel instances, fold_kernel's BatchNorm fold and every launch_conv form ALIKED uses) against `aliked_oracle.encoder` (float64,
BatchNorm applied as written; pinned to the reference's own module in test_aliked_oracle_cpu.py).  The four level maps x1 .. x4, read through
`ALIKED.level_maps` over their whole padded extent, and the score map are compared per quantity; end to end (test_gpu_aliked.py) only the score
map is, at 1e-5, behind a projection that averages the deep levels away.

Cases: the table `ENC_STAGES` of tools/make_golden_aliked.py (noise images, so the replicate-padding seam and the pooling phase show; odd pads;
B = 2; gray; 1 x 1, 1 x 2, 2 x 2, 2 x 10 and 3 x 3 fourth levels; a second, partial conv tile at the 1/8 level), each at offset gain 1 (fractional
offsets) and 4 (most offsets on the +-max(h, w) / 4 clamp, samples inside, across the border of and outside the map: counted from the oracle's own
offsets in test_aliked_oracle_cpu.py), one of them with BatchNorm variances of 1e-6 .. 1e-3, where the fold's epsilon decides the result.

Bar: 4 x aliked_oracle.T_REF of the quantity (the reference's own fp32 distance from the float64 oracle; x 2 because the kernels sum in another
order than torch's CPU kernels, x 2 for expf / division implementations; it also has to hold the rounding of the folded weights).  x1 depends on
block1 alone, x2 on blocks 1 - 2, and so on: the first level that fails names the block.

Worst |kernel - oracle| / bar of the first run on an MI355X, the larger of the two gains (every test prints its own figures):

    case                                  x1     x2     x3     x4   scores
    enc_8x8_b1_rgb_noise_g1              0.18   0.27   0.15   0.13   0.01
    enc_8x8_b1_rgb_noise_g4_smallvar     0.14   0.26   0.18   0.13   0.00
    enc_24x17_b2_rgb_noise_g4            0.32   0.27   0.13   0.12   0.00
    enc_31x33_b1_gray_noise_g1           0.16   0.21   0.15   0.24   0.01
    enc_40x56_b1_rgb_image_g4            0.17   0.23   0.27   0.20   0.03
    enc_40x300_b1_rgb_noise_g4           0.30   0.23   0.18   0.33   0.11
    enc_72x90_b1_rgb_noise_g1            0.25   0.26   0.28   0.37   0.04
    ragged canvas, image 0 (24 x 17)     0.26   0.28   0.15   0.15   0.00
    ragged canvas, image 1 (31 x 33)     0.25   0.21   0.14   0.17   0.00

The kernels sit at or below the reference's own fp32 distance from the oracle (a ratio of 0.25 is 1 x T_REF).  With `1e-5f` replaced by `0.f` in
fold_kernel the small-variance case is off by 3e5 .. 7e5 bars at every level and every other case by 4 .. 7 bars.
"""
import functools

import numpy as np
import pytest
import torch

import make_golden_aliked as G
from conftest import require_gpu
from oracle import aliked_oracle as AO

QUANTITIES = ("x1", "x2", "x3", "x4", "encoder_scores")
BAR = {q: 4 * AO.T_REF[q] for q in QUANTITIES}
SHIFTS = (0, 1, 3, 5)
CASES = [(name, gain) for name in sorted(G.ENC_STAGES) for gain in (1.0, 4.0)]


@functools.lru_cache(maxsize=None)
def model_and_weights(name, gain):
    """one ALIKED per (case, offset gain), shared by the tests (weights are never modified), and its weights for the oracle"""
    from lightglue_amd import ALIKED
    sd, _ = G.encoder_inputs(name, gain)
    return ALIKED(weights=sd, model_name="aliked-n16").eval().cuda(), {k: v.numpy() for k, v in sd.items()}


def image_of(name):
    return G.encoder_inputs(name)[1]


@functools.lru_cache(maxsize=None)
def oracle(name, gain):
    """(levels, scores) of the float64 oracle on the case's float32 inputs; computed once, shared, never modified"""
    return AO.encoder(image_of(name).numpy(), model_and_weights(name, gain)[1])


def encode(model, image, valid_size=None):
    """(level maps x1 .. x4 [B, Hp >> s, Wp >> s, 32], scores [B, H, W]) as numpy arrays"""
    image = image.cuda()
    scores, levels = model.encode(image, valid_size=valid_size)
    maps = [m.cpu().numpy() for m in model.level_maps(levels, (image.shape[0],) + tuple(image.shape[-2:]))]
    torch.cuda.synchronize()
    return maps, scores.cpu().numpy()


def compare(what, got_levels, got_scores, ref_levels, ref_scores):
    """every level map over the extent of the oracle's, and the scores, finite and within 4 x T_REF; prints worst / bar per quantity"""
    worst = {}
    for q, got, ref in zip(QUANTITIES, [*got_levels, got_scores], [*ref_levels, ref_scores]):
        assert got.shape == ref.shape, (q, got.shape, ref.shape)
        assert np.isfinite(got).all(), f"{what}: {q} is not finite"
        worst[q] = float(np.abs(got - ref).max())
    print(f"{what}: " + "  ".join(f"{q} {worst[q]:.2e} / {BAR[q]:.2e} = {worst[q] / BAR[q]:.2f}" for q in QUANTITIES))
    for q in QUANTITIES:          # in the encoder's order: the first failure names the block
        assert worst[q] <= BAR[q], f"{what}: {q} off by {worst[q]:.2e}, bar {BAR[q]:.2e}"


@pytest.mark.gpu
@pytest.mark.parametrize("name,gain", CASES)
def test_level_maps_and_scores_match_the_oracle(name, gain):
    require_gpu()
    model, _ = model_and_weights(name, gain)
    levels, scores = encode(model, image_of(name))
    ref_levels, ref_scores = oracle(name, gain)
    compare(f"{name} gain {gain:g}", levels, scores, ref_levels, ref_scores)


def assert_same_bits(a, b, what):
    for q, x, y in zip(QUANTITIES, [*a[0], a[1]], [*b[0], b[1]]):
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), f"{what}: {q} differs"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["enc_8x8_b1_rgb_noise_g1", "enc_40x56_b1_rgb_image_g4"])
def test_both_halves_of_a_doubled_batch_equal_the_single_call(name):
    """[img, img] at B = 2: every buffer's batch stride.  Both halves of every level map and of the scores equal the B = 1 call bit for bit."""
    require_gpu()
    model, _ = model_and_weights(name, 4.0)
    img = image_of(name)
    one = encode(model, img)
    two = encode(model, torch.cat([img, img], 0))
    for half in (0, 1):
        assert_same_bits(([m[half:half + 1] for m in two[0]], two[1][half:half + 1]), one, f"half {half}")


@pytest.mark.gpu
def test_repeated_call_and_stale_workspace_give_the_same_bits():
    """the same call twice, and once more after the encode of a larger image has left other values in the freed workspace and level buffers"""
    require_gpu()
    name = "enc_24x17_b2_rgb_noise_g4"
    model, _ = model_and_weights(name, 4.0)
    first = encode(model, image_of(name))
    assert_same_bits(encode(model, image_of(name)), first, "second call")
    big = encode(model, image_of("enc_40x300_b1_rgb_noise_g4"))
    assert np.isfinite(big[1]).all()
    assert_same_bits(encode(model, image_of(name)), first, "after a larger image")


@pytest.mark.gpu
def test_gray_equals_its_three_channel_broadcast_at_the_level_maps():
    require_gpu()
    name = "enc_31x33_b1_gray_noise_g1"
    model, _ = model_and_weights(name, 1.0)
    gray = image_of(name)
    assert gray.shape[1] == 1
    assert_same_bits(encode(model, gray), encode(model, gray.expand(-1, 3, -1, -1).contiguous()), "gray against rgb")


@pytest.mark.gpu
@pytest.mark.parametrize("gain", [1.0, 4.0])
def test_ragged_canvas_matches_the_oracle_per_image(gain):
    """24 x 17 and 31 x 33 noise images in the corners of a 40 x 48 canvas (pads to 64 x 64) whose padding is NaN, against the oracle run on each
    image alone: inside every image's padded level extents the maps meet the same bar, and so do its scores.  test_gpu_aliked_ragged.py pins the
    ragged call to the uniform one bit for bit; this pins it to an independent definition, the per-image clamp max(h_b', w_b') / 4 included: on the
    1/8 level it is 1 px for image 0 (4 x 4) where the canvas (8 x 8) and image 1 (4 x 8) give 2."""
    require_gpu()
    model, weights = model_and_weights("enc_24x17_b2_rgb_noise_g4", gain)
    images = [G.noise_image(11, 1, 24, 17, 3), G.noise_image(12, 1, 31, 33, 3)]
    canvas = torch.full((2, 3, 40, 48), float("nan"))
    for b, img in enumerate(images):
        canvas[b, :, : img.shape[-2], : img.shape[-1]] = img[0]
    levels, scores = encode(model, canvas, valid_size=[[img.shape[-1], img.shape[-2]] for img in images])
    for b, img in enumerate(images):
        h, w = img.shape[-2:]
        hp, wp, _, _ = AO.padded_dims(h, w)
        ref_levels, ref_scores = AO.encoder(img.numpy(), weights)
        compare(f"ragged gain {gain:g} image {b} ({h} x {w})", [m[b:b + 1, : hp >> s, : wp >> s] for m, s in zip(levels, SHIFTS)], scores[b:b + 1, :h, :w],
                ref_levels, ref_scores)
        outside = scores[b].copy()
        outside[:h, :w] = 0
        assert not outside.any(), "scores outside the image are 0"
