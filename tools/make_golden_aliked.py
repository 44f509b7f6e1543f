#!/usr/bin/env python3
"""Generate tests/golden/aliked/*.npz with the reference's OWN ALIKED class (lightglue/aliked.py), executed unmodified on CPU.

aliked.py imports torchvision (deform_conv2d, resnet.conv1x1 / conv3x3), kornia (grayscale_to_rgb) and the package's utils (cv2),
none of which exist here, so the module is executed standalone with stand-ins for those imports:
  * lgref.utils.Extractor: the conf merge of utils.py:131-135;
  * kornia.color.grayscale_to_rgb: the 1 -> 3 channel broadcast;
  * torchvision.models.resnet.conv1x1 / conv3x3: the standard bias-free definitions;
  * torch.hub.load_state_dict_from_url: returns the seeded state dict, so the reference's own strict=True load checks every name;
  * torchvision.ops.deform_conv2d: `deform_conv2d` below, a plain-torch restatement of torchvision's CPU kernel (bilinear sampling with
    its bounds rules, offsets (dy, dx) per tap in channels (2k, 2k + 1)).  This is the ONLY non-reference arithmetic in the fixtures;
    tests/test_aliked_cpu.py checks it against F.conv2d at zero offset and against a grid_sample construction at other offsets.
The fixtures store the unpadded score map and the outputs; weights and images are regenerated from seeds by `aliked_state_dict` /
`aliked_image`, which never touch the reference (the GPU tests import them).

`--stages` writes tests/golden/aliked_stages/*.npz instead: the reference's own DKD and SDDH modules on the seeded crafted inputs of the
"stage inputs" section below (score maps, level maps, keypoints; plain functions that never touch the reference either).  Those fixtures hold
the reference's outputs and the case parameters only; they pin oracle/aliked_oracle.py (tests/test_aliked_oracle_cpu.py), which the GPU stage
tests then compare the kernels with.  The encoder fixtures (`ENC_STAGES`) come from the reference's whole ALIKED module on seeded images
(`noise_image` / `aliked_image`) and seeded weights (`scaled_encoder_offsets`, `small_variance`): forward hooks on conv1 .. conv4 record the
gated level maps x1 .. x4, stored with the unpadded score map.
    python tools/make_golden_aliked.py [NAME ...] # whole-model fixtures (all, or the named cases)
    python tools/make_golden_aliked.py --stages   # stage fixtures
"""
from __future__ import annotations

import json
import math
import sys
import types
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parent.parent
REF = Path("/root/reference/lightglue/aliked.py")
GOLD = ROOT / "tests" / "golden" / "aliked"
SCORE_GAIN = 2.5   # score_head.6 weight scale of the seeded networks: sigmoid scores spread over ~(0.01, 0.9), no ties at 1.0

# (weight seed, image seed) of the small-image cases
SEED_8X8, SEED_8X8_ZERO, SEED_31X33, SEED_40X300 = (10, 10), (9, 9), (52, 52), (65, 65)

# name -> (model, weight seed, image seed, B, C, H, W, conf)
CASES = {
    "n16_rgb_b1_120x160_th": ("aliked-n16", 0, 0, 1, 3, 120, 160, {"detection_threshold": 0.5}),
    "n32_gray_b1_75x109_limit40": ("aliked-n32", 1, 1, 1, 1, 75, 109, {"detection_threshold": 0.3, "max_num_keypoints": 40}),
    "n16_rgb_b2_64x96_top60": ("aliked-n16", 2, 2, 2, 3, 64, 96, {"detection_threshold": -1, "max_num_keypoints": 60}),
    "n16_gray_b1_96x128_fallback": ("aliked-n16", 3, 3, 1, 1, 96, 128, {"detection_threshold": 0.9999}),
    "n32_rgb_b1_240x320_limit300": ("aliked-n32", 4, 4, 1, 3, 240, 320, {"detection_threshold": 0.3, "max_num_keypoints": 300}),
    "n16_rgb_b1_96x128_r6": ("aliked-n16", 8, 8, 1, 3, 96, 128, {"detection_threshold": 0.3, "nms_radius": 6}),
    # images that pad to ONE 32-pixel tile row / column (a 1 x 1, 1 x 2, 2 x 10 fourth level); seeds chosen for margins >= 1e-4
    "n16_rgb_b1_8x8_min": ("aliked-n16", SEED_8X8[0], SEED_8X8[1], 1, 3, 8, 8, {"detection_threshold": 0.2}),
    "n16_rgb_b1_8x8_zero": ("aliked-n16", SEED_8X8_ZERO[0], SEED_8X8_ZERO[1], 1, 3, 8, 8, {"detection_threshold": 0.2}),   # no keypoint: forward with nmax == 0
    "n16_gray_b2_31x33_top20": ("aliked-n16", SEED_31X33[0], SEED_31X33[1], 2, 1, 31, 33, {"detection_threshold": -1, "max_num_keypoints": 20}),
    "n32_rgb_b1_40x300_th": ("aliked-n32", SEED_40X300[0], SEED_40X300[1], 1, 3, 40, 300, {"detection_threshold": 0.2}),
}
# ragged pair: two images of one size, each run by the reference on its own (its torch.stack needs equal counts), batched on the GPU
RAGGED = {"n16_rgb_ragged_2x80x104": ("aliked-n16", 5, (6, 7), 3, 80, 104, {"detection_threshold": 0.45})}


# ---------------------------------------------------------------------------------------------------- seeded inputs
def aliked_state_dict(seed: int, model: str = "aliked-n16") -> dict:
    """Seeded weights with the module tree of the reference: LeCun-normal convs (SELU network), randomised BatchNorm statistics,
    small offset convs (fractional, partly out-of-range deformable offsets), agg_weights as torch.rand, score_head.6 scaled by SCORE_GAIN."""
    from lightglue_amd.aliked import ALIKED
    g = torch.Generator().manual_seed(1000 + seed)
    out = {}
    for name, t in ALIKED(model_name=model).state_dict().items():
        shape = t.shape
        if name.endswith("num_batches_tracked"):
            v = torch.zeros((), dtype=torch.long)
        elif name.endswith("running_mean"):
            v = torch.randn(shape, generator=g) * 0.1
        elif name.endswith("running_var"):
            v = torch.rand(shape, generator=g) + 0.5
        elif ".bn" in name and name.endswith("weight"):
            v = torch.rand(shape, generator=g) * 0.8 + 0.6
        elif name.endswith("agg_weights"):
            v = torch.rand(shape, generator=g)
        elif name.endswith("bias"):
            v = torch.randn(shape, generator=g) * (0.8 if "offset_conv" in name else 0.1)
        else:
            fan_in = int(np.prod(shape[1:]))
            v = torch.randn(shape, generator=g) / math.sqrt(fan_in)
            if "offset_conv" in name:
                v = v * 0.5
            if name == "score_head.6.weight":
                v = v * SCORE_GAIN
        out[name] = v.to(t.dtype)
    return out


def aliked_image(seed: int, b: int, h: int, w: int, c: int = 3) -> torch.Tensor:
    """[b, c, h, w] in [0, 1]: smooth random texture plus sharp blobs and edges (keypoint-like structure)."""
    rng = np.random.Generator(np.random.PCG64(77 + seed))
    img = np.zeros((b, c, h, w), np.float32)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    for i in range(b):
        low = rng.random((c, h // 8 + 2, w // 8 + 2)).astype(np.float32)
        t = F.interpolate(torch.from_numpy(low)[None], size=(h, w), mode="bilinear", align_corners=False)[0].numpy()
        for _ in range(25):
            cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(1.5, 6.0)
            t += (rng.uniform(-0.8, 0.8, (c, 1, 1)) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * r * r))).astype(np.float32)
        t += 0.15 * rng.standard_normal((c, h, w)).astype(np.float32)
        img[i] = np.clip(t, 0.0, 1.0)
    return torch.from_numpy(img)


# ---------------------------------------------------------------------------------------------------- stage inputs
def score_maps(seed: int, b: int, h: int, w: int) -> np.ndarray:
    """[b, h, w] fp32, independent uniform(0.05, 0.95) pixels: about one NMS maximum per (2r+1)^2 pixels, all above ALIKED's 0.2 rarely tied"""
    rng = np.random.Generator(np.random.PCG64(500 + seed))
    return rng.uniform(0.05, 0.95, (b, h, w)).astype(np.float32)


def quantised_maps(seed: int, b: int, h: int, w: int) -> np.ndarray:
    """score_maps rounded to 1/16: a dozen distinct values, so NMS plateaus and large tie groups at every cut"""
    return (np.round(score_maps(seed, b, h, w) * 16) / 16).astype(np.float32)


def plateau_maps(h: int = 48, w: int = 80) -> np.ndarray:
    """[3, h, w]: constant 0.5 (every pixel an NMS maximum, all tied); 0.75 in the top half, 0.5 below; 0.75 in the top quarter, 0.5 below"""
    m = np.full((3, h, w), 0.5, np.float32)
    m[1, : h // 2] = 0.75
    m[2, : h // 4] = 0.75
    return m


def ulp_ladder_map(seed: int, h: int, w: int, r: int):
    """([1, h, w] map, number of peaks): isolated peaks every 2r + 1 pixels from (r, r) on a 0.01 background, valued by the consecutive fp32 bit
    patterns 0x3F000001, 0x3F000002, ... (fewer than 256: they agree in their top 24 bits) in shuffled order"""
    m = np.full((1, h, w), 0.01, np.float32)
    ys, xs = np.arange(r, h - r, 2 * r + 1), np.arange(r, w - r, 2 * r + 1)
    n = len(ys) * len(xs)
    assert n < 256
    bits = (np.uint32(0x3F000001) + np.random.Generator(np.random.PCG64(600 + seed)).permutation(n).astype(np.uint32)).astype(np.uint32)
    m[0][np.ix_(ys, xs)] = bits.view(np.float32).reshape(len(ys), len(xs))
    return m, n


def padded_dims(h: int, w: int):
    """InputPadder(divis_by=32): (Hp, Wp, top, left)"""
    ph, pw = ((h // 32 + 1) * 32 - h) % 32, ((w // 32 + 1) * 32 - w) % 32
    return h + ph, w + pw, ph // 2, pw // 2


def crafted_levels(seed: int, b: int, h: int, w: int) -> list:
    """the four level maps x1 .. x4 of an h x w image, [b, Hp >> s, Wp >> s, 32] fp32 for s = 0, 1, 3, 5: independent normal values (the
    sharpest dense map the upsampling can produce), each level at its own scale"""
    rng = np.random.Generator(np.random.PCG64(700 + seed))
    hp, wp, _, _ = padded_dims(h, w)
    return [(rng.standard_normal((b, hp >> s, wp >> s, 32)) * g).astype(np.float32) for s, g in ((0, 1.0), (1, 0.7), (3, 1.3), (5, 0.9))]


def crafted_knorm(seed: int, n: int, h: int, w: int) -> np.ndarray:
    """[n, 2] fp32 normalised keypoints (x, y): the four corners, the four edge midpoints, then exact pixel centres (every third one, from
    both ends), then random positions at least 1e-3 px away from an integer pixel coordinate (the .long() of SDDH is discontinuous there, and
    no test should hang on which side a round-off falls)."""
    rng = np.random.Generator(np.random.PCG64(800 + seed))
    pts = [(-1, -1), (1, -1), (-1, 1), (1, 1), (0, -1), (0, 1), (-1, 0), (1, 0)]
    wm1, hm1 = np.float32(w - 1), np.float32(h - 1)
    for i in range(6):
        x, y = (3 * i + 1) % w, (h - 2 - 3 * i) % h
        pts.append((np.float32(x) / wm1 * np.float32(2) - np.float32(1), np.float32(y) / hm1 * np.float32(2) - np.float32(1)))
    while len(pts) < n:
        p = rng.uniform(0, 1, 2) * (w - 1, h - 1)
        k = (p / (w - 1, h - 1) * 2 - 1).astype(np.float32)
        back = (k / np.float32(2) + np.float32(0.5)) * np.array([wm1, hm1])
        if (np.abs(back - np.round(back)) >= 1e-3).all():
            pts.append((k[0], k[1]))
    return np.array(pts[:n], np.float32)


def scaled_offset_weights(sd: dict, gain: float) -> dict:
    """`sd` with desc_head.offset_conv.2 (weight and bias) times `gain`: the sample offsets grow until most hit SDDH's +-max(h, w) / 4 clamp
    and many sample positions leave the map"""
    out = dict(sd)
    for k in ("desc_head.offset_conv.2.weight", "desc_head.offset_conv.2.bias"):
        out[k] = sd[k] * gain
    return out


def noise_image(seed: int, b: int, h: int, w: int, c: int = 3) -> torch.Tensor:
    """[b, c, h, w] fp32, independent uniform(0, 1) pixels: every pixel differs from its neighbours, so the replicate-padding seam and the phase of
    the pooling windows show in the first level (on the smooth `aliked_image` they barely do)"""
    rng = np.random.Generator(np.random.PCG64(900 + seed))
    return torch.from_numpy(rng.uniform(0.0, 1.0, (b, c, h, w)).astype(np.float32))


ENCODER_OFFSET_CONVS = tuple(f"block{b}.conv{c}.offset_conv" for b in (3, 4) for c in (1, 2))


def scaled_encoder_offsets(sd: dict, gain: float) -> dict:
    """`sd` with the four offset convs of the deformable blocks (weight and bias) times `gain`: the encoder's counterpart of `scaled_offset_weights`.  The
    offsets grow until most hit the +-max(h, w) / 4 clamp of DeformableConv2d and many samples fall partly or wholly off the map"""
    out = dict(sd)
    for n in ENCODER_OFFSET_CONVS:
        for k in (f"{n}.weight", f"{n}.bias"):
            out[k] = sd[k] * gain
    return out


def small_variance(sd: dict, seed: int) -> dict:
    """`sd` with every BatchNorm `running_var` redrawn log-uniform in [1e-6, 1e-3] and the matching weight multiplied by sqrt(var + 1e-5), so the
    activations keep their scale while BatchNorm's epsilon (1e-5) decides the result: 1 / sqrt(var + eps) moves by 0.5 % .. 70 % without it"""
    rng = np.random.Generator(np.random.PCG64(950 + seed))
    out = dict(sd)
    for name in sd:
        if name.endswith("running_var"):
            var = torch.from_numpy(np.exp(rng.uniform(math.log(1e-6), math.log(1e-3), tuple(sd[name].shape))).astype(np.float32))
            out[name] = var
            out[name[:-len("running_var")] + "weight"] = sd[name[:-len("running_var")] + "weight"] * torch.sqrt(var + 1e-5)
    return out


STAGES = ROOT / "tests" / "golden" / "aliked_stages"
OFFSET_GAIN = 40.0
# The encoder on whole images (aliked-n16; the encoder does not depend on n_pos).  name -> (weight seed, image generator, image seed, B, C, H, W,
# offset gain, small_variance seed or None, whether x1 and x2 are stored: on the two large cases x1 alone is above the size limit of a committed file)
ENC_STAGES = {
    "enc_8x8_b1_rgb_noise_g1": (30, "noise_image", 1, 1, 3, 8, 8, 1.0, None, True),
    "enc_8x8_b1_rgb_noise_g4_smallvar": (42, "noise_image", 2, 1, 3, 8, 8, 4.0, 1, True),
    "enc_24x17_b2_rgb_noise_g4": (38, "noise_image", 3, 2, 3, 24, 17, 4.0, None, True),
    "enc_31x33_b1_gray_noise_g1": (33, "noise_image", 4, 1, 1, 31, 33, 1.0, None, True),
    "enc_40x56_b1_rgb_image_g4": (58, "aliked_image", 5, 1, 3, 40, 56, 4.0, None, True),
    "enc_40x300_b1_rgb_noise_g4": (35, "noise_image", 6, 1, 3, 40, 300, 4.0, None, False),
    "enc_72x90_b1_rgb_noise_g1": (36, "noise_image", 7, 1, 3, 72, 90, 1.0, None, False),
}


def encoder_inputs(name: str, gain: float = None):
    """(state dict, image [B, C, H, W]) of an ENC_STAGES case; `gain` replaces the table's offset gain"""
    wseed, gen, iseed, b, c, h, w, g, sv, _ = ENC_STAGES[name]
    sd = aliked_state_dict(wseed, "aliked-n16")
    if sv is not None:
        sd = small_variance(sd, sv)
    sd = scaled_encoder_offsets(sd, g if gain is None else gain)
    return sd, {"noise_image": noise_image, "aliked_image": aliked_image}[gen](iseed, b, h, w, c)
# DKD on crafted score maps.  name -> (map generator, its arguments, radius, top_k, scores_th, n_limit, image_size or None).  Only cases the
# reference defines: image_size absent or equal to the map, and in top-k mode at least top_k positive maxima.
DKD_STAGES = {
    "dkd_tall_b2_300x40_r2_th": ("score_maps", (1, 2, 300, 40), 2, -1, 0.2, 20000, None),
    "dkd_wide_b2_24x600_r2_limit500": ("score_maps", (2, 2, 24, 600), 2, -1, 0.2, 500, None),
    "dkd_many_b1_272x96_r1_top1500": ("score_maps", (3, 1, 272, 96), 1, 1500, -1.0, 20000, None),
    "dkd_many_b1_272x96_r1_limit1025": ("score_maps", (3, 1, 272, 96), 1, -1, 0.04, 1025, None),
    "dkd_quantised_b1_272x96_r1_limit1500": ("quantised_maps", (3, 1, 272, 96), 1, -1, 0.04, 1500, None),
    "dkd_radius5_b2_70x130": ("score_maps", (4, 2, 70, 130), 5, -1, 0.2, 20000, None),
    "dkd_radius8_b2_70x130": ("score_maps", (4, 2, 70, 130), 8, -1, 0.2, 20000, None),
    "dkd_fallback_b3_40x56_r2": ("score_maps", (5, 3, 40, 56), 2, -1, 0.99, 20000, None),       # nothing passes: per-image means
    "dkd_mean_b2_40x56_r2": ("score_maps", (6, 2, 40, 56), 2, -1, -1.0, 20000, None),           # scores_th <= 0: the mean mode
    "dkd_image_size_b2_40x56_r3": ("score_maps", (7, 2, 40, 56), 3, -1, 0.2, 20000, [[56, 40], [56, 40]]),
}
# SDDH on crafted level maps.  name -> (model, weight seed, offset gain, level seed, B, H, W, N, keypoint seed)
SDDH_STAGES = {
    "sddh_n16_b2_40x56_n33": ("aliked-n16", 20, 1.0, 1, 2, 40, 56, 33, 1),
    "sddh_n32_b2_40x56_n33": ("aliked-n32", 21, 1.0, 2, 2, 40, 56, 33, 2),
    "sddh_n16_b2_40x56_n33_clamped": ("aliked-n16", 20, OFFSET_GAIN, 1, 2, 40, 56, 33, 1),
    "sddh_n32_b2_40x56_n33_clamped": ("aliked-n32", 21, OFFSET_GAIN, 2, 2, 40, 56, 33, 2),
    "sddh_n16_b1_8x8_n20": ("aliked-n16", 22, 1.0, 3, 1, 8, 8, 20, 3),
    "sddh_n32_b1_8x8_n20_clamped": ("aliked-n32", 23, OFFSET_GAIN, 4, 1, 8, 8, 20, 4),
}


def stage_knorm(kseed: int, b: int, n: int, h: int, w: int) -> np.ndarray:
    """[b, n, 2]: crafted_knorm per image (the special points in every image, other random ones)"""
    return np.stack([crafted_knorm(10 * kseed + i, n, h, w) for i in range(b)])


def torch_dense_map(levels: list, h: int, w: int) -> torch.Tensor:
    """x1234 as extract_dense_map forms it from the level maps, in torch fp32: [B, 128, H, W]"""
    hp, wp, pt, pl = padded_dims(h, w)
    ups = [F.interpolate(torch.from_numpy(l).permute(0, 3, 1, 2), size=(hp, wp), mode="bilinear", align_corners=True) for l in levels]
    x = F.normalize(torch.cat(ups, dim=1), p=2, dim=1)
    return x[..., pt:pt + h, pl:pl + w].contiguous()


def make_stages(mod):
    STAGES.mkdir(parents=True, exist_ok=True)
    gens = {"score_maps": score_maps, "quantised_maps": quantised_maps}
    for name, (gen, args, radius, top_k, th, n_limit, image_size) in DKD_STAGES.items():
        smap = gens[gen](*args)
        b, h, w = smap.shape
        dkd = mod.DKD(radius=radius, top_k=top_k, scores_th=th, n_limit=n_limit)
        isz = None if image_size is None else torch.tensor(image_size, dtype=torch.float32)
        with torch.no_grad():
            s = torch.from_numpy(smap)[:, None]
            kn, ks, _ = dkd(s.clone(), sub_pixel=True, image_size=isz)
            k0, _, _ = dkd(s.clone(), sub_pixel=False, image_size=isz)      # the unrefined positions: the raster indices
        wh = torch.tensor([w - 1, h - 1])
        idx = [((k + 1) / 2 * wh).round().long() for k in k0]
        idx = [(i[:, 1] * w + i[:, 0]).numpy().astype(np.int32) for i in idx]
        pix = [(wh * (k + 1) / 2.0).numpy() for k in kn]                     # aliked.py:757
        counts = np.array([len(i) for i in idx], np.int32)
        if top_k > 0:
            assert all((smap[i].reshape(-1)[idx[i]] > 0).all() for i in range(b)), "top-k beyond the positive maxima: the reference is undefined there"
        meta = {"gen": gen, "args": list(args), "radius": radius, "top_k": top_k, "scores_th": th, "n_limit": n_limit, "image_size": image_size}
        np.savez_compressed(STAGES / f"{name}.npz", meta=json.dumps(meta), counts=counts, indices=np.concatenate(idx),
                            knorm=np.concatenate([k.numpy() for k in kn]), keypoints=np.concatenate(pix), keypoint_scores=np.concatenate([k.numpy() for k in ks]))
        print(f"{name}: counts {counts.tolist()}")
    for name, (model, wseed, gain, lseed, b, h, w, n, kseed) in SDDH_STAGES.items():
        sd = scaled_offset_weights(aliked_state_dict(wseed, model), gain)
        n_pos = 32 if model.endswith("32") else 16
        head = mod.SDDH(128, 3, n_pos, gate=torch.nn.SELU(inplace=True), conv2D=False, mask=False)
        head.load_state_dict({k[len("desc_head."):]: v for k, v in sd.items() if k.startswith("desc_head.")}, strict=True)
        x = torch_dense_map(crafted_levels(lseed, b, h, w), h, w)
        kn = stage_knorm(kseed, b, n, h, w)
        with torch.no_grad():
            desc, offsets = head(x, [torch.from_numpy(k) for k in kn])
        clamped = float(np.mean([(o.abs() >= max(h, w) / 4.0).float().mean().item() for o in offsets]))
        meta = {"model": model, "wseed": wseed, "gain": gain, "lseed": lseed, "b": b, "h": h, "w": w, "n": n, "kseed": kseed}
        np.savez_compressed(STAGES / f"{name}.npz", meta=json.dumps(meta), descriptors=np.stack([d.numpy() for d in desc]))
        print(f"{name}: {clamped:.0%} of the offsets at the clamp")
    for name, (wseed, gen, iseed, b, c, h, w, gain, sv, store_x12) in ENC_STAGES.items():
        sd, image = encoder_inputs(name)
        mod.torch.hub.load_state_dict_from_url = lambda url, map_location=None, _sd=sd: _sd
        net = mod.ALIKED(model_name="aliked-n16").eval()
        taps = {}   # conv1 .. conv4: (the output tensor itself, which the in-place SELU of extract_dense_map then gates; a copy taken before that)
        hooks = [getattr(net, f"conv{i}").register_forward_hook(lambda m, a, out, _i=i: taps.__setitem__(_i, (out, out.detach().clone()))) for i in range(1, 5)]
        with torch.no_grad():
            _, score_map = net.extract_dense_map(image if c == 3 else mod.grayscale_to_rgb(image))
        for hk in hooks:
            hk.remove()
        levels = {}
        for i in range(1, 5):
            gated, raw = taps[i]
            assert torch.equal(gated, F.selu(raw)) and not torch.equal(gated, raw), "the hooked tensor must hold the gated level map"
            levels[f"x{i}"] = gated.permute(0, 2, 3, 1).contiguous().numpy()              # [B, Hp >> s, Wp >> s, 32]: the layout of ALIKED.level_maps
        if not store_x12:
            del levels["x1"], levels["x2"]
        meta = {"wseed": wseed, "gen": gen, "iseed": iseed, "b": b, "c": c, "h": h, "w": w, "gain": gain, "small_variance": sv}
        np.savez_compressed(STAGES / f"{name}.npz", meta=json.dumps(meta), scores=score_map[:, 0].numpy(), **levels)
        size = (STAGES / f"{name}.npz").stat().st_size
        assert size < 952 * 1024, f"{name}: {size} bytes"
        print(f"{name}: levels {sorted(levels)} {size} bytes, score range [{float(score_map.min()):.3f}, {float(score_map.max()):.3f}]")


# ---------------------------------------------------------------------------------------------------- deform_conv2d restatement
def _bilinear_tv(x, py, px):
    """torchvision's deform_conv2d bilinear_interpolate: x [B, C, H, W], py / px [B, 1, Ho, Wo] -> [B, C, Ho, Wo]"""
    B, C, H, W = x.shape
    hl, wl = torch.floor(py), torch.floor(px)
    lh, lw = py - hl, px - wl
    hh, hw = 1 - lh, 1 - lw
    hl, wl = hl.long(), wl.long()
    flat = x.reshape(B, C, H * W)

    def corner(yy, xx, ok):
        idx = (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).reshape(B, 1, -1).expand(B, C, -1)
        return torch.gather(flat, 2, idx).reshape(B, C, *yy.shape[2:]) * ok.to(x.dtype)

    v1 = corner(hl, wl, (hl >= 0) & (wl >= 0))
    v2 = corner(hl, wl + 1, (hl >= 0) & (wl + 1 <= W - 1))
    v3 = corner(hl + 1, wl, (hl + 1 <= H - 1) & (wl >= 0))
    v4 = corner(hl + 1, wl + 1, (hl + 1 <= H - 1) & (wl + 1 <= W - 1))
    val = hh * hw * v1 + hh * lw * v2 + lh * hw * v3 + lh * lw * v4
    valid = ~((py <= -1) | (py >= H) | (px <= -1) | (px >= W))
    return val * valid.to(x.dtype)


def deform_conv2d(input, offset, weight, bias=None, stride=(1, 1), padding=(0, 0), dilation=(1, 1), mask=None):
    """torchvision.ops.deform_conv2d for stride 1, dilation 1, one offset group, no mask (what ALIKED uses)."""
    assert mask is None
    pad = (padding, padding) if isinstance(padding, int) else tuple(padding)
    B, Cin, H, W = input.shape
    Cout, _, kh, kw = weight.shape
    Ho, Wo = H + 2 * pad[0] - (kh - 1), W + 2 * pad[1] - (kw - 1)
    ys = torch.arange(Ho, dtype=input.dtype).view(1, 1, Ho, 1)
    xs = torch.arange(Wo, dtype=input.dtype).view(1, 1, 1, Wo)
    cols = []
    for k in range(kh * kw):
        i, j = divmod(k, kw)
        py = (ys - pad[0] + i) + offset[:, 2 * k:2 * k + 1]
        px = (xs - pad[1] + j) + offset[:, 2 * k + 1:2 * k + 2]
        cols.append(_bilinear_tv(input, py, px))
    col = torch.stack(cols, 2)                                        # [B, Cin, k, Ho, Wo]
    out = torch.einsum("bckhw,ock->bohw", col, weight.reshape(Cout, Cin, kh * kw))
    if bias is not None:
        out = out + bias.view(1, -1, 1, 1)
    return out


# ---------------------------------------------------------------------------------------------------- the reference module
def load_reference(state_dict_for):
    """Execute aliked.py with the stand-ins; `state_dict_for(model_name)` feeds torch.hub.load_state_dict_from_url."""
    tv = types.ModuleType("torchvision"); tv_ops = types.ModuleType("torchvision.ops"); tv_models = types.ModuleType("torchvision.models")
    resnet = types.ModuleType("torchvision.models.resnet")
    resnet.conv1x1 = lambda i, o, stride=1: torch.nn.Conv2d(i, o, kernel_size=1, stride=stride, bias=False)
    resnet.conv3x3 = lambda i, o, stride=1, groups=1, dilation=1: torch.nn.Conv2d(i, o, kernel_size=3, stride=stride, padding=dilation, groups=groups,
                                                                                  bias=False, dilation=dilation)
    tv_ops.deform_conv2d = deform_conv2d
    tv.ops = tv_ops; tv.models = tv_models; tv_models.resnet = resnet
    kornia = types.ModuleType("kornia"); color = types.ModuleType("kornia.color")
    color.grayscale_to_rgb = lambda x: torch.cat([x, x, x], dim=-3)
    kornia.color = color
    pkg = types.ModuleType("lgref"); pkg.__path__ = []
    utils = types.ModuleType("lgref.utils")

    class Extractor(torch.nn.Module):   # utils.py:131-135
        def __init__(self, **conf):
            super().__init__()
            self.conf = types.SimpleNamespace(**{**self.default_conf, **conf})

    utils.Extractor = Extractor
    mods = {"torchvision": tv, "torchvision.ops": tv_ops, "torchvision.models": tv_models, "torchvision.models.resnet": resnet,
            "kornia": kornia, "kornia.color": color, "lgref": pkg, "lgref.utils": utils}
    saved = {k: sys.modules.get(k) for k in mods}
    sys.modules.update(mods)
    try:
        mod = types.ModuleType("lgref.aliked"); mod.__package__ = "lgref"
        exec(compile(REF.read_text(), str(REF), "exec"), mod.__dict__)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    mod.torch.hub.load_state_dict_from_url = lambda url, map_location=None: state_dict_for(url.rsplit("/", 1)[-1][:-4])
    return mod


def margins(mod, score_map, radius, th):
    """(smallest |nms score - threshold| over the NMS maxima, smallest gap between a pixel and the largest other value of its window)"""
    s = score_map[:, None]
    nms = mod.simple_nms(s, radius)
    nz = nms[nms > 0]
    th_margin = float((nz - th).abs().min()) if nz.numel() and th is not None else float("inf")
    k = 2 * radius + 1
    pat = F.unfold(s, k, padding=radius)   # zero padding: the map is positive, so pads never tie
    centre = pat[:, k * k // 2].clone()
    pat[:, k * k // 2] = -1.0
    tie = float((centre - pat.max(dim=1).values).abs().min())
    return th_margin, tie


def run_reference(mod, model, wseed, image, conf):
    sd = aliked_state_dict(wseed, model)
    net = mod.ALIKED(model_name=model, **conf).eval()
    with torch.no_grad():
        img = image if image.shape[1] == 3 else mod.grayscale_to_rgb(image)
        _, score_map = net.extract_dense_map(img)
        out = net({"image": image})
    sm = score_map[:, 0]
    if net.dkd.top_k > 0:
        th = None
    elif net.dkd.scores_th > 0 and bool(((mod.simple_nms(score_map, net.dkd.radius) > net.dkd.scores_th).sum() > 0)):
        th = net.dkd.scores_th
    else:
        th = sm.reshape(sm.shape[0], -1).mean(dim=1).tolist()   # per image
    return sd, sm, out, th


def main():
    mod = load_reference(lambda name: None)
    if "--stages" in sys.argv[1:]:
        make_stages(mod)
        return
    GOLD.mkdir(parents=True, exist_ok=True)
    tree = {}   # names / shapes of the reference's module tree
    for model in ("aliked-n16", "aliked-n32"):
        mod.torch.hub.load_state_dict_from_url = lambda url, map_location=None, _m=model: aliked_state_dict(0, _m)
        net = mod.ALIKED(model_name=model)
        tree[model] = [[k, list(v.shape)] for k, v in net.state_dict().items()]
    (ROOT / "tests" / "golden" / "reference_aliked_state_dict.json").write_text(json.dumps(tree, indent=0) + "\n")

    def record(name, model, wseed, iseeds, b, c, h, w, conf, outs):
        kp = [o[2]["keypoints"][0] for o in outs]; ks = [o[2]["keypoint_scores"][0] for o in outs]; ds = [o[2]["descriptors"][0] for o in outs]
        counts = np.array([len(k) for k in kp], np.int32)
        n = int(counts.max())
        K = np.zeros((b, n, 2), np.float32); S = np.zeros((b, n), np.float32); D = np.zeros((b, n, 128), np.float32)
        for i in range(b):
            K[i, :counts[i]] = kp[i].numpy(); S[i, :counts[i]] = ks[i].numpy(); D[i, :counts[i]] = ds[i].numpy()
        smap = np.concatenate([o[1].numpy() for o in outs], 0)
        ths = [o[3] for o in outs]
        mg = [margins(mod, o[1], conf.get("nms_radius", 2), o[3]) for o in outs]
        meta = {"model": model, "wseed": wseed, "iseeds": list(iseeds), "b": b, "c": c, "h": h, "w": w, "conf": conf, "thresholds": ths,
                "threshold_margin": min(m[0] for m in mg), "nms_tie_margin": min(m[1] for m in mg)}
        np.savez_compressed(GOLD / f"{name}.npz", meta=json.dumps(meta), scores=smap, keypoints=K, keypoint_scores=S, descriptors=D, counts=counts)
        print(f"{name}: counts {counts.tolist()} score range [{smap.min():.3f}, {smap.max():.3f}] th {ths} margins {meta['threshold_margin']:.2e} / {meta['nms_tie_margin']:.2e}")

    only = [a for a in sys.argv[1:] if not a.startswith("-")]
    for name, (model, wseed, iseed, b, c, h, w, conf) in CASES.items():
        if only and name not in only:
            continue
        img = aliked_image(iseed, b, h, w, c)
        sd, sm, out, th = None, None, None, None
        mod.torch.hub.load_state_dict_from_url = lambda url, map_location=None, _m=model, _s=wseed: aliked_state_dict(_s, _m)
        sd, sm, out, th = run_reference(mod, model, wseed, img, conf)
        outs = []
        for i in range(b):   # split per image for `record` (the reference ran the batch at once)
            outs.append((None, sm[i:i + 1], {k: v[i:i + 1] for k, v in out.items()}, th[i] if isinstance(th, list) else th))
        record(name, model, wseed, [iseed], b, c, h, w, conf, outs)
    for name, (model, wseed, iseeds, c, h, w, conf) in RAGGED.items():
        if only and name not in only:
            continue
        mod.torch.hub.load_state_dict_from_url = lambda url, map_location=None, _m=model, _s=wseed: aliked_state_dict(_s, _m)
        outs = []
        for s in iseeds:
            sd, sm, out, th = run_reference(mod, model, wseed, aliked_image(s, 1, h, w, c), conf)
            outs.append((None, sm, out, th[0] if isinstance(th, list) else th))
        record(name, model, wseed, iseeds, len(iseeds), c, h, w, conf, outs)


if __name__ == "__main__":
    sys.path.insert(0, str(ROOT))
    main()
