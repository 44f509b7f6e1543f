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
    python tools/make_golden_aliked.py
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

# name -> (model, weight seed, image seed, B, C, H, W, conf)
CASES = {
    "n16_rgb_b1_120x160_th": ("aliked-n16", 0, 0, 1, 3, 120, 160, {"detection_threshold": 0.5}),
    "n32_gray_b1_75x109_limit40": ("aliked-n32", 1, 1, 1, 1, 75, 109, {"detection_threshold": 0.3, "max_num_keypoints": 40}),
    "n16_rgb_b2_64x96_top60": ("aliked-n16", 2, 2, 2, 3, 64, 96, {"detection_threshold": -1, "max_num_keypoints": 60}),
    "n16_gray_b1_96x128_fallback": ("aliked-n16", 3, 3, 1, 1, 96, 128, {"detection_threshold": 0.9999}),
    "n32_rgb_b1_240x320_limit300": ("aliked-n32", 4, 4, 1, 3, 240, 320, {"detection_threshold": 0.3, "max_num_keypoints": 300}),
    "n16_rgb_b1_96x128_r6": ("aliked-n16", 8, 8, 1, 3, 96, 128, {"detection_threshold": 0.3, "nms_radius": 6}),
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
    GOLD.mkdir(parents=True, exist_ok=True)
    mod = load_reference(lambda name: None)
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

    for name, (model, wseed, iseed, b, c, h, w, conf) in CASES.items():
        img = aliked_image(iseed, b, h, w, c)
        sd, sm, out, th = None, None, None, None
        mod.torch.hub.load_state_dict_from_url = lambda url, map_location=None, _m=model, _s=wseed: aliked_state_dict(_s, _m)
        sd, sm, out, th = run_reference(mod, model, wseed, img, conf)
        outs = []
        for i in range(b):   # split per image for `record` (the reference ran the batch at once)
            outs.append((None, sm[i:i + 1], {k: v[i:i + 1] for k, v in out.items()}, th[i] if isinstance(th, list) else th))
        record(name, model, wseed, [iseed], b, c, h, w, conf, outs)
    for name, (model, wseed, iseeds, c, h, w, conf) in RAGGED.items():
        mod.torch.hub.load_state_dict_from_url = lambda url, map_location=None, _m=model, _s=wseed: aliked_state_dict(_s, _m)
        outs = []
        for s in iseeds:
            sd, sm, out, th = run_reference(mod, model, wseed, aliked_image(s, 1, h, w, c), conf)
            outs.append((None, sm, out, th[0] if isinstance(th, list) else th))
        record(name, model, wseed, iseeds, len(iseeds), c, h, w, conf, outs)


if __name__ == "__main__":
    sys.path.insert(0, str(ROOT))
    main()
