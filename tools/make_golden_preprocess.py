#!/usr/bin/env python3
"""Generate tests/golden/preprocess/*.npz: the reference's OWN `ImagePreprocessor` and `Extractor.extract` (lightglue/utils.py:12-38, :131-147),
executed unmodified on CPU over stand-ins for the imports that do not exist here.

utils.py imports cv2 (file I/O only: an empty stand-in) and kornia, of which it calls exactly one function:
`kornia.geometry.transform.resize(img, size, side=, antialias=, align_corners=)`.  kornia is not installed where these fixtures were made
(nor cv2, nor torchvision), so that call lands in `kornia_resize` below, a plain-torch restatement written from kornia's published source
(>= 0.6.11, the floor of the reference's requirements.txt).  THE RESTATEMENT HAS NOT BEEN CHECKED AGAINST KORNIA ITSELF: what the fixtures
hold is "the reference's utils.py executed over this stand-in", nothing more.  It is kept in one function so that whoever has kornia can
compare in one call:  torch.testing.assert_close(kornia_resize(x, s, side=..., antialias=...), kornia.geometry.transform.resize(x, s, ...)).

Per case the fixture stores the case itself, the reference output in float32, `scale`, the plan (target size, per-axis ks / sigma) and
`err64` = max |float32 output - the same definition evaluated entirely in float64|: the reference's own float32 error, which the GPU test's
bound is built from.  Inputs are regenerated from seeds by `preprocess_image` (tests import it), so only outputs are stored.

End-to-end fixtures (`e2e_*`): the reference SuperPoint / ALIKED CLASS's own `extract(img, resize=R)` — utils.py's real `Extractor` base, not
the stand-in base of make_golden_superpoint.py / make_golden_aliked.py — on the seeded weights and images of those tools.  Asserted at
generation time: the extractor run on the float32-resized and on the float64-resized image gives keypoint sets that differ by at most 0.25 %
(the GPU test allows 1 %; a fixture whose reference alone uses that up would prove nothing).
    python tools/make_golden_preprocess.py
"""
from __future__ import annotations

import contextlib
import json
import sys
import types
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(ROOT))
import make_golden_aliked as GA  # noqa: E402
import make_golden_superpoint as GS  # noqa: E402

REF_DIR = GS.REF.parent
GOLD = ROOT / "tests" / "golden" / "preprocess"

# name -> case.  resize: an int (edge length, with `side`) or an (h, w) pair.
CASES = {
    "rgb_long_480x640_to256": dict(seed=0, dtype="float32", B=1, C=3, H=480, W=640, resize=256, side="long", antialias=True, align_corners=None),
    "gray_short_300x400_to150": dict(seed=1, dtype="float32", B=1, C=1, H=300, W=400, resize=150, side="short", antialias=True, align_corners=None),
    "gray_vert_200x310_to80": dict(seed=2, dtype="float32", B=1, C=1, H=200, W=310, resize=80, side="vert", antialias=True, align_corners=None),
    "rgb_horz_210x280_to100": dict(seed=3, dtype="float32", B=1, C=3, H=210, W=280, resize=100, side="horz", antialias=True, align_corners=None),
    "rgb_pair_360x500_to90x200": dict(seed=4, dtype="float32", B=1, C=3, H=360, W=500, resize=(90, 200), side="long", antialias=True, align_corners=None),
    "gray_portrait_640x427_to256": dict(seed=5, dtype="float32", B=1, C=1, H=640, W=427, resize=256, side="long", antialias=True, align_corners=None),
    "rgb_upscale_60x80_to200": dict(seed=6, dtype="float32", B=1, C=3, H=60, W=80, resize=200, side="long", antialias=True, align_corners=None),
    "gray_noaa_480x640_to160": dict(seed=7, dtype="float32", B=1, C=1, H=480, W=640, resize=160, side="long", antialias=False, align_corners=None),
    "rgb_aligncorners_240x320_to128": dict(seed=8, dtype="float32", B=1, C=3, H=240, W=320, resize=128, side="long", antialias=True, align_corners=True),
    "gray_strong_256x2048_to128": dict(seed=9, dtype="float32", B=1, C=1, H=256, W=2048, resize=128, side="long", antialias=True, align_corners=None),
    "rgb_b2_150x200_to96": dict(seed=10, dtype="float32", B=2, C=3, H=150, W=200, resize=96, side="long", antialias=True, align_corners=None),
    "gray_trunc_187x250_to64": dict(seed=11, dtype="float32", B=1, C=1, H=187, W=250, resize=64, side="long", antialias=True, align_corners=None),
    "rgb_uint8_300x400_to160": dict(seed=12, dtype="uint8", B=1, C=3, H=300, W=400, resize=160, side="long", antialias=True, align_corners=None),
    "gray_strip_16x1003_to12x1002": dict(seed=13, dtype="float32", B=1, C=1, H=16, W=1003, resize=(12, 1002), side="long", antialias=True, align_corners=None),
    "gray_mixed_100x100_to50x150": dict(seed=14, dtype="float32", B=1, C=1, H=100, W=100, resize=(50, 150), side="long", antialias=True, align_corners=None),
}

# end to end: name -> (extractor, weight seed, image seed, C, H, W, resize, conf)
E2E_CASES = {
    "e2e_superpoint_240x320_to160": ("superpoint", 0, 10, 1, 240, 320, 160, {}),
    "e2e_aliked_n16_240x320_to160": ("aliked", 0, 0, 3, 240, 320, 160, {"model_name": "aliked-n16", "detection_threshold": 0.5}),
}


# ---------------------------------------------------------------------------------------------------- seeded inputs
def preprocess_image(seed: int, dtype: str, b: int, c: int, h: int, w: int) -> torch.Tensor:
    """[b, c, h, w]: seeded noise plus structure (a low-frequency field, blobs, a hard edge) in [0, 1] as float32, or the same rounded to uint8."""
    rng = np.random.Generator(np.random.PCG64(4200 + seed))
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.empty((b, c, h, w), np.float32)
    for i in range(b):
        t = 0.5 * rng.random((c, h, w), dtype=np.float32)
        for _ in range(12):
            cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(2.0, 0.2 * max(h, w))
            t += (rng.uniform(-0.5, 0.5, (c, 1, 1)) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * r * r))).astype(np.float32)
        t += 0.25 * (np.sin(xx * rng.uniform(0.02, 0.3) + yy * rng.uniform(0.02, 0.3)) > 0).astype(np.float32)
        t[:, :, w // 3] += 0.4            # a one-pixel line and a hard edge: what antialiasing is for
        t[:, h // 2:, :] += 0.1
        img[i] = np.clip(t, 0.0, 1.0)
    if dtype == "uint8":
        return torch.from_numpy(np.round(img * 255.0).astype(np.uint8))
    assert dtype == "float32"
    return torch.from_numpy(img)


# ---------------------------------------------------------------------------------------------------- kornia.geometry.transform.resize, restated
def resize_rule(h: int, w: int, size, side: str = "short", antialias: bool = False):
    """Target size and blur parameters of `kornia_resize` for an h x w image: (h_out, w_out, (ks_y, ks_x), (sigma_y, sigma_x)).  ks = 1 and
    sigma = 0 where nothing is blurred.  Python floats (double) throughout, int() truncates."""
    if isinstance(size, int):
        ar = w / h
        if side == "vert":
            size = (size, int(size * ar))
        elif side == "horz":
            size = (int(size / ar), size)
        elif (side == "short") ^ (ar < 1.0):
            size = (size, int(size * ar))
        else:
            size = (int(size / ar), size)
    h_out, w_out = int(size[0]), int(size[1])
    ks, sigma = (1, 1), (0.0, 0.0)
    if (h_out, w_out) != (h, w) and antialias and h_out > 0 and w_out > 0 and max(h / h_out, w / w_out) > 1:
        sigma = tuple(max((f - 1) / 2, 0.001) for f in (h / h_out, w / w_out))
        ks = tuple(int(max(4 * s, 3)) for s in sigma)
        ks = tuple(k + 1 if k % 2 == 0 else k for k in ks)
    return h_out, w_out, ks, sigma


def _gaussian(ks: int, sigma: float, like: torch.Tensor) -> torch.Tensor:
    x = torch.arange(ks, dtype=like.dtype) - ks // 2
    g = torch.exp(-x.pow(2) / (2 * sigma ** 2))
    return g / g.sum()


def kornia_resize(input, size, interpolation="bilinear", align_corners=None, side="short", antialias=False):
    """kornia.geometry.transform.resize for floating [..., C, H, W] input, in the dtype of `input`: side_to_image_size, the Gaussian antialias
    of kornia.filters.gaussian_blur2d (separable, x then y, border_type "reflect") and F.interpolate.  NOT checked against kornia (module docstring)."""
    h, w = input.shape[-2:]
    h_out, w_out, ks, sigma = resize_rule(h, w, size, side, antialias)
    if (h_out, w_out) == (h, w):
        return input
    x = input.reshape(-1, 1, h, w)
    if ks != (1, 1):
        ky, kx = _gaussian(ks[0], sigma[0], x), _gaussian(ks[1], sigma[1], x)
        x = F.conv2d(F.pad(x, (ks[1] // 2, ks[1] // 2, 0, 0), mode="reflect"), kx.view(1, 1, 1, -1))
        x = F.conv2d(F.pad(x, (0, 0, ks[0] // 2, ks[0] // 2), mode="reflect"), ky.view(1, 1, -1, 1))
    x = F.interpolate(x, size=(h_out, w_out), mode=interpolation, align_corners=align_corners)
    return x.reshape(*input.shape[:-2], h_out, w_out)


# ---------------------------------------------------------------------------------------------------- the reference modules
@contextlib.contextmanager
def _stand_ins():
    cv2 = types.ModuleType("cv2")
    kornia = types.ModuleType("kornia"); geometry = types.ModuleType("kornia.geometry"); transform = types.ModuleType("kornia.geometry.transform")
    color = types.ModuleType("kornia.color")
    transform.resize = kornia_resize
    geometry.transform = transform; kornia.geometry = geometry; kornia.color = color
    color.grayscale_to_rgb = lambda x: torch.cat([x, x, x], dim=-3)
    color.rgb_to_grayscale = lambda x: 0.299 * x[..., 0:1, :, :] + 0.587 * x[..., 1:2, :, :] + 0.114 * x[..., 2:3, :, :]
    tv = types.ModuleType("torchvision"); tv_ops = types.ModuleType("torchvision.ops"); tv_models = types.ModuleType("torchvision.models")
    resnet = types.ModuleType("torchvision.models.resnet")
    resnet.conv1x1 = lambda i, o, stride=1: torch.nn.Conv2d(i, o, kernel_size=1, stride=stride, bias=False)
    resnet.conv3x3 = lambda i, o, stride=1, groups=1, dilation=1: torch.nn.Conv2d(i, o, kernel_size=3, stride=stride, padding=dilation, groups=groups,
                                                                                  bias=False, dilation=dilation)
    tv_ops.deform_conv2d = GA.deform_conv2d        # the restatement make_golden_aliked.py documents and tests/test_aliked_cpu.py checks
    tv.ops = tv_ops; tv.models = tv_models; tv_models.resnet = resnet
    pkg = types.ModuleType("lgref"); pkg.__path__ = []
    mods = {"cv2": cv2, "kornia": kornia, "kornia.geometry": geometry, "kornia.geometry.transform": transform, "kornia.color": color,
            "torchvision": tv, "torchvision.ops": tv_ops, "torchvision.models": tv_models, "torchvision.models.resnet": resnet, "lgref": pkg}
    saved = {k: sys.modules.get(k) for k in list(mods) + ["lgref.utils"]}
    sys.modules.update(mods)
    try:
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def load_reference(*names):
    """Execute the reference's utils.py over the stand-ins, then the named extractor modules ("superpoint", "aliked") on top of the REAL
    utils.Extractor.  Returns {"utils": module, name: module, ...}."""
    out = {}
    with _stand_ins():
        for name in ("utils",) + names:
            path = REF_DIR / f"{name}.py"
            mod = types.ModuleType(f"lgref.{name}"); mod.__package__ = "lgref"
            exec(compile(path.read_text(), str(path), "exec"), mod.__dict__)
            sys.modules[f"lgref.{name}"] = mod
            out[name] = mod
        for name in names:
            sys.modules.pop(f"lgref.{name}", None)
    return out


@contextlib.contextmanager
def _state_dict_from(sd):
    """torch.hub.load_state_dict_from_url — the network download in the extractors' constructors — returns the seeded state dict."""
    orig = torch.hub.load_state_dict_from_url
    torch.hub.load_state_dict_from_url = lambda url, *a, **k: sd
    try:
        yield
    finally:
        torch.hub.load_state_dict_from_url = orig


# ---------------------------------------------------------------------------------------------------- fixtures
def run_case(utils, case: dict) -> dict:
    img = preprocess_image(case["seed"], case["dtype"], case["B"], case["C"], case["H"], case["W"])
    if case["dtype"] == "uint8":   # the reference's own conversion (numpy_image_to_torch: image / 255.0 in float64, cast to float32)
        f32 = torch.tensor(img.numpy() / 255.0, dtype=torch.float)
        f64 = img.double() / 255.0
    else:
        f32, f64 = img, img.double()
    resize = case["resize"]
    pre = utils.ImagePreprocessor(resize=resize, side=case["side"], antialias=case["antialias"], align_corners=case["align_corners"])
    out32, scale = pre(f32)
    out64, _ = pre(f64)
    assert out32.dtype == torch.float32 and out64.dtype == torch.float64
    h_out, w_out, ks, sigma = resize_rule(case["H"], case["W"], resize, case["side"], case["antialias"])
    assert tuple(out32.shape[-2:]) == (h_out, w_out)
    pair = isinstance(resize, (tuple, list))
    return {
        "seed": np.int64(case["seed"]), "dtype": np.str_(case["dtype"]), "B": np.int64(case["B"]), "C": np.int64(case["C"]), "H": np.int64(case["H"]),
        "W": np.int64(case["W"]), "resize": np.array(resize if pair else [resize], np.int64), "side": np.str_(case["side"]),
        "antialias": np.bool_(case["antialias"]), "align_corners": np.int64(-1 if case["align_corners"] is None else int(case["align_corners"])),
        "out": out32.numpy(), "scale": scale.numpy().astype(np.float32), "h_out": np.int64(h_out), "w_out": np.int64(w_out),
        "ks": np.array(ks, np.int64), "sigma": np.array(sigma, np.float64),
        "err64": np.float64((out32.double() - out64).abs().max()),
    }


def case_from_fixture(z) -> dict:
    """The `CASES` entry a stored fixture was made from."""
    r = [int(v) for v in z["resize"]]
    ac = int(z["align_corners"])
    return dict(seed=int(z["seed"]), dtype=str(z["dtype"]), B=int(z["B"]), C=int(z["C"]), H=int(z["H"]), W=int(z["W"]), resize=r[0] if len(r) == 1 else tuple(r),
                side=str(z["side"]), antialias=bool(z["antialias"]), align_corners=None if ac < 0 else bool(ac))


def e2e_image(kind: str, iseed: int, c: int, h: int, w: int) -> torch.Tensor:
    """[1, c, h, w] in [0, 1]: the seeded images of the existing extractor fixtures."""
    if kind == "superpoint":
        return torch.from_numpy(np.clip(GS.encoder_image(iseed, 1, h, w), 0.0, 1.0))
    return GA.aliked_image(iseed, 1, h, w, c)


def e2e_state_dict(kind: str, wseed: int, conf: dict) -> dict:
    return GS.encoder_state_dict(wseed) if kind == "superpoint" else GA.aliked_state_dict(wseed, conf["model_name"])


def _keypoints_differ(a: torch.Tensor, b: torch.Tensor, tol: float = 1e-2) -> int:
    """keypoints of either set without a partner within `tol` pixels in the other"""
    a, b = a.reshape(-1, 2).double(), b.reshape(-1, 2).double()
    if len(a) == 0 or len(b) == 0:
        return len(a) + len(b)
    d = torch.cdist(a, b)
    return int((d.min(1).values >= tol).sum() + (d.min(0).values >= tol).sum())


def run_e2e(mods, name: str) -> dict:
    kind, wseed, iseed, c, h, w, resize, conf = E2E_CASES[name]
    img = e2e_image(kind, iseed, c, h, w)
    sd = e2e_state_dict(kind, wseed, conf)
    utils, mod = mods["utils"], mods[kind]
    with _state_dict_from(sd), torch.no_grad():
        net = (mod.SuperPoint if kind == "superpoint" else mod.ALIKED)(**conf).eval()
        feats = net.extract(img, resize=resize)                                  # the reference's own extract(): utils.py:136-147
        # the generation-time condition: the reference's float32 resize error must not move the keypoint set
        pre = utils.ImagePreprocessor(**{**net.preprocess_conf, "resize": resize})
        r32, _ = pre(img)
        r64, scale = pre(img.double())
        k32 = net({"image": r32})["keypoints"]; k64 = net({"image": r64.float()})["keypoints"]
        differ = _keypoints_differ(k32, k64)
        assert differ <= 0.0025 * max(k32.shape[1], 1), f"{name}: {differ} of {k32.shape[1]} keypoints move with the reference's own float32 resize error: pick another seed"
        arrays = {"keypoints": feats["keypoints"].numpy(), "keypoint_scores": feats["keypoint_scores"].numpy(), "descriptors": feats["descriptors"].numpy(),
                  "image_size": feats["image_size"].numpy(), "scale": scale.float().numpy()}
        meta = {"kind": kind, "wseed": wseed, "iseed": iseed, "c": c, "h": h, "w": w, "resize": resize, "conf": conf, "b": 1, "differ_f32_f64": differ}
        if kind == "aliked":   # what tests/test_gpu_aliked.py's comparison reads: counts and the tie margins of the score map the detector saw
            rgb = r32 if r32.shape[1] == 3 else mod.grayscale_to_rgb(r32)
            _, score_map = net.extract_dense_map(rgb)
            sm = score_map[:, 0]
            if net.dkd.top_k > 0:
                th = None
            elif net.dkd.scores_th > 0 and bool((mod.simple_nms(score_map, net.dkd.radius) > net.dkd.scores_th).sum() > 0):
                th = net.dkd.scores_th
            else:
                th = float(sm.mean())
            tm, tie = GA.margins(mod, sm, conf.get("nms_radius", 2), th)
            meta.update(model=conf["model_name"], threshold_margin=tm, nms_tie_margin=tie)
            arrays["counts"] = np.array([feats["keypoints"].shape[1]], np.int32)
    arrays["meta"] = np.str_(json.dumps(meta))
    print(f"{name}: {feats['keypoints'].shape[1]} keypoints, {differ} differ between the float32- and float64-resized image")
    return arrays


def main():
    GOLD.mkdir(parents=True, exist_ok=True)
    only = set(sys.argv[1:])
    mods = load_reference("superpoint", "aliked")
    for name, case in CASES.items():
        if only and name not in only:
            continue
        arrays = run_case(mods["utils"], case)
        np.savez_compressed(GOLD / f"{name}.npz", **arrays)
        print(f"{name}: -> {int(arrays['h_out'])} x {int(arrays['w_out'])} ks {arrays['ks'].tolist()} sigma {arrays['sigma'].tolist()} err64 {float(arrays['err64']):.2e}")
    for name in E2E_CASES:
        if only and name not in only:
            continue
        np.savez_compressed(GOLD / f"{name}.npz", **run_e2e(mods, name))


if __name__ == "__main__":
    main()
