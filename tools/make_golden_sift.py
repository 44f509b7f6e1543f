#!/usr/bin/env python3
"""Generate tests/golden/sift/sift_helpers.npz with the reference's OWN `filter_dog_point` and `sift_to_rootsift` (lightglue/sift.py), executed unmodified on CPU.

sift.py imports cv2, kornia.color, packaging and its package's utils at module level; none of them is touched by the two functions, so empty stand-ins
(a `cv2.Feature2D` name for an annotation, `rgb_to_grayscale`, `Extractor`) let the file execute.  The fixture holds data only: the seeded inputs below and
what the reference returned for them.

    python tools/make_golden_sift.py --reference /path/to/LightGlue

Inputs (float32 throughout, as cv2 / pycolmap hand them over):
  * image "a": 300 detections on a 24 x 40 image, "b": 200 on 17 x 23.  The second half of each set repeats points of the first half (several orientations per
    point): a third with another scale and angle, a third with the same scale and another angle, a third with the same scale and the angle negated (equal
    |angle|: both stay).  Scores are distinct (no ties for top-k) and a few are negative (they lose against the 0 the buffer starts with).
  * keep arrays for nms_radius 0 / 1 / 3, with and without scores; `topk_a`: filter (radius 0, scores) + torch.topk(64), the reference's order.
  * descriptor rows: uint8 [300, 128] (row 0 all zero, row 1 one-hot 255, row 2 all 255) and [260, 64], and their RootSIFT from float32 copies.
"""
import argparse
import os
import sys
import types
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
OUT = ROOT / "tests" / "golden" / "sift" / "sift_helpers.npz"   # a directory of its own: every tests/golden/*.npz is a matcher fixture (tests/conftest.py)
RADII = (0, 1, 3)
TOPK = 64


def load_reference(ref_dir: Path):
    src = ref_dir / "lightglue" / "sift.py"
    cv2 = types.ModuleType("cv2"); cv2.Feature2D = object
    kornia = types.ModuleType("kornia"); color = types.ModuleType("kornia.color"); color.rgb_to_grayscale = None; kornia.color = color
    pkg = types.ModuleType("lgref"); pkg.__path__ = []
    utils = types.ModuleType("lgref.utils"); utils.Extractor = torch.nn.Module
    mods = {"cv2": cv2, "kornia": kornia, "kornia.color": color, "lgref": pkg, "lgref.utils": utils}
    try:
        import packaging.version  # noqa: F401
    except ImportError:
        packaging = types.ModuleType("packaging"); packaging.version = types.ModuleType("packaging.version")
        mods.update({"packaging": packaging, "packaging.version": packaging.version})
    saved = {k: sys.modules.get(k) for k in mods}
    sys.modules.update(mods)
    try:
        mod = types.ModuleType("lgref.sift"); mod.__package__ = "lgref"
        exec(compile(src.read_text(), str(src), "exec"), mod.__dict__)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mod


def detections(seed: int, n: int, h: int, w: int):
    """Seeded raw detections: (points [n, 2] (x, y), scales, angles, scores), float32."""
    rng = np.random.default_rng(seed)
    half = n // 2
    pts = np.stack([rng.uniform(0.01, w - 0.01, half), rng.uniform(0.01, h - 0.01, half)], -1).astype(np.float32)
    scales = rng.uniform(1.0, 8.0, half).astype(np.float32)
    angles = rng.uniform(-np.pi, np.pi, half).astype(np.float32)
    src = rng.integers(0, half, n - half)
    kind = np.arange(n - half) % 3
    d_scales = np.where(kind == 0, rng.uniform(1.0, 8.0, n - half).astype(np.float32), scales[src]).astype(np.float32)
    d_angles = np.where(kind == 2, -angles[src], rng.uniform(-np.pi, np.pi, n - half).astype(np.float32)).astype(np.float32)
    pts, scales, angles = np.concatenate([pts, pts[src]]), np.concatenate([scales, d_scales]), np.concatenate([angles, d_angles])
    scores = (rng.permutation(n).astype(np.float32) - 5.0) / np.float32(n)      # distinct; five of them negative, one zero
    return pts, scales, angles, scores


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reference", default=os.environ.get("LIGHTGLUE_REFERENCE"), help="checkout of the reference (the directory that holds lightglue/sift.py)")
    args = ap.parse_args()
    if not args.reference:
        ap.error("--reference (or LIGHTGLUE_REFERENCE) is required")
    ref = load_reference(Path(args.reference))
    out = {"radii": np.array(RADII), "topk": np.array(TOPK)}
    for name, seed, n, (h, w) in (("a", 11, 300, (24, 40)), ("b", 12, 200, (17, 23))):
        pts, scales, angles, scores = detections(seed, n, h, w)
        out.update({f"points_{name}": pts, f"scales_{name}": scales, f"angles_{name}": angles, f"scores_{name}": scores, f"shape_{name}": np.array([h, w])})
        for r in RADII:
            for tag, sc in (("scale", None), ("score", scores)):
                keep = ref.filter_dog_point(pts, scales, angles, (h, w), r, scores=sc)
                assert 0 < len(keep) < n, "a case must be neither empty nor full"
                out[f"keep_{name}_r{r}_{tag}"] = keep.astype(np.int64)
                print(f"image {name} ({h} x {w}, {n} detections) radius {r} by {tag}: {len(keep)} kept")
    keep = out["keep_a_r0_score"]
    assert len(keep) > TOPK
    out["topk_a"] = keep[torch.topk(torch.from_numpy(out["scores_a"][keep]), TOPK).indices.numpy()]      # sift.py:189-194
    rng = np.random.default_rng(13)
    desc = rng.integers(0, 256, (300, 128), dtype=np.uint8)
    desc[0] = 0; desc[1] = 0; desc[1, 37] = 255; desc[2] = 255
    desc64 = rng.integers(0, 256, (260, 64), dtype=np.uint8)
    out.update({"desc": desc, "desc64": desc64})
    for key in ("desc", "desc64"):
        out[f"rootsift_{key}"] = ref.sift_to_rootsift(torch.from_numpy(out[key]).float()).numpy()
    print("all-zero row -> uniform", out["rootsift_desc"][0, :2], "1 / sqrt(128) =", 1 / np.sqrt(128))
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
