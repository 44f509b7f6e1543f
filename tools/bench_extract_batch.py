#!/usr/bin/env python3
"""An extractor on a mixed-size image set: `extract_batch` (ragged batches, one forward per group) against the per-image `extract` loop followed by
`collate_features` — the only correct path for such a set before ragged batches.  Two sets of K = 16 images, alternating 480x640 / 640x480 and
768x1024 / 683x1024; three repeats of every timing.  `--extractor superpoint` (default) runs both conv precisions in one process on seeded noise images;
`--extractor aliked` runs aliked-n16 (exact fp32, max_num_keypoints = 2048) on seeded 3-channel textured images.  `extract_batch` is timed twice: with the
planner's size order (like sizes share a canvas: no padding on these sets) and in input order (every canvas mixes both sizes: the padding share is printed).
`--loop-only` times the loop alone (a build without extract_batch).  One JSON line per timing on stdout."""
import argparse, json, sys, time
from pathlib import Path
import torch
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tools"))
from lightglue_amd import collate_features

SETS = {"480x640+640x480": [(480, 640), (640, 480)] * 8, "768x1024+683x1024": [(768, 1024), (683, 1024)] * 8}


def timed(fn, warmup, iters):
    for _ in range(warmup): fn()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(iters): fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def configurations(extractor):
    """(label, model, images(sizes)) per configuration of the extractor"""
    if extractor == "superpoint":
        import make_golden_superpoint as G
        from lightglue_amd import SuperPoint
        def noise(sizes):
            g = torch.Generator(device="cuda").manual_seed(0)
            return [torch.rand(1, h, w, device="cuda", generator=g) for h, w in sizes]
        for prec in ("fp32", "f16x3"):
            yield prec, SuperPoint(weights=G.encoder_state_dict(0), max_num_keypoints=2048, conv_precision=prec).cuda().eval(), noise
    else:
        import make_golden_aliked as G
        from lightglue_amd import ALIKED
        yield "fp32", ALIKED(weights=G.aliked_state_dict(0), max_num_keypoints=2048).cuda().eval(), \
            lambda sizes: [G.aliked_image(i, 1, h, w, 3)[0].cuda() for i, (h, w) in enumerate(sizes)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--extractor", choices=("superpoint", "aliked"), default="superpoint")
    ap.add_argument("--loop-only", action="store_true"); ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5); ap.add_argument("--warmup", type=int, default=2); ap.add_argument("--batch-size", type=int, default=8)
    a = ap.parse_args()
    for prec, model, make_images in configurations(a.extractor):
        for name, sizes in SETS.items():
            images = make_images(sizes)
            modes = {"loop": lambda: collate_features([model.extract(i) for i in images])}
            if not a.loop_only:
                from lightglue_amd import plan_image_batches
                for order in ("size", "input"):
                    plan = plan_image_batches(sizes, a.batch_size, order=order)
                    pad = 1.0 - sum(h * w for h, w in sizes) / sum(len(idx) * hc * wc for idx, (hc, wc) in plan)
                    modes[f"extract_batch[{order}]"] = (lambda order=order: model.extract_batch(images, batch_size=a.batch_size, order=order))
                    modes[f"extract_batch[{order}]"].padding = pad
            for mode, fn in modes.items():
                for rep in range(a.repeats):
                    dt = timed(fn, a.warmup, a.iters)
                    print(json.dumps({"extractor": a.extractor, "precision": prec, "set": name, "mode": mode, "repeat": rep, "ms_per_set": round(dt * 1e3, 3),
                                      "images_per_s": round(len(images) / dt, 1), "canvas_padding": round(getattr(fn, "padding", 0.0), 4)}), flush=True)


if __name__ == "__main__":
    main()
