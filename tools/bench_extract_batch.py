#!/usr/bin/env python3
"""An extractor on a mixed-size image set: `extract_batch` (ragged batches, one forward per group) against the per-image `extract` loop followed by
`collate_features` — the only correct path for such a set before ragged batches.  Two sets of K = 16 images, alternating 480x640 / 640x480 and
768x1024 / 683x1024; three repeats of every timing.  `--extractor superpoint` (default) runs both conv precisions in one process on seeded noise images;
`--extractor aliked` runs aliked-n16 (exact fp32, max_num_keypoints = 2048) on seeded 3-channel textured images.  `extract_batch` is timed twice: with the
planner's size order (like sizes share a canvas: no padding on these sets) and in input order (every canvas mixes both sizes: the padding share is printed).
`--loop-only` times the loop alone (a build without extract_batch).  One JSON line per timing on stdout.

The front end (everything in front of the extractor's `forward`): `--source u8hwc` feeds uint8 RGB channels-last photos generated on the device from a seed instead
of float32 images at their final size, `--resize N` extracts with `resize=N`, and `--sets` picks among the two sets above (the default) and two photo workflows:
`photo` (K = 16, 1536x2048 / 2048x1536, u8hwc, resize 1024) and `vga-rgb` (480x640 / 640x480, u8hwc, no resize).  Per set one more line, mode "front_end", with
`front_end_ms`: the preprocessing of the planned groups alone (`ImagePreprocessor.to_canvas` per group; `--front-end per-image`: the per-image resize, gray
conversion and canvas copy of a build without to_canvas), timed with device events.  `--count-front-end` instead runs that front end once under the torch
profiler and prints its kernel launches and host-to-device copies."""
import argparse, json, sys, time
from pathlib import Path
import torch
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tools"))
from lightglue_amd import collate_features

SETS = {"480x640+640x480": [(480, 640), (640, 480)] * 8, "768x1024+683x1024": [(768, 1024), (683, 1024)] * 8,
        "photo": [(1536, 2048), (2048, 1536)] * 8, "vga-rgb": [(480, 640), (640, 480)] * 8}
DEFAULT_SETS = ("480x640+640x480", "768x1024+683x1024")
SET_DEFAULTS = {"photo": ("u8hwc", 1024), "vga-rgb": ("u8hwc", None)}      # (source, resize) a named workflow implies


def photos(sizes):
    """uint8 RGB channels-last photos, [3, h, w] views of [h, w, 3] arrays, generated on the device from a seed"""
    g = torch.Generator(device="cuda").manual_seed(0)
    return [torch.randint(0, 256, (h, w, 3), device="cuda", dtype=torch.uint8, generator=g).permute(2, 0, 1) for h, w in sizes]


def front_end(model, images, batch_size, conf, how):
    """the callable that preprocesses the planned groups of `images` and nothing else: what extract_batch does in front of its forward calls"""
    from lightglue_amd import ImagePreprocessor, plan_image_batches
    prep = ImagePreprocessor(**{**model.preprocess_conf, **conf})
    gray = type(model).__name__ == "SuperPoint"
    if how == "to_canvas":
        plans = prep.plan_images([tuple(i.shape[-2:]) for i in images])
        groups = plan_image_batches([(p.h_out, p.w_out) for p in plans], batch_size)
        return lambda: [prep.to_canvas([images[i] for i in idx], channels=1 if gray else None, canvas_size=size) for idx, size in groups]
    def per_image():
        ready = []
        for img in images:
            out, _ = prep(img[None])
            if gray and out.shape[1] == 3:
                out = 0.299 * out[:, 0:1] + 0.587 * out[:, 1:2] + 0.114 * out[:, 2:3]
            ready.append(out.to(torch.float32))
        canvases = []
        for idx, (hc, wc) in plan_image_batches([tuple(t.shape[-2:]) for t in ready], batch_size):
            canvas = torch.zeros((len(idx), max(ready[i].shape[1] for i in idx), hc, wc), device="cuda", dtype=torch.float32)
            for r, i in enumerate(idx):
                h, w = ready[i].shape[-2:]
                canvas[r, :, :h, :w].copy_(ready[i][0])
            canvases.append(canvas)
        return canvases
    return per_image


def event_timed(fn, warmup, iters):
    """ms per call between two device events"""
    for _ in range(warmup): fn()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); start.record()
    for _ in range(iters): fn()
    stop.record(); torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters


def count_device_activity(fn):
    from torch.profiler import ProfilerActivity, profile
    fn(); torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        fn(); torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return {"kernels": len([n for n in names if "Memcpy" not in n and "Memset" not in n]), "memcpy_h2d": len([n for n in names if "Memcpy HtoD" in n]),
            "memcpy_other": len([n for n in names if "Memcpy" in n and "HtoD" not in n]), "memset": len([n for n in names if "Memset" in n])}


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
    ap.add_argument("--sets", nargs="+", choices=sorted(SETS), default=list(DEFAULT_SETS))
    ap.add_argument("--source", choices=("f32", "u8hwc"), default=None, help="default: f32 (the extractor's seeded images), u8hwc for the sets photo and vga-rgb")
    ap.add_argument("--resize", type=int, default=None, help="default: none, 1024 for the set photo")
    ap.add_argument("--front-end", choices=("to_canvas", "per-image"), default="to_canvas"); ap.add_argument("--count-front-end", action="store_true")
    ap.add_argument("--skip-loop", action="store_true", help="leave out the per-image extract loop")
    a = ap.parse_args()
    for prec, model, make_images in configurations(a.extractor):
        for name in a.sets:
            sizes = SETS[name]
            source = a.source or SET_DEFAULTS.get(name, ("f32", None))[0]
            resize = a.resize if a.resize is not None else SET_DEFAULTS.get(name, ("f32", None))[1]
            conf = {} if resize is None else {"resize": resize}
            images = photos(sizes) if source == "u8hwc" else make_images(sizes)
            base = {"extractor": a.extractor, "precision": prec, "set": name}
            if source != "f32" or resize is not None:
                base.update({"source": source, "resize": resize})
            if not a.loop_only:
                fe = front_end(model, images, a.batch_size, conf, a.front_end)
                if a.count_front_end:
                    print(json.dumps({**base, "mode": f"front_end[{a.front_end}]", **count_device_activity(fe)}), flush=True)
                    continue
                for rep in range(a.repeats):
                    print(json.dumps({**base, "mode": f"front_end[{a.front_end}]", "repeat": rep, "front_end_ms": round(event_timed(fe, a.warmup, a.iters), 4)}), flush=True)
            modes = {} if a.skip_loop else {"loop": lambda: collate_features([model.extract(i, **conf) for i in images])}
            if not a.loop_only:
                from lightglue_amd import plan_image_batches
                for order in ("size", "input"):
                    if resize is not None:      # the canvases hold the resized images
                        from lightglue_amd.preprocess import make_plan
                        planned = [(p.h_out, p.w_out) for p in (make_plan(h, w, resize) for h, w in sizes)]
                    else:
                        planned = sizes
                    plan = plan_image_batches(planned, a.batch_size, order=order)
                    pad = 1.0 - sum(h * w for h, w in planned) / sum(len(idx) * hc * wc for idx, (hc, wc) in plan)
                    modes[f"extract_batch[{order}]"] = (lambda order=order: model.extract_batch(images, batch_size=a.batch_size, order=order, **conf))
                    modes[f"extract_batch[{order}]"].padding = pad
            for mode, fn in modes.items():
                for rep in range(a.repeats):
                    dt = timed(fn, a.warmup, a.iters)
                    print(json.dumps({**base, "mode": mode, "repeat": rep, "ms_per_set": round(dt * 1e3, 3),
                                      "images_per_s": round(len(images) / dt, 1), "canvas_padding": round(getattr(fn, "padding", 0.0), 4)}), flush=True)


if __name__ == "__main__":
    main()
