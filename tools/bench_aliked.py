#!/usr/bin/env python3
"""ALIKED extractor throughput on one MI355X: images/s of `forward` at 640 x 480 and 1024 x 768 for B = 1 and 8 (aliked-n16, default
conf: threshold 0.2, seeded weights from tools/make_golden_aliked.py), the per-kernel time table of one 1024 x 768 forward, and
images -> matches with a 128-d LightGlue, the configuration of LightGlue(features="aliked") (seeded matcher weights).
    python tools/bench_aliked.py"""
from __future__ import annotations

import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tools"))

import make_golden_aliked as G  # noqa: E402
from lightglue_amd import ALIKED, LightGlue, synthetic as synth  # noqa: E402


def timed(fn, iters=20, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    model = ALIKED(weights=G.aliked_state_dict(0), max_num_keypoints=2048, detection_threshold=0.2).eval().cuda()
    print("| image | B | ms / forward | images / s | keypoints / image |")
    print("|---|---|---|---|---|")
    for h, w in ((480, 640), (768, 1024)):
        for b in (1, 8):
            img = torch.cat([G.aliked_image(s, 1, h, w, 3) for s in range(b)]).cuda()
            out = model({"image": img})
            ms = timed(lambda: model({"image": img}))
            print(f"| {w}x{h} | {b} | {ms:.3f} | {b * 1000 / ms:.0f} | {float(out['num_keypoints'].float().mean()):.0f} |")
    img = G.aliked_image(0, 1, 768, 1024, 3).cuda()
    model({"image": img}); torch.cuda.synchronize()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        model({"image": img}); torch.cuda.synchronize()
    rows = {}
    for e in prof.events():
        if e.device_type == torch.autograd.DeviceType.CUDA:
            t = rows.setdefault(e.name, [0, 0.0]); t[0] += 1; t[1] += e.device_time_total / 1000.0
    print("\nkernels of one 1024x768 forward (B = 1)\n| kernel | calls | ms |\n|---|---|---|")
    for name, (n, ms) in sorted(rows.items(), key=lambda kv: -kv[1][1]):
        print(f"| {name[:90]} | {n} | {ms:.3f} |")
    aten = [n for n in rows if not (n.startswith("void lg::") or n.startswith("lg::") or "ak_" in n or "Memset" in n or "Memcpy" in n or "memcpy" in n.lower())]
    print(f"\nnon-project kernels inside forward: {aten if aten else 'none'}")
    sd = synth.make_state_dict(0, input_dim=128, recipe="A")
    matcher = LightGlue(features=None, input_dim=128, depth_confidence=-1, width_confidence=-1).eval()
    matcher.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    matcher = matcher.cuda()
    for h, w in ((480, 640), (768, 1024)):
        i0, i1 = G.aliked_image(1, 1, h, w, 3).cuda(), G.aliked_image(2, 1, h, w, 3).cuda()

        def pair():
            f0, f1 = model.extract(i0[0]), model.extract(i1[0])
            return matcher({"image0": f0, "image1": f1})
        ms = timed(pair, iters=10)
        print(f"images -> matches {w}x{h}: {ms:.2f} ms per pair ({1000 / ms:.0f} pairs/s)")


if __name__ == "__main__":
    main()
