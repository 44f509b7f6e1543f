#!/usr/bin/env python3
"""ImagePreprocessor on one MI355X: the fused resize kernel (lg_preprocess_resize) against the same definition as a chain of ATen ops
(F.pad reflect, two grouped conv2d, F.interpolate — the reference's own path through kornia, and what a caller had to run before the
kernel existed), same GPU, same process, alternating.

Per shape: HIP-event time per call after warm-up (kernel launches only: plan and output buffer are made once, as a pipeline would), the
source bytes over that time, and that rate as a fraction of the 6.3 TB/s a float4 copy reaches on this chip.  The source rotates over
enough copies to exceed the 256 MB Infinity Cache, so the rate is an HBM rate.  The uint8 rows read a channels-last (H, W, 3) photo in
place; their ATen chain starts with the `.permute(2, 0, 1).float() / 255` a caller would need.  Also printed: the largest difference
between the two outputs, and the wall time of `ImagePreprocessor.__call__` (allocation and the host -> device copy of `scale` included).
    python tools/bench_preprocess.py"""
from __future__ import annotations

import ctypes as C
import sys
import time
from pathlib import Path

import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tools"))

import make_golden_preprocess as GP  # noqa: E402
from lightglue_amd import ImagePreprocessor, _cabi  # noqa: E402
from lightglue_amd.preprocess import make_plan  # noqa: E402

COPY_RATE = 6.3e12   # float4 copy on the MI355X (microarchitecture guide)
SHAPES = (("480x640 gray f32", 1, 480, 640, 512, "float32"), ("1200x1600 RGB f32", 3, 1200, 1600, 1024, "float32"),
          ("3000x4000 RGB f32", 3, 3000, 4000, 1024, "float32"), ("480x640 gray u8", 1, 480, 640, 512, "uint8"),
          ("1200x1600 RGB u8 HWC", 3, 1200, 1600, 1024, "uint8"), ("3000x4000 RGB u8 HWC", 3, 3000, 4000, 1024, "uint8"))


def timed(fns, iters, warmup=5, rounds=3):
    """ms per call of each fn: `rounds` windows of `iters` calls per fn, the fns alternating; the best window of each"""
    for fn in fns:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    best = [float("inf")] * len(fns)
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record(); torch.cuda.synchronize()
            best[i] = min(best[i], a.elapsed_time(b) / iters)
    return best


def image(c, h, w, dtype):
    """a tiled seeded image (the generator's image function at photo sizes would take minutes on the host)"""
    tile = GP.preprocess_image(7, dtype, 1, c, 240, 320).cuda()
    return tile.repeat(1, 1, (h + 239) // 240, (w + 319) // 320)[:, :, :h, :w].contiguous()


def main():
    assert torch.cuda.is_available(), "bench_preprocess needs a GPU"
    lib = _cabi.load()
    print(f"device: {torch.cuda.get_device_name(0)}\n")
    print("| shape -> long side | out | ks | kernel ms | source GB/s | of 6.3 TB/s copy | ATen chain ms | chain / kernel | max abs diff | __call__ wall ms |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for label, c, h, w, resize, dtype in SHAPES:
        base = image(c, h, w, dtype)
        if dtype == "uint8" and c == 3:
            base = base[0].permute(1, 2, 0).contiguous().permute(2, 0, 1)[None]      # an (H, W, 3) photo viewed as [1, 3, H, W]
        nbytes = base.numel() * base.element_size()
        copies = max(2, min(8, -(-512 * 2 ** 20 // nbytes)))
        srcs = [base] + [base.clone(memory_format=torch.preserve_format) for _ in range(copies - 1)]
        assert all(s.stride() == base.stride() for s in srcs)
        plan = make_plan(h, w, resize)
        out = torch.empty((1, c, plan.h_out, plan.w_out), device="cuda")
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        code = _cabi.LG_DTYPE_U8 if dtype == "uint8" else _cabi.LG_DTYPE_F32
        state = {"k": 0, "a": 0}

        def kernel():
            s = srcs[state["k"] % copies]; state["k"] += 1
            _cabi.check(lib.lg_preprocess_resize(s.data_ptr(), code, 1, c, h, w, *s.stride(), C.byref(plan), out.data_ptr(), stream))

        ky = GP._gaussian(plan.ks_y, plan.sigma_y, torch.zeros(1)).cuda() if plan.ks_y > 1 else None
        kx = GP._gaussian(plan.ks_x, plan.sigma_x, torch.zeros(1)).cuda() if plan.ks_x > 1 else None
        res = {}

        def chain():
            s = srcs[state["a"] % copies]; state["a"] += 1
            x = s.float() / 255 if dtype == "uint8" else s
            x = x.reshape(-1, 1, h, w)
            if kx is not None:
                x = F.conv2d(F.pad(x, (plan.ks_x // 2, plan.ks_x // 2, 0, 0), mode="reflect"), kx.view(1, 1, 1, -1))
            if ky is not None:
                x = F.conv2d(F.pad(x, (0, 0, plan.ks_y // 2, plan.ks_y // 2), mode="reflect"), ky.view(1, 1, -1, 1))
            res["y"] = F.interpolate(x, size=(plan.h_out, plan.w_out), mode="bilinear", align_corners=None).reshape(1, c, plan.h_out, plan.w_out)

        iters = 200 if nbytes < 2 ** 24 else 40
        ms_k, ms_a = timed((kernel, chain), iters)
        diff = float((res["y"] - out).abs().max())
        pre = ImagePreprocessor(resize=resize)
        pre(base); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(20):
            pre(srcs[1])
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) / 20 * 1e3
        rate = nbytes / (ms_k * 1e-3)
        print(f"| {label} -> {resize} | {plan.w_out}x{plan.h_out} | {plan.ks_y}x{plan.ks_x} | {ms_k:.4f} | {rate / 1e9:.0f} | {rate / COPY_RATE:.1%} | {ms_a:.4f} | {ms_a / ms_k:.1f}x | "
              f"{diff:.1e} | {wall:.3f} |")
        del srcs, base, out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
