#!/usr/bin/env python3
"""`NearestNeighborMatcher.match_pairs` (lg_nn_match: the similarity matrix is never written) against the torch formulation a caller had to write without it, on
the same box: per chunk of `--chunk` pairs `index_select` both sides out of the store, widen / RootSIFT / normalise, `bmm` into the [chunk, N, N] fp32 similarity
tensor, one `topk(2)` per direction, ratio test and mutual check.

Workload: a store of K = 16 images x N = 2 048 rows, the exhaustive pair list (120 pairs), mutual nearest neighbour with ratio 0.8; per configuration
(dim, store dtype) in {128, 256} x {f32, f16, u8 + rootsift}.  Per configuration and route: wall-clock ms for the whole list (synchronised before and after,
one warm-up call each, the two routes ALTERNATING, `--runs` repeats: median and range), peak device memory of one call above what was allocated before it, and
the number of GPU kernels of one call (torch.profiler; `null` where the profiler gives none).  `agree` is the share of rows on which both routes return the same
match (they differ where two similarities tie within fp32 round-off: the torch route sums in another order).  One JSON line per configuration.

usage: bench_nn_matcher.py [--images 16] [--kpts 2048] [--chunk 32] [--runs 3] [--dims 128 256] [--dtypes f32 f16 u8] [--no-kernel-count]"""
import argparse
import itertools
import json
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from lightglue_amd import NearestNeighborMatcher

RATIO = 0.8


def make_store(K, N, dim, dtype, seed=0):
    """K views of one scene: permutations of the same N unit rows with 45 % noise, 30 % of them replaced by unrelated rows"""
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(N, dim, generator=g)
    out = torch.empty(K, N, dim)
    for k in range(K):
        x = base[torch.randperm(N, generator=g)] + 0.45 * torch.randn(N, dim, generator=g)
        rep = torch.rand(N, generator=g) < 0.3
        x[rep] = torch.randn(int(rep.sum()), dim, generator=g)
        out[k] = x
    if dtype == "u8":
        out = out.abs()
        return (out / out.norm(dim=-1, keepdim=True) * 512).round().clamp(0, 255).to(torch.uint8).cuda()
    out = out / out.norm(dim=-1, keepdim=True)
    return out.cuda().to(torch.float16 if dtype == "f16" else torch.float32)


def torch_route(desc, pairs_dev, chunk, rootsift):
    """the formulation without the matcher: everything a [chunk, N, N] similarity tensor needs"""
    m0s, m1s = [], []
    for start in range(0, pairs_dev.shape[0], chunk):
        idx = pairs_dev[start:start + chunk]
        sides = []
        for s in (0, 1):
            x = desc.index_select(0, idx[:, s].contiguous()).float()
            if rootsift:
                x = torch.nn.functional.normalize(x, p=1, dim=-1, eps=1e-6).clip_(min=1e-6).sqrt_()
            sides.append(torch.nn.functional.normalize(x, dim=-1))
        sim = torch.bmm(sides[0], sides[1].transpose(1, 2))
        raw = []
        for d in (2, 1):
            top, arg = sim.topk(2, dim=d)
            s1, s2 = top.select(d, 0), top.select(d, 1)
            keep = (2 * (1 - s1)).clamp_(min=0) <= RATIO * RATIO * (2 * (1 - s2)).clamp_(min=0)
            raw.append(torch.where(keep, arg.select(d, 0), -1))
        r0, r1 = raw
        back0 = torch.gather(r1, 1, r0.clamp(min=0))
        back1 = torch.gather(r0, 1, r1.clamp(min=0))
        ar0, ar1 = torch.arange(r0.shape[1], device=r0.device), torch.arange(r1.shape[1], device=r1.device)
        m0s.append(torch.where((r0 >= 0) & (back0 == ar0), r0, -1))
        m1s.append(torch.where((r1 >= 0) & (back1 == ar1), r1, -1))
    return torch.cat(m0s), torch.cat(m1s)


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def peak_above_baseline(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    del out
    return torch.cuda.max_memory_allocated() - before


def kernel_count(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA"))
        return n or None
    except Exception as exc:      # no profiler on this build: the count stays unmeasured, the timings stand
        print(f"kernel count not measured: {exc!r}", file=sys.stderr)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--kpts", type=int, default=2048)
    ap.add_argument("--chunk", type=int, default=32)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--dims", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--dtypes", nargs="+", default=["f32", "f16", "u8"], choices=["f32", "f16", "u8"])
    ap.add_argument("--no-kernel-count", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_nn_matcher.py measures on an MI355X; there is nothing to measure without one")
    pairs = list(itertools.combinations(range(args.images), 2))
    pairs_dev = torch.tensor(pairs, device="cuda")
    matcher = NearestNeighborMatcher(ratio_threshold=RATIO)
    for dim, dtype in itertools.product(args.dims, args.dtypes):
        desc = make_store(args.images, args.kpts, dim, dtype)
        rootsift = dtype == "u8"
        feats = {"descriptors": desc, "descriptor_transform": "rootsift" if rootsift else None}
        routes = {"fused": lambda: matcher.match_pairs(feats, pairs_dev, validate=False),
                  "torch": lambda: torch_route(desc, pairs_dev, args.chunk, rootsift)}
        outs = {name: fn() for name, fn in routes.items()}          # warm-up of every shape of the timed window
        ms = {name: [] for name in routes}
        for _ in range(args.runs):
            for name, fn in routes.items():                         # alternating
                ms[name].append(timed(fn)[0])
        agree = float((outs["fused"]["matches0"] == outs["torch"][0]).float().mean())
        res = {"dim": dim, "store": dtype + ("+rootsift" if rootsift else ""), "images": args.images, "kpts": args.kpts, "pairs": len(pairs), "chunk": args.chunk,
               "device": torch.cuda.get_device_name(0), "store_bytes": desc.numel() * desc.element_size(), "agree": round(agree, 6),
               "matched": int((outs["fused"]["matches0"] > -1).sum())}
        del outs
        for name, fn in routes.items():
            res[name] = {"ms_median": round(statistics.median(ms[name]), 3), "ms_min": round(min(ms[name]), 3), "ms_max": round(max(ms[name]), 3),
                         "peak_bytes": peak_above_baseline(fn), "kernels": None if args.no_kernel_count else kernel_count(fn)}
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
