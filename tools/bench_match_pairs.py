#!/usr/bin/env python3
"""A pair list over a device feature store: `LightGlue.match_pairs` (the engine reads every pair's rows in the store, LG_FLAG_INDEXED) against the stacked
route a caller had to write before it — per batch of `--batch` pairs, `index_select` the two sides out of the store, then `forward`.  Workload: the exhaustive
pair list over K synthetic images of one scene (K = 32: 496 pairs), N keypoints each, 256-d descriptors, fixed depth, pruning off (the matcher of bench.py's
headline configuration).  Both routes produce the same bits (checked once); the figures are wall-clock ms for the whole list, median and range of `--runs` runs.

match_pairs is timed twice: with `max_rows_per_call` lowered to the stacked route's batch (same workspace, same number of engine calls, minus the stacking
and all but one host synchronisation) and, unless --no-uncapped, with the engine's own envelope (the whole list in as few calls as fit).

--store-dtype f16 keeps the store's descriptors as float16 (read in place, LG_FLAG_DESC0_F16 / _DESC1_F16; the stacked route then gathers float16 rows); the last
lines report the store's bytes and the peak device memory of one match_pairs call above what was allocated before it.

--features sift is a workload of its own: a SIFT store as COLMAP / OpenCV write it (128-d uint8 descriptors, scales, oris), matched by
LightGlue(input_dim = 128, add_scale_ori) over the exhaustive pair list in two ways — (a) the route a caller had before uint8 stores: RootSIFT as the reference's
torch expression on `store.float()`, then match_pairs on the fp32 result; (b) --store-dtype u8 --descriptor-transform rootsift: match_pairs on the uint8 store
itself, transformed where the engine reads it.  Reported: ms per list (the transform of (a) included: it is paid per list unless a second, 4 x larger store is
kept), bytes of the resident store, and the framework kernels in front of the engine's first launch.  The two routes differ in summation order inside RootSIFT
(1e-7-class descriptor differences), so their outputs are compared by count, not bit for bit.

usage: bench_match_pairs.py [--images 32] [--kpts 1024] [--batch 32] [--runs 3] [--no-uncapped] [--store-dtype f32|f16|u8] [--features superpoint|sift]
                            [--descriptor-transform none|rootsift]"""
import argparse
import itertools
import json
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import gpu_util
from lightglue_amd import synthetic as synth


def make_store(K, N, seed=0, dim=256, dtype=torch.float32):
    """K views of one synthetic scene: every image a jittered permutation of the same N keypoints with 5 % descriptor noise, so that pairs match."""
    g = torch.Generator().manual_seed(seed)
    base_k = torch.rand(N, 2, generator=g) * torch.tensor([1024.0, 768.0])
    base_d = torch.nn.functional.normalize(torch.randn(N, dim, generator=g), dim=-1)
    kpts, desc = torch.empty(K, N, 2), torch.empty(K, N, dim)
    for i in range(K):
        perm = torch.randperm(N, generator=g)
        kpts[i] = base_k[perm] + 2.0 * torch.randn(N, 2, generator=g)
        desc[i] = torch.nn.functional.normalize(base_d[perm] + 0.05 * torch.randn(N, dim, generator=g), dim=-1)
    size = torch.tensor([[1024.0, 768.0]]).expand(K, 2).contiguous()
    return {"keypoints": kpts.cuda(), "descriptors": desc.cuda().to(dtype), "image_size": size.cuda()}


def stacked_route(model, store, pairs_dev, batch):
    """Today's public route: per batch, gather both sides out of the store (three index_select per side), then one forward."""
    outs = []
    for start in range(0, pairs_dev.shape[0], batch):
        idx = pairs_dev[start:start + batch]
        i0, i1 = idx[:, 0].contiguous(), idx[:, 1].contiguous()
        outs.append(model({"image0": {k: v.index_select(0, i0) for k, v in store.items()}, "image1": {k: v.index_select(0, i1) for k, v in store.items()}}))
    return outs


def make_sift_store(K, N, seed=0, dim=128):
    """K views of one scene in the stored SIFT format: uint8 descriptors (sparse: most bins small, a few large), scales, oris."""
    g = torch.Generator().manual_seed(seed)
    base_k = torch.rand(N, 2, generator=g) * torch.tensor([1024.0, 768.0])
    base_d = (torch.randn(N, dim, generator=g).abs() ** 3 * 12.0).clamp(0, 255)
    kpts, desc = torch.empty(K, N, 2), torch.empty(K, N, dim, dtype=torch.uint8)
    for i in range(K):
        perm = torch.randperm(N, generator=g)
        kpts[i] = base_k[perm] + 2.0 * torch.randn(N, 2, generator=g)
        desc[i] = (base_d[perm] + 2.0 * torch.randn(N, dim, generator=g)).clamp(0, 255).to(torch.uint8)
    size = torch.tensor([[1024.0, 768.0]]).expand(K, 2).contiguous()
    scales, oris = 1.0 + 4.0 * torch.rand(K, N, generator=g), (torch.rand(K, N, generator=g) * 2 - 1) * 3.14159
    return {"keypoints": kpts.cuda(), "descriptors": desc.cuda(), "image_size": size.cuda(), "scales": scales.cuda(), "oris": oris.cuda()}


def torch_rootsift(x, eps=1e-6):
    """RootSIFT in framework kernels, what a caller ran before the engine could: L1-normalise, clip, sqrt, L2-normalise."""
    l1 = x.abs().sum(dim=-1, keepdim=True).clamp_min(eps)
    root = (x / l1).clamp_min(eps).sqrt()
    return root / root.norm(dim=-1, keepdim=True).clamp_min(eps)


def kernels_in_front(call):
    """(framework kernels launched before the engine's first one, engine kernels) of one call, as the profiler sees them."""
    from torch.profiler import ProfilerActivity, profile
    call(); torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        call(); torch.cuda.synchronize()
    ev = sorted((e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "Memcpy" not in e.name and "Memset" not in e.name),
                key=lambda e: e.time_range.start)
    names = [e.name for e in ev]
    first = next((i for i, n in enumerate(names) if "lg::" in n), len(names))
    return names[:first], sum("lg::" in n for n in names)


def sift_main(a):
    K, N = a.images, a.kpts
    model = gpu_util.make_model(synth.make_state_dict(0, input_dim=128, add_scale_ori=True, recipe="A"), "f16x3", input_dim=128, add_scale_ori=True,
                                depth_confidence=-1, width_confidence=-1)
    store = make_sift_store(K, N)
    pairs_dev = torch.tensor(list(itertools.combinations(range(K), 2)), device="cuda")
    P = int(pairs_dev.shape[0])
    nbytes = lambda st: sum(v.numel() * v.element_size() for v in st.values() if torch.is_tensor(v))
    res = {"features": "sift", "images": K, "kpts": N, "pairs": P, "runs": a.runs, "device": torch.cuda.get_device_name(0)}
    route_a = lambda: model.match_pairs({**store, "descriptors": torch_rootsift(store["descriptors"].float())}, pairs_dev, validate=False)
    tagged = {**store, "descriptor_transform": "rootsift"}
    route_b = lambda: model.match_pairs(tagged, pairs_dev, validate=False)
    rows = []
    for name, route, st in (("(a) torch RootSIFT on store.float(), then match_pairs", route_a, {**store, "descriptors": store["descriptors"].float()}),
                            ("(b) uint8 store, descriptor_transform = rootsift", route_b, store)):
        t, out = timed(route, a.runs)
        front, ours = kernels_in_front(route)
        rows.append((name, t))
        res[name[:3]] = {"ms": {"median": statistics.median(t), "min": min(t), "max": max(t)}, "resident_store_bytes": nbytes(st),
                         "framework_kernels_in_front": len(front), "engine_kernels": ours, "matches_per_pair": sum(len(x) for x in out["matches"]) / P,
                         "chunks": len(model.last_pair_chunks)}
        print(f"  {name:<60s} median {statistics.median(t):8.2f} ms  (min {min(t):8.2f}, max {max(t):8.2f})  store {nbytes(st) / 2 ** 20:7.1f} MiB  "
              f"framework kernels in front of the engine {len(front)}  matches per pair {res[name[:3]]['matches_per_pair']:.0f}", flush=True)
        del out
    print(json.dumps(res))
    return 0


def timed(fn, runs):
    fn(); torch.cuda.synchronize()                      # warm-up: workspace growth, caches
    times = []
    for _ in range(runs):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(); times.append((time.perf_counter() - t0) * 1e3)
    return times, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--kpts", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=32, help="pairs per forward of the stacked route (and per engine call of the capped match_pairs run)")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--no-uncapped", action="store_true", help="skip the match_pairs run with the engine's own per-call limits (its workspace is about 14 KB per keypoint row of a call)")
    ap.add_argument("--store-dtype", default="f32", choices=["f32", "f16", "u8"], help="element type of the store's descriptors (u8: with --features sift)")
    ap.add_argument("--features", default="superpoint", choices=["superpoint", "sift"], help="sift: 128-d uint8 descriptors with scales / oris, routes (a) and (b) of the docstring")
    ap.add_argument("--descriptor-transform", default="none", choices=["none", "rootsift"], help="rootsift: the store carries descriptor_transform = 'rootsift' (with --features sift)")
    a = ap.parse_args()
    if a.features == "sift":
        if a.store_dtype != "u8" or a.descriptor_transform != "rootsift":
            ap.error("--features sift measures the stored format: pass --store-dtype u8 --descriptor-transform rootsift")
        return sift_main(a)
    if a.store_dtype == "u8" or a.descriptor_transform != "none":
        ap.error("--store-dtype u8 / --descriptor-transform rootsift belong to --features sift")
    K, N, B = a.images, a.kpts, a.batch
    model = gpu_util.make_model(synth.make_state_dict(0, recipe="A"), "f16x3", depth_confidence=-1, width_confidence=-1)
    store = make_store(K, N, dtype=torch.float16 if a.store_dtype == "f16" else torch.float32)
    pairs = list(itertools.combinations(range(K), 2))
    pairs_dev = torch.tensor(pairs, device="cuda")
    P = len(pairs)
    cap = (N + 127) // 128 * 128
    res = {"images": K, "kpts": N, "pairs": P, "batch": B, "runs": a.runs, "store_dtype": a.store_dtype, "device": torch.cuda.get_device_name(0)}
    res["store_bytes"] = sum(v.numel() * v.element_size() for v in store.values())

    t_stack, outs = timed(lambda: stacked_route(model, store, pairs_dev, B), a.runs)
    model.max_rows_per_call = B * 2 * cap
    t_capped, got = timed(lambda: model.match_pairs(store, pairs_dev, validate=False), a.runs)
    res["chunks_capped"] = len(model.last_pair_chunks)
    same = all(torch.equal(torch.cat([o[k] for o in outs]), got[k]) for k in ("matches0", "matches1", "matching_scores0", "matching_scores1"))
    same = same and all(torch.equal(x, y) for x, y in zip(itertools.chain.from_iterable(o["matches"] for o in outs), got["matches"]))
    res["bit_identical"] = bool(same)
    res["matches_per_pair"] = sum(len(x) for x in got["matches"]) / P
    t_host, _ = timed(lambda: model.match_pairs(store, pairs), a.runs)       # the list as a Python sequence, validated on the host
    rows = [("stacked: index_select + forward per batch", t_stack), (f"match_pairs, {res['chunks_capped']} calls (max_rows_per_call = {B * 2 * cap})", t_capped),
            ("match_pairs, same plan, pairs as a validated host list", t_host)]
    if not a.no_uncapped:
        model.max_rows_per_call = None
        t_free, got2 = timed(lambda: model.match_pairs(store, pairs_dev, validate=False), a.runs)
        res["chunks_uncapped"] = len(model.last_pair_chunks)
        res["bit_identical"] = bool(same and torch.equal(got2["matches0"], got["matches0"]) and torch.equal(got2["matching_scores0"], got["matching_scores0"]))
        rows.append((f"match_pairs, {res['chunks_uncapped']} call(s) (the engine's envelope)", t_free))
    # peak device memory of ONE capped match_pairs call over what is allocated in front of it (workspace grown, outputs of the earlier runs released)
    model.max_rows_per_call = B * 2 * cap
    del outs, got
    torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats(); before = torch.cuda.memory_allocated()
    model.match_pairs(store, pairs_dev, validate=False); torch.cuda.synchronize()
    res["match_pairs_peak_bytes_over_start"] = torch.cuda.max_memory_allocated() - before
    print(f"{K} images x {N} keypoints, {P} pairs, {res['matches_per_pair']:.0f} matches per pair, bit-identical routes: {res['bit_identical']}  [{res['device']}]")
    print(f"  store ({a.store_dtype} descriptors) {res['store_bytes'] / 2 ** 20:.1f} MiB; one match_pairs call peaks {res['match_pairs_peak_bytes_over_start'] / 2 ** 20:.1f} MiB above the memory allocated before it")
    for name, t in rows:
        print(f"  {name:<72s} median {statistics.median(t):8.2f} ms  (min {min(t):8.2f}, max {max(t):8.2f})  {P / statistics.median(t) * 1e3:7.0f} pairs/s", flush=True)
    res["ms"] = {name: {"median": statistics.median(t), "min": min(t), "max": max(t)} for name, t in rows}
    print(json.dumps(res))
    return 0 if res["bit_identical"] else 1


if __name__ == "__main__":
    sys.exit(main())
