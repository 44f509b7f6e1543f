#!/usr/bin/env python3
"""A pair list over a device feature store: `LightGlue.match_pairs` (the engine reads every pair's rows in the store, LG_FLAG_INDEXED) against the stacked
route a caller had to write before it — per batch of `--batch` pairs, `index_select` the two sides out of the store, then `forward`.  Workload: the exhaustive
pair list over K synthetic images of one scene (K = 32: 496 pairs), N keypoints each, 256-d descriptors, fixed depth, pruning off (the matcher of bench.py's
headline configuration).  Both routes produce the same bits (checked once); the figures are wall-clock ms for the whole list, median and range of `--runs` runs.

match_pairs is timed twice: with `max_rows_per_call` lowered to the stacked route's batch (same workspace, same number of engine calls, minus the stacking
and all but one host synchronisation) and, unless --no-uncapped, with the engine's own envelope (the whole list in as few calls as fit).

--store-dtype f16 keeps the store's descriptors as float16 (read in place, LG_FLAG_DESC0_F16 / _DESC1_F16; the stacked route then gathers float16 rows); the last
lines report the store's bytes and the peak device memory of one match_pairs call above what was allocated before it.

usage: bench_match_pairs.py [--images 32] [--kpts 1024] [--batch 32] [--runs 3] [--no-uncapped] [--store-dtype f32|f16]"""
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
    ap.add_argument("--store-dtype", default="f32", choices=["f32", "f16"], help="element type of the store's descriptors")
    a = ap.parse_args()
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
