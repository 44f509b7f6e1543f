#!/usr/bin/env python3
"""`RelativePoseEstimator.estimate_pairs` (lg_relpose_estimate: compaction, solve, score, finalise; one call, one host synchronisation) next to what a
calibrated user ran before it — `TwoViewVerifier(model="fundamental")` at the same budgets, followed by a host-side decomposition that is not timed here —,
next to the `match_pairs` calls whose result it reads, and next to the float64 numpy definition on the host.

Workload: tools/bench_verify_pairs.py's store (K = 16 views x N = 2 048 keypoints of one 3-D point cloud, camera (500, 500, 320, 240), 30 % of every view's rows
replaced by unrelated ones) and its 120 exhaustive pairs, matched by `NearestNeighborMatcher` (mutual, ratio 0.8).  Per num_hypotheses 256 / 1 024 / 4 096 x
refine on / off: the wall-clock ms of `estimate_pairs` and of the fundamental `verify_pairs` on the matcher's result (synchronised before and after, one
warm-up each, the configurations visited in turn `--runs` times: median and range), inliers and points in front per pair.  `match_pairs` of both matchers
on the same list.  The host route is tests/relpose_oracle.py (float64)
over the pairs on `--threads` CPU threads after one device-to-host copy of `matches0`, timed once at `--host-hypotheses` (refine on).  One JSON line.
The split over the four launches is read from a kernel trace of `--only-pose` (profiles/relative_pose.md says how).

usage: bench_relative_pose.py [--images 16] [--kpts 2048] [--runs 5] [--threads 16] [--host-hypotheses 256] [--no-host] [--no-lightglue] [--only-pose]"""
import argparse
import itertools
import json
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests")); sys.path.insert(0, str(ROOT / "tools"))
import gpu_util
import relpose_oracle as P
from bench_verify_pairs import make_store, stats, timed
from lightglue_amd import NearestNeighborMatcher, RelativePoseEstimator, TwoViewVerifier
from lightglue_amd import synthetic as synth

T = 3.0
CAMERA = (500.0, 500.0, 320.0, 240.0)


def host_route(store, pairs, result, hyps, threads):
    """matches0 to the host, then the float64 definition, pair by pair on a thread pool"""
    kpts = store["keypoints"].cpu().numpy()

    def one(item):
        (i, j), m0 = item
        rows, corr = P.correspondences(kpts[i], kpts[j], m0)
        return P.verify(corr, CAMERA, CAMERA, T, hyps, 0, True)["count"]
    t = time.perf_counter()
    m0 = result["matches0"].cpu().numpy()
    with ThreadPoolExecutor(threads) as pool:
        counts = list(pool.map(one, zip(pairs, m0)))
    return (time.perf_counter() - t) * 1e3, counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--kpts", type=int, default=2048)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--host-hypotheses", type=int, default=256)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-lightglue", action="store_true")
    ap.add_argument("--only-pose", action="store_true", help="one estimate_pairs call per configuration and nothing else: the run to put under a kernel trace")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_relative_pose.py measures on an MI355X; there is nothing to measure without one")
    store = make_store(args.images, args.kpts)
    pairs = list(itertools.combinations(range(args.images), 2))
    pairs_dev = torch.tensor(pairs, device="cuda")
    cameras = torch.tensor([CAMERA] * args.images, device="cuda")
    nn = NearestNeighborMatcher(ratio_threshold=0.8)
    match = lambda: nn.match_pairs(store, pairs_dev, validate=False)
    result = match()
    configs = list(itertools.product((256, 1024, 4096), (False, True)))
    poses = {c: RelativePoseEstimator(threshold=T, num_hypotheses=c[0], refine=c[1]) for c in configs}
    verifiers = {c: TwoViewVerifier(model="fundamental", threshold=T, num_hypotheses=c[0], refine=c[1]) for c in configs}
    run_pose = {c: (lambda e=e: e.estimate_pairs(store, pairs_dev, result, cameras, validate=False)) for c, e in poses.items()}
    run_f = {c: (lambda v=v: v.verify_pairs(store, pairs_dev, result, validate=False)) for c, v in verifiers.items()}
    outs = {c: fn() for c, fn in run_pose.items()}                              # warm-up of every timed shape
    if args.only_pose:
        for c, fn in run_pose.items():
            print(json.dumps({"num_hypotheses": c[0], "refine": c[1], "ms": round(timed(fn)[0], 3)}), flush=True)
        return
    outs_f = {c: fn() for c, fn in run_f.items()}
    ms, ms_f, match_ms, lg_ms = {c: [] for c in configs}, {c: [] for c in configs}, [], []
    lg = None if args.no_lightglue else gpu_util.make_model(synth.make_state_dict(0, recipe="A"), "f16x3", depth_confidence=-1, width_confidence=-1)
    lg_match = None if lg is None else (lambda: lg.match_pairs(store, pairs_dev, validate=False))
    if lg_match:
        lg_match()
    for _ in range(args.runs):
        match_ms.append(timed(match)[0])
        if lg_match:
            lg_ms.append(timed(lg_match)[0])
        for c in configs:                                                       # in turn, not back to back
            ms[c].append(timed(run_pose[c])[0])
            ms_f[c].append(timed(run_f[c])[0])
    res = {"images": args.images, "kpts": args.kpts, "pairs": len(pairs), "device": torch.cuda.get_device_name(0), "runs": args.runs,
           "matched_per_pair": round(float((result["matches0"] > -1).sum()) / len(pairs), 1), "nn_match_pairs": stats(match_ms),
           "lightglue_match_pairs": stats(lg_ms) if lg_ms else None, "estimate_pairs": [], "verify_pairs_fundamental": []}
    for c in configs:
        o = outs[c]
        res["estimate_pairs"].append({"num_hypotheses": c[0], "refine": c[1], **stats(ms[c]), "inliers_per_pair": round(float(o["num_inliers"].sum()) / len(pairs), 1),
                                      "in_front_per_pair": round(float(o["num_in_front"].sum()) / len(pairs), 1),
                                      "ratio_to_verify_pairs": round(statistics.median(ms[c]) / statistics.median(ms_f[c]), 3)})
        res["verify_pairs_fundamental"].append({"num_hypotheses": c[0], "refine": c[1], **stats(ms_f[c]),
                                                "inliers_per_pair": round(float(outs_f[c]["num_inliers"].sum()) / len(pairs), 1)})
    if not args.no_host:
        host_ms, counts = host_route(store, pairs, result, args.host_hypotheses, args.threads)
        dev = statistics.median(ms[(args.host_hypotheses, True)]) if (args.host_hypotheses, True) in ms else None
        res["host"] = {"num_hypotheses": args.host_hypotheses, "refine": True, "threads": args.threads, "ms": round(host_ms, 1),
                       "inliers_per_pair": round(sum(counts) / len(pairs), 1), "factor_over_device": None if dev is None else round(host_ms / dev, 1)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
