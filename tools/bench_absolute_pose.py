#!/usr/bin/env python3
"""`AbsolutePoseEstimator.estimate_pairs` (lg_abspose_estimate: compaction with centring, solve + score fused, finalise; one call, one host synchronisation),
one problem per pair and pooled by query, next to `RelativePoseEstimator.estimate_pairs` on the same list, next to the `match_pairs` call whose result both
read, and next to the float64 numpy definition on the host.

Workload: tools/bench_verify_pairs.py's store (K = 16 views x N = 2 048 keypoints of one 3-D point cloud, camera (500, 500, 320, 240), 30 % of every view's rows
replaced by unrelated ones) and its 120 exhaustive pairs (i, j), i < j: image i is the query, image j the database image, matched by `NearestNeighborMatcher`
(mutual, ratio 0.8).  The world point of a database keypoint row is the cloud's point it was projected from, moved by (100, -50, 20) so that the centring has
work to do, and NaN on the unrelated rows (`world_points` replays `make_store`'s random stream to know which is which).  Pooled, the 120 pairs are 15 problems of
15 .. 1 pairs.  Per num_hypotheses 256 / 1 024 / 4 096 x refine on / off x per pair / pooled: the wall-clock ms of `estimate_pairs` (synchronised before and
after, one warm-up each, the configurations visited in turn `--runs` times: median and range) and the inliers per pair; the relative pose at the same budgets
in the same loop.  The host route is tests/abspose_oracle.py (float64) over the pairs on `--threads` CPU threads after one device-to-host copy of `matches0`,
timed once at `--host-hypotheses` (refine on, per pair).  One JSON line.

usage: bench_absolute_pose.py [--images 16] [--kpts 2048] [--runs 5] [--threads 16] [--host-hypotheses 256] [--no-host] [--only-pose]"""
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
import abspose_oracle as A
from bench_verify_pairs import make_store, stats, timed
from lightglue_amd import AbsolutePoseEstimator, NearestNeighborMatcher, RelativePoseEstimator

T = 3.0
CAMERA = (500.0, 500.0, 320.0, 240.0)
OFFSET = np.array([100.0, -50.0, 20.0])


def world_points(K, N, dim=256, seed=0):
    """[K, N, 3] float32: the world point behind every keypoint row of make_store(K, N, dim, seed), NaN on the rows it replaced by unrelated keypoints — the
    same random stream drawn again, draw for draw"""
    rng = np.random.default_rng(seed)
    X = rng.uniform([-2.5, -1.8, 4.0], [2.5, 1.8, 8.0], (N, 3))
    rng.standard_normal((N, dim))
    out = np.empty((K, N, 3), np.float32)
    for k in range(K):
        rng.uniform(-0.15, 0.15, 2); rng.uniform(-0.6, 0.6, 3); rng.normal(0, 0.5, (N, 2)); rng.standard_normal((N, dim))
        rep = rng.random(N) < 0.3
        rng.uniform([0, 0], [640, 480], (int(rep.sum()), 2)); rng.standard_normal((int(rep.sum()), dim))
        order = rng.permutation(N)
        out[k] = np.where(rep[:, None], np.nan, X + OFFSET)[order]
    return out


def host_route(store, points, pairs, result, hyps, threads):
    """matches0 to the host, then the float64 definition, pair by pair on a thread pool"""
    kpts = store["keypoints"].cpu().numpy()

    def one(item):
        (i, j), m0 = item
        rows, corr = A.correspondences(kpts[i], points[j], m0)
        return A.verify(corr, CAMERA, T, hyps, 0, True)["count"]
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
    ap.add_argument("--only-pose", action="store_true", help="one estimate_pairs call per configuration and nothing else: the run to put under a kernel trace")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_absolute_pose.py measures on an MI355X; there is nothing to measure without one")
    store = make_store(args.images, args.kpts)
    points_host = world_points(args.images, args.kpts)
    points = torch.from_numpy(points_host).cuda()
    pairs = list(itertools.combinations(range(args.images), 2))
    pairs_dev = torch.tensor(pairs, device="cuda")
    cameras = torch.tensor([CAMERA] * args.images, device="cuda")
    nn = NearestNeighborMatcher(ratio_threshold=0.8)
    match = lambda: nn.match_pairs(store, pairs_dev, validate=False)
    result = match()
    configs = list(itertools.product((256, 1024, 4096), (False, True), (False, True)))          # (hypotheses, refine, pooled)
    ests = {c: AbsolutePoseEstimator(threshold=T, num_hypotheses=c[0], refine=c[1]) for c in configs}
    rels = {c: RelativePoseEstimator(threshold=T, num_hypotheses=c[0], refine=c[1]) for c in configs if not c[2]}
    run_abs = {c: (lambda e=e, pool=c[2]: e.estimate_pairs(store, pairs_dev, result, cameras, points, pool=pool, validate=False)) for c, e in ests.items()}
    run_rel = {c: (lambda e=e: e.estimate_pairs(store, pairs_dev, result, cameras, validate=False)) for c, e in rels.items()}
    outs = {c: fn() for c, fn in run_abs.items()}                               # warm-up of every timed shape
    if args.only_pose:
        for c, fn in run_abs.items():
            print(json.dumps({"num_hypotheses": c[0], "refine": c[1], "pooled": c[2], "ms": round(timed(fn)[0], 3)}), flush=True)
        return
    outs_rel = {c: fn() for c, fn in run_rel.items()}
    ms, ms_rel, match_ms = {c: [] for c in configs}, {c: [] for c in rels}, []
    for _ in range(args.runs):
        match_ms.append(timed(match)[0])
        for c in configs:                                                       # in turn, not back to back
            ms[c].append(timed(run_abs[c])[0])
            if c in run_rel:
                ms_rel[c].append(timed(run_rel[c])[0])
    matched = result["matches0"] > -1
    with_point = matched & torch.isfinite(points[pairs_dev[:, 1, None], result["matches0"].clamp(min=0)]).all(-1)
    res = {"images": args.images, "kpts": args.kpts, "pairs": len(pairs), "device": torch.cuda.get_device_name(0), "runs": args.runs,
           "matched_per_pair": round(float(matched.sum()) / len(pairs), 1), "correspondences_per_pair": round(float(with_point.sum()) / len(pairs), 1),
           "nn_match_pairs": stats(match_ms), "absolute_pose": [], "relative_pose": []}
    for c in configs:
        o = outs[c]
        res["absolute_pose"].append({"num_hypotheses": c[0], "refine": c[1], "pooled": c[2], "problems": int(o["R"].shape[0]), **stats(ms[c]),
                                     "inliers_per_pair": round(float(o["pair_num_inliers"].sum()) / len(pairs), 1),
                                     "ratio_to_relative_pose": round(statistics.median(ms[c]) / statistics.median(ms_rel[(c[0], c[1], False)]), 3)})
        if c in rels:
            res["relative_pose"].append({"num_hypotheses": c[0], "refine": c[1], **stats(ms_rel[c]), "inliers_per_pair": round(float(outs_rel[c]["num_inliers"].sum()) / len(pairs), 1)})
    if not args.no_host:
        host_ms, counts = host_route(store, points_host, pairs, result, args.host_hypotheses, args.threads)
        key = (args.host_hypotheses, True, False)
        dev = statistics.median(ms[key]) if key in ms else None
        res["host"] = {"num_hypotheses": args.host_hypotheses, "refine": True, "threads": args.threads, "ms": round(host_ms, 1),
                       "inliers_per_pair": round(sum(counts) / len(pairs), 1), "factor_over_device": None if dev is None else round(host_ms / dev, 1)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
