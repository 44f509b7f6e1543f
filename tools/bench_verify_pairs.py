#!/usr/bin/env python3
"""`TwoViewVerifier.verify_pairs` (lg_twoview_verify: compaction, hypotheses, finalise; one call, one host synchronisation) next to the `match_pairs` call whose
result it verifies, and next to the only route there was without it: `matches0` copied to the host and a CPU RANSAC per pair.

Workload: a store of K = 16 views x N = 2 048 keypoints of one 3-D point cloud (30 % of every view's rows replaced by unrelated ones), the 120 exhaustive pairs.
Matchers: `NearestNeighborMatcher` (mutual, ratio 0.8) and `LightGlue` with synthetic weights (recipe A, f16x3, fixed depth).  Per matcher: the wall-clock ms of
`match_pairs` on the list, then of `verify_pairs` on its result for both models x num_hypotheses 256 / 1 024 / 4 096 x refine on / off (synchronised before
and after, one warm-up each, the configurations visited in turn `--runs` times: median and range), and the inliers found.  The host route is the float32
restatement of the same definition (tests/twoview_oracle.py, numpy) over the pairs on `--threads` CPU threads after one device-to-host copy of `matches0`,
timed once per model at `--host-hypotheses` (refine on).  One JSON line per matcher.

usage: bench_verify_pairs.py [--images 16] [--kpts 2048] [--runs 5] [--threads 16] [--host-hypotheses 1024] [--no-host] [--no-lightglue]"""
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
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import gpu_util
import twoview_oracle as O
from lightglue_amd import NearestNeighborMatcher, TwoViewVerifier
from lightglue_amd import synthetic as synth

T = 3.0


def make_store(K, N, dim=256, seed=0):
    """K views of one cloud of N 3-D points: view k is camera k's projection (640 x 480, focal 500, small rotations about a common centre) in a permuted row
    order, descriptors the cloud's rows with 30 % noise; 30 % of a view's rows are unrelated keypoints with unrelated descriptors"""
    rng = np.random.default_rng(seed)
    X = rng.uniform([-2.5, -1.8, 4.0], [2.5, 1.8, 8.0], (N, 3))
    base = rng.standard_normal((N, dim))
    Kc = np.array([[500.0, 0, 320.0], [0, 500.0, 240.0], [0, 0, 1.0]])
    kpts, desc = np.empty((K, N, 2), np.float32), np.empty((K, N, dim), np.float32)
    for k in range(K):
        a, b = rng.uniform(-0.15, 0.15, 2)
        Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
        p = (X @ (Ry @ Rx).T + rng.uniform(-0.6, 0.6, 3)) @ Kc.T
        x = p[:, :2] / p[:, 2:] + rng.normal(0, 0.5, (N, 2))
        d = base + 0.3 * rng.standard_normal((N, dim))
        rep = rng.random(N) < 0.3
        x[rep], d[rep] = rng.uniform([0, 0], [640, 480], (int(rep.sum()), 2)), rng.standard_normal((int(rep.sum()), dim))
        order = rng.permutation(N)
        kpts[k], desc[k] = x[order], (d / np.linalg.norm(d, axis=1, keepdims=True))[order]
    size = np.tile(np.array([[640.0, 480.0]], np.float32), (K, 1))
    return {"keypoints": torch.from_numpy(kpts).cuda(), "descriptors": torch.from_numpy(desc).cuda(), "image_size": torch.from_numpy(size).cuda()}


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def stats(ms):
    return {"ms_median": round(statistics.median(ms), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3)}


def host_route(kind, store, pairs, result, hyps, threads):
    """what there was without the verifier: matches0 to the host, then the same definition in float32 numpy, pair by pair on a thread pool"""
    kpts = store["keypoints"].cpu().numpy()

    def one(item):
        (i, j), m0 = item
        rows, corr = O.correspondences(kpts[i], kpts[j], m0)
        return O.verify(kind, corr, T, hyps, 0, True, np.float32)["count"]
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
    ap.add_argument("--host-hypotheses", type=int, default=1024)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-lightglue", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_verify_pairs.py measures on an MI355X; there is nothing to measure without one")
    store = make_store(args.images, args.kpts)
    pairs = list(itertools.combinations(range(args.images), 2))
    pairs_dev = torch.tensor(pairs, device="cuda")
    matchers = {"nn": NearestNeighborMatcher(ratio_threshold=0.8)}
    if not args.no_lightglue:
        matchers["lightglue"] = gpu_util.make_model(synth.make_state_dict(0, recipe="A"), "f16x3", depth_confidence=-1, width_confidence=-1)
    configs = list(itertools.product(("homography", "fundamental"), (256, 1024, 4096), (False, True)))
    for name, matcher in matchers.items():
        match = lambda: matcher.match_pairs(store, pairs_dev, validate=False)
        result = match()
        verifiers = {c: TwoViewVerifier(model=c[0], threshold=T, num_hypotheses=c[1], refine=c[2]) for c in configs}
        runs = {c: (lambda v=v: v.verify_pairs(store, pairs_dev, result, validate=False)) for c, v in verifiers.items()}
        outs = {c: fn() for c, fn in runs.items()}                              # warm-up of every timed shape
        ms, match_ms = {c: [] for c in configs}, []
        for _ in range(args.runs):
            match_ms.append(timed(match)[0])
            for c, fn in runs.items():                                          # in turn, not back to back
                ms[c].append(timed(fn)[0])
        res = {"matcher": name, "images": args.images, "kpts": args.kpts, "pairs": len(pairs), "device": torch.cuda.get_device_name(0), "runs": args.runs,
               "matched_per_pair": round(float((result["matches0"] > -1).sum()) / len(pairs), 1), "match_pairs": stats(match_ms), "verify_pairs": []}
        med_match = statistics.median(match_ms)
        for c in configs:
            row = {"model": c[0], "num_hypotheses": c[1], "refine": c[2], **stats(ms[c]), "inliers_per_pair": round(float(outs[c]["num_inliers"].sum()) / len(pairs), 1)}
            row["share_of_match_pairs"] = round(row["ms_median"] / med_match, 4)
            res["verify_pairs"].append(row)
        if not args.no_host:
            res["host"] = []
            for kind in ("homography", "fundamental"):
                host_ms, counts = host_route(kind, store, pairs, result, args.host_hypotheses, args.threads)
                dev = statistics.median(ms[(kind, args.host_hypotheses, True)]) if (kind, args.host_hypotheses, True) in ms else None
                res["host"].append({"model": kind, "num_hypotheses": args.host_hypotheses, "refine": True, "threads": args.threads, "ms": round(host_ms, 1),
                                    "inliers_per_pair": round(sum(counts) / len(pairs), 1), "factor_over_device": None if dev is None else round(host_ms / dev, 1)})
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
