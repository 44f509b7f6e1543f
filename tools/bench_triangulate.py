#!/usr/bin/env python3
"""`Triangulator.triangulate` and `.build_tracks` (lg_triangulate: records, union, flatten, scan, fill, sort + triangulate, number, scatter; one call, one
host synchronisation), on a matcher's raw matches and on the verifier's, next to the `match_pairs` and `verify_pairs` calls whose results they read and next to
the float64 numpy definition on the host.

Workload: tools/bench_verify_pairs.py's store (K = 16 views x N = 2 048 keypoints of one 3-D point cloud, camera (500, 500, 320, 240), 30 % of every view's rows
replaced by unrelated ones) and its 120 exhaustive pairs, matched by `NearestNeighborMatcher` (mutual, ratio 0.8).  The poses are the synthetic ones the store
was projected with (`view_poses` replays `make_store`'s random stream, as does `cloud_points` for the point behind every row).  Per source (raw matches /
verified matches) x refine on / off, and for build_tracks: the wall-clock ms of the call (synchronised before and after, one warm-up each, the configurations
visited in turn `--runs` times: median and range), the tracks per state, and the distance of the triangulated points to the cloud's.  The host route is
tests/triangulate_oracle.py (float64, one thread) after one device-to-host copy of `matches0`, timed once on the verified matches with refine on.  One JSON line.
`--only-triangulate`: one call per configuration and nothing else — the run to put under a kernel trace for the per-launch times.
`--robust` adds the robust mode (lg_triangulate_robust: `--num-hypotheses` per round, `--max-tracks` rounds per component, refine on) on either source, next to
the plain calls of the same job, with its outliers and split components.  `--contaminate F` replaces the fraction F of every source's matches by wrong rows
(a seeded choice of the matched rows, each sent to a uniformly drawn row of the other image) before anything is triangulated: what a mode keeps of a list
with wrong matches in it.  The host route is skipped on a contaminated list.

usage: bench_triangulate.py [--images 16] [--kpts 2048] [--runs 5] [--no-host] [--only-triangulate] [--robust] [--num-hypotheses 64] [--max-tracks 2]
                            [--contaminate 0]"""
import argparse
import itertools
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests")); sys.path.insert(0, str(ROOT / "tools"))
import triangulate_oracle as O
from bench_verify_pairs import make_store, stats, timed
from lightglue_amd import NearestNeighborMatcher, Triangulator, TwoViewVerifier

CAMERA = (500.0, 500.0, 320.0, 240.0)


def replay(K, N, dim=256, seed=0):
    """(poses [K, 3, 4] float32, points [K, N, 3]: the cloud point behind every keypoint row of make_store(K, N, dim, seed), NaN on the rows it replaced by
    unrelated keypoints) — the same random stream drawn again, draw for draw"""
    rng = np.random.default_rng(seed)
    X = rng.uniform([-2.5, -1.8, 4.0], [2.5, 1.8, 8.0], (N, 3))
    rng.standard_normal((N, dim))
    poses, points = np.empty((K, 3, 4), np.float32), np.empty((K, N, 3))
    for k in range(K):
        a, b = rng.uniform(-0.15, 0.15, 2)
        Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
        poses[k] = np.concatenate([Ry @ Rx, rng.uniform(-0.6, 0.6, 3)[:, None]], 1)
        rng.normal(0, 0.5, (N, 2)); rng.standard_normal((N, dim))
        rep = rng.random(N) < 0.3
        rng.uniform([0, 0], [640, 480], (int(rep.sum()), 2)); rng.standard_normal((int(rep.sum()), dim))
        points[k] = np.where(rep[:, None], np.nan, X)[rng.permutation(N)]
    return poses, points


def summary(out, truth):
    """what a call found: tracks per state, lengths, errors, and the distance of the points to the cloud's at each track's rows"""
    res = {"num_tracks": out["num_tracks"], "state_counts": out["state_counts"]}
    res.update({k: out[k] for k in ("num_outliers", "num_split") if k in out})
    if out["num_tracks"]:
        res["mean_track_length"] = round(float(out["track_length"].float().mean()), 2)
    if "xyz" in out and out["num_tracks"]:
        res["median_track_error_px"] = round(float(out["track_error"].median()), 3)
        d = (out["points3d"].double().cpu() - torch.from_numpy(truth)).norm(dim=-1)
        d = d[torch.isfinite(d)]
        res["rows_with_point_and_truth"] = int(d.numel())
        res["median_distance_to_cloud"], res["p95_distance_to_cloud"] = round(float(d.median()), 4), round(float(d.quantile(0.95)), 4)
    return res


def contaminate(m0, fraction, seed=0):
    """matches0 [P, N] with the fraction `fraction` of its matches replaced by uniformly drawn rows (a seeded choice, made on the host)"""
    m0 = m0.cpu().numpy().copy()
    rng = np.random.default_rng(seed)
    at = np.flatnonzero(m0.reshape(-1) >= 0)
    pick = rng.choice(at, int(round(fraction * len(at))), replace=False)
    m0.reshape(-1)[pick] = rng.integers(0, m0.shape[1], len(pick))
    return torch.from_numpy(m0).cuda(), len(pick)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--kpts", type=int, default=2048)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--only-triangulate", action="store_true", help="one call per configuration and nothing else: the run to put under a kernel trace")
    ap.add_argument("--robust", action="store_true", help="also the robust mode on either source")
    ap.add_argument("--num-hypotheses", type=int, default=64)
    ap.add_argument("--max-tracks", type=int, default=2)
    ap.add_argument("--contaminate", type=float, default=0.0, help="the fraction of every source's matches replaced by wrong rows")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_triangulate.py measures on an MI355X; there is nothing to measure without one")
    store = make_store(args.images, args.kpts)
    poses_host, truth = replay(args.images, args.kpts)
    poses = torch.from_numpy(poses_host).cuda()
    pairs = list(itertools.combinations(range(args.images), 2))
    pairs_dev = torch.tensor(pairs, device="cuda")
    cameras = torch.tensor([CAMERA] * args.images, device="cuda")
    nn = NearestNeighborMatcher(ratio_threshold=0.8)
    verifier = TwoViewVerifier(model="fundamental", threshold=3.0, num_hypotheses=1024, refine=True)
    match = lambda: nn.match_pairs(store, pairs_dev, validate=False)
    raw = match()
    verify = lambda: verifier.verify_pairs(store, pairs_dev, raw, validate=False)
    sources = {"raw": raw, "verified": verify()}
    replaced = {}
    if args.contaminate > 0:
        for name in sources:
            m0, replaced[name] = contaminate(sources[name]["matches0"], args.contaminate)
            sources[name] = {"matches0": m0}
    configs = [(s, r) for s in sources for r in (False, True)]
    tris = {r: Triangulator(refine=r) for r in (False, True)}
    runs = {(s, r): (lambda s=s, r=r: tris[r].triangulate(store, pairs_dev, sources[s], cameras, poses, validate=False)) for s, r in configs}
    runs.update({(s, "tracks"): (lambda s=s: tris[True].build_tracks(store, pairs_dev, sources[s], validate=False)) for s in sources})
    if args.robust:
        robust = Triangulator(robust=True, num_hypotheses=args.num_hypotheses, max_tracks=args.max_tracks)
        runs.update({(s, "robust"): (lambda s=s: robust.triangulate(store, pairs_dev, sources[s], cameras, poses, validate=False)) for s in sources})
    outs = {c: fn() for c, fn in runs.items()}                                  # warm-up of every timed shape
    if args.only_triangulate:
        for c, fn in runs.items():
            print(json.dumps({"source": c[0], "mode": c[1], "ms": round(timed(fn)[0], 3)}), flush=True)
        return
    ms, match_ms, verify_ms = {c: [] for c in runs}, [], []
    for _ in range(args.runs):
        match_ms.append(timed(match)[0])
        verify_ms.append(timed(verify)[0])
        for c in runs:                                                          # in turn, not back to back
            ms[c].append(timed(runs[c])[0])
    res = {"images": args.images, "kpts": args.kpts, "pairs": len(pairs), "device": torch.cuda.get_device_name(0), "runs": args.runs,
           **({"contaminate": args.contaminate, "matches_replaced": replaced} if replaced else {}),
           **({"num_hypotheses": args.num_hypotheses, "max_tracks": args.max_tracks} if args.robust else {}),
           "matched_per_pair": {s: round(float((r["matches0"] > -1).sum()) / len(pairs), 1) for s, r in sources.items()},
           "nn_match_pairs": stats(match_ms), "verify_pairs": stats(verify_ms), "triangulate": []}
    for c in runs:
        mode = "build_tracks" if c[1] == "tracks" else "robust" if c[1] == "robust" else "refine" if c[1] else "start"
        res["triangulate"].append({"source": c[0], "mode": mode, **stats(ms[c]), **summary(outs[c], truth)})
    if not args.no_host and not replaced:
        t = time.perf_counter()
        inp = dict(kpts=store["keypoints"].cpu().numpy(), num=None, pairs=np.asarray(pairs), matches0=sources["verified"]["matches0"].cpu().numpy(),
                   cams=np.asarray([CAMERA] * args.images, np.float32), poses=poses_host)
        host = O.triangulate(inp)
        host_ms = (time.perf_counter() - t) * 1e3
        dev = outs["verified", True]
        same = host["num_tracks"] == dev["num_tracks"] and bool((torch.from_numpy(host["node_state"]) == dev["node_state"].cpu()).all())
        res["host"] = {"source": "verified", "mode": "refine", "threads": 1, "ms": round(host_ms, 1), "num_tracks": host["num_tracks"], "same_tracks_and_states_as_device": same,
                       "factor_over_device": round(host_ms / stats(ms["verified", True])["ms_median"], 1)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
