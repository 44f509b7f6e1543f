#!/usr/bin/env python3
"""`BundleAdjuster(solver="pcg")` beyond the dense solver's 256 images, on a planted scene of tests/bundle_oracle.py's recipe (K images of N rows, T tracks of
2 .. 5 views, images 0 and 1 constant, free poses off by about 0.01 rad and 0.03 units, points by 0.03 units): no matcher and no triangulation in front, so the
image count is free.  tools/bench_bundle_adjust.py's exhaustive pair list stops being a workload long before 1 024 images.  Wall-clock ms of one call
(synchronised before and after, one warm-up, `--runs` calls: median and range), the iterations, the solver iterations and the costs; with at most 256 images
the dense solver on the same scene next to it, the two visited in turn.  One JSON line.
`--only-adjust`: one call and nothing else — the run to put under a kernel trace for the per-launch times.

usage: bench_bundle_pcg_scale.py [--images 1024] [--keypoints 256] [--tracks 30000] [--iterations 4] [--max-cg-iterations 100] [--cg-tolerance 1e-6]
                                 [--runs 5] [--only-adjust]"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests")); sys.path.insert(0, str(ROOT / "tools"))
import bundle_oracle as B
from bench_verify_pairs import stats, timed
from lightglue_amd import BundleAdjuster, _cabi


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--keypoints", type=int, default=256)
    ap.add_argument("--tracks", type=int, default=30000)
    ap.add_argument("--iterations", type=int, default=4)
    ap.add_argument("--max-cg-iterations", type=int, default=100)
    ap.add_argument("--cg-tolerance", type=float, default=1e-6)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=77)
    ap.add_argument("--only-adjust", action="store_true", help="one call and nothing else: the run to put under a kernel trace")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bundle_pcg_scale.py measures on an MI355X; there is nothing to measure without one")
    sc = B.scene(args.images, args.keypoints, args.tracks, args.seed, hi=5)
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    feats, tracks, cams, poses, const = {"keypoints": cuda(sc["kpts"])}, (cuda(sc["track_id"]), cuda(sc["xyz"])), cuda(sc["cams"]), cuda(sc["poses"]), torch.from_numpy(sc["constant"])
    conf = {"pcg": dict(solver="pcg", max_cg_iterations=args.max_cg_iterations, cg_tolerance=args.cg_tolerance)}
    if args.images <= _cabi.LG_BA_MAX_IMAGES and not args.only_adjust:
        conf["cholesky"] = dict()
    runs = {name: (lambda c=c: BundleAdjuster(num_iterations=args.iterations, **c).adjust(feats, tracks, cams, poses, const)) for name, c in conf.items()}
    outs = {name: fn() for name, fn in runs.items()}                             # warm-up of every timed shape
    if args.only_adjust:
        ms, out = timed(runs["pcg"])
        print(json.dumps({"num_iterations": out["num_iterations"], "cg_iterations": out["cg_iterations"], "ms": round(ms, 3)}), flush=True)
        return
    ms = {name: [] for name in runs}
    for _ in range(args.runs):
        for name in runs:                                                        # in turn, not back to back
            ms[name].append(timed(runs[name])[0])
    res = {"images": args.images, "keypoints": args.keypoints, "tracks": args.tracks, "device": torch.cuda.get_device_name(0), "runs": args.runs,
           "budget": args.iterations, "max_cg_iterations": args.max_cg_iterations, "cg_tolerance": args.cg_tolerance, "adjust": []}
    for name, o in outs.items():
        res["adjust"].append({"solver": name, **stats(ms[name]), "iterations_run": o["num_iterations"], "accepted": o["num_accepted"], "converged": o["converged"],
                              "observations": o["num_observations"], "initial_cost": round(o["initial_cost"], 3), "final_cost": round(o["final_cost"], 3),
                              "cg_iterations": o.get("cg_iterations"), "cg_unconverged": o.get("cg_unconverged")})
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
