#!/usr/bin/env python3
"""`GlobalPoseEstimator.estimate` (lg_posegraph_solve: adjacency, tree, per iteration assemble / Cholesky panels / update for rotations and then for positions;
one call, one host synchronisation) next to the float64 numpy definition on the host, at two sizes:

  K = 16   tools/bench_bundle_adjust.py's scene (16 views x N keypoints of one point cloud, 120 exhaustive pairs matched by `NearestNeighborMatcher`), the
           relative poses from `RelativePoseEstimator.estimate_pairs`, its dict passed as is;
  K = 256  tests/posegraph_oracle.py's ring plus 768 chords (1 024 pairs), 0.3 degrees of noise on every pair.

Per size: the wall-clock ms of the call (synchronised before and after, one warm-up, the sizes visited in turn `--runs` times: median and range), the launches
of the call (8 + n (4 + 2 ceil(K / 48) + 2 ceil(3 K / 48)), all enqueued whatever converges), the iterations run, the host's ms (tests/posegraph_oracle.py's
`estimate_once`, one run) and whether its states are the device's; for K = 16 also the error against the poses the store was projected with.  One JSON line,
and the same as a table in `--out` (default profiles/global_poses.md; what stands below the notes marker of an existing file is kept).

`--solver pcg` measures the iterative solver instead (lg_posegraph_solve_pcg; default --out profiles/global_poses_pcg.md): K = 16 and K = 256 as above with
both solvers in the same job, visited in turn, and K = 1 024 and K = 4 096 at 8 pairs per image (ring plus 7 K chords, 0.3 degrees of noise) with "pcg" alone;
per row also the launches enqueued (9 + 2 n (2 + rotation_cg_iterations + position_cg_iterations)), the solver iterations run per stage and the solves that
ended on their budget.  `--sizes` picks among 16, 256, 1024, 4096.

usage: bench_global_poses.py [--kpts 2048] [--runs 5] [--solver cholesky|pcg] [--sizes 16,256,1024,4096] [--out profiles/global_poses.md]"""
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
import posegraph_oracle as G
from bench_triangulate import CAMERA, replay
from bench_verify_pairs import make_store, stats, timed
from lightglue_amd import GlobalPoseEstimator, NearestNeighborMatcher, RelativePoseEstimator


NOTES = "\n<!-- notes: kept by tools/bench_global_poses.py -->\n"


def launches(K, n):
    return 8 + n * (4 + 2 * -(-K // 48) + 2 * -(-3 * K // 48))


def launches_pcg(n, rotation_cg, position_cg):
    return 9 + 2 * n * (2 + rotation_cg + position_cg)


def main_pcg(args):
    """the iterative solver: every size with "pcg", K <= 256 also with "cholesky", all visited in turn"""
    solvers = {"pcg": GlobalPoseEstimator(solver="pcg"), "cholesky": GlobalPoseEstimator()}
    n = solvers["pcg"].num_iterations
    sizes = [int(k) for k in args.sizes.split(",")]
    calls, truth = {}, {}
    if 16 in sizes:
        store = make_store(16, args.kpts)
        poses_host, _ = replay(16, args.kpts)
        pairs16 = torch.tensor(list(itertools.combinations(range(16), 2)), device="cuda")
        cameras = torch.tensor([CAMERA] * 16, device="cuda")
        raw = NearestNeighborMatcher(ratio_threshold=0.8).match_pairs(store, pairs16, validate=False)
        rel = RelativePoseEstimator(threshold=3.0, num_hypotheses=1024, refine=True, seed=0).estimate_pairs(store, pairs16, raw, cameras, validate=False)
        for name, est in solvers.items():
            calls[(16, 120, name)] = lambda est=est: est.estimate(pairs16, rel, 16)
    for K in (k for k in sizes if k != 16):
        sc = G.scene(K, chords=768 if K == 256 else 7 * K, noise=0.3)
        dev = (torch.from_numpy(sc["pairs"]).cuda(), (torch.from_numpy(sc["R"]).cuda(), torch.from_numpy(sc["t"]).cuda()), torch.from_numpy(sc["weights"]).cuda())
        truth[K] = sc
        for name, est in solvers.items():
            if name == "pcg" or K <= 256:
                calls[(K, len(sc["pairs"]), name)] = lambda est=est, dev=dev, K=K: est.estimate(dev[0], dev[1], K, weights=dev[2])
    outs = {k: fn() for k, fn in calls.items()}                                  # warm-up of every timed shape
    ms = {k: [] for k in calls}
    for _ in range(args.runs):
        for k in calls:                                                          # in turn, not back to back
            ms[k].append(timed(calls[k])[0])
    res = {"device": torch.cuda.get_device_name(0), "runs": args.runs, "num_iterations": n, "rotation_cg_iterations": solvers["pcg"].rotation_cg_iterations,
           "position_cg_iterations": solvers["pcg"].position_cg_iterations, "cg_tolerance": solvers["pcg"].cg_tolerance, "sizes": []}
    for (K, P, name), o in outs.items():
        row = {"images": K, "pairs": P, "solver": name, **stats(ms[(K, P, name)]),
               "launches": launches(K, n) if name == "cholesky" else launches_pcg(n, res["rotation_cg_iterations"], res["position_cg_iterations"]),
               "rotation_iterations": o["rotation_iterations"], "position_iterations": o["position_iterations"],
               "rotation_cg_iterations": o.get("rotation_cg_iterations", ""), "position_cg_iterations": o.get("position_cg_iterations", ""),
               "rotation_cg_unconverged": o.get("rotation_cg_unconverged", ""), "position_cg_unconverged": o.get("position_cg_unconverged", ""),
               "num_posed": o["num_posed"], "positions_ok": o["positions_ok"]}
        sc = truth.get(K)
        if K == 16 and o["baseline"] is not None:
            sc = dict(zip(("Rg", "cg"), G.in_gauge(poses_host, o["origin"], o["baseline"])))
        if sc is not None and o["num_posed"]:
            P64 = o["poses"].double().cpu().numpy()
            mine = dict(image_state=o["image_state"].cpu().numpy(), poses64=P64, centres64=-np.einsum("kji,kj->ki", P64[:, :, :3], P64[:, :, 3]))
            rot, centre = G.against_truth(mine, sc)
            row["worst_rotation_error_deg"], row["worst_centre_error_of_extent"] = round(rot, 4), round(centre, 5)
        res["sizes"].append(row)
    print(json.dumps(res), flush=True)
    keys = list(res["sizes"][0])
    lines = ["# GlobalPoseEstimator(solver=\"pcg\"): per-call time", "",
             "`tools/bench_global_poses.py --solver pcg` on %s, %d runs per row, num_iterations = %d, budgets %d / %d, cg_tolerance = %g." % (
                 res["device"], args.runs, n, res["rotation_cg_iterations"], res["position_cg_iterations"], res["cg_tolerance"]), "",
             "| " + " | ".join(keys) + " |", "|" + "---|" * len(keys)]
    for row in res["sizes"]:
        lines.append("| " + " | ".join(str(row.get(k, "")) for k in keys) + " |")
    out = Path(args.out or ROOT / "profiles" / "global_poses_pcg.md")
    out.parent.mkdir(parents=True, exist_ok=True)
    notes = out.read_text().partition(NOTES)[2] if out.exists() else ""
    out.write_text("\n".join(lines) + "\n" + (NOTES + notes if notes else ""))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kpts", type=int, default=2048)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--solver", choices=("cholesky", "pcg"), default="cholesky")
    ap.add_argument("--sizes", default="16,256,1024,4096")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_global_poses.py measures on an MI355X; there is nothing to measure without one")
    if args.solver == "pcg":
        return main_pcg(args)
    args.out = args.out or str(ROOT / "profiles" / "global_poses.md")
    est = GlobalPoseEstimator()
    n = est.num_iterations
    # K = 16: the chain's own relative poses
    K = 16
    store = make_store(K, args.kpts)
    poses_host, _ = replay(K, args.kpts)
    pairs16 = torch.tensor(list(itertools.combinations(range(K), 2)), device="cuda")
    cameras = torch.tensor([CAMERA] * K, device="cuda")
    raw = NearestNeighborMatcher(ratio_threshold=0.8).match_pairs(store, pairs16, validate=False)
    rel = RelativePoseEstimator(threshold=3.0, num_hypotheses=1024, refine=True, seed=0).estimate_pairs(store, pairs16, raw, cameras, validate=False)
    # K = 256: the oracle's scene
    sc = G.scene(256, chords=768, noise=0.3)
    big = (torch.from_numpy(sc["pairs"]).cuda(), (torch.from_numpy(sc["R"]).cuda(), torch.from_numpy(sc["t"]).cuda()), torch.from_numpy(sc["weights"]).cuda())
    calls = {16: lambda: est.estimate(pairs16, rel, 16), 256: lambda: est.estimate(big[0], big[1], 256, weights=big[2])}
    outs = {k: fn() for k, fn in calls.items()}                                  # warm-up of every timed shape
    ms = {k: [] for k in calls}
    for _ in range(args.runs):
        for k in calls:                                                          # in turn, not back to back
            ms[k].append(timed(calls[k])[0])
    host_in = {16: dict(pairs=pairs16.cpu().numpy(), R=rel["R"].cpu().numpy(), t=rel["t"].cpu().numpy(), kw=dict(num_inliers=rel["num_inliers"].cpu().numpy())),
               256: dict(pairs=sc["pairs"], R=sc["R"], t=sc["t"], kw=dict(weights=sc["weights"]))}
    res = {"device": torch.cuda.get_device_name(0), "runs": args.runs, "num_iterations": n, "sizes": []}
    for k, o in outs.items():
        h = host_in[k]
        t0 = time.perf_counter()
        host = G.estimate_once(h["pairs"], h["R"], h["t"], k, **h["kw"])
        host_ms = (time.perf_counter() - t0) * 1e3
        row = {"images": k, "pairs": int(len(h["pairs"])), **stats(ms[k]), "launches": launches(k, n), "rotation_iterations": o["rotation_iterations"],
               "position_iterations": o["position_iterations"], "num_posed": o["num_posed"], "positions_ok": o["positions_ok"],
               "rotation_outliers": int((o["pair_state"] == 4).sum()), "host_ms": round(host_ms, 1), "host_threads": 1,
               "same_states_as_host": bool((torch.from_numpy(host["pair_state"]) == o["pair_state"].cpu()).all()
                                           and (torch.from_numpy(host["image_state"]) == o["image_state"].cpu()).all())}
        truth = dict(Rg=None, cg=None)
        if k == 16 and o["baseline"] is not None:
            truth["Rg"], truth["cg"] = G.in_gauge(poses_host, o["origin"], o["baseline"])
        elif k == 256:
            truth = sc
        if truth["Rg"] is not None and o["num_posed"]:
            P = o["poses"].double().cpu().numpy()
            mine = dict(image_state=o["image_state"].cpu().numpy(), poses64=P, centres64=-np.einsum("kji,kj->ki", P[:, :, :3], P[:, :, 3]))
            rot, centre = G.against_truth(mine, truth)
            row["worst_rotation_error_deg"], row["worst_centre_error_of_extent"] = round(rot, 4), round(centre, 5)
        res["sizes"].append(row)
    print(json.dumps(res), flush=True)
    keys = list(res["sizes"][0].keys() | res["sizes"][1].keys())
    keys = [k for k in res["sizes"][1] if k in keys] + [k for k in res["sizes"][0] if k not in res["sizes"][1]]
    lines = ["# GlobalPoseEstimator: per-call time", "", "`tools/bench_global_poses.py` on %s, %d runs per size, num_iterations = %d for each solver." % (
        res["device"], args.runs, n), "", "| " + " | ".join(keys) + " |", "|" + "---|" * len(keys)]
    for row in res["sizes"]:
        lines.append("| " + " | ".join(str(row.get(k, "")) for k in keys) + " |")
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    notes = out.read_text().partition(NOTES)[2] if out.exists() else ""          # what a reader wrote below the table stays
    out.write_text("\n".join(lines) + "\n" + (NOTES + notes if notes else ""))


if __name__ == "__main__":
    main()
