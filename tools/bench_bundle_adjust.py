#!/usr/bin/env python3
"""`BundleAdjuster.adjust` (lg_bundle_adjust: records, track lists, then per iteration points / reduce / Cholesky panels / back substitution / trial points /
trial cost / decide, and the scatter; one call, one host synchronisation) on the tracks `Triangulator` builds, next to that `triangulate` call and next to the
float64 numpy definition on the host.

Workload: tools/bench_triangulate.py's (K = 16 views x N = 2 048 keypoints of one point cloud, 120 exhaustive pairs matched by `NearestNeighborMatcher` and
verified by `TwoViewVerifier`, triangulated under the poses the store was projected with).  The adjuster then gets the poses of images 2 .. K - 1 moved by about
0.002 rad and 0.01 units (images 0 and 1 are held constant) and the triangulated points as they are.  Per iteration budget: the wall-clock ms of the call
(synchronised before and after, one warm-up, the configurations visited in turn `--runs` times: median and range), the iterations run, the costs.  The host
route is tests/bundle_oracle.py (float64, one thread) with `--host-iterations` iterations, timed once.  One JSON line.
`--only-adjust`: one call and nothing else — the run to put under a kernel trace for the per-launch times.
`--loss`, `--loss-scale`, `--filter-rounds`, `--max-reproj-error`: the adjuster's robust mode (lg_bundle_adjust_robust; the host route is then
tests/bundle_robust_oracle.py).  `--contaminate F`: after the triangulation, the keypoints of a fraction F of the observations — of tracks with at least
3 observations, at most one per track — are moved by 20 .. 80 pixels in a random direction; the result line then also counts how many of them end above
4 pixels or filtered, how many clean observations do, and the tracks still adjusted at the end.

`--refine-focal`: the focal lengths are unknowns too (lg_bundle_adjust_focal; the host route is then tests/bundle_focal_oracle.py).  `--focal-error F`: the
adjuster's cameras get fx and fy multiplied by 1 + F in the even images and 1 - F in the odd ones (the tracks are still those triangulated under the true
cameras); the result line then holds the relative focal error per budget before and after (median and worst over the images).

`--solver pcg [--max-cg-iterations 100 --cg-tolerance 1e-6]`: the iterative solver (lg_bundle_adjust_pcg; the host route is then tests/bundle_pcg_oracle.py);
the result line then holds the solver iterations and the iterations that ended on the budget.  Beyond 256 images this tool's exhaustive pair list stops being
a workload: tools/bench_bundle_pcg_scale.py times the solver on planted scenes there.

usage: bench_bundle_adjust.py [--solver cholesky|pcg] [--max-cg-iterations 100] [--cg-tolerance 1e-6] [--images 16] [--kpts | --keypoints 2048] [--runs 5] [--host-iterations 2] [--only-adjust] [--loss squared|huber|cauchy] [--loss-scale 2]
                              [--filter-rounds 0] [--max-reproj-error 4] [--contaminate 0] [--refine-focal] [--focal-error 0]"""
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
import bundle_focal_oracle as F
import bundle_oracle as B
import bundle_pcg_oracle as P
import bundle_robust_oracle as R
from abspose_oracle import rodrigues
from bench_triangulate import CAMERA, replay
from bench_verify_pairs import make_store, stats, timed
from lightglue_amd import BundleAdjuster, NearestNeighborMatcher, Triangulator, TwoViewVerifier


def moved_poses(poses, rot=0.002, shift=0.01, seed=1):
    rng = np.random.default_rng(seed)
    out = poses.astype(np.float64)
    for k in range(2, len(out)):
        Q = rodrigues(rot * rng.standard_normal(3) / np.sqrt(3))
        R, c = out[k][:, :3], -out[k][:, :3].T @ out[k][:, 3]
        c = c + shift * rng.standard_normal(3) / np.sqrt(3)
        out[k] = np.concatenate([Q @ R, (-(Q @ R) @ c)[:, None]], 1)
    return out.astype(np.float32)


def contaminate(store, tracks, fraction, seed=5):
    """-> (a store with moved keypoints, the moved nodes as a [K, N] bool mask on the device)"""
    tid = tracks["track_id"].cpu().numpy()
    kpts = store["keypoints"].cpu().numpy().copy()
    rng = np.random.default_rng(seed)
    length = np.bincount(tid[tid >= 0], minlength=int(tid.max()) + 2)
    nodes = np.argwhere((tid >= 0) & (length[np.maximum(tid, 0)] >= 3))
    want, taken, mask = int(round(fraction * (tid >= 0).sum())), set(), np.zeros(tid.shape, bool)
    for at in rng.permutation(len(nodes)):
        if len(taken) >= want:
            break
        k, i = nodes[at]
        if int(tid[k, i]) in taken:
            continue
        taken.add(int(tid[k, i]))
        angle, dist = rng.uniform(0.0, 2.0 * np.pi), rng.uniform(20.0, 80.0)
        kpts[k, i] += (dist * np.array([np.cos(angle), np.sin(angle)])).astype(np.float32)
        mask[k, i] = True
    return dict(store, keypoints=torch.from_numpy(kpts).to(store["keypoints"].device)), torch.from_numpy(mask).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--kpts", "--keypoints", type=int, default=2048)
    ap.add_argument("--solver", default="cholesky", choices=("cholesky", "pcg"), help="pcg: lg_bundle_adjust_pcg, up to 4096 images")
    ap.add_argument("--max-cg-iterations", type=int, default=100)
    ap.add_argument("--cg-tolerance", type=float, default=1e-6)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--host-iterations", type=int, default=2, help="iterations of the numpy definition on the host (0: skip)")
    ap.add_argument("--only-adjust", action="store_true", help="one call and nothing else: the run to put under a kernel trace")
    ap.add_argument("--loss", default="squared", choices=("squared", "huber", "cauchy"))
    ap.add_argument("--loss-scale", type=float, default=2.0)
    ap.add_argument("--filter-rounds", type=int, default=0)
    ap.add_argument("--max-reproj-error", type=float, default=4.0)
    ap.add_argument("--contaminate", type=float, default=0.0, help="fraction of the observations moved by 20 .. 80 pixels after the triangulation")
    ap.add_argument("--refine-focal", action="store_true", help="refine one focal length per image with the poses and points (lg_bundle_adjust_focal)")
    ap.add_argument("--focal-error", type=float, default=0.0, help="relative error of the focal lengths given to the adjuster, the sign alternating by image")
    args = ap.parse_args()
    conf = dict(loss=args.loss, loss_scale=args.loss_scale, filter_rounds=args.filter_rounds, max_reproj_error=args.max_reproj_error)
    if args.refine_focal:
        conf["refine_focal"] = True
    if args.solver == "pcg":
        conf.update(solver="pcg", max_cg_iterations=args.max_cg_iterations, cg_tolerance=args.cg_tolerance)
    if not torch.cuda.is_available():
        raise SystemExit("bench_bundle_adjust.py measures on an MI355X; there is nothing to measure without one")
    K = args.images
    store = make_store(K, args.kpts)
    poses_host, truth = replay(K, args.kpts)
    pairs_dev = torch.tensor(list(itertools.combinations(range(K), 2)), device="cuda")
    cameras = torch.tensor([CAMERA] * K, device="cuda")
    raw = NearestNeighborMatcher(ratio_threshold=0.8).match_pairs(store, pairs_dev, validate=False)
    verified = TwoViewVerifier(model="fundamental", threshold=3.0, num_hypotheses=1024, refine=True).verify_pairs(store, pairs_dev, raw, validate=False)
    tri = Triangulator()
    true_poses = torch.from_numpy(poses_host).cuda()
    triangulate = lambda: tri.triangulate(store, pairs_dev, verified, cameras, true_poses, validate=False)
    tracks = triangulate()
    start = torch.from_numpy(moved_poses(poses_host)).cuda()
    clean_store, planted = store, None
    if args.contaminate > 0:
        store, planted = contaminate(store, tracks, args.contaminate)
    constant = [0, 1]
    true_cameras = cameras
    if args.focal_error:                                                         # the triangulation above and below keeps the true cameras
        factor = torch.tensor([1.0 + args.focal_error if k % 2 == 0 else 1.0 - args.focal_error for k in range(K)], device="cuda")
        cameras = torch.cat([true_cameras[:, :2] * factor[:, None], true_cameras[:, 2:]], 1).float()
    triangulate = lambda: tri.triangulate(clean_store, pairs_dev, verified, true_cameras, true_poses, validate=False)
    budgets = (1, 10)
    runs = {n: (lambda n=n: BundleAdjuster(num_iterations=n, **conf).adjust(store, tracks, cameras, start, constant)) for n in budgets}
    outs = {n: fn() for n, fn in runs.items()}                                   # warm-up of every timed shape
    if args.only_adjust:
        ms, out = timed(runs[10])
        print(json.dumps({"num_iterations": out["num_iterations"], "ms": round(ms, 3), **({"cg_iterations": out["cg_iterations"]} if "cg_iterations" in out else {})}),
              flush=True)
        return
    ms, tri_ms = {n: [] for n in runs}, []
    for _ in range(args.runs):
        tri_ms.append(timed(triangulate)[0])
        for n in runs:                                                           # in turn, not back to back
            ms[n].append(timed(runs[n])[0])
    res = {"images": K, "kpts": args.kpts, "pairs": int(pairs_dev.shape[0]), "device": torch.cuda.get_device_name(0), "runs": args.runs,
           "tracks": tracks["num_tracks"], "triangulate": stats(tri_ms), **conf, "contaminate": args.contaminate,
           "planted": 0 if planted is None else int(planted.sum()), "refine_focal": args.refine_focal, "focal_error": args.focal_error, "solver": args.solver, "adjust": []}
    focal_error = lambda c: (c[:, 0].double() / true_cameras[:, 0].double() - 1.0).abs().cpu()
    for n in runs:
        o = outs[n]
        d = (o["points3d"].double().cpu() - torch.from_numpy(truth)).norm(dim=-1)
        d0 = (tracks["points3d"].double().cpu() - torch.from_numpy(truth)).norm(dim=-1)
        res["adjust"].append({"budget": n, **stats(ms[n]), "iterations_run": o["num_iterations"], "accepted": o["num_accepted"], "converged": o["converged"],
                              "observations": o["num_observations"], "initial_cost": round(o["initial_cost"], 3), "final_cost": round(o["final_cost"], 3),
                              "median_distance_to_cloud_before": round(float(d0[torch.isfinite(d0)].median()), 5),
                              "median_distance_to_cloud_after": round(float(d[torch.isfinite(d)].median()), 5)})
        active = o["node_state"] == 1
        kept = torch.bincount(tracks["track_id"][active], minlength=1)
        above = torch.nan_to_num(o["observation_error"]) > 4.0
        res["adjust"][-1].update({"filtered": o["num_filtered"], "filter_stages": o["num_filter_stages"], "tracks_adjusted_at_the_end": int((kept >= 2).sum()),
                                  "clean_above_4px": int((above & ~planted).sum()) if planted is not None else int(above.sum()),
                                  "clean_filtered": int(((o["node_state"] == 7) & ~planted).sum()) if planted is not None else o["num_filtered"]})
        if args.solver == "pcg":
            res["adjust"][-1].update({"cg_iterations": o["cg_iterations"], "cg_unconverged": o["cg_unconverged"]})
        if args.refine_focal:
            before, after = focal_error(cameras), focal_error(o["cameras"])
            res["adjust"][-1].update({"free_cameras": o["num_free_cameras"], "focal_error_before_median": round(float(before.median()), 6),
                                      "focal_error_before_max": round(float(before.max()), 6), "focal_error_after_median": round(float(after.median()), 6),
                                      "focal_error_after_max": round(float(after.max()), 6)})
        if planted is not None:
            res["adjust"][-1].update({"planted_above_4px": int((above & planted).sum()), "planted_filtered": int(((o["node_state"] == 7) & planted).sum())})
    ten, one = res["adjust"][1], res["adjust"][0]
    if ten["iterations_run"] > one["iterations_run"]:          # with filter rounds both figures hold the rebuilds between the stages
        res["ms_per_iteration"] = round((ten["ms_median"] - one["ms_median"]) / (ten["iterations_run"] - one["iterations_run"]), 3)
    if args.host_iterations:
        inp = dict(kpts=store["keypoints"].cpu().numpy(), num=None, track_id=tracks["track_id"].cpu().numpy(), xyz=tracks["xyz"].cpu().numpy(),
                   cams=cameras.cpu().numpy(), poses=start.cpu().numpy(), constant=np.arange(K) < 2)
        t = time.perf_counter()
        robust = args.loss != "squared" or args.filter_rounds > 0
        host_conf = {k: v for k, v in conf.items() if k not in ("refine_focal", "solver")}
        host = ((P if args.solver == "pcg" else F if args.refine_focal else R).adjust(inp, num_iterations=args.host_iterations, **host_conf)
                if robust or args.refine_focal or args.solver == "pcg" else B.adjust(inp, num_iterations=args.host_iterations))
        host_ms = (time.perf_counter() - t) * 1e3
        dev = BundleAdjuster(num_iterations=args.host_iterations, **conf).adjust(store, tracks, cameras, start, constant)
        res["host"] = {"threads": 1, "iterations": host["num_iterations"], "ms": round(host_ms, 1), "final_cost": round(host["final_cost"], 3),
                       "device_final_cost_same_budget": round(dev["final_cost"], 3), "near_decisions": host["near"],
                       "same_states_as_device": bool((torch.from_numpy(host["node_state"]) == dev["node_state"].cpu()).all())}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
