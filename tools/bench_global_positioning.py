#!/usr/bin/env python3
"""`GlobalPositioner.solve` (lg_positioning_solve: records, track lists, who takes part, then per iteration points / reduce / Cholesky panels / centres / point
update, and the classification; one call, one host synchronisation) next to `GlobalPoseEstimator.estimate` and `Triangulator.triangulate` on the same inputs in
the same job, at two sizes:

  K = 16   tools/bench_bundle_adjust.py's scene (16 views x N keypoints of one point cloud, 120 exhaustive pairs matched by `NearestNeighborMatcher` and
           verified by `TwoViewVerifier`: the 2 048-track list the other rows use), relative poses from `RelativePoseEstimator.estimate_pairs`, rotations and
           the two held images from `GlobalPoseEstimator`'s dict, labels from `Triangulator.build_tracks`;
  K = 256  tests/positioning_oracle.py's scene: 256 cameras on the arc, 64 keypoints each, 3 600 planted tracks of 3 .. 5 views with 0.5 px of noise; the pair
           list is every image pair that shares a track, its relative poses the exact ones with 0.3 degrees of noise per pair.

Per size: the wall-clock ms of each call (synchronised before and after, one warm-up, the calls visited in turn `--runs` times: median and range), the
launches of the positioner's call (8 + n (4 + 2 ceil(3 K / 48)), all enqueued whatever converges), the iterations run, the counts, the host's ms
(tests/positioning_oracle.py's `solve_once`, one run) and whether its states are the device's, and the accuracy against the poses the scene was built from
before (direction averaging) and after.  One JSON line, and the same as a table in `--out` (default profiles/global_positioning.md; what stands below the
notes marker of an existing file is kept).
`--trace K`: one warm-up and ONE call of the positioner at that size and nothing else timed — the run to put under a kernel trace; `--kernel-stats FILE`
reads the statistics such a trace wrote (csv: Name, Calls, TotalDurationNs, ...) and prints the positioner's launch kinds per call.

usage: bench_global_positioning.py [--kpts 2048] [--runs 5] [--out profiles/global_positioning.md] [--trace 16|256] [--kernel-stats FILE --calls 2]"""
import argparse
import csv
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
import positioning_oracle as P
from bench_triangulate import CAMERA, replay
from bench_verify_pairs import make_store, stats, timed
from lightglue_amd import GlobalPoseEstimator, GlobalPositioner, NearestNeighborMatcher, RelativePoseEstimator, Triangulator, TwoViewVerifier

NOTES = "\n<!-- notes: kept by tools/bench_global_positioning.py -->\n"


def launches(K, n):
    return 8 + n * (4 + 2 * -(-3 * K // 48))


def kernel_stats(path, calls):
    """the positioner's launch kinds out of a kernel trace's statistics: [(kind, launches per call, us per call, us per launch)]"""
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r["Name"]
            if "lg::pos_" not in name and not name.startswith("pos_"):       # (not the pose-graph solver's pg_pos_* kernels)
                continue
            kind = name[name.index("pos_"):].split("(")[0].split("_kernel")[0]
            rows.append((kind, int(r["Calls"]) / calls, float(r["TotalDurationNs"]) / calls / 1e3, float(r["AverageNs"]) / 1e3))
    return sorted(rows, key=lambda r: -r[2])


def small_scene(kpts):
    K = 16
    store = make_store(K, kpts)
    poses_host, _ = replay(K, kpts)
    pairs = torch.tensor(list(itertools.combinations(range(K), 2)), device="cuda")
    cameras = torch.tensor([CAMERA] * K, device="cuda")
    raw = NearestNeighborMatcher(ratio_threshold=0.8).match_pairs(store, pairs, validate=False)
    verified = TwoViewVerifier(model="fundamental", threshold=3.0, num_hypotheses=1024, refine=True).verify_pairs(store, pairs, raw, validate=False)
    rel = RelativePoseEstimator(threshold=3.0, num_hypotheses=1024, refine=True, seed=0).estimate_pairs(store, pairs, raw, cameras, validate=False)
    return dict(K=K, store=store, pairs=pairs, cameras=cameras, matches=verified, relative=rel, weights=None, truth=poses_host, cams=np.asarray([CAMERA] * K, np.float32))


def large_scene():
    K, N, T = 256, 64, 3600
    sc = P.scene(K, N, T)
    index, pairs = {}, []
    for at in sc["planted"]["rows"]:
        for a, b in itertools.combinations(sorted(at), 2):
            if (a, b) not in index:
                index[a, b] = len(pairs)
                pairs.append((a, b))
    m0 = np.full((len(pairs), N), -1, np.int64)
    for at in sc["planted"]["rows"]:
        for a, b in itertools.combinations(sorted(at), 2):
            m0[index[a, b], at[a]] = at[b]
    pairs = np.asarray(pairs, np.int64)
    rng = np.random.default_rng(3)
    Rab, t = G.relative(*G.in_gauge(sc["poses"], 0, 1), pairs)
    for p in range(len(pairs)):
        Rab[p] = G.random_rotation(rng, rng.uniform(0.2, 1.0) * 0.3) @ Rab[p]
        t[p] = G.random_rotation(rng, rng.uniform(0.2, 1.0) * 0.3) @ t[p]
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return dict(K=K, store={"keypoints": cuda(sc["kpts"])}, pairs=cuda(pairs), cameras=cuda(sc["cams"]), matches=cuda(m0),
                relative=(cuda(Rab.astype(np.float32)), cuda(t.astype(np.float32))), weights=torch.ones(len(pairs), device="cuda"), truth=sc["poses"], cams=sc["cams"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kpts", type=int, default=2048)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "global_positioning.md"))
    ap.add_argument("--trace", type=int, default=0, choices=(0, 16, 256))
    ap.add_argument("--kernel-stats", default="")
    ap.add_argument("--calls", type=int, default=2, help="calls of the positioner in the traced run (--trace makes two)")
    args = ap.parse_args()
    if args.kernel_stats:
        rows = kernel_stats(args.kernel_stats, args.calls)
        total = sum(r[2] for r in rows)
        print("| launch kind | launches per call | us per call | us per launch | share |\n|---|---|---|---|---|")
        for kind, count, us, each in rows:
            print("| %s | %g | %.1f | %.2f | %.1f %% |" % (kind, count, us, each, 100.0 * us / total))
        print("| all | %g | %.1f | | |" % (sum(r[1] for r in rows), total))
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench_global_positioning.py measures on an MI355X; there is nothing to measure without one")
    est, pos, tri = GlobalPoseEstimator(), GlobalPositioner(), Triangulator(max_reproj_error=8.0)
    n = pos.num_iterations
    res = {"device": torch.cuda.get_device_name(0), "runs": args.runs, "num_iterations": n, "sizes": []}
    for scene in (small_scene, large_scene):
        if args.trace and (scene is small_scene) != (args.trace == 16):
            continue
        s = scene(args.kpts) if scene is small_scene else scene()
        K, store, pairs, cameras = s["K"], s["store"], s["pairs"], s["cameras"]
        kw = {} if s["weights"] is None else {"weights": s["weights"]}
        averaged = est.estimate(pairs, s["relative"], K, **kw)
        tracks = Triangulator().build_tracks(store, pairs, s["matches"], validate=False)
        calls = {"position": lambda: pos.solve(store, tracks, cameras, averaged),
                 "estimate": lambda: est.estimate(pairs, s["relative"], K, **kw),
                 "triangulate": lambda: tri.triangulate(store, pairs, s["matches"], cameras, averaged["poses"], validate=False)}
        out = calls["position"]()                                                # warm-up
        if args.trace:
            ms, out = timed(calls["position"])
            print(json.dumps({"images": K, "ms": round(ms, 3), "iterations": out["iterations"], "launches": launches(K, n)}), flush=True)
            return
        from_averaged = calls["triangulate"]()
        from_positioned = tri.triangulate(store, pairs, s["matches"], cameras, out["poses"], validate=False)
        ms = {k: [] for k in calls}
        for _ in range(args.runs):
            for k in calls:                                                      # in turn, not back to back
                ms[k].append(timed(calls[k])[0])
        held = np.zeros(K, bool)
        held[[averaged["origin"], averaged["baseline"]]] = True
        inp = dict(kpts=store["keypoints"].cpu().numpy(), num=None, track_id=tracks["track_id"].cpu().numpy(), T=tracks["num_tracks"], cams=s["cams"],
                   poses=averaged["poses"].cpu().numpy(), held=held)
        t0 = time.perf_counter()
        host = P.solve_once(inp)
        host_ms = (time.perf_counter() - t0) * 1e3
        _, cg = G.in_gauge(s["truth"], averaged["origin"], averaged["baseline"])
        centres = lambda poses: -np.einsum("kji,kj->ki", poses[:, :, :3], poses[:, :, 3])
        before, after = averaged["poses"].double().cpu().numpy(), out["poses"].double().cpu().numpy()
        row = {"images": K, "keypoints": int(store["keypoints"].shape[1]), "pairs": int(pairs.shape[0]), "tracks": tracks["num_tracks"],
               "observations": int((out["node_state"] != 0).sum()), **{"position_" + k: v for k, v in stats(ms["position"]).items()},
               "estimate_ms_median": stats(ms["estimate"])["ms_median"], "triangulate_ms_median": stats(ms["triangulate"])["ms_median"],
               "launches": launches(K, n), "iterations": out["iterations"], "num_posed": out["num_posed"], "num_points": out["num_points"],
               "num_outliers": out["num_outliers"], "positions_ok": out["positions_ok"], "host_ms": round(host_ms, 1), "host_threads": 1,
               "same_states_as_host": bool((torch.from_numpy(host["node_state"]) == out["node_state"].cpu()).all()
                                           and (torch.from_numpy(host["image_state"]) == out["image_state"].cpu()).all()),
               "centre_error_of_extent_averaged": round(P.centre_error(centres(before), cg), 5),
               "centre_error_of_extent_positioned": round(P.centre_error(centres(after), cg), 5),
               "tracks_within_8px_averaged": from_averaged["num_tracks"], "tracks_within_8px_positioned": from_positioned["num_tracks"]}
        res["sizes"].append(row)
    print(json.dumps(res), flush=True)
    keys = list(res["sizes"][0])
    lines = ["# GlobalPositioner: per-call time", "", "`tools/bench_global_positioning.py` on %s, %d runs per size, num_iterations = %d." % (res["device"], args.runs, n),
             "", "| " + " | ".join(keys) + " |", "|" + "---|" * len(keys)]
    for row in res["sizes"]:
        lines.append("| " + " | ".join(str(row.get(k, "")) for k in keys) + " |")
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    notes = out.read_text().partition(NOTES)[2] if out.exists() else ""          # what a reader wrote below the table stays
    out.write_text("\n".join(lines) + "\n" + (NOTES + notes if notes else ""))


if __name__ == "__main__":
    main()
