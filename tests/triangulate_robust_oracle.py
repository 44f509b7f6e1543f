"""Numpy restatement of the triangulator's robust mode (include/lightglue_amd.h, lg_triangulate_robust), float64.  Nodes, edges, components, the image records,
the linear start, the residual and the fit with its acceptance tests are those of tests/triangulate_oracle.py; the rounds are restated here with a selection of
its own: the hypotheses are read off the enumerated list of index pairs (no closed form), the score is a set of images, the consensus a dictionary per image.
A component is `near` when the oracle alone places it within a relative NEAR of a decision: an observation's error under ANY hypothesis within
NEAR x max_reproj_error of the bar (a score could differ), two passing candidates of one image under the winner within a relative NEAR of each other (the
consensus could differ), or a fit that `classify` reports near.  Also the scenes of tests/test_gpu_triangulate_robust.py, built without a GPU.  No GPU, no torch."""
import functools
import itertools

import numpy as np

import triangulate_oracle as O
from triangulate_oracle import NEAR, classify, components, edges, record, residual, start_point, tracks_of

OUTLIER = 8
NUM_HYPOTHESES, MAX_TRACKS = 64, 2


def hypotheses(L, num_hypotheses):
    """the index pairs a round over L nodes tries, in the order of their numbers h"""
    every = list(itertools.combinations(range(L), 2))                   # lexicographic
    Q = len(every)
    return every if Q <= num_hypotheses else [every[h * Q // num_hypotheses] for h in range(num_hypotheses)]


def errors(obs, X):
    """[L]: the reprojection error of every observation at X, inf where pz <= 0 or the error is not a number"""
    out = []
    for xy, rec in obs:
        rx, ry, pz = residual(xy, rec, X)
        e = np.sqrt(rx * rx + ry * ry) if pz > 0 else np.inf
        out.append(e if e == e else np.inf)
    return np.asarray(out)


def one_round(rest, flat, recs, N, max_err, min_angle, refine_on, num_hypotheses):
    """-> (state, consensus nodes (ascending) or None, X, mean error, near)"""
    obs = [(flat[v], recs[v // N]) for v in rest]
    image = [int(v) // N for v in rest]
    best, near = None, False
    for h, (i, j) in enumerate(hypotheses(len(rest), num_hypotheses)):
        if image[i] == image[j]:
            continue
        X = start_point([obs[i], obs[j]])
        if X is None:
            continue
        err = errors(obs, X)
        near = near or bool((abs(err - max_err) <= NEAR * max_err).any())
        score = len({image[q] for q in np.flatnonzero(err <= max_err)})
        if best is None or score > best[0]:                             # ties: the lowest h stays
            best = (score, h, err)
    if best is None:
        return O.DEGENERATE, None, None, None, near
    if best[0] < 2:
        return O.REPROJECTION, None, None, None, near
    chosen = {}                                                         # image -> (error, position); strict <: a tie keeps the lowest node
    for q in np.flatnonzero(best[2] <= max_err):
        e = best[2][q]
        if image[q] in chosen:
            near = near or abs(e - chosen[image[q]][0]) < NEAR * max(e, chosen[image[q]][0])
        if image[q] not in chosen or e < chosen[image[q]][0]:
            chosen[image[q]] = (e, q)
    picked = sorted(q for _, q in chosen.values())
    state, X, mean, fit_near = classify([obs[q] for q in picked], max_err, min_angle, refine_on)
    return state, np.asarray([rest[q] for q in picked], int), X, mean, near or fit_near


def triangulate(inp, max_err=O.MAX_ERR, min_angle=O.MIN_ANGLE, max_len=O.MAX_LEN, refine_on=True, num_hypotheses=NUM_HYPOTHESES, max_tracks=MAX_TRACKS):
    """inp as tests/triangulate_oracle.py's.  -> its dict (state_counts [8]: the tracks at [1], the components whose round 0 failed at their state; tracks:
    [(name, nodes, round-0 state, near, whole: the round-0 consensus is the component)]; names [T]: the component of every numbered track) plus num_outliers,
    num_split"""
    kpts = np.asarray(inp["kpts"], np.float32)
    K, N = kpts.shape[:2]
    ok = np.array([O.image_ok(inp["cams"][k], inp["poses"][k]) for k in range(K)])
    edge_set, status = edges(inp["pairs"], inp["matches0"], K, N, inp.get("num"), ok)
    name = components(K * N, edge_set)
    recs = [record(inp["cams"][k], inp["poses"][k]) if ok[k] else None for k in range(K)]
    flat, bar = kpts.reshape(-1, 2), np.float64(np.float32(max_err))
    pts, tid, state = np.full((K * N, 3), np.nan, np.float32), np.full(K * N, -1, np.int64), np.zeros(K * N, np.uint8)
    xyz, lengths, errs, names, listed, counts, outliers, split = [], [], [], [], [], np.zeros(8, int), 0, 0
    for root, nodes in tracks_of(name):
        if len(nodes) > max_len:
            counts[O.TOO_LONG] += 1
            state[nodes] = O.TOO_LONG
            listed.append((root, nodes, O.TOO_LONG, False, False))
            continue
        rest, made, near, first, whole = np.sort(nodes), 0, False, None, False
        for rnd in range(max_tracks):
            st, picked, X, mean, rnear = one_round(rest, flat, recs, N, bar, min_angle, refine_on, num_hypotheses)
            near = near or rnear
            if rnd == 0:
                first, whole = st, picked is not None and len(picked) == len(nodes)
            if st != O.DONE:
                break
            tid[picked], pts[picked], state[picked] = len(names), X.astype(np.float32), O.DONE
            names.append(root); lengths.append(len(picked)); xyz.append(X); errs.append(mean)
            made += 1
            rest = np.setdiff1d(rest, picked)
            if len(rest) < 2:
                break
        if first != O.DONE:
            counts[first] += 1
            state[nodes] = first
        else:
            left = nodes[state[nodes] != O.DONE]
            state[left] = OUTLIER
            outliers += len(left)
            split += made > 1
        listed.append((root, nodes, first, near, whole))
    counts[O.DONE] = len(names)
    xyz64, err64 = np.asarray(xyz, np.float64).reshape(-1, 3), np.asarray(errs, np.float64)
    return dict(points3d=pts.reshape(K, N, 3), track_id=tid.reshape(K, N), node_state=state.reshape(K, N), num_tracks=len(names), xyz=xyz64.astype(np.float32),
                xyz64=xyz64, track_length=np.asarray(lengths, int), track_error=err64.astype(np.float32), error64=err64, state_counts=counts, status=status,
                tracks=listed, names=np.asarray(names, int), num_outliers=outliers, num_split=int(split))


# ---------------------------------------------------------------------- the stray scene: K = 8, N = 96, 60 planted tracks of 3 - 8 views, all 28 pairs, 20 wrong
# matches to free rows (tracks 0 .. 19) and 5 wrong matches that merge two tracks each (20/21 .. 28/29)
STRAY_K, STRAY_TRACKS, STRAYS, MERGES = 8, 60, 20, 5
STRAY_PAIRS = [(a, b) for a in range(STRAY_K) for b in range(a + 1, STRAY_K)]


def tie(m0, at, a, ra, b, rb):
    """one match between row ra of image a and row rb of image b, written into the pair's row of matches0 whichever way the pair is listed; what either row was
    matched to in that pair before is gone, so matches0 stays one-to-one"""
    if a > b:
        a, ra, b, rb = b, rb, a, ra
    row = m0[at[a, b]]
    row[row == rb] = -1
    row[ra] = rb


@functools.lru_cache(maxsize=None)
def stray_scene():
    """-> the oracle's input dict plus `planted`, `strays` (the 20 free rows wrongly tied to the tracks 0 .. 19) and `merged` [(track, track)].  The stray of an
    even track lies in an image that does not see the track (the highest such image), tied to the track's lowest image.  The stray of an odd track, and of an
    even track that every image sees, lies in the track's highest image, tied to the track's lowest image: the component holds two rows of that image, which is
    a conflict in lg_triangulate.  A merge is one match from track j in its lowest image to track j + 1 in that track's highest other image."""
    poses, cams = O.cameras(count=STRAY_K)
    rng = np.random.default_rng(3)
    views = O.random_views(STRAY_K, STRAY_TRACKS, rng, lo=3)
    pl = O.plant(poses, cams, views, 21, num=(O.N,) * STRAY_K)
    m0 = O.match_rows(STRAY_PAIRS, pl["rows"])
    at = {pair: p for p, pair in enumerate(STRAY_PAIRS)}
    free, rows, strays = [list(v) for v in pl["free"]], pl["rows"], []
    for j in range(STRAYS):
        unseen = [k for k in range(STRAY_K) if k not in rows[j]]
        k, anchor = (max(unseen) if j % 2 == 0 and unseen else max(rows[j])), min(rows[j])
        row = free[k].pop()
        tie(m0, at, anchor, rows[j][anchor], k, row)
        strays.append(k * O.N + row)
    merged = []
    for j in range(STRAYS, STRAYS + 2 * MERGES, 2):
        a = min(rows[j])
        b = max(k for k in rows[j + 1] if k != a)
        tie(m0, at, a, rows[j][a], b, rows[j + 1][b])
        merged.append((j, j + 1))
    inp = dict(kpts=pl["kpts"], num=None, pairs=np.asarray(STRAY_PAIRS), matches0=m0, cams=cams, poses=poses)
    return dict(inp, planted=pl, strays=np.asarray(strays), merged=merged)


# ---------------------------------------------------------------------- the stride scene: 12 cameras, 8 tracks seen by all, three strays each: L = 15, Q = 105
WIDE_K, WIDE_TRACKS, WIDE_STRAYS = 12, 8, 3
WIDE_PAIRS = [(a, b) for a in range(WIDE_K) for b in range(a + 1, WIDE_K)]


@functools.lru_cache(maxsize=None)
def wide_scene():
    """-> the oracle's input dict plus `planted` and `strays`: every track is seen by all 12 images and takes a free row of the images 1, 4 and 7, each matched
    onto the track's row in the next image (components of 15 nodes with three conflicts each)"""
    poses, cams = O.cameras(count=WIDE_K, seed=4)
    views = [list(range(WIDE_K))] * WIDE_TRACKS
    pl = O.plant(poses, cams, views, 27, num=(O.N,) * WIDE_K)
    m0 = O.match_rows(WIDE_PAIRS, pl["rows"])
    at = {pair: p for p, pair in enumerate(WIDE_PAIRS)}
    free, strays = [list(v) for v in pl["free"]], []
    for j in range(WIDE_TRACKS):
        for s in range(WIDE_STRAYS):                                    # a free row of image k = 3 s + 1, matched onto the track's row in image k + 1
            k = 3 * s + 1
            row = free[k].pop()
            tie(m0, at, k, row, k + 1, pl["rows"][j][k + 1])
            strays.append(k * O.N + row)
    inp = dict(kpts=pl["kpts"], num=None, pairs=np.asarray(WIDE_PAIRS), matches0=m0, cams=cams, poses=poses)
    return dict(inp, planted=pl, strays=np.asarray(strays))


# ---------------------------------------------------------------------- shared answers (treat as read-only)
BIG_CONF = dict(max_len=1024, num_hypotheses=256, max_tracks=4)


@functools.lru_cache(maxsize=None)
def answer(scene, num_hypotheses=NUM_HYPOTHESES, max_tracks=MAX_TRACKS):
    """the definition's answer on a named scene"""
    if scene == "big":
        return triangulate(O.big_component(), **BIG_CONF)
    inp = {"stray": stray_scene, "wide": wide_scene, "main": O.main_scene, "bad cameras": lambda: O.bad_camera_scene()[0]}[scene]()
    return triangulate(O.oracle_input(inp), num_hypotheses=num_hypotheses, max_tracks=max_tracks)
