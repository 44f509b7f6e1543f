"""Numpy restatement of the bundle adjuster's robust mode (include/lightglue_amd.h, lg_bundle_adjust_robust), float64: the loss and its weight, the weighted
linearisation (A, B and r scaled by sqrt(w) once), the stages, the filter between them, the rebuild of the lists and every output.  It shares the small pieces
and the scenes of tests/bundle_oracle.py (which it does not edit) and runs the prescribed Schur complement + Cholesky in the definition's ascending orders.
Every decision within a relative NEAR of its bar is recorded in `near`: those of tests/bundle_oracle.py plus every Huber branch (|s - c c|) and every filter
test (|s - e e|).  Also the scenes of tests/test_bundle_robust_cpu.py and tests/test_gpu_bundle_robust.py.  No GPU, no torch."""
import functools

import numpy as np

import bundle_oracle as B
import triangulate_oracle as O
from abspose_oracle import rodrigues
from bundle_oracle import ACTIVE, NEAR, SHORT

FILTERED = 7
LOSSES = ("squared", "huber", "cauchy")
MAX_FILTER_ROUNDS = 4
LOSS_SCALE, MAX_REPROJ_ERROR = 2.0, 4.0


def rho_and_weight(loss, s, c, near):
    """(rho(s), w(s)) of the definition; s = rx rx + ry ry"""
    if loss == "squared":
        return s, 1.0
    c2 = c * c
    if loss == "huber":
        if abs(s - c2) <= NEAR * c2:
            near.append("huber branch")
        if s <= c2:
            return s, 1.0
        return (2.0 * c) * np.sqrt(s) - c2, c / np.sqrt(s)
    assert loss == "cauchy", loss
    return c2 * np.log1p(s / c2), 1.0 / (1.0 + s / c2)


def adjust(inp, loss="squared", loss_scale=LOSS_SCALE, filter_rounds=0, max_reproj_error=MAX_REPROJ_ERROR, num_iterations=B.ITERATIONS,
           initial_damping=B.DAMPING, function_tolerance=B.TOLERANCE):
    """inp: as tests/bundle_oracle.py adjust -> its dict plus num_filtered, num_filter_stages, first_state (the node states of the first stage) and
    free_end / adjusted_end; `free` and `adjusted` are "in any stage" (what decides whether the last accepted state or the input bits come back)"""
    assert loss in LOSSES and 0 <= filter_rounds <= MAX_FILTER_ROUNDS
    c, e2 = float(loss_scale), float(max_reproj_error) * float(max_reproj_error)
    kpts = np.asarray(inp["kpts"], np.float32)
    K, N = kpts.shape[:2]
    tid = np.asarray(inp["track_id"], np.int64).reshape(K, N)
    xyz32 = np.asarray(inp["xyz"], np.float32).reshape(-1, 3)
    T = len(xyz32)
    cams32, poses32 = np.asarray(inp["cams"], np.float32), np.asarray(inp["poses"], np.float32)
    ok = np.array([O.image_ok(cams32[k], poses32[k]) for k in range(K)])
    cam = cams32.astype(np.float64)
    P = np.where(ok[:, None, None], poses32.astype(np.float64), 0.0)
    X = xyz32.astype(np.float64)
    live = O.live_rows(inp.get("num"), K, N)
    constant = np.asarray(inp["constant"], bool)
    near = []
    state = np.zeros((K, N), np.uint8)
    with np.errstate(all="ignore"):
        for k in range(K):
            for i in range(live[k]):
                j = int(tid[k, i])
                if not 0 <= j < T:
                    continue
                if not ok[k]:
                    state[k, i] = B.BAD_IMAGE
                elif not np.isfinite(X[j]).all():
                    state[k, i] = B.NON_FINITE
                else:
                    p = B.project(P[k], X[j])
                    if abs(p[2]) <= NEAR * np.linalg.norm(p):
                        near.append("behind at the start")
                    state[k, i] = ACTIVE if p[2] > 0 else B.BEHIND

    sets = {}

    def rebuild():
        """the tracks' lists, the rows of every image and the free images from the nodes in state 1 (ascending node order)"""
        cand = [[] for _ in range(T)]
        for k, i in np.argwhere(state == ACTIVE):
            cand[tid[k, i]].append((int(k), int(i)))
        adjusted = np.array([2 <= len(cd) <= B.MAX_LEN for cd in cand], bool)
        for j, cd in enumerate(cand):
            if not adjusted[j]:
                for k, i in cd:
                    state[k, i] = SHORT if len(cd) < 2 else B.TOO_LONG
        active = state == ACTIVE
        sets.update(adjusted=adjusted, active=active, free=ok & ~constant & active.any(1), rows_of=[np.flatnonzero(active[k]).tolist() for k in range(K)],
                    obs_of=[cd if adjusted[j] else [] for j, cd in enumerate(cand)])

    def cost_of(Ps, Xs):
        total, failed = 0.0, False
        with np.errstate(all="ignore"):
            for k in range(K):
                sk = 0.0
                for i in sets["rows_of"][k]:
                    p = B.project(Ps[k], Xs[tid[k, i]])
                    r = B.residual(cam[k], p, kpts[k, i])
                    s = r[0] * r[0] + r[1] * r[1]
                    if abs(p[2]) <= NEAR * np.linalg.norm(p):
                        near.append("pz = 0")
                    if not p[2] > 0 or not np.isfinite(s):
                        failed, s = True, 0.0
                    sk += rho_and_weight(loss, s, c, near)[0]
                total += sk
        return total, failed

    def step(Ps, Xs, lam):
        """tests/bundle_oracle.py step with the weighted linearisation: (pose steps [K, 6], point steps [T, 3]) or None if a pivot failed"""
        rows_of, obs_of, free, adjusted = sets["rows_of"], sets["obs_of"], sets["free"], sets["adjusted"]
        lin = {}
        U, gc = np.zeros((K, 6, 6)), np.zeros((K, 6))
        for k in range(K):
            for i in rows_of[k]:
                p = B.project(Ps[k], Xs[tid[k, i]])
                A, Bm = B.jacobians(Ps[k], cam[k], p)
                r = B.residual(cam[k], p, kpts[k, i])
                if loss != "squared":
                    sw = np.sqrt(rho_and_weight(loss, r[0] * r[0] + r[1] * r[1], c, near)[1])
                    A, Bm, r = sw * A, sw * Bm, sw * r
                lin[k, i] = (A, Bm, r)
                U[k] += A.T @ A
                gc[k] += A.T @ r
        V, gp = np.zeros((T, 3, 3)), np.zeros((T, 3))
        for j in range(T):
            for k, i in obs_of[j]:
                A, Bm, r = lin[k, i]
                V[j] += Bm.T @ Bm
                gp[j] += Bm.T @ r
        for k in range(K):
            for d in range(6):
                U[k, d, d] = B.damped(U[k, d, d], lam)
        for j in range(T):
            for d in range(3):
                V[j, d, d] = B.damped(V[j, d, d], lam)
        W = lambda k, i: lin[k, i][0].T @ lin[k, i][1]
        tracks = np.flatnonzero(adjusted)
        Vi, y = np.zeros((T, 3, 3)), np.zeros((T, 3))
        for j in tracks:
            for col in range(3):
                x = B.solve3(V[j], np.eye(3)[col], near)
                if x is None:
                    return None
                Vi[j][:, col] = x
            y[j] = Vi[j] @ gp[j]
        S, rhs = np.zeros((6 * K, 6 * K)), np.zeros(6 * K)
        for a in range(K):
            sa = slice(6 * a, 6 * a + 6)
            if not free[a]:
                S[sa, sa] = np.eye(6)
                continue
            E, wy = np.zeros((K, 6, 6)), np.zeros(6)
            for i in rows_of[a]:
                j = tid[a, i]
                Y = W(a, i) @ Vi[j]
                wy += W(a, i) @ y[j]
                for b, i2 in obs_of[j]:
                    if free[b] and b <= a:
                        E[b] += Y @ W(b, i2).T
            for b in range(a + 1):
                if free[b]:
                    S[sa, 6 * b:6 * b + 6] = (U[a] if b == a else 0.0) - E[b]
            rhs[sa] = wy - gc[a]
        L = B.cholesky(S, near)
        if L is None:
            return None
        s = B.substitute(L, rhs).reshape(K, 6)
        dX = np.zeros((T, 3))
        for j in tracks:
            acc = np.zeros(3)
            for k, i in obs_of[j]:
                if free[k]:
                    acc += W(k, i).T @ s[k]
            dX[j] = -(y[j] + Vi[j] @ acc)
        return s, dX

    rebuild()
    first_state = state.copy()
    ever_free, ever_adjusted = sets["free"].copy(), sets["adjusted"].copy()
    cost, _ = cost_of(P, X)
    initial, lam, iters, accepted, converged, costs = cost, float(initial_damping), 0, 0, False, [cost]
    filtered, fstages = 0, 0
    for stage in range(filter_rounds + 1):
        if stage:
            removed = 0
            with np.errstate(all="ignore"):
                for k in range(K):
                    for i in sets["rows_of"][k]:
                        r = B.residual(cam[k], B.project(P[k], X[tid[k, i]]), kpts[k, i])
                        s = r[0] * r[0] + r[1] * r[1]
                        if abs(s - e2) <= NEAR * e2:
                            near.append("filter")
                        if s > e2:
                            state[k, i] = FILTERED
                            removed += 1
            rebuild()
            ever_free |= sets["free"]              # nothing new can appear; kept for symmetry with the definition's wording
            ever_adjusted |= sets["adjusted"]
            if removed:
                cost, _ = cost_of(P, X)
                lam, converged, filtered, fstages = float(initial_damping), False, filtered + removed, fstages + 1
                costs.append(cost)
        for _ in range(num_iterations):
            if converged:
                break
            iters += 1
            with np.errstate(all="ignore"):
                st = step(P, X, lam)
            good = st is not None
            if good:
                s, dX = st
                Pt, Xt = P.copy(), X + dX
                for k in np.flatnonzero(sets["free"]):
                    Q = rodrigues(s[k, :3])
                    Pt[k] = np.concatenate([Q @ P[k][:, :3], (Q @ P[k][:, 3] + s[k, 3:])[:, None]], 1)
                new, failed = cost_of(Pt, Xt)
                good = not failed and np.isfinite(Pt).all() and np.isfinite(Xt[sets["adjusted"]]).all() and np.isfinite(new)
            conv = accept = False
            if good:
                bar = function_tolerance * cost
                if abs(abs(cost - new) - bar) <= NEAR * bar:
                    near.append("convergence")
                if abs(cost - new) <= NEAR * cost:
                    near.append("accept")
                conv, accept = abs(cost - new) <= bar, new < cost
            if accept:
                P, X, cost, accepted, lam = Pt, Xt, new, accepted + 1, max(lam / 10.0, 1e-12)
                costs.append(cost)
            else:
                lam = min(10.0 * lam, 1e12)
            converged = bool(conv)
    active = sets["active"]
    pts, err = np.full((K, N, 3), np.nan), np.full((K, N), np.nan)
    for k in range(K):
        for i in np.flatnonzero(active[k]):
            pts[k, i] = X[tid[k, i]]
            r = B.residual(cam[k], B.project(P[k], X[tid[k, i]]), kpts[k, i])
            err[k, i] = np.sqrt(r[0] * r[0] + r[1] * r[1])
    poses64 = np.where(ever_free[:, None, None], P, poses32.astype(np.float64))
    xyz64 = np.where(ever_adjusted[:, None], X, xyz32.astype(np.float64))
    return dict(poses64=poses64, xyz64=xyz64, points3d64=pts, node_state=state, error64=err, initial_cost=initial, final_cost=cost, num_iterations=iters,
                num_accepted=accepted, converged=converged, num_observations=int(active.sum()), status=np.where(ok, B.LG_OK, B.LG_ERR_CAMERA), free=ever_free,
                adjusted=ever_adjusted, free_end=sets["free"], adjusted_end=sets["adjusted"], first_state=first_state, num_filtered=filtered,
                num_filter_stages=fstages, costs=costs, near=near)


def scales(inp, out):
    """tests/bundle_oracle.py scales over the observations of the FIRST stage: a track that a filter took out of the adjustment keeps the scale it moved under"""
    return B.scales(inp, dict(out, node_state=out["first_state"]))


# ---------------------------------------------------------------------- the planted scene: the main scene with `count` keypoints moved by 20 .. 80 pixels
PLANT_SEED = 5


@functools.lru_cache(maxsize=None)
def planted_scene(draws=14):
    """-> (input, planted nodes [(k, i)], truth [T, 3]).  Of the labelled nodes whose track has at least 3 labelled nodes, in ascending (k, i), `draws` are
    chosen without replacement; in that order, skipping a node whose track already has one, an angle uniform in [0, 2 pi) and then a distance uniform in
    [20, 80) move the keypoint.  draws = 14 plants 12 of the 212 observations, draws = 30 plants 23"""
    sc = B.main_scene()
    inp = B.oracle_input(sc)
    rng = np.random.default_rng(PLANT_SEED)
    tid = inp["track_id"]
    length = np.bincount(tid[tid >= 0], minlength=len(inp["xyz"]))
    nodes = [(int(k), int(i)) for k, i in np.argwhere(tid >= 0) if length[tid[k, i]] >= 3]
    kpts, taken, planted = inp["kpts"].copy(), set(), []
    for at in rng.choice(len(nodes), draws, replace=False):
        k, i = nodes[at]
        if int(tid[k, i]) in taken:
            continue
        taken.add(int(tid[k, i]))
        angle = rng.uniform(0.0, 2.0 * np.pi)
        dist = rng.uniform(20.0, 80.0)
        kpts[k, i] = (kpts[k, i].astype(np.float64) + dist * np.array([np.cos(angle), np.sin(angle)])).astype(np.float32)
        planted.append((k, i))
    return dict(inp, kpts=kpts), sorted(planted), sc["truth"]


def point_errors(inp, out, truth):
    """the distance of every track adjusted at the end from the truth"""
    adj = out["adjusted_end"]
    return np.linalg.norm(out["xyz64"] - truth, axis=1)[adj]


# ---------------------------------------------------------------------- edge scenes of the filter
@functools.lru_cache(maxsize=None)
def short_scene():
    """the main scene with one observation of a TWO-view track moved by 50 pixels: under the Cauchy loss the point stays with the good observation, the filter
    takes the moved one and the good one is left alone in its track (state 5) -> (input, the moved node, the node left alone, the track)"""
    inp = B.oracle_input(B.main_scene())
    tid = inp["track_id"]
    length = np.bincount(tid[tid >= 0], minlength=len(inp["xyz"]))
    j = int(np.flatnonzero(length == 2)[-1])
    (k0, i0), (k1, i1) = [(int(k), int(i)) for k, i in np.argwhere(tid == j)]
    kpts = inp["kpts"].copy()
    kpts[k1, i1] = kpts[k1, i1] + np.array([40.0, 30.0], np.float32)
    return dict(inp, kpts=kpts), (k1, i1), (k0, i0), j


LAST_IMAGE, LAST_KEEP, LAST_SHIFT = 5, 7, 15.0


@functools.lru_cache(maxsize=None)
def last_observation_scene():
    """the main scene with image 5 (free) left with seven labelled rows, all of tracks with at least 4 labelled nodes, whose keypoints are moved by 15 pixels
    in seven directions (0.3 + 4 pi q / 7): no pose explains them.  With ONE iteration per stage (LAST below; a free pose given ten would end up fitting three
    of them exactly) all seven are still above 4 pixels at the filter, which takes them, and the image stops being free with the pose it had reached
    -> (input, the seven nodes)"""
    inp = B.oracle_input(B.main_scene())
    tid = inp["track_id"].copy()
    length = np.bincount(tid[tid >= 0], minlength=len(inp["xyz"]))
    rows = [int(i) for i in np.flatnonzero(tid[LAST_IMAGE] >= 0) if length[tid[LAST_IMAGE, i]] >= 4][:LAST_KEEP]
    assert len(rows) == LAST_KEEP
    keep = tid[LAST_IMAGE, rows].copy()
    tid[LAST_IMAGE] = -1
    tid[LAST_IMAGE, rows] = keep
    angle = 0.3 + 4.0 * np.pi * np.arange(LAST_KEEP) / LAST_KEEP
    kpts = inp["kpts"].copy()
    kpts[LAST_IMAGE, rows] = kpts[LAST_IMAGE, rows] + (LAST_SHIFT * np.stack([np.cos(angle), np.sin(angle)], 1)).astype(np.float32)
    return dict(inp, kpts=kpts, track_id=tid), [(LAST_IMAGE, i) for i in rows]


# ---------------------------------------------------------------------- the chain: contaminated matches -> plain triangulation -> robust adjustment -> localisation
CHAIN_MAX_REPROJ_ERROR, CHAIN_PLANTED = 64.0, 8


@functools.lru_cache(maxsize=None)
def chain_scene():
    """tests/bundle_oracle.py's chain scene (five images with slightly wrong poses, triangulated with a generous bar) in which eight matches lead to
    mislocalised detections: in images 2, 3 and 4, eight keypoints of different tracks with at least 3 views among images 0 .. 4 are moved by 20 .. 50
    pixels.  -> its dict with `kpts` replaced and `moved`: the nodes"""
    sc = B.chain_scene()
    rng = np.random.default_rng(PLANT_SEED)
    rows = sc["planted"]["rows"]
    tracks = [j for j, at in enumerate(rows) if sum(k < 5 for k in at) >= 3]
    kpts, moved = sc["kpts"].copy(), []
    for j in rng.choice(tracks, CHAIN_PLANTED, replace=False):
        k = int(rng.choice([k for k in rows[j] if 2 <= k < 5]))
        angle, dist = rng.uniform(0.0, 2.0 * np.pi), rng.uniform(20.0, 50.0)
        kpts[k, rows[j][k]] = (kpts[k, rows[j][k]].astype(np.float64) + dist * np.array([np.cos(angle), np.sin(angle)])).astype(np.float32)
        moved.append((k, int(rows[j][k])))
    return dict(sc, kpts=kpts, moved=sorted(moved))


# ---------------------------------------------------------------------- the calls the tests share (read-only)
CAUCHY = dict(loss="cauchy", loss_scale=2.0)
HUBER = dict(loss="huber", loss_scale=2.0)
ONE_ROUND = dict(filter_rounds=1, max_reproj_error=4.0)
LAST = dict(CAUCHY, **ONE_ROUND, num_iterations=1)
SCENES = {"planted": lambda: planted_scene()[0], "planted 23": lambda: planted_scene(30)[0], "short": lambda: short_scene()[0],
          "last": lambda: last_observation_scene()[0], "main": B.GPU_SCENES["main"], "K = 9": B.GPU_SCENES["K = 9"], "edge": B.GPU_SCENES["edge"],
          "edge clean": B.GPU_SCENES["edge clean"], "long": B.GPU_SCENES["long"]}


@functools.lru_cache(maxsize=None)
def _answer(name, conf):
    return adjust(SCENES[name](), **dict(conf))


def answer(name, **conf):
    """The definition's answer on a scene of SCENES (shared by the tests; treat as read-only)"""
    return _answer(name, tuple(sorted(conf.items())))
