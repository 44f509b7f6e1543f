"""Numpy restatement of the global pose estimator's definition (include/lightglue_amd.h, lg_posegraph_solve), float64: pair states, the adjacency, the
breadth-first tree, rotation averaging, which images get a position, position averaging, the outputs.  Sums over pairs run vectorised here (in pair order,
not in the device's (neighbour, pair) order: the difference is rounding of float64, far below the float32 outputs).  Also the scenes of
tests/test_posegraph_cpu.py and tests/test_gpu_posegraph.py, built on the cameras of tests/triangulate_oracle.py."""
import functools

import numpy as np

import triangulate_oracle as O

USED, BAD_INDEX, NO_MODEL, OUTSIDE, ROTATION_OUTLIER, NO_POSITION = 0, 1, 2, 3, 4, 5          # pair_state
POSED, ROTATION_ONLY, NOT_CONNECTED = 0, 1, 2                                                # image_state
ROTATION_TOL, SMALL_SINE, PIVOT_FLOOR = 1e-3, 1e-6, 1e-10
ROT_DONE, POS_DONE, MIN_SQ = 1e-10, 1e-12, 1e-12
# A converged stage's step is the rounding of its fp64 solve: on the exact scenes below the position step settles between 4e-14 and 6e-11 and moves by up to
# 70 x from one iteration to the next (K = 49: 5.7e-11, 2.5e-12, 7.0e-12, 3.5e-11, 8.5e-13), around the bar 1e-12; the rotation step settles at 5e-17.  So
# `estimate` runs the definition twice, the second time with every system solved by LU (np.linalg.solve) in place of the Cholesky.  A tested step that is
# rounding (the two runs differ by more than NEAR_NOISE of it) and lies within NEAR_FACTOR of the bar (the spread seen above, rounded up) is decided by
# chance, as is a test the two runs decide differently: `near` names the stage.  A comparison of that stage's iteration count with another fp64
# implementation means nothing then (the outputs still agree: such steps are far below a float32 ulp).  First run on the device: K = 16 stopped after 8
# position iterations, this oracle after 7 with the steps 5.8e-14, 2.8e-13, 1.1e-13, 4.3e-14 before it
NEAR_FACTOR, NEAR_NOISE = 100.0, 0.01


# ---------------------------------------------------------------------- SO(3)
def so3_log(M):
    """[..., 3, 3] -> [..., 3]: theta = atan2(|v| / 2, (tr - 1) / 2), v the skew part; |v| < SMALL_SINE: v / 2 (tr >= 0) or 0 (tr < 0)"""
    v = np.stack([M[..., 2, 1] - M[..., 1, 2], M[..., 0, 2] - M[..., 2, 0], M[..., 1, 0] - M[..., 0, 1]], -1)
    tr = M[..., 0, 0] + M[..., 1, 1] + M[..., 2, 2]
    nv = np.sqrt((v * v).sum(-1))
    theta = np.arctan2(0.5 * nv, 0.5 * (tr - 1.0))
    small = nv < SMALL_SINE
    scale = np.where(small, np.where(tr < 0.0, 0.0, 0.5), theta / np.where(small, 1.0, nv))
    return v * scale[..., None]


def so3_exp(w):
    """Rodrigues, [..., 3] -> [..., 3, 3] (the bundle adjuster's form: I + sin(th) [k]x + (1 - cos(th)) [k]x^2, I for th = 0)"""
    w = np.asarray(w, np.float64)
    th = np.sqrt((w * w).sum(-1))
    k = w / np.where(th > 0.0, th, 1.0)[..., None]
    Kx = np.zeros(w.shape[:-1] + (3, 3))
    Kx[..., 0, 1], Kx[..., 0, 2], Kx[..., 1, 0], Kx[..., 1, 2], Kx[..., 2, 0], Kx[..., 2, 1] = -k[..., 2], k[..., 1], k[..., 2], -k[..., 0], -k[..., 1], k[..., 0]
    return np.eye(3) + np.sin(th)[..., None, None] * Kx + (1.0 - np.cos(th))[..., None, None] * (Kx @ Kx)


def angle_to(d, e):
    """atan2(|e - (d . e) d|, d . e) for unit d"""
    de = (d * e).sum(-1)
    r = e - de[..., None] * d
    return np.arctan2(np.sqrt((r * r).sum(-1)), de)


# ---------------------------------------------------------------------- the Cholesky of the definition
def cholesky_solve(A, B, lu=False):
    """A x = B by A = L L^T (lower triangle of A read), a pivot that is not finite or not above PIVOT_FLOOR times its diagonal entry replaced by 1 -> x, ok"""
    n = len(A)
    A = np.tril(A) + np.tril(A, -1).T
    L = None
    try:
        L = np.linalg.cholesky(A)
        if not (np.diag(L) ** 2 > 4.0 * PIVOT_FLOOR * np.diag(A)).all():      # a pivot near the floor: decide it column by column
            L = None
    except np.linalg.LinAlgError:
        pass
    ok = True
    if L is None:
        L = np.zeros_like(A)
        for j in range(n):
            d = A[j, j] - L[j, :j] @ L[j, :j]
            if not (np.isfinite(d) and d > PIVOT_FLOOR * A[j, j]):
                ok, d = False, 1.0
            L[j, j] = np.sqrt(d)
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    if lu and ok:
        return np.linalg.solve(A, B), ok
    z = np.linalg.solve(L, B)
    return np.linalg.solve(L.T, z), ok


# ---------------------------------------------------------------------- the definition
def classify(pairs, R, t, w, num_inliers, min_inliers, K):
    P = len(pairs)
    state = np.zeros(P, np.uint8)
    a, b = pairs[:, 0], pairs[:, 1]
    with np.errstate(invalid="ignore", over="ignore"):
        RtR = np.swapaxes(R, 1, 2) @ R
        rot = np.isfinite(R).all((1, 2)) & (abs(RtR - np.eye(3)).max((1, 2)) <= ROTATION_TOL) & (np.linalg.det(np.nan_to_num(R)) > 0.0)
        tt = (t * t).sum(1)
        good = rot & np.isfinite(t).all(1) & np.isfinite(tt) & (tt > 0.0) & np.isfinite(w) & (w > 0.0)
    if num_inliers is not None:
        good &= np.asarray(num_inliers) >= min_inliers
    state[~good] = NO_MODEL
    state[(a < 0) | (a >= K) | (b < 0) | (b >= K) | (a == b)] = BAD_INDEX
    return state


def adjacency(pairs, usable, K):
    """per image the sorted list of (neighbour, pair)"""
    adj = [[] for _ in range(K)]
    for p in np.flatnonzero(usable):
        a, b = int(pairs[p, 0]), int(pairs[p, 1])
        adj[a].append((b, int(p)))
        adj[b].append((a, int(p)))
    return [sorted(x) for x in adj]


def estimate(pairs, R, t, K, **kw):
    """the definition, and which of its two convergence decisions rounding decides (`near`)"""
    out, other = estimate_once(pairs, R, t, K, **kw), estimate_once(pairs, R, t, K, lu=True, **kw)
    near = []
    for stage, bar in (("rotation", ROT_DONE), ("position", POS_DONE)):
        x, y = out["steps"][stage], other["steps"][stage]
        if len(x) != len(y) or any(abs(u - v) > NEAR_NOISE * u and bar / NEAR_FACTOR < u < bar * NEAR_FACTOR for u, v in zip(x, y)):
            near.append(stage)
    with np.errstate(invalid="ignore"):
        own = {k: float(np.nan_to_num(abs(out[k] - other[k])).max()) for k in ("rotation_error64", "direction_error64")}
    return dict(out, near=near, own=own)


def estimate_once(pairs, R, t, K, origin=0, baseline=None, weights=None, num_inliers=None, num_iterations=12, rotation_scale=5.0, max_rotation_error=15.0,
                  direction_scale=5.0, min_inliers=15, lu=False):
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    P, n = len(pairs), int(num_iterations)
    R, t = np.asarray(R, np.float64).reshape(P, 3, 3), np.asarray(t, np.float64).reshape(P, 3)
    if weights is None:
        weights = np.ones(P) if num_inliers is None else np.asarray(num_inliers, np.float64)
    w = np.asarray(weights, np.float64)
    state = classify(pairs, R, t, w, num_inliers, min_inliers, K)
    adj = adjacency(pairs, state == USED, K)
    a, b = np.clip(pairs[:, 0], 0, K - 1), np.clip(pairs[:, 1], 0, K - 1)

    # 2. the tree
    level = np.full(K, -1)
    Rot = np.tile(np.eye(3), (K, 1, 1))
    level[origin] = 0
    L = 0
    while True:
        found = []
        for i in range(K):
            if level[i] >= 0:
                continue
            best = None
            for j, p in adj[i]:
                if level[j] == L and (best is None or w[p] > w[best[1]]):
                    best = (j, p)
            if best is not None:
                found.append((i,) + best)
        if not found:
            break
        for i, j, p in found:
            Rot[i] = R[p] @ Rot[j] if pairs[p, 1] == i else R[p].T @ Rot[j]
            level[i] = L + 1
        L += 1
    inside = level >= 0
    state[(state == USED) & ~inside[a]] = OUTSIDE
    live = state == USED

    # 3. rotation averaging
    sigma0, rot_iters, steps = np.radians(rotation_scale), 0, dict(rotation=[], position=[])
    free = inside.copy()
    free[origin] = False
    la, lb, lw, lR = a[live], b[live], w[live], R[live]
    for it in range(n):
        mult = max(1.0, 2.0 ** (n - 5 - it))
        om = so3_log(np.swapaxes(Rot[lb], 1, 2) @ lR @ Rot[la])
        we = lw / (1.0 + ((om * om).sum(1) ** 0.5 / (sigma0 * mult)) ** 2)
        A, rhs = np.zeros((K, K)), np.zeros((K, 3))
        np.add.at(A, (la, la), we)
        np.add.at(A, (lb, lb), we)
        np.add.at(A, (la, lb), -we)
        np.add.at(A, (lb, la), -we)
        np.add.at(rhs, lb, we[:, None] * om)
        np.add.at(rhs, la, -we[:, None] * om)
        A[~free, :], A[:, ~free], rhs[~free] = 0.0, 0.0, 0.0
        A[~free, ~free] = 1.0
        delta, _ = cholesky_solve(A, rhs, lu)
        Rot[free] = Rot[free] @ so3_exp(delta[free])
        rot_iters = it + 1
        if mult == 1.0:
            steps["rotation"].append(abs(delta).max())
        if mult == 1.0 and abs(delta).max() < ROT_DONE:
            break
    rot_err = np.full(P, np.nan)
    rot_err[live] = np.degrees((so3_log(np.swapaxes(Rot[lb], 1, 2) @ lR @ Rot[la]) ** 2).sum(1) ** 0.5)
    state[live & (rot_err > max_rotation_error)] = ROTATION_OUTLIER
    live = state == USED

    # 4. the baseline and the images that get a position
    d = np.zeros((P, 3))
    d[live] = -np.einsum("pji,pj->pi", Rot[b[live]], t[live] / np.sqrt((t[live] ** 2).sum(1))[:, None])
    chosen = None
    for j, p in adj[origin]:
        if live[p] and (baseline is None or j == baseline) and (chosen is None or w[p] > w[chosen[1]]):
            chosen = (j, p)
    present = np.zeros(K, bool)
    C = np.zeros((K, 3))
    pos_iters, ok = 0, chosen is not None
    if ok:
        base, pb = chosen
        C[base] = d[pb] if pairs[pb, 0] == origin else -d[pb]
        present = inside.copy()
        while True:
            nxt = present.copy()
            for i in range(K):
                if present[i] and i not in (origin, base):
                    nxt[i] = len({j for j, p in adj[i] if live[p] and present[j]}) >= 2
            if (nxt == present).all():
                break
            present = nxt
        state[live & ~(present[a] & present[b])] = NO_POSITION
        live = state == USED
        # 5. position averaging
        la, lb, lw, ld = a[live], b[live], w[live], d[live]
        fre = present.copy()
        fre[[origin, base]] = False
        f3 = np.repeat(fre, 3)
        proj = np.eye(3) - ld[:, :, None] * ld[:, None, :]
        tau0 = np.radians(direction_scale)
        for it in range(n):
            mult = max(1.0, 2.0 ** (n - 6 - it))
            rho = np.ones(len(la))
            if it > 0:
                e = C[lb] - C[la]
                rho = 1.0 / np.maximum((e * e).sum(1), MIN_SQ) / (1.0 + (angle_to(ld, e) / (tau0 * mult)) ** 2)
            M = (lw * rho)[:, None, None] * proj
            A = np.zeros((K, 3, K, 3))
            for x, y, s in ((la, la, 1.0), (lb, lb, 1.0), (la, lb, -1.0), (lb, la, -1.0)):
                np.add.at(A, (x, slice(None), y, slice(None)), s * M)
            A = A.reshape(3 * K, 3 * K)
            rhs = -A[:, 3 * base:3 * base + 3] @ C[base]
            A[~f3, :], A[:, ~f3], rhs[~f3] = 0.0, 0.0, 0.0
            A[~f3, ~f3] = 1.0
            x, good = cholesky_solve(A, rhs[:, None], lu)
            x = x[:, 0].reshape(K, 3)
            ok = ok and good
            step = abs(x[fre] - C[fre]).max() if fre.any() else 0.0
            C[fre] = x[fre]
            pos_iters = it + 1
            if mult == 1.0:
                steps["position"].append(step)
            if mult == 1.0 and step < POS_DONE:
                break
    dir_err = np.full(P, np.nan)
    if ok:
        dir_err[live] = np.degrees(angle_to(d[live], C[b[live]] - C[a[live]]))
    poses = np.full((K, 3, 4), np.nan)
    poses[inside, :, :3] = Rot[inside]
    posed = present & ok
    poses[posed, :, 3] = -np.einsum("kij,kj->ki", Rot[posed], C[posed])
    image_state = np.where(posed, POSED, np.where(inside, ROTATION_ONLY, NOT_CONNECTED)).astype(np.uint8)
    return dict(poses64=poses, centres64=np.where(posed[:, None], C, np.nan), image_state=image_state, pair_state=state, rotation_error64=rot_err,
                direction_error64=dir_err, origin=int(origin), baseline=int(chosen[0]) if chosen else -1, num_posed=int(posed.sum()),
                rotation_iterations=rot_iters, position_iterations=pos_iters, positions_ok=bool(ok), steps=steps)


# ---------------------------------------------------------------------- scenes
def random_rotation(rng, degrees=None):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    return so3_exp(axis * (rng.uniform(0, np.pi) if degrees is None else np.radians(degrees)))


def in_gauge(poses, origin, baseline):
    """the poses (R | t) re-expressed so that `origin` is the identity and the centre of `baseline` lies at distance 1 -> R [K, 3, 3], centres [K, 3].  The
    float32 rotations are made orthonormal in float64 first (the nearest rotation: U V^T of the singular value decomposition)"""
    R = poses[:, :, :3].astype(np.float64)
    c = -np.einsum("kji,kj->ki", R, poses[:, :, 3].astype(np.float64))
    U, _, Vt = np.linalg.svd(R)
    R = U @ Vt
    s = np.linalg.norm(c[baseline] - c[origin])
    return R @ R[origin].T, (c - c[origin]) @ R[origin].T / s


def relative(Rg, cg, pairs):
    """exact (R_ab, t_ab) of the convention X_b = R X_a + t, t a unit direction"""
    a, b = pairs[:, 0], pairs[:, 1]
    Rab = Rg[b] @ np.swapaxes(Rg[a], 1, 2)
    t = -np.einsum("pij,pj->pi", Rg[b], cg[b] - cg[a])
    with np.errstate(invalid="ignore"):                    # a self pair has no direction
        return Rab, t / np.linalg.norm(t, axis=1)[:, None]


def view_graph(K, chords, rng):
    """a ring plus `chords` random chords, every image pair once, listed (low, high)"""
    have = {tuple(sorted((k, (k + 1) % K))) for k in range(K)}
    ring = sorted(have)
    extra = []
    room = K * (K - 1) // 2 - len(have)
    while len(extra) < min(chords, room):
        i, j = sorted(rng.choice(K, 2, replace=False).tolist())
        if (i, j) not in have:
            have.add((i, j))
            extra.append((i, j))
    return np.asarray(ring + extra, np.int64), len(ring)


@functools.lru_cache(maxsize=None)
def scene(K, seed=0, chords=None, noise=0.0, outliers=0.0, origin=0):
    """-> dict(pairs, R64, t64 (exact or noisy, float64), R, t (the same in float32), weights, K, origin, baseline, Rg, cg (the truth in the call's gauge),
    planted [P] bool: the chords replaced by random poses).  The baseline is the one the definition picks: the origin's neighbour over its heaviest pair."""
    rng = np.random.default_rng(9000 + 31 * K + seed)
    poses, _ = O.cameras(K, seed)
    pairs, ring = view_graph(K, 3 * K if chords is None else chords, rng)
    w = rng.integers(40, 400, len(pairs)).astype(np.float32)
    at_origin = [(-(w[p]), int(pairs[p, 0] + pairs[p, 1] - origin), p) for p in range(len(pairs)) if origin in pairs[p]]
    baseline = sorted(at_origin)[0][1]
    Rg, cg = in_gauge(poses, origin, baseline)
    Rab, t = relative(Rg, cg, pairs)
    planted = np.zeros(len(pairs), bool)
    if noise:
        for p in range(len(pairs)):
            Rab[p] = random_rotation(rng, rng.uniform(0.2, 1.0) * noise) @ Rab[p]
            t[p] = random_rotation(rng, rng.uniform(0.2, 1.0) * noise) @ t[p]
    if outliers:
        pick = ring + rng.choice(len(pairs) - ring, int(round(outliers * (len(pairs) - ring))), replace=False)
        planted[pick] = True
        for p in pick:
            Rab[p] = random_rotation(rng, rng.uniform(40.0, 180.0)) @ Rab[p]
            t[p] = random_rotation(rng) @ t[p]
    return dict(pairs=pairs, R64=Rab, t64=t, R=Rab.astype(np.float32), t=t.astype(np.float32), weights=w, K=K, origin=origin, baseline=baseline, Rg=Rg, cg=cg,
                planted=planted)


def against_truth(out, sc):
    """worst rotation error in degrees (no alignment: the origin is the identity on both sides) and the worst centre error after a similarity alignment, as a
    fraction of the scene's extent, over the posed images"""
    m = out["image_state"] == POSED
    rel = out["poses64"][m, :, :3] @ np.swapaxes(sc["Rg"][m], 1, 2)
    rot = np.degrees((so3_log(rel) ** 2).sum(1) ** 0.5).max()
    X, Y = out["centres64"][m], sc["cg"][m]
    mx, my = X.mean(0), Y.mean(0)
    U, S, Vt = np.linalg.svd((Y - my).T @ (X - mx))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    Q = U @ D @ Vt
    s = (S * np.diag(D)).sum() / ((X - mx) ** 2).sum()
    fit = s * (X - mx) @ Q.T + my
    extent = np.linalg.norm(Y.max(0) - Y.min(0))
    return float(rot), float(np.linalg.norm(fit - Y, axis=1).max() / extent)


def run(sc, exact=False, **kw):
    """the oracle on a scene: the float64 inputs (exact) or the float32 ones the device reads"""
    R, t = (sc["R64"], sc["t64"]) if exact else (sc["R"], sc["t"])
    kw.setdefault("origin", sc["origin"])
    return estimate(sc["pairs"], R, t, sc["K"], weights=sc["weights"], **kw)


def edge_scene():
    """-> (with, without, what): K = 12.  Images 0 .. 6 ring + chords; image 7 hangs on one pair (rotation only); images 8, 9, 10 a second component; image 11
    alone.  `with` adds a pair with an index outside the store, a self pair, an all-zero R, a zero t, and one pair listed again reversed (which DOES enter)."""
    sc = scene(7, seed=3, chords=8)
    poses, _ = O.cameras(12, 3)
    Rg, cg = in_gauge(poses, 0, sc["baseline"])
    pairs = np.concatenate([sc["pairs"], [(3, 7), (8, 9), (9, 10), (8, 10)]])
    R, t = relative(Rg, cg, pairs)
    w = np.concatenate([sc["weights"], [100, 90, 80, 70]]).astype(np.float32)
    # one pair listed again as (b, a): R^T, -R^T t
    p = len(sc["pairs"]) - 1
    a, b = pairs[p]
    pairs = np.concatenate([pairs, [(b, a)]])
    R = np.concatenate([R, R[p].T[None]])
    t = np.concatenate([t, (-R[p].T @ t[p])[None]])
    w = np.concatenate([w, [55]]).astype(np.float32)
    clean = dict(pairs=pairs, R=R.astype(np.float32), t=t.astype(np.float32), weights=w, K=12, origin=0)
    extra_pairs = np.asarray([(2, 12), (4, 4), (1, 5), (2, 6), (-1, 3)])
    eR, et = relative(Rg, cg, np.clip(extra_pairs, 0, 11))
    eR[1], et[1] = np.eye(3), [1.0, 0.0, 0.0]
    eR[2] = 0.0
    et[3] = 0.0
    order = [0, 1, 2]                                   # entries put in front, the rest behind: pair indices of the clean entries shift uniformly
    bad = dict(pairs=np.concatenate([extra_pairs[order], pairs, extra_pairs[3:]]), R=np.concatenate([eR[order], R, eR[3:]]).astype(np.float32),
               t=np.concatenate([et[order], t, et[3:]]).astype(np.float32), weights=np.concatenate([[500, 500, 500], w, [500, 500]]).astype(np.float32),
               K=12, origin=0)
    what = dict(front=3, clean=len(pairs), states=[BAD_INDEX, BAD_INDEX, NO_MODEL] + [None] * len(pairs) + [NO_MODEL, BAD_INDEX], hanging=7,
                second=(8, 9, 10), alone=11)
    return bad, clean, what


def collinear_scene():
    """five cameras on the x axis, rotated about it: every direction is exactly (1, 0, 0) in the origin's frame, so every free centre can slide along the line"""
    K = 5
    R = np.stack([so3_exp([0.1 * k, 0.0, 0.0]) for k in range(K)])
    c = np.asarray([[float(k * k + k), 0.0, 0.0] for k in range(K)]) / 2.0
    pairs = np.asarray([(i, j) for i in range(K) for j in range(i + 1, K)], np.int64)
    Rab, t = relative(R, c, pairs)
    return dict(pairs=pairs, R=Rab.astype(np.float32), t=t.astype(np.float32), weights=np.ones(len(pairs), np.float32), K=K, origin=0)


@functools.lru_cache(maxsize=None)
def chain_scene(count=6, rows=128, tracks=110):
    """planted matches over all pairs of `count` images of `rows` keypoints: every track is seen by three or more images -> dict(kpts, pairs, matches0, cams,
    poses (the truth, world frame))"""
    rng = np.random.default_rng(77)
    poses, cams = O.cameras(count, 4)
    views = O.random_views(count, tracks, rng, lo=3)
    pl = O.plant(poses, cams, views, 78, (rows,) * count, rows)
    pairs = [(a, b) for a in range(count) for b in range(a + 1, count)]
    return dict(kpts=pl["kpts"], pairs=np.asarray(pairs), matches0=O.match_rows(pairs, pl["rows"], rows), cams=cams, poses=poses)


def gauge_poses(poses, origin, baseline):
    """the true poses [K, 3, 4] float32 in the gauge of a call: `origin` the identity, the centre of `baseline` at distance 1"""
    Rg, cg = in_gauge(poses, origin, baseline)
    return np.concatenate([Rg, -np.einsum("kij,kj->ki", Rg, cg)[:, :, None]], 2).astype(np.float32)
