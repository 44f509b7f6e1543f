"""Numpy restatement of the global positioner's definition (include/lightglue_amd.h, lg_positioning_solve), float64: the rays, the candidates, who takes part,
the reweighted linear solve of all free centres and all points, the classification at the final state, the outputs.  Sums run vectorised here (np.add.at in
observation order, not in the device's list order: the difference is rounding of float64, far below the float32 outputs).  The Cholesky is the pose-graph
oracle's restatement of the shared one.  Also the scenes of tests/test_positioning_cpu.py and tests/test_gpu_positioning.py, built on the cameras and the
planting of tests/triangulate_oracle.py.  No GPU, no torch."""
import functools

import numpy as np

import posegraph_oracle as G
import triangulate_oracle as O

NONE, INLIER, BAD_IMAGE, TOO_LONG, PEELED, NOT_CONNECTED, DEGENERATE, OUTLIER, NO_POINT, NO_SOLUTION = range(10)      # node_state
POSED, HELD, TOO_FEW_TRACKS, IMG_NOT_CONNECTED, IMG_BAD, IMG_NO_SOLUTION = range(6)                                   # image_state
LG_OK, LG_ERR_CAMERA = 0, 7
MAX_LEN, MIN_SQ, POS_DONE = 1024, 1e-12, 1e-12
# the stop test against fp64 rounding: tests/posegraph_oracle.py has the reasoning and the figures; the same two constants decide `near` here
NEAR_FACTOR, NEAR_NOISE = G.NEAR_FACTOR, G.NEAR_NOISE


def inverse3(V):
    """[T, 3, 3] symmetric -> (Vi [T, 3, 3], ok [T]): column c of Vi solves V x = e_c by the triangulator's elimination and pivot rule (the row operations
    do not depend on the right-hand side, so the three columns are eliminated at once)"""
    T = len(V)
    M = np.concatenate([V, np.tile(np.eye(3), (T, 1, 1))], 2)
    bar = O.EPS * np.maximum(np.maximum(V[:, 0, 0], V[:, 1, 1]), V[:, 2, 2])
    ok = np.ones(T, bool)
    with np.errstate(all="ignore"):
        for c in range(3):
            for r in range(c + 1, 3):
                swap = abs(M[:, r, c]) > abs(M[:, c, c])
                lo, hi = M[:, c].copy(), M[:, r].copy()
                M[:, c], M[:, r] = np.where(swap[:, None], hi, lo), np.where(swap[:, None], lo, hi)
            ok &= abs(M[:, c, c]) > bar
            for r in range(c + 1, 3):
                f = M[:, r, c] / M[:, c, c]
                M[:, r, c + 1:] = M[:, r, c + 1:] - f[:, None] * M[:, c, c + 1:]
        x2 = M[:, 2, 3:] / M[:, 2, 2, None]
        x1 = (M[:, 1, 3:] - M[:, 1, 2, None] * x2) / M[:, 1, 1, None]
        x0 = ((M[:, 0, 3:] - M[:, 0, 1, None] * x1) - M[:, 0, 2, None] * x2) / M[:, 0, 0, None]
    Vi = np.stack([x0, x1, x2], 1)
    return Vi, ok & np.isfinite(Vi).all((1, 2))


def held_centres(poses, held):
    """the centres -R^T t of the held images from the widened poses"""
    P = np.asarray(poses, np.float64)[np.asarray(held, bool)]
    return -np.einsum("kji,kj->ki", P[:, :, :3], P[:, :, 3])


def solve(inp, **kw):
    """the definition, and whether fp64 rounding decides its stop test (`near`); `own`: how far angle_error moves when the systems are solved by LU"""
    out, other = solve_once(inp, **kw), solve_once(inp, lu=True, **kw)
    x, y = out["steps"], other["steps"]
    near = len(x) != len(y) or any(abs(u - v) > NEAR_NOISE * u and POS_DONE / NEAR_FACTOR < u < POS_DONE * NEAR_FACTOR for u, v in zip(x, y))
    with np.errstate(invalid="ignore"):
        own = float(np.nan_to_num(abs(out["angle_error64"] - other["angle_error64"])).max())
    return dict(out, near=bool(near), own=own)


def solve_once(inp, num_iterations=12, angle_scale=1.0, max_angle_error=2.0, lu=False):
    """inp: dict(kpts [K, N, 2] float32, num [K] or None, track_id [K, N], T, cams [K, 4], poses [K, 3, 4], held [K] bool, wide (optional))"""
    widen = (lambda x: np.asarray(x, np.float64)) if inp.get("wide") else (lambda x: np.asarray(x, np.float32).astype(np.float64))      # wide: float64 inputs as they are
    kpts = widen(inp["kpts"])
    K, N = kpts.shape[:2]
    T, n = int(inp["T"]), int(num_iterations)
    tid = np.asarray(inp["track_id"], np.int64).reshape(K, N)
    cams, poses = widen(inp["cams"]), widen(inp["poses"]).reshape(K, 3, 4)
    held = np.asarray(inp["held"], bool)
    R, t = poses[:, :, :3], poses[:, :, 3]
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(cams).all(1) & (cams[:, :2] > 0).all(1) & np.isfinite(R).all((1, 2)) & (~held | np.isfinite(t).all(1))
    hok = held & ok
    if hok.sum() < 2 or (abs(held_centres(poses, hok) - held_centres(poses, hok)[0]).max() == 0.0):
        raise ValueError("the gauge needs two held images with finite poses and distinct centres")
    live = np.arange(N)[None, :] < O.live_rows(inp.get("num"), K, N)[:, None]
    labelled = live & (tid >= 0) & (tid < T)
    state = np.zeros((K, N), np.uint8)
    state[labelled & ~ok[:, None]] = BAD_IMAGE
    cand = labelled & ok[:, None]
    ck, ci = np.nonzero(cand)                                  # ascending node order
    cj = tid[ck, ci]
    count = np.bincount(cj, minlength=T)
    long_ = count[cj] > MAX_LEN
    state[ck[long_], ci[long_]] = TOO_LONG
    ck, ci, cj = ck[~long_], ci[~long_], cj[~long_]

    # who takes part: the greatest set that satisfies the three rules (removal is monotone, so the order of the rounds does not matter)
    img_in, trk_in = ok.copy(), np.zeros(T, bool)
    trk_in[cj] = True
    while True:
        use = img_in[ck] & trk_in[cj]
        images_of = np.zeros(T, int)
        np.add.at(images_of, np.unique(np.stack([cj[use], ck[use]]), axis=1)[0], 1)
        tracks_of = np.zeros(K, int)
        np.add.at(tracks_of, np.unique(np.stack([ck[use], cj[use]]), axis=1)[0], 1)
        nt, ni = trk_in & (images_of >= 2), img_in & (held | (tracks_of >= 2))
        if (nt == trk_in).all() and (ni == img_in).all():
            break
        trk_in, img_in = nt, ni
    peeled_img = ok & ~img_in
    use = img_in[ck] & trk_in[cj]
    reach_i, reach_t = hok & img_in, np.zeros(T, bool)
    while True:
        rt = reach_t.copy()
        rt[cj[use & reach_i[ck]]] = True
        ri = reach_i.copy()
        ri[ck[use & rt[cj]]] = True
        if (rt == reach_t).all() and (ri == reach_i).all():
            break
        reach_t, reach_i = rt, ri
    lost_t, lost_i = trk_in & ~reach_t, img_in & ~reach_i
    trk_in, img_in = trk_in & reach_t, img_in & reach_i
    tstate = np.where(trk_in, INLIER, np.where(lost_t, NOT_CONNECTED, PEELED))
    state[ck, ci] = np.where(img_in[ck] | ~trk_in[cj], tstate[cj], PEELED)
    use = img_in[ck] & trk_in[cj]
    ok_, oi, oj = ck[use], ci[use], cj[use]                    # the observations taking part, ascending node order

    # rays
    cam = cams[ok_]
    u = np.stack([(kpts[ok_, oi, 0] - cam[:, 2]) / cam[:, 0], (kpts[ok_, oi, 1] - cam[:, 3]) / cam[:, 1], np.ones(len(ok_))], 1)
    w = np.einsum("oji,oj->oi", R[ok_], u)
    v = w / np.sqrt((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2])[:, None]      # of the rotated vector: a float32 R is orthonormal to 1e-7 only
    proj = np.eye(3) - v[:, :, None] * v[:, None, :]
    free = ok & ~held & img_in
    C = np.zeros((K, 3))
    C[hok] = held_centres(poses, hok)
    X = np.zeros((T, 3))
    f3 = np.repeat(free, 3)
    good_all, iters, steps, dropped = True, 0, [], np.zeros(T, bool)
    # ordered pairs of observations of one track whose images are both free (the blocks of the reduced system)
    order = np.argsort(oj, kind="stable")
    starts = np.flatnonzero(np.r_[True, np.diff(oj[order]) != 0]) if len(order) else np.zeros(0, int)
    p1, p2 = [], []
    for g in np.split(order, starts[1:]) if len(order) else []:
        g = g[free[ok_[g]]]
        if len(g):
            a, b = np.meshgrid(g, g, indexing="ij")
            p1.append(a.ravel())
            p2.append(b.ravel())
    p1, p2 = (np.concatenate(p1), np.concatenate(p2)) if p1 else (np.zeros(0, int), np.zeros(0, int))
    rad = np.pi / 180.0
    for it in range(n):
        mult = max(1.0, 2.0 ** (n - 6 - it))
        act = ~dropped[oj]
        rho = np.ones(len(oj))
        if it > 0:
            e = X[oj] - C[ok_]
            with np.errstate(all="ignore"):
                rho = 1.0 / np.maximum((e * e).sum(1), MIN_SQ) / (1.0 + (G.angle_to(v, e) / (angle_scale * rad * mult)) ** 2)
        M = rho[:, None, None] * proj
        V, g = np.zeros((T, 3, 3)), np.zeros((T, 3))
        np.add.at(V, oj[act], M[act])
        hm = act & held[ok_]
        np.add.at(g, oj[hm], np.einsum("oij,oj->oi", M[hm], C[ok_[hm]]))
        Vi, piv = inverse3(np.where((trk_in & ~dropped)[:, None, None], V, np.eye(3)))
        dropped |= trk_in & ~piv
        act = ~dropped[oj]
        Vi[dropped | ~trk_in] = 0.0
        fa = act & free[ok_]
        A = np.zeros((K, 3, K, 3))
        np.add.at(A, (ok_[fa], slice(None), ok_[fa], slice(None)), M[fa])
        rhs = np.zeros((K, 3))
        np.add.at(rhs, ok_[fa], np.einsum("oij,ojk,ok->oi", M[fa], Vi[oj[fa]], g[oj[fa]]))
        keep = ~dropped[oj[p1]]
        q1, q2 = p1[keep], p2[keep]
        np.add.at(A, (ok_[q1], slice(None), ok_[q2], slice(None)), -(M[q1] @ Vi[oj[q1]] @ M[q2]))
        A, rhs = A.reshape(3 * K, 3 * K), rhs.reshape(-1)
        A[~f3, :], A[:, ~f3], rhs[~f3] = 0.0, 0.0, 0.0
        A[~f3, ~f3] = 1.0
        with np.errstate(all="ignore"):
            x, good = G.cholesky_solve(A, rhs[:, None], lu)
        x = x[:, 0].reshape(K, 3)
        good_all = good_all and good
        with np.errstate(invalid="ignore"):
            step = abs(x[free] - C[free]).max() if free.any() else 0.0
        C[free] = x[free]
        acc = g.copy()
        np.add.at(acc, oj[fa], np.einsum("oij,oj->oi", M[fa], C[ok_[fa]]))
        X = np.einsum("tij,tj->ti", Vi, acc)
        iters = it + 1
        if mult == 1.0:
            steps.append(step)
        if mult == 1.0 and np.isfinite(step) and step < POS_DONE:
            break

    # the classification at the final state and the outputs
    ang = np.full((K, N), np.nan)
    degenerate = dropped[oj]
    state[ok_[degenerate], oi[degenerate]] = DEGENERATE
    has_point = np.zeros(T, bool)
    if good_all:
        act = ~degenerate
        e = X[oj] - C[ok_]
        with np.errstate(all="ignore"):
            de = (v * e).sum(1)
            phi = G.angle_to(v, e) * (180.0 / np.pi)
            inl = act & (de > 0.0) & (phi <= max_angle_error)
        ang[ok_[act], oi[act]] = phi[act]
        state[ok_[act], oi[act]] = np.where(inl[act], INLIER, OUTLIER)
        images_of = np.zeros(T, int)
        if inl.any():
            np.add.at(images_of, np.unique(np.stack([oj[inl], ok_[inl]]), axis=1)[0], 1)
        has_point = images_of >= 2
        lone = inl & ~has_point[oj]
        state[ok_[lone], oi[lone]] = NO_POINT
    else:
        state[ok_[~degenerate], oi[~degenerate]] = NO_SOLUTION
    posed = free & good_all
    image_state = np.where(~ok, IMG_BAD, np.where(held, HELD, np.where(posed, POSED, np.where(free, IMG_NO_SOLUTION, np.where(lost_i, IMG_NOT_CONNECTED,
                                                                                                                         TOO_FEW_TRACKS))))).astype(np.uint8)
    out_poses = np.full((K, 3, 4), np.nan)
    out_poses[ok, :, :3] = R[ok]
    out_poses[hok, :, 3] = t[hok]
    out_poses[posed, :, 3] = -np.einsum("kij,kj->ki", R[posed], C[posed])
    centres = np.full((K, 3), np.nan)
    centres[hok | posed] = C[hok | posed]
    xyz = np.where(has_point[:, None], X, np.nan)
    inlier = state == INLIER
    pts = np.full((K, N, 3), np.nan)
    pts[inlier] = xyz[tid[inlier]]
    return dict(poses64=out_poses, centres64=centres, xyz64=xyz, points3d64=pts, track_id=np.where(inlier, tid, -1), node_state=state, image_state=image_state,
                angle_error64=ang, status=np.where(ok, LG_OK, LG_ERR_CAMERA).astype(np.int32), num_posed=int((hok | posed).sum()), num_points=int(has_point.sum()),
                num_outliers=int((state == OUTLIER).sum()), iterations=iters, positions_ok=bool(good_all), steps=steps)


# ---------------------------------------------------------------------- scenes
def views_within(count, tracks, rng, lo, hi, capacity):
    """per track the images that see it, no image seen more often than it has rows"""
    left, views = np.full(count, capacity), []
    for _ in range(tracks):
        room = np.flatnonzero(left > 0)
        seen = sorted(rng.choice(room, min(int(rng.integers(lo, hi + 1)), len(room)), replace=False).tolist())
        left[seen] -= 1
        views.append(seen)
    return views


def labels(rows, K, N):
    """track_id [K, N] from the planted rows: track j at row rows[j][k] of image k, -1 elsewhere"""
    tid = np.full((K, N), -1, np.int64)
    for j, at in enumerate(rows):
        for k, r in at.items():
            tid[k, r] = j
    return tid


@functools.lru_cache(maxsize=None)
def scene(K, N, tracks, seed=0, lo=3, hi=5, exact=False):
    """K cameras on the arc, `tracks` planted tracks of lo .. hi views with 0.5 px noise (exact: the clean projections) -> the oracle's input with the true
    poses, images 0 and K - 1 held, plus `planted` and the truth (Rg, cg)"""
    rng = np.random.default_rng(4100 + 7 * K + seed)
    poses, cams = O.cameras(K, seed)
    views = views_within(K, tracks, rng, lo, min(hi, K), N)
    pl = O.plant(poses, cams, views, 4200 + seed, (N,) * K, N)
    kpts = pl["kpts"].copy()
    if exact:
        m = ~np.isnan(pl["clean"][:, :, 0])
        kpts[m] = pl["clean"][m].astype(np.float32)
    held = np.zeros(K, bool)
    held[[0, K - 1]] = True
    R = poses[:, :, :3].astype(np.float64)
    return dict(kpts=kpts, num=None, track_id=labels(pl["rows"], K, N), T=tracks, cams=cams, poses=poses, held=held, planted=pl,
                cg=-np.einsum("kji,kj->ki", R, poses[:, :, 3].astype(np.float64)))


def oracle_input(sc):
    return {k: sc[k] for k in ("kpts", "num", "track_id", "T", "cams", "poses", "held")}


def noisy_rotations(poses, degrees, seed, held):
    """the true poses with every free image's rotation turned by up to `degrees` about a random axis (its t is left alone: a free image's t is not read)"""
    rng = np.random.default_rng(seed)
    out = np.asarray(poses, np.float64).copy()
    for k in np.flatnonzero(~np.asarray(held, bool)):
        out[k, :, :3] = G.random_rotation(rng, rng.uniform(0.2, 1.0) * degrees) @ out[k, :, :3]
    return out.astype(np.float32)


def centre_error(centres, truth, mask=None):
    """the worst centre error after a similarity alignment, as a fraction of the scene's extent (tests/posegraph_oracle.py, against_truth)"""
    m = np.isfinite(centres).all(1) if mask is None else mask
    X, Y = centres[m], truth[m]
    mx, my = X.mean(0), Y.mean(0)
    U, S, Vt = np.linalg.svd((Y - my).T @ (X - mx))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    s = (S * np.diag(D)).sum() / ((X - mx) ** 2).sum()
    fit = s * (X - mx) @ (U @ D @ Vt).T + my
    return float(np.linalg.norm(fit - Y, axis=1).max() / np.linalg.norm(Y.max(0) - Y.min(0)))


def reprojection(kpts, track_id, cams, poses64, xyz64):
    """pixel errors of every labelled row whose track has a point and whose image has a pose, [observations]"""
    k, i = np.nonzero(track_id >= 0)
    j = track_id[k, i]
    P = poses64[k]
    with np.errstate(all="ignore"):
        p = np.einsum("oij,oj->oi", P[:, :, :3], xyz64[j]) + P[:, :, 3]
        px = np.stack([cams[k, 0] * p[:, 0] / p[:, 2] + cams[k, 2], cams[k, 1] * p[:, 1] / p[:, 2] + cams[k, 3]], 1)
        err = np.linalg.norm(px - kpts[k, i].astype(np.float64), axis=1)
    return err[np.isfinite(err)]


def triangulated(kpts, track_id, T, cams, poses64):
    """every track's point from the given poses by the triangulator's linear start over all its labelled rows (what averaging's poses give the tracks)"""
    K, N = track_id.shape
    recs = [O.record(cams[k], poses64[k]) if np.isfinite(poses64[k]).all() else None for k in range(K)]
    xyz = np.full((T, 3), np.nan)
    for j in range(T):
        obs = [(kpts[k, i], recs[k]) for k, i in zip(*np.nonzero(track_id == j)) if recs[k] is not None]
        if len(obs) >= 2:
            X = O.start_point(obs)
            if X is not None:
                xyz[j] = X
    return xyz


@functools.lru_cache(maxsize=None)
def edge_scene():
    """K = 9, N = 32, images 0 and 4 held.  Images 0 .. 4 share 30 tracks; image 5 sees ONE track (with images 1 and 2): it is peeled, the track stays; images
    6, 7, 8 share eight tracks among themselves only: an island; one track of images 1 and 2 has parallel rays (image 2's pixel is where image 1's ray
    points): its 3 x 3 pivot fails; one label sits on a single row (a short track); image 3 has two dead rows that carry labels.
    -> the oracle's input plus `what`: the tracks and rows planted"""
    K, N = 9, 32
    rng = np.random.default_rng(4300)
    poses, cams = O.cameras(K, 5)
    views = views_within(5, 30, rng, 3, 5, 24)
    one, parallel = len(views), len(views) + 1
    views += [[1, 2, 5], [1, 2]]
    island = list(range(len(views), len(views) + 8))
    views += [sorted((6 + rng.choice(3, int(rng.integers(2, 4)), replace=False)).tolist()) for _ in island]
    num = (N, N, N, N - 2, N, N, N, N, N)
    pl = O.plant(poses, cams, views, 4301, num, N)
    kpts, rows = pl["kpts"].copy(), pl["rows"]
    tid = labels(rows, K, N)
    T = len(views) + 1
    short = (0, pl["free"][0][-1])
    tid[short] = T - 1                                           # one node alone under its label
    tid[3, N - 2], tid[3, N - 1] = 0, 1                          # dead rows with labels
    R = poses[:, :, :3].astype(np.float64)
    c1 = cams[1].astype(np.float64)
    x = kpts[1, rows[parallel][1]].astype(np.float64)
    u = np.array([(x[0] - c1[2]) / c1[0], (x[1] - c1[3]) / c1[1], 1.0])
    w = R[2] @ (R[1].T @ u)                                      # image 1's ray in image 2's frame
    kpts[2, rows[parallel][2]] = (cams[2, 0] * w[0] / w[2] + cams[2, 2], cams[2, 1] * w[1] / w[2] + cams[2, 3])
    held = np.zeros(K, bool)
    held[[0, 4]] = True
    return dict(kpts=kpts, num=np.asarray(num), track_id=tid, T=T, cams=cams, poses=poses, held=held,
                what=dict(one=one, parallel=parallel, island=island, short=short, lonely=5, island_images=(6, 7, 8), rows=rows))


def stray_scene(K=8, N=48, tracks=60, count=10, seed=2):
    """scene(K, N, tracks) with `count` observations of tracks with four or more views moved by 30 .. 60 px -> (the input, the clean input, planted [K, N] bool)"""
    sc = scene(K, N, tracks, seed=seed, lo=4, hi=6)
    rng = np.random.default_rng(4400 + seed)
    kpts, planted = sc["kpts"].copy(), np.zeros((K, N), bool)
    for j in rng.choice(tracks, count, replace=False):
        k = int(rng.choice(list(sc["planted"]["rows"][j])))
        r = sc["planted"]["rows"][j][k]
        ang = rng.uniform(0, 2 * np.pi)
        kpts[k, r] += (rng.uniform(30, 60) * np.array([np.cos(ang), np.sin(ang)])).astype(np.float32)
        planted[k, r] = True
    return dict(oracle_input(sc), kpts=kpts), oracle_input(sc), planted, sc
