"""Numpy restatement of the bundle adjuster's definition (include/lightglue_amd.h, lg_bundle_adjust), float64: candidates, node states, the tracks' lists, the
free images, Levenberg-Marquardt with Marquardt's damping, the accept / reject / convergence decisions and every output, with a solver of its own.  `solver`
selects the prescribed Schur complement + Cholesky ("schur") or ONE np.linalg.solve on the full damped (6 K + 3 T) system ("full"); `order` the accumulation
order of every sum ("ascending": the definition's, or "descending"), so that tests/test_bundle_cpu.py can measure what those choices are worth.  Every decision
that lies within a relative NEAR of its bar is recorded in `near`.  Also the scenes of tests/test_gpu_bundle.py, built on the generators of
tests/triangulate_oracle.py without a GPU.  No GPU, no torch."""
import functools

import numpy as np

import triangulate_oracle as O
from abspose_oracle import rodrigues

NEAR, EPS, MAX_LEN = 1e-9, 1e-12, 1024
LG_OK, LG_ERR_CAMERA = 0, 7
NONE, ACTIVE, BAD_IMAGE, NON_FINITE, BEHIND, SHORT, TOO_LONG = range(7)
ITERATIONS, DAMPING, TOLERANCE = 10, 1e-4, 1e-6
SLOW_DAMPING = 1e4                      # a start so damped that ten iterations do not converge on the main scene


# ---------------------------------------------------------------------- small pieces
def solve3(M, b, near):
    """the triangulator's elimination (tests/triangulate_oracle.py solve3), recording a pivot within NEAR of its bar: x or None"""
    M = np.concatenate([np.asarray(M, np.float64), np.asarray(b, np.float64)[:, None]], 1)
    bar = EPS * max(M[0, 0], M[1, 1], M[2, 2])
    for c in range(3):
        for r in range(c + 1, 3):
            if abs(M[r, c]) > abs(M[c, c]):
                M[[c, r]] = M[[r, c]]
        if abs(abs(M[c, c]) - bar) <= NEAR * bar:
            near.append("pivot3")
        if not abs(M[c, c]) > bar:
            return None
        for r in range(c + 1, 3):
            f = M[r, c] / M[c, c]
            for j in range(c + 1, 4):
                M[r, j] = M[r, j] - f * M[c, j]
    x2 = M[2, 3] / M[2, 2]
    x1 = (M[1, 3] - M[1, 2] * x2) / M[1, 1]
    x0 = ((M[0, 3] - M[0, 1] * x1) - M[0, 2] * x2) / M[0, 0]
    x = np.array([x0, x1, x2])
    return x if np.isfinite(x).all() else None


def damped(d, lam):
    return d + lam * min(max(d, 1e-6), 1e32)


def project(P, X):
    return np.array([((P[r, 0] * X[0] + P[r, 1] * X[1]) + P[r, 2] * X[2]) + P[r, 3] for r in range(3)])


def jacobians(P, cam, p):
    """A [2, 6] (pose, camera-frame twist (w, d)), B [2, 3] (point)"""
    iz, fx, fy = 1.0 / p[2], cam[0], cam[1]
    ax, az, by, bz = fx * iz, -(((fx * p[0]) * iz) * iz), fy * iz, -(((fy * p[1]) * iz) * iz)
    A = np.array([[az * p[1], ax * p[2] - az * p[0], -(ax * p[1]), ax, 0.0, az], [bz * p[1] - by * p[2], -(bz * p[0]), by * p[0], 0.0, by, bz]])
    B = np.stack([ax * P[0, :3] + az * P[2, :3], by * P[1, :3] + bz * P[2, :3]])
    return A, B


def residual(cam, p, xy):
    with np.errstate(all="ignore"):
        iz = 1.0 / p[2]
        return np.array([((cam[0] * p[0]) * iz + cam[2]) - np.float64(np.float32(xy[0])), ((cam[1] * p[1]) * iz + cam[3]) - np.float64(np.float32(xy[1]))])


def cholesky(S, near):
    """L of the lower triangle of S (row by row, a sum of its own), or None on a pivot that is not > 0"""
    n = len(S)
    L = np.zeros((n, n))
    for j in range(n):
        d = S[j, j] - L[j, :j] @ L[j, :j]
        if abs(d) <= NEAR * abs(S[j, j]):
            near.append("pivot")
        if not (d > 0 and np.isfinite(d)):
            return None
        L[j, j] = np.sqrt(d)
        if j + 1 < n:
            L[j + 1:, j] = (S[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def substitute(L, b):
    n = len(b)
    z = np.zeros(n)
    for i in range(n):
        z[i] = (b[i] - L[i, :i] @ z[:i]) / L[i, i]
    s = np.zeros(n)
    for i in range(n - 1, -1, -1):
        s[i] = (z[i] - L[i + 1:, i] @ s[i + 1:]) / L[i, i]
    return s


# ---------------------------------------------------------------------- the whole definition
def adjust(inp, num_iterations=ITERATIONS, initial_damping=DAMPING, function_tolerance=TOLERANCE, solver="schur", order="ascending"):
    """inp: dict(kpts [K, N, 2] float32, num [K] or None, track_id [K, N], xyz [T, 3] float32, cams [K, 4], poses [K, 3, 4] float32, constant [K] bool) ->
    dict(poses64 [K, 3, 4], xyz64 [T, 3], points3d64 [K, N, 3] (NaN off the active rows), node_state, error64 [K, N], initial_cost, final_cost, num_iterations,
    num_accepted, converged, num_observations, status [K], free [K], adjusted [T], costs: the accepted costs in order, near: the decisions within NEAR of a bar)"""
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
    near = []
    state = np.zeros((K, N), np.uint8)
    cand = [[] for _ in range(T)]
    with np.errstate(all="ignore"):
        for k in range(K):
            for i in range(live[k]):
                j = int(tid[k, i])
                if not 0 <= j < T:
                    continue
                if not ok[k]:
                    state[k, i] = BAD_IMAGE
                elif not np.isfinite(X[j]).all():
                    state[k, i] = NON_FINITE
                else:
                    p = project(P[k], X[j])
                    if abs(p[2]) <= NEAR * np.linalg.norm(p):
                        near.append("behind at the start")
                    state[k, i] = ACTIVE if p[2] > 0 else BEHIND
                    if p[2] > 0:
                        cand[j].append((k, i))
    adjusted = np.array([2 <= len(c) <= MAX_LEN for c in cand], bool)
    for j, c in enumerate(cand):
        if not adjusted[j]:
            for k, i in c:
                state[k, i] = SHORT if len(c) < 2 else TOO_LONG
    active = state == ACTIVE
    free = ok & ~np.asarray(inp["constant"], bool) & active.any(1)
    flip = (lambda seq: list(seq)) if order == "ascending" else (lambda seq: list(seq)[::-1])
    rows_of = [flip(np.flatnonzero(active[k]).tolist()) for k in range(K)]
    obs_of = [flip(c) if adjusted[j] else [] for j, c in enumerate(cand)]

    def cost_of(Ps, Xs):
        """(cost, failed): per image in row order, the images in order"""
        total, failed = 0.0, False
        with np.errstate(all="ignore"):
            for k in flip(range(K)):
                s = 0.0
                for i in rows_of[k]:
                    p = project(Ps[k], Xs[tid[k, i]])
                    r = residual(cam[k], p, kpts[k, i])
                    c = r[0] * r[0] + r[1] * r[1]
                    if abs(p[2]) <= NEAR * np.linalg.norm(p):
                        near.append("pz = 0")
                    if not p[2] > 0 or not np.isfinite(c):
                        failed, c = True, 0.0
                    s += c
                total += s
        return total, failed

    def step(Ps, Xs, lam):
        """(pose steps [K, 6], point steps [T, 3]) or None if a pivot failed"""
        lin = {}
        U, gc = np.zeros((K, 6, 6)), np.zeros((K, 6))
        for k in range(K):
            for i in rows_of[k]:
                p = project(Ps[k], Xs[tid[k, i]])
                A, B = jacobians(Ps[k], cam[k], p)
                r = residual(cam[k], p, kpts[k, i])
                lin[k, i] = (A, B, r)
                U[k] += A.T @ A
                gc[k] += A.T @ r
        V, gp = np.zeros((T, 3, 3)), np.zeros((T, 3))
        for j in range(T):
            for k, i in obs_of[j]:
                A, B, r = lin[k, i]
                V[j] += B.T @ B
                gp[j] += B.T @ r
        for k in range(K):
            for d in range(6):
                U[k, d, d] = damped(U[k, d, d], lam)
        for j in range(T):
            for d in range(3):
                V[j, d, d] = damped(V[j, d, d], lam)
        W = lambda k, i: lin[k, i][0].T @ lin[k, i][1]
        tracks = np.flatnonzero(adjusted)
        if solver == "full":
            at = {int(j): 6 * K + 3 * q for q, j in enumerate(tracks)}
            n = 6 * K + 3 * len(tracks)
            H, g = np.zeros((n, n)), np.zeros(n)
            for k in range(K):
                H[6 * k:6 * k + 6, 6 * k:6 * k + 6] = U[k] if free[k] else np.eye(6)
                g[6 * k:6 * k + 6] = gc[k] if free[k] else 0.0
            for j in tracks:
                a = at[int(j)]
                H[a:a + 3, a:a + 3], g[a:a + 3] = V[j], gp[j]
                for k, i in obs_of[j]:
                    if free[k]:
                        H[6 * k:6 * k + 6, a:a + 3] += W(k, i)
                        H[a:a + 3, 6 * k:6 * k + 6] += W(k, i).T
            if not np.isfinite(H).all() or np.linalg.eigvalsh(H)[0] <= 0:
                return None
            x = np.linalg.solve(H, -g)
            dX = np.zeros((T, 3))
            for j in tracks:
                dX[j] = x[at[int(j)]:at[int(j)] + 3]
            return x[:6 * K].reshape(K, 6), dX
        Vi, y = np.zeros((T, 3, 3)), np.zeros((T, 3))
        for j in tracks:
            for c in range(3):
                col = solve3(V[j], np.eye(3)[c], near)
                if col is None:
                    return None
                Vi[j][:, c] = col
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
        L = cholesky(S, near)
        if L is None:
            return None
        s = substitute(L, rhs).reshape(K, 6)
        dX = np.zeros((T, 3))
        for j in tracks:
            acc = np.zeros(3)
            for k, i in obs_of[j]:
                if free[k]:
                    acc += W(k, i).T @ s[k]
            dX[j] = -(y[j] + Vi[j] @ acc)
        return s, dX

    cost, _ = cost_of(P, X)
    initial, lam, iters, accepted, converged, costs = cost, float(initial_damping), 0, 0, False, [cost]
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
            for k in np.flatnonzero(free):
                Q = rodrigues(s[k, :3])
                Pt[k] = np.concatenate([Q @ P[k][:, :3], (Q @ P[k][:, 3] + s[k, 3:])[:, None]], 1)
            new, failed = cost_of(Pt, Xt)
            good = not failed and np.isfinite(Pt).all() and np.isfinite(Xt[adjusted]).all() and np.isfinite(new)
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
    pts, err = np.full((K, N, 3), np.nan), np.full((K, N), np.nan)
    for k in range(K):
        for i in np.flatnonzero(active[k]):
            pts[k, i] = X[tid[k, i]]
            r = residual(cam[k], project(P[k], X[tid[k, i]]), kpts[k, i])
            err[k, i] = np.sqrt(r[0] * r[0] + r[1] * r[1])
    poses64 = np.where(free[:, None, None], P, poses32.astype(np.float64))
    xyz64 = np.where(adjusted[:, None], X, xyz32.astype(np.float64))
    return dict(poses64=poses64, xyz64=xyz64, points3d64=pts, node_state=state, error64=err, initial_cost=initial, final_cost=cost, num_iterations=iters,
                num_accepted=accepted, converged=converged, num_observations=int(active.sum()), status=np.where(ok, LG_OK, LG_ERR_CAMERA), free=free,
                adjusted=adjusted, costs=costs, near=near)


def scales(inp, out):
    """(per track [T], per image [K]): the largest coordinate magnitude among a point and the centres of the cameras that see it — the triangulator's scale — and,
    for an image's t, among its centre and its t; what one float32 ulp is taken of (R: 1)"""
    poses = np.asarray(inp["poses"], np.float64)
    centres = np.array([-(p[:, :3].T @ p[:, 3]) if np.isfinite(p).all() else np.zeros(3) for p in poses])
    tid, T = np.asarray(inp["track_id"]), len(out["xyz64"])
    track = np.ones(T)
    for j in range(T):
        ks = np.unique(np.nonzero((tid == j) & (out["node_state"] == ACTIVE))[0])
        if out["adjusted"][j]:
            track[j] = max(abs(out["xyz64"][j]).max(), max(abs(centres[k]).max() for k in ks))
    image = np.array([max(abs(centres[k]).max(), abs(np.nan_to_num(poses[k][:, 3])).max(), 1.0) for k in range(len(poses))])
    return track, image


# ---------------------------------------------------------------------- scenes: the triangulator's recipe (640 x 480 images, camera (500, 500, 320, 240), cameras
# about 6 units from a box centred at (100, -50, 20), pixel noise 0.5); free poses off by about 0.01 rad and 0.03 units, points by 0.03 units
ROT, SHIFT = 0.01, 0.03


def scene(count, rows, tracks, seed, constant=(0, 1), hi=None, num=None, special=()):
    """-> the oracle's input dict plus planted (the plant) and truth [T, 3]; special: views put in front of the random ones"""
    rng = np.random.default_rng(seed)
    poses, cams = O.cameras(count, seed)
    views = list(special) + O.random_views(count, tracks - len(special), rng, 2, hi)
    num = (rows,) * count if num is None else num
    pl = O.plant(poses, cams, views, seed + 1, num, rows)
    tid = np.full((count, rows), -1, np.int64)
    for j, at in enumerate(pl["rows"]):
        for k, i in at.items():
            tid[k, i] = j
    const = np.zeros(count, bool)
    const[list(constant)] = True
    moved = poses.astype(np.float64)
    for k in np.flatnonzero(~const):
        Q = rodrigues(ROT * rng.standard_normal(3) / np.sqrt(3))
        R, c = moved[k][:, :3], -moved[k][:, :3].T @ moved[k][:, 3]
        c = c + SHIFT * rng.standard_normal(3) / np.sqrt(3)
        moved[k] = np.concatenate([Q @ R, (-(Q @ R) @ c)[:, None]], 1)
    xyz = (pl["X"] + SHIFT * rng.standard_normal(pl["X"].shape) / np.sqrt(3)).astype(np.float32)
    return dict(kpts=pl["kpts"], num=None if num == (rows,) * count else np.asarray(num), track_id=tid, xyz=xyz, cams=cams, poses=moved.astype(np.float32),
                constant=const, planted=pl, truth=pl["X"])


def oracle_input(sc):
    return {k: sc[k] for k in ("kpts", "num", "track_id", "xyz", "cams", "poses", "constant")}


@functools.lru_cache(maxsize=None)
def main_scene():
    """K = 6, N = 96, 50 tracks of 2 .. 6 views, images 0 and 1 constant, dead rows in images 0, 2 and 5"""
    return scene(O.K, O.N, 50, 70, num=O.NUM, special=([0, 1, 2, 3, 4, 5], [2, 3]))


EDGE_K = 7


@functools.lru_cache(maxsize=None)
def edge_scene():
    """-> (bad, clean, what).  Seven images, image 6 sees nothing.  bad: a track seen by the constant images only, one of length 2, one seen by all six images,
    a point behind image 2 at the start (its other view is left alone: a short track), a NaN point, image 3 with fx = 0, a label >= T and a label below -1.
    clean: the same call with the labels of the bad entries taken out (-1) and image 3's camera mended: what must come back bit for bit elsewhere"""
    base = scene(EDGE_K, O.N, 48, 91, hi=5, special=([0, 1], [2, 4], [0, 1, 2, 3, 4, 5], [2, 5], [1, 4, 5]))
    tid = base["track_id"].copy()
    tid[6] = -1                                                         # image 6: no observation
    bad = dict(oracle_input(base), track_id=tid.copy(), xyz=base["xyz"].copy(), cams=base["cams"].copy())
    rows = base["planted"]["rows"]
    P2 = base["poses"][2].astype(np.float64)
    centre, axis = -P2[:, :3].T @ P2[:, 3], P2[2, :3]
    bad["xyz"][3] = (centre - 0.5 * axis).astype(np.float32)            # behind image 2; in front of image 5, whose observation is then alone
    bad["xyz"][4] = np.float32(np.nan)
    bad["cams"][3, 0] = 0.0
    free_rows = base["planted"]["free"]
    bad["track_id"][4, free_rows[4][0]] = len(base["xyz"]) + 3          # a label >= T
    bad["track_id"][5, free_rows[5][0]] = -7
    clean = dict(bad, track_id=bad["track_id"].copy(), cams=base["cams"].copy())
    clean["track_id"][3] = -1
    for j in (3, 4):
        for k, i in rows[j].items():
            clean["track_id"][k, i] = -1
    clean["track_id"][4, free_rows[4][0]] = clean["track_id"][5, free_rows[5][0]] = -1
    return bad, clean, dict(constant_only=0, pair=1, full=2, behind=3, nan=4, bad_image=3, empty_image=6, rows=rows)


CHOLESKY_N = 32


@functools.lru_cache(maxsize=None)
def cholesky_scene(count):
    """count images of 32 rows: 6 count crosses the Cholesky's 48-column panels (count = 9: one full panel and 6 columns; 24: three full panels)"""
    return scene(count, CHOLESKY_N, 4 * count, 110 + count, hi=5)


GPU_SCENES = {"main": lambda: oracle_input(main_scene()), "edge": lambda: edge_scene()[0], "edge clean": lambda: edge_scene()[1],
              "K = 9": lambda: oracle_input(cholesky_scene(9)), "K = 24": lambda: oracle_input(cholesky_scene(24))}


@functools.lru_cache(maxsize=None)
def answer(name, num_iterations=ITERATIONS, solver="schur", order="ascending"):
    """The definition's answer on a GPU-test scene (shared by the tests; treat as read-only)"""
    return adjust(GPU_SCENES[name](), num_iterations=num_iterations, solver=solver, order=order)


def relabel(inp, seed=0):
    """the same problem with the tracks renamed by a random permutation: row j of xyz goes to row perm[j] -> (input, perm)"""
    T = len(inp["xyz"])
    perm = np.random.default_rng(seed).permutation(T)
    tid = np.asarray(inp["track_id"]).copy()
    inside = (tid >= 0) & (tid < T)
    tid[inside] = perm[tid[inside]]
    xyz = np.empty_like(inp["xyz"])
    xyz[perm] = inp["xyz"]
    return dict(inp, track_id=tid, xyz=xyz), perm


# ---------------------------------------------------------------------- the chain: triangulate five images under slightly wrong poses, adjust, localise the sixth
@functools.lru_cache(maxsize=None)
def chain_scene():
    """tests/triangulate_oracle.py's chain scene with the poses of images 2, 3 and 4 off by about 0.01 rad and 0.03 units (triangulate with max_reproj_error = 8): what an incremental reconstruction
    hands to the adjuster.  -> its dict with `poses` replaced and `constant` (images 0 and 1; image 5 sees no track)"""
    sc = O.chain_scene()
    rng = np.random.default_rng(57)
    poses = sc["poses"].astype(np.float64)
    for k in (2, 3, 4):
        Q = rodrigues(ROT * rng.standard_normal(3) / np.sqrt(3))
        R, c = poses[k][:, :3], -poses[k][:, :3].T @ poses[k][:, 3]
        c = c + SHIFT * rng.standard_normal(3) / np.sqrt(3)
        poses[k] = np.concatenate([Q @ R, (-(Q @ R) @ c)[:, None]], 1)
    const = np.zeros(O.K, bool)
    const[:2] = True
    return dict(sc, poses=poses.astype(np.float32), true_poses=sc["poses"], constant=const)


# ---------------------------------------------------------------------- a far start: steps are rejected on the way
FAR_SHIFT, FAR_SEED = 2.0, 7


@functools.lru_cache(maxsize=None)
def far_scene():
    """the main scene with every point about 2 units off (a third of the distance to the cameras): some trial steps raise the cost or put a point behind a
    camera and are rejected, lambda rises and falls again"""
    sc = main_scene()
    xyz = (sc["truth"] + FAR_SHIFT * np.random.default_rng(FAR_SEED).standard_normal(sc["truth"].shape)).astype(np.float32)
    return dict(oracle_input(sc), xyz=xyz)


# ---------------------------------------------------------------------- labels shared inside an image, and a track beyond the longest the adjuster takes
LONG_N = 288


@functools.lru_cache(maxsize=None)
def long_scene():
    """the main scene widened to 288 rows per image (all live).  Track T: rows 96 .. 287 of all six images, 1 148 candidates > 1 024: reported too long and left
    out.  Track T + 1: one planted point seen by rows 100 and 101 of image 2 (two observations of one image), row 100 of image 0 and row 100 of image 3 —
    these rows are relabelled from track T.  -> (the input, the same input without the labels of track T: what must come back bit for bit elsewhere)"""
    sc = main_scene()
    base = dict(oracle_input(sc), num=None)
    rng = np.random.default_rng(131)
    T = len(base["xyz"])
    true_poses, _ = O.cameras(O.K, 70)                                   # the poses the main scene was planted under
    kpts = np.concatenate([base["kpts"], rng.uniform([0, 0], O.FRAME, (O.K, LONG_N - O.N, 2)).astype(np.float32)], 1)
    tid = np.concatenate([base["track_id"], np.full((O.K, LONG_N - O.N), T, np.int64)], 1)
    X = O.BOX_CENTRE + np.array([0.3, -0.2, 0.1])
    for k, i in ((0, 100), (2, 100), (2, 101), (3, 100)):
        px, _ = O.project_pixels(true_poses[k], base["cams"][k], X[None])
        kpts[k, i] = (px[0] + rng.normal(0, O.SIGMA, 2)).astype(np.float32)
        tid[k, i] = T + 1
    xyz = np.concatenate([base["xyz"], O.BOX_CENTRE[None].astype(np.float32), (X + 0.03)[None].astype(np.float32)])
    inp = dict(base, kpts=kpts, track_id=tid, xyz=xyz)
    return inp, dict(inp, track_id=np.where(tid == T, -1, tid))


GPU_SCENES.update({"far": far_scene, "long": lambda: long_scene()[0], "long clean": lambda: long_scene()[1]})
