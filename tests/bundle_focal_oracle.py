"""Numpy restatement of the bundle adjuster with per-image focal lengths refined (include/lightglue_amd.h, lg_bundle_adjust_focal), float64: the robust
mode's definition (tests/bundle_robust_oracle.py: loss, weights, stages, filter) with a seventh unknown d per image, fx <- fx exp(d), fy <- fy exp(d), whose
Jacobian column is (ax px, by py); poses and cameras are held independently.  It imports the small pieces and the scenes of tests/bundle_oracle.py and
tests/bundle_robust_oracle.py (and edits neither), has a dense solve of its own (`solve_spd`) and keeps the `near` list of those oracles: every decision
within a relative NEAR of its bar.  Also the scenes of tests/test_bundle_focal_cpu.py and tests/test_gpu_bundle_focal.py.  No GPU, no torch."""
import functools

import numpy as np

import bundle_oracle as B
import bundle_robust_oracle as R
import triangulate_oracle as O
from abspose_oracle import rodrigues
from bundle_oracle import ACTIVE, NEAR, SHORT

D = 7                                   # unknowns per image: the pose's six, then d


def jacobians(P, cam, p):
    """A [2, 7] (tests/bundle_oracle.py's six pose columns, then the log focal scale's (ax px, by py)), B [2, 3]"""
    A6, Bm = B.jacobians(P, cam, p)
    iz = 1.0 / p[2]
    ax, by = cam[0] * iz, cam[1] * iz
    return np.concatenate([A6, np.array([[ax * p[0]], [by * p[1]]])], 1), Bm


def solve_spd(S, rhs, near):
    """x of S x = rhs for a symmetric S given by its lower triangle: an outer-product Cholesky and two substitutions; None on a pivot that is not > 0"""
    n = len(rhs)
    M = np.tril(S).copy()
    for j in range(n):
        if abs(M[j, j]) <= NEAR * abs(S[j, j]):
            near.append("pivot")
        if not (M[j, j] > 0 and np.isfinite(M[j, j])):
            return None
        M[j, j] = np.sqrt(M[j, j])
        M[j + 1:, j] /= M[j, j]
        for c in range(j + 1, n):
            M[c:, c] -= M[c:, j] * M[c, j]
    z = np.zeros(n)
    for i in range(n):
        z[i] = (rhs[i] - M[i, :i] @ z[:i]) / M[i, i]
    x = np.zeros(n)
    for i in range(n - 1, -1, -1):
        x[i] = (z[i] - M[i + 1:, i] @ x[i + 1:]) / M[i, i]
    return x


def adjust(inp, loss="squared", loss_scale=R.LOSS_SCALE, filter_rounds=0, max_reproj_error=R.MAX_REPROJ_ERROR, num_iterations=B.ITERATIONS,
           initial_damping=B.DAMPING, function_tolerance=B.TOLERANCE):
    """inp: as tests/bundle_oracle.py adjust plus constant_camera ([K] bool, or None / absent: no camera is held) -> tests/bundle_robust_oracle.py's dict plus
    cameras64 [K, 4], free_camera [K] (free in any stage) and num_free_cameras"""
    assert loss in R.LOSSES and 0 <= filter_rounds <= R.MAX_FILTER_ROUNDS
    c, e2 = float(loss_scale), float(max_reproj_error) * float(max_reproj_error)
    kpts = np.asarray(inp["kpts"], np.float32)
    K, N = kpts.shape[:2]
    tid = np.asarray(inp["track_id"], np.int64).reshape(K, N)
    xyz32 = np.asarray(inp["xyz"], np.float32).reshape(-1, 3)
    T = len(xyz32)
    cams32, poses32 = np.asarray(inp["cams"], np.float32), np.asarray(inp["poses"], np.float32)
    ok = np.array([O.image_ok(cams32[k], poses32[k]) for k in range(K)])
    cam = cams32.astype(np.float64)                 # the state: columns 0 and 1 move
    P = np.where(ok[:, None, None], poses32.astype(np.float64), 0.0)
    X = xyz32.astype(np.float64)
    live = O.live_rows(inp.get("num"), K, N)
    constant = np.asarray(inp["constant"], bool)
    held = inp.get("constant_camera")
    held = np.zeros(K, bool) if held is None else np.asarray(held, bool)
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
        cand = [[] for _ in range(T)]
        for k, i in np.argwhere(state == ACTIVE):
            cand[tid[k, i]].append((int(k), int(i)))
        adjusted = np.array([2 <= len(cd) <= B.MAX_LEN for cd in cand], bool)
        for j, cd in enumerate(cand):
            if not adjusted[j]:
                for k, i in cd:
                    state[k, i] = SHORT if len(cd) < 2 else B.TOO_LONG
        active = state == ACTIVE
        sets.update(adjusted=adjusted, active=active, free=ok & ~constant & active.any(1), free_camera=ok & ~held & active.any(1),
                    rows_of=[np.flatnonzero(active[k]).tolist() for k in range(K)], obs_of=[cd if adjusted[j] else [] for j, cd in enumerate(cand)])

    def cost_of(Ps, Xs, Cs):
        total, failed = 0.0, False
        with np.errstate(all="ignore"):
            for k in range(K):
                sk = 0.0
                for i in sets["rows_of"][k]:
                    p = B.project(Ps[k], Xs[tid[k, i]])
                    r = B.residual(Cs[k], p, kpts[k, i])
                    s = r[0] * r[0] + r[1] * r[1]
                    if abs(p[2]) <= NEAR * np.linalg.norm(p):
                        near.append("pz = 0")
                    if not p[2] > 0 or not np.isfinite(s):
                        failed, s = True, 0.0
                    sk += R.rho_and_weight(loss, s, c, near)[0]
                total += sk
        return total, failed

    def step(Ps, Xs, Cs, lam):
        """(image steps [K, 7], point steps [T, 3]) or None if a pivot failed.  A held column's Jacobian column is zero, which is its identity diagonal, zero
        coupling and zero right-hand side once the diagonal is set to 1"""
        rows_of, obs_of, adjusted = sets["rows_of"], sets["obs_of"], sets["adjusted"]
        alive = np.concatenate([np.repeat(sets["free"][:, None], 6, 1), sets["free_camera"][:, None]], 1)          # [K, 7]
        lin = {}
        U, gc = np.zeros((K, D, D)), np.zeros((K, D))
        for k in range(K):
            for i in rows_of[k]:
                p = B.project(Ps[k], Xs[tid[k, i]])
                A, Bm = jacobians(Ps[k], Cs[k], p)
                r = B.residual(Cs[k], p, kpts[k, i])
                if loss != "squared":
                    sw = np.sqrt(R.rho_and_weight(loss, r[0] * r[0] + r[1] * r[1], c, near)[1])
                    A, Bm, r = sw * A, sw * Bm, sw * r
                A = np.where(alive[k][None, :], A, 0.0)
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
            for d in range(D):
                U[k, d, d] = B.damped(U[k, d, d], lam) if alive[k, d] else 1.0
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
        S, rhs = np.zeros((D * K, D * K)), np.zeros(D * K)
        for a in range(K):
            sa = slice(D * a, D * a + D)
            E, wy = np.zeros((K, D, D)), np.zeros(D)
            for i in rows_of[a]:
                j = tid[a, i]
                Y = W(a, i) @ Vi[j]
                wy += W(a, i) @ y[j]
                for b, i2 in obs_of[j]:
                    if b <= a:
                        E[b] += Y @ W(b, i2).T
            for b in range(a + 1):
                S[sa, D * b:D * b + D] = (U[a] if b == a else 0.0) - E[b]
            rhs[sa] = wy - gc[a]
        s = solve_spd(S, rhs, near)
        if s is None:
            return None
        s = s.reshape(K, D)
        dX = np.zeros((T, 3))
        for j in tracks:
            acc = np.zeros(3)
            for k, i in obs_of[j]:
                acc += W(k, i).T @ s[k]
            dX[j] = -(y[j] + Vi[j] @ acc)
        return s, dX

    rebuild()
    first_state = state.copy()
    ever_free, ever_adjusted, ever_camera = sets["free"].copy(), sets["adjusted"].copy(), sets["free_camera"].copy()
    cost, _ = cost_of(P, X, cam)
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
                            state[k, i] = R.FILTERED
                            removed += 1
            rebuild()
            if removed:
                cost, _ = cost_of(P, X, cam)
                lam, converged, filtered, fstages = float(initial_damping), False, filtered + removed, fstages + 1
                costs.append(cost)
        for _ in range(num_iterations):
            if converged:
                break
            iters += 1
            with np.errstate(all="ignore"):
                st = step(P, X, cam, lam)
                good = st is not None
                if good:
                    s, dX = st
                    Pt, Xt, Ct = P.copy(), X + dX, cam.copy()
                    for k in np.flatnonzero(sets["free"]):
                        Q = rodrigues(s[k, :3])
                        Pt[k] = np.concatenate([Q @ P[k][:, :3], (Q @ P[k][:, 3] + s[k, 3:6])[:, None]], 1)
                    for k in np.flatnonzero(sets["free_camera"]):
                        Ct[k, :2] = cam[k, :2] * np.exp(s[k, 6])
                    focal_ok = bool((np.isfinite(Ct[sets["free_camera"], :2]) & (Ct[sets["free_camera"], :2] > 0)).all())
                    new, failed = cost_of(Pt, Xt, Ct)
                    good = not failed and focal_ok and np.isfinite(Pt).all() and np.isfinite(Xt[sets["adjusted"]]).all() and np.isfinite(new)
            conv = accept = False
            if good:
                bar = function_tolerance * cost
                if abs(abs(cost - new) - bar) <= NEAR * bar:
                    near.append("convergence")
                if abs(cost - new) <= NEAR * cost:
                    near.append("accept")
                conv, accept = abs(cost - new) <= bar, new < cost
            if accept:
                P, X, cam, cost, accepted, lam = Pt, Xt, Ct, new, accepted + 1, max(lam / 10.0, 1e-12)
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
    cameras64 = np.where(ever_camera[:, None] & (np.arange(4) < 2)[None, :], cam, cams32.astype(np.float64))
    return dict(poses64=poses64, xyz64=xyz64, cameras64=cameras64, points3d64=pts, node_state=state, error64=err, initial_cost=initial, final_cost=cost,
                num_iterations=iters, num_accepted=accepted, converged=converged, num_observations=int(active.sum()),
                status=np.where(ok, B.LG_OK, B.LG_ERR_CAMERA), free=ever_free, adjusted=ever_adjusted, free_camera=ever_camera,
                num_free_cameras=int(ever_camera.sum()), free_end=sets["free"], adjusted_end=sets["adjusted"], first_state=first_state, num_filtered=filtered,
                num_filter_stages=fstages, costs=costs, near=near)


scales = R.scales


# ---------------------------------------------------------------------- scenes: those of the two oracles with every focal length off by a factor of its own
FOCAL_LOW, FOCAL_HIGH, FOCAL_SEED = 0.92, 1.08, 23


def focal_factors(K, seed=FOCAL_SEED):
    """one factor per image, uniform in [0.92, 1.08]"""
    return np.random.default_rng(seed).uniform(FOCAL_LOW, FOCAL_HIGH, K)


def wrong_focal(inp, seed=FOCAL_SEED):
    """the same input with fx and fy of every camera multiplied by the image's factor (rounded to float32: what the call is given)"""
    cams = np.asarray(inp["cams"], np.float32).copy()
    cams[:, :2] = (cams[:, :2].astype(np.float64) * focal_factors(len(cams), seed)[:, None]).astype(np.float32)
    return dict(inp, cams=cams)


def triangulate_dlt(inp):
    """every track's point by the linear (DLT) triangulation from ALL its labelled live rows under inp's poses and cameras, float32 -> xyz [T, 3]"""
    kpts, tid, cams, poses = np.asarray(inp["kpts"], np.float64), np.asarray(inp["track_id"]), np.asarray(inp["cams"], np.float64), np.asarray(inp["poses"], np.float64)
    K, N = tid.shape
    live = O.live_rows(inp.get("num"), K, N)
    xyz = np.asarray(inp["xyz"], np.float32).copy()
    for j in range(len(xyz)):
        rows = []
        for k, i in np.argwhere(tid == j):
            if i >= live[k]:
                continue
            x, y = (kpts[k, i, 0] - cams[k, 2]) / cams[k, 0], (kpts[k, i, 1] - cams[k, 3]) / cams[k, 1]
            rows += [x * poses[k][2] - poses[k][0], y * poses[k][2] - poses[k][1]]
        if len(rows) >= 4:
            h = np.linalg.svd(np.array(rows))[2][-1]
            xyz[j] = (h[:3] / h[3]).astype(np.float32)
    return xyz


RECOVERY_K, RECOVERY_N, RECOVERY_TRACKS, RECOVERY_SEED = 6, 64, 60, 301
RECOVERY_ITERATIONS = 30


@functools.lru_cache(maxsize=None)
def recovery_scene(sigma=0.0):
    """-> (input, true cameras [K, 4]).  Six images of 64 rows, 60 tracks of 3 .. 6 views in the box of tests/triangulate_oracle.py (generic, not planar), the
    TRUE poses for all images (0 and 1 held), observations exact up to float32 (sigma = 0) or with `sigma` pixels of noise, every focal length off by its
    factor, and the points triangulated linearly under those wrong cameras"""
    rng = np.random.default_rng(RECOVERY_SEED)
    poses, cams = O.cameras(RECOVERY_K, RECOVERY_SEED)
    views = O.random_views(RECOVERY_K, RECOVERY_TRACKS, rng, 3, None)
    pl = O.plant(poses, cams, views, RECOVERY_SEED + 1, (RECOVERY_N,) * RECOVERY_K, RECOVERY_N)
    tid = np.full((RECOVERY_K, RECOVERY_N), -1, np.int64)
    kpts = pl["kpts"].copy()
    for j, at in enumerate(pl["rows"]):
        for k, i in at.items():
            tid[k, i] = j
            px, _ = O.project_pixels(poses[k], cams[k], pl["X"][j][None])
            kpts[k, i] = (px[0] + (rng.normal(0, sigma, 2) if sigma else 0.0)).astype(np.float32)
    const = np.zeros(RECOVERY_K, bool)
    const[:2] = True
    inp = dict(kpts=kpts, num=None, track_id=tid, xyz=pl["X"].astype(np.float32), cams=np.asarray(cams, np.float32), poses=poses.astype(np.float32), constant=const)
    inp = wrong_focal(inp)
    return dict(inp, xyz=triangulate_dlt(inp)), np.asarray(cams, np.float64)


def focal_error(cameras, truth):
    """the relative error of fx per image (fy has the same factor)"""
    return np.abs(np.asarray(cameras, np.float64)[:, 0] / truth[:, 0] - 1.0)


# ---------------------------------------------------------------------- the scenes of tests/test_gpu_bundle_focal.py and the calls the tests share (read-only)
def _focal(name):
    return lambda: wrong_focal(R.SCENES[name]() if name in R.SCENES else B.GPU_SCENES[name]())


def _held(name, pose=None, camera=None):
    """scene `name` with the pose mask and the camera mask given as index lists (None: the scene's own / none held)"""
    def make():
        inp = SCENES[name]()
        K = len(inp["cams"])
        out = dict(inp)
        if pose is not None:
            out["constant"] = np.isin(np.arange(K), pose)
        if camera is not None:
            out["constant_camera"] = np.isin(np.arange(K), camera)
        return out
    return make


SCENES = {"main": _focal("main"), "K = 7": _focal("edge clean"), "K = 9": _focal("K = 9"), "planted": _focal("planted"), "long": _focal("long"),
          "edge": _focal("edge"), "edge clean": _focal("edge clean")}
# main scene: images 0 and 1 hold their poses.  "pose held, camera free" is what those two are with no camera held ("main"); "pose free, camera held": images
# 3 and 4; "all held": every camera
SCENES.update({"camera held": _held("main", camera=[3, 4]), "all held": _held("main", camera=list(range(O.K)))})
CONF = {"main": {}, "K = 7": {}, "K = 9": {}, "planted": dict(R.CAUCHY, **R.ONE_ROUND), "long": dict(R.CAUCHY), "edge": {}, "edge clean": {},
        "camera held": {}, "all held": {}}


@functools.lru_cache(maxsize=None)
def answer(name):
    """The definition's answer on a GPU-test scene under CONF[name] (shared by the tests; treat as read-only)"""
    return adjust(SCENES[name](), **CONF[name])
