"""Numpy restatement of the bundle adjuster's iterative solver (include/lightglue_amd.h, lg_bundle_adjust_pcg), float64: the block-Jacobi preconditioner, the
matrix-free operator q = S p (one pass over the tracks, one over the images), the conjugate-gradient recurrences with the definition's fixed orders of every
sum, the stopping rule and the two counters.  Everything that is not the solve is lg_bundle_adjust_robust's definition as tests/bundle_robust_oracle.py
states it (that file and tests/bundle_oracle.py are not edited: their small pieces, scenes and scales are used from here, and the Levenberg-Marquardt loop
around the solve is written out again because theirs closes over its solver).  Sums over observations run through np.add.at, which accumulates in index
order; W is precomputed per observation (the definition fixes sums, not storage).  `order="descending"` reverses the observations, the images of a dot
product and the entries of the 6-vectors, to measure what the orders are worth.  Every stopping decision and every p.q test within a relative NEAR of its
bar is recorded in `near`, next to the decisions the other two oracles record.  No GPU, no torch."""
import functools

import numpy as np

import bundle_oracle as B
import bundle_robust_oracle as R
import triangulate_oracle as O
from bundle_oracle import ACTIVE, NEAR, SHORT

MAX_CG_ITERATIONS, CG_TOLERANCE = 100, 1e-6
TIGHT = 1e-13                               # the tolerance at which the tests compare with the dense definition
PARTIALS = 256
MAX_IMAGES, MAX_CG, MAX_SOLVER_ITERATIONS = 4096, 1000, 20000


def mat3(M, v):
    """rows (M[r][0] v0 + M[r][1] v1) + M[r][2] v2 of a [.., R, 3] stack times [.., 3]"""
    return (M[..., 0] * v[..., None, 0] + M[..., 1] * v[..., None, 1]) + M[..., 2] * v[..., None, 2]


def rows6(M, v, flip=False):
    """[K, 6, 6] times [K, 6]: entry r the products over c in order, the first starts the sum"""
    cs = range(5, -1, -1) if flip else range(6)
    out = None
    for c in cs:
        term = M[:, :, c] * v[:, None, c]
        out = term if out is None else out + term
    return out


def dot_images(a, b, free, flip=False):
    """THE dot product of the definition: per image over its 6 entries, 256 interleaved partials over the images, a halving tree"""
    es = range(5, -1, -1) if flip else range(6)
    d = None
    for e in es:
        term = a[:, e] * b[:, e]
        d = term if d is None else d + term
    d = np.where(free, d, 0.0)
    K = len(d)
    pad = np.zeros((K + PARTIALS - 1) // PARTIALS * PARTIALS)
    pad[:K] = d
    layers = pad.reshape(-1, PARTIALS)
    part = np.zeros(PARTIALS)
    for row in (layers[::-1] if flip else layers):
        part = part + row
    h = PARTIALS // 2
    while h >= 1:
        part = part[:h] + part[h:2 * h]
        h //= 2
    return float(part[0])


def inverse6(S, near):
    """M = S^-1 of the definition: S = L L^T by rows from the lower triangle (every product subtracted on its own, k ascending), then column by column
    L w = e forwards and L^T m = w backwards; None on a pivot that is not > 0 (or not finite)"""
    L = np.zeros((6, 6))
    for i in range(6):
        for j in range(i + 1):
            d = S[i, j]
            for k in range(j):
                d = d - L[i, k] * L[j, k]
            if i == j:
                if abs(d) <= NEAR * abs(S[i, i]):
                    near.append("pivot6")
                if not (d > 0 and np.isfinite(d)):
                    return None
                L[i, i] = np.sqrt(d)
            else:
                L[i, j] = d / L[j, j]
    M = np.zeros((6, 6))
    for c in range(6):
        w, m = np.zeros(6), np.zeros(6)
        for i in range(6):
            d = 1.0 if i == c else 0.0
            for k in range(i):
                d = d - L[i, k] * w[k]
            w[i] = d / L[i, i]
        for i in range(5, -1, -1):
            d = w[i]
            for k in range(i + 1, 6):
                d = d - L[k, i] * m[k]
            m[i] = d / L[i, i]
        M[:, c] = m
    return M


def trial_pose(P, x):
    """R <- Rodrigues(w) R, t <- Rodrigues(w) t + d for the step x = (w, d), in the kernels' order of operations"""
    w = x[:3]
    th = np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    Q = np.eye(3)
    if th > 0.0:
        kx, ky, kz = w[0] / th, w[1] / th, w[2] / th
        sn, c1 = np.sin(th), 1.0 - np.cos(th)
        Kx = np.array([[0.0, -kz, ky], [kz, 0.0, -kx], [-ky, kx, 0.0]])
        kk = (Kx[:, 0, None] * Kx[None, 0, :] + Kx[:, 1, None] * Kx[None, 1, :]) + Kx[:, 2, None] * Kx[None, 2, :]
        Q = (Q + sn * Kx) + c1 * kk
    out = (Q[:, 0, None] * P[None, 0, :] + Q[:, 1, None] * P[None, 1, :]) + Q[:, 2, None] * P[None, 2, :]
    out[:, 3] = out[:, 3] + x[3:]
    return out


def adjust(inp, loss="squared", loss_scale=R.LOSS_SCALE, filter_rounds=0, max_reproj_error=R.MAX_REPROJ_ERROR, num_iterations=B.ITERATIONS,
           initial_damping=B.DAMPING, function_tolerance=B.TOLERANCE, max_cg_iterations=MAX_CG_ITERATIONS, cg_tolerance=CG_TOLERANCE, order="ascending"):
    """inp: as tests/bundle_oracle.py adjust -> tests/bundle_robust_oracle.py adjust's dict plus cg_iterations, cg_unconverged, cg_counts (the solver
    iterations of every Levenberg-Marquardt iteration) and accepts (its accept / reject sequence)"""
    assert loss in R.LOSSES and 0 <= filter_rounds <= R.MAX_FILTER_ROUNDS and order in ("ascending", "descending")
    flip = order == "descending"
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
        """the active observations in ascending node order (which is every track's order and every image's row order) and the free images"""
        cand = [[] for _ in range(T)]
        for k, i in np.argwhere(state == ACTIVE):
            cand[tid[k, i]].append((int(k), int(i)))
        adjusted = np.array([2 <= len(cd) <= B.MAX_LEN for cd in cand], bool)
        for j, cd in enumerate(cand):
            if not adjusted[j]:
                for k, i in cd:
                    state[k, i] = SHORT if len(cd) < 2 else B.TOO_LONG
        active = state == ACTIVE
        obs = np.argwhere(active)                               # ascending node order
        sets.update(adjusted=adjusted, active=active, free=ok & ~constant & active.any(1), obs=obs, ok_=obs[:, 0], oi=obs[:, 1], oj=tid[obs[:, 0], obs[:, 1]])

    def cost_of(Ps, Xs):
        total, failed = 0.0, False
        sk = np.zeros(K)
        with np.errstate(all="ignore"):
            for k, i in sets["obs"]:
                p = B.project(Ps[k], Xs[tid[k, i]])
                r = B.residual(cam[k], p, kpts[k, i])
                s = r[0] * r[0] + r[1] * r[1]
                if abs(p[2]) <= NEAR * np.linalg.norm(p):
                    near.append("pz = 0")
                if not p[2] > 0 or not np.isfinite(s):
                    failed, s = True, 0.0
                sk[k] += R.rho_and_weight(loss, s, c, near)[0]
            for k in range(K):
                total += sk[k]
        return total, failed

    counters = dict(cg=0, unconverged=0, counts=[])

    def step(Ps, Xs, lam):
        """(pose steps [K, 6], point steps [T, 3]) or None if the trial failed in the points, the setup or the solve"""
        free, adjusted, ok_, oi, oj = sets["free"], sets["adjusted"], sets["ok_"], sets["oi"], sets["oj"]
        n = len(ok_)
        A, Bm, r = np.zeros((n, 2, 6)), np.zeros((n, 2, 3)), np.zeros((n, 2))
        for o in range(n):
            k, i = int(ok_[o]), int(oi[o])
            p = B.project(Ps[k], Xs[oj[o]])
            A[o], Bm[o] = B.jacobians(Ps[k], cam[k], p)
            r[o] = B.residual(cam[k], p, kpts[k, i])
            if loss != "squared":
                sw = np.sqrt(R.rho_and_weight(loss, r[o, 0] * r[o, 0] + r[o, 1] * r[o, 1], c, near)[1])
                A[o], Bm[o], r[o] = sw * A[o], sw * Bm[o], sw * r[o]
        seq = np.arange(n)[::-1] if flip else np.arange(n)
        outer = lambda a, b: a[:, 0, :, None] * b[:, 0, None, :] + a[:, 1, :, None] * b[:, 1, None, :]
        U, gc, V, gp = np.zeros((K, 6, 6)), np.zeros((K, 6)), np.zeros((T, 3, 3)), np.zeros((T, 3))
        np.add.at(U, ok_[seq], outer(A, A)[seq])
        np.add.at(gc, ok_[seq], (A[:, 0] * r[:, None, 0] + A[:, 1] * r[:, None, 1])[seq])
        np.add.at(V, oj[seq], outer(Bm, Bm)[seq])
        np.add.at(gp, oj[seq], (Bm[:, 0] * r[:, None, 0] + Bm[:, 1] * r[:, None, 1])[seq])
        for d in range(6):
            U[:, d, d] = [B.damped(u, lam) for u in U[:, d, d]]
        tracks = np.flatnonzero(adjusted)
        Vi, y = np.zeros((T, 3, 3)), np.zeros((T, 3))
        for j in tracks:
            Vd = V[j].copy()
            for d in range(3):
                Vd[d, d] = B.damped(Vd[d, d], lam)
            for col in range(3):
                x = B.solve3(Vd, np.eye(3)[col], near)
                if x is None:
                    return None
                Vi[j][:, col] = x
        y[tracks] = mat3(Vi[tracks], gp[tracks])
        W = outer(A, Bm)                                        # [n, 6, 3]
        Y = np.stack([mat3(np.swapaxes(Vi[oj], 1, 2), W[:, q]) for q in range(6)], 1)      # Y[r][m] = (W[r][0] Vi[0][m] + W[r][1] Vi[1][m]) + W[r][2] Vi[2][m]
        wy = np.zeros((K, 6))
        np.add.at(wy, ok_[seq], mat3(W, y[oj])[seq])
        b = np.where(free[:, None], wy - gc, 0.0)
        # E_aa: per row of image a, over the observations of the row's track in image a in the track's order
        same = {}
        for o in range(n):
            same.setdefault((int(ok_[o]), int(oj[o])), []).append(o)
        E = np.zeros((K, 6, 6))
        for o in seq:
            k = int(ok_[o])
            if free[k]:
                group = same[k, int(oj[o])]
                for o2 in (group[::-1] if flip else group):
                    Yo, Wb = Y[o], W[o2]                         # entry (r, c): (Y[r][0] Wb[c][0] + Y[r][1] Wb[c][1]) + Y[r][2] Wb[c][2]
                    E[k] += (Yo[:, None, 0] * Wb[None, :, 0] + Yo[:, None, 1] * Wb[None, :, 1]) + Yo[:, None, 2] * Wb[None, :, 2]
        M = np.zeros((K, 6, 6))
        for k in np.flatnonzero(free):
            Mk = inverse6(U[k] - E[k], near)                    # reads the lower triangle; a failed pivot fails the trial
            if Mk is None:
                return None
            M[k] = Mk
        mask = free[ok_]

        def tracks_sum(v):
            """per track the sum over its observations of free images, in order, of W^T v_k (over r ascending from 0)"""
            w = np.zeros((n, 3))
            for q in (range(5, -1, -1) if flip else range(6)):
                w = w + W[:, q, :] * v[ok_, q, None]
            acc = np.zeros((T, 3))
            sel = seq[mask[seq]]
            np.add.at(acc, oj[sel], w[sel])
            return acc

        def operator(p):
            u = np.zeros((T, 3))
            u[tracks] = mat3(Vi[tracks], tracks_sum(p)[tracks])
            acc = np.zeros((K, 6))
            np.add.at(acc, ok_[seq], mat3(W, u[oj])[seq])
            return np.where(free[:, None], rows6(U, p, flip) - acc, 0.0)

        dot = lambda a_, b_: dot_images(a_, b_, free, flip)
        x, res = np.zeros((K, 6)), b.copy()
        z = np.where(free[:, None], rows6(M, res, flip), 0.0)
        p = z.copy()
        rz0 = rz = dot(res, z)
        if not (np.isfinite(rz) and rz >= 0.0):
            return None
        ran = 0
        if rz0 > 0.0:
            for it in range(max_cg_iterations):
                q = operator(p)
                pq = dot(p, q)
                if abs(pq) <= NEAR * np.sqrt(dot(p, p) * dot(q, q)):
                    near.append("p.q")
                if not (np.isfinite(pq) and pq > 0.0):
                    return None
                alpha = rz / pq
                x = x + alpha * p
                res = res - alpha * q
                z = np.where(free[:, None], rows6(M, res, flip), 0.0)
                new = dot(res, z)
                ran += 1
                counters["cg"] += 1
                if not (np.isfinite(new) and new >= 0.0):
                    counters["counts"].append(ran)
                    return None
                bar = cg_tolerance * np.sqrt(rz0)
                if abs(np.sqrt(new) - bar) <= NEAR * bar:
                    near.append("cg stop")
                if np.sqrt(new) <= bar:
                    break
                if it == max_cg_iterations - 1:
                    counters["unconverged"] += 1
                    break
                p = z + (new / rz) * p
                rz = new
        counters["counts"].append(ran)
        dX = np.zeros((T, 3))
        dX[tracks] = -(y[tracks] + mat3(Vi[tracks], tracks_sum(x)[tracks]))
        return x, dX

    rebuild()
    first_state = state.copy()
    ever_free, ever_adjusted = sets["free"].copy(), sets["adjusted"].copy()
    cost, _ = cost_of(P, X)
    initial, lam, iters, accepted, converged, costs, accepts = cost, float(initial_damping), 0, 0, False, [cost], []
    filtered, fstages = 0, 0
    for stage in range(filter_rounds + 1):
        if stage:
            removed = 0
            with np.errstate(all="ignore"):
                for k, i in sets["obs"]:
                    r = B.residual(cam[k], B.project(P[k], X[tid[k, i]]), kpts[k, i])
                    s = r[0] * r[0] + r[1] * r[1]
                    if abs(s - e2) <= NEAR * e2:
                        near.append("filter")
                    if s > e2:
                        state[k, i] = R.FILTERED
                        removed += 1
            rebuild()
            ever_free |= sets["free"]
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
                    Pt[k] = trial_pose(P[k], s[k])
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
            accepts.append(bool(accept))
            if accept:
                P, X, cost, accepted, lam = Pt, Xt, new, accepted + 1, max(lam / 10.0, 1e-12)
                costs.append(cost)
            else:
                lam = min(10.0 * lam, 1e12)
            converged = bool(conv)
    active = sets["active"]
    pts, err = np.full((K, N, 3), np.nan), np.full((K, N), np.nan)
    for k, i in sets["obs"]:
        pts[k, i] = X[tid[k, i]]
        r = B.residual(cam[k], B.project(P[k], X[tid[k, i]]), kpts[k, i])
        err[k, i] = np.sqrt(r[0] * r[0] + r[1] * r[1])
    poses64 = np.where(ever_free[:, None, None], P, poses32.astype(np.float64))
    xyz64 = np.where(ever_adjusted[:, None], X, xyz32.astype(np.float64))
    return dict(poses64=poses64, xyz64=xyz64, points3d64=pts, node_state=state, error64=err, initial_cost=initial, final_cost=cost, num_iterations=iters,
                num_accepted=accepted, converged=converged, num_observations=int(active.sum()), status=np.where(ok, B.LG_OK, B.LG_ERR_CAMERA), free=ever_free,
                adjusted=ever_adjusted, free_end=sets["free"], adjusted_end=sets["adjusted"], first_state=first_state, num_filtered=filtered,
                num_filter_stages=fstages, costs=costs, near=near, cg_iterations=counters["cg"], cg_unconverged=counters["unconverged"],
                cg_counts=counters["counts"], accepts=accepts)


# ---------------------------------------------------------------------- beyond the dense envelope
BIG_K, BIG_N, BIG_T, BIG_SEED, BIG_ITERATIONS = 300, 32, 1200, 410, 4


@functools.lru_cache(maxsize=None)
def big_scene():
    """300 images of 32 rows, 1 200 tracks of 2 .. 5 views, images 0 and 1 constant: 44 more images than the dense solver takes; neither count is a multiple
    of 64 or 256"""
    return B.oracle_input(B.scene(BIG_K, BIG_N, BIG_T, BIG_SEED, hi=5))


SCENES = dict(R.SCENES, far=B.GPU_SCENES["far"], big=big_scene)
SCENES["K = 24"] = B.GPU_SCENES["K = 24"]
SCENES["long cauchy"] = SCENES["long"]


# the calls of tests/test_gpu_bundle_pcg.py (tests/test_bundle_pcg_cpu.py checks their preconditions): at the tight tolerance against the dense definition, and
# at the default tolerance.  Every budget is the oracle's largest solver-iteration count of the call (COUNTS) plus at least a quarter
TIGHT_CALLS = {"main": dict(cg_tolerance=TIGHT, max_cg_iterations=40), "K = 9": dict(cg_tolerance=TIGHT, max_cg_iterations=60),
               "K = 24": dict(cg_tolerance=TIGHT, max_cg_iterations=90), "edge": dict(cg_tolerance=TIGHT, max_cg_iterations=40),
               "edge clean": dict(cg_tolerance=TIGHT, max_cg_iterations=40), "far": dict(cg_tolerance=TIGHT, max_cg_iterations=40),
               "planted": dict(R.CAUCHY, **R.ONE_ROUND, cg_tolerance=TIGHT, max_cg_iterations=40),
               "big": dict(num_iterations=BIG_ITERATIONS, cg_tolerance=TIGHT, max_cg_iterations=150),
               # two observations of one track in one image (rows 100 and 101 of image 2): the E_aa branches for a repeated track, squared and weighted
               "long": dict(cg_tolerance=TIGHT, max_cg_iterations=40), "long cauchy": dict(R.CAUCHY, cg_tolerance=TIGHT, max_cg_iterations=40)}
DEFAULT_CALLS = {"main": dict(), "far": dict(), "big": dict(num_iterations=BIG_ITERATIONS, max_cg_iterations=120)}
COUNTS = {"tight": {"main": 22, "K = 9": 34, "K = 24": 60, "edge": 18, "edge clean": 18, "far": 22, "planted": 22, "big": 110, "long": 22, "long cauchy": 22},
          "default": {"main": 16, "far": 16, "big": 83}}


def dense_answer(name):
    """the dense definition's answer to the call TIGHT_CALLS[name] (without the solver's two settings)"""
    if name == "big":
        return dense_big()
    if name == "planted":
        return R.answer("planted", **R.CAUCHY, **R.ONE_ROUND)
    if name == "long cauchy":
        return R.answer("long", **R.CAUCHY)
    return B.answer(name)


@functools.lru_cache(maxsize=None)
def _answer(name, conf):
    return adjust(SCENES[name](), **dict(conf))


def answer(name, **conf):
    """The definition's answer on a scene of SCENES (shared by the tests; treat as read-only)"""
    return _answer(name, tuple(sorted(conf.items())))


@functools.lru_cache(maxsize=None)
def dense_big(num_iterations=BIG_ITERATIONS):
    """the dense definition (Schur complement + Cholesky) on the big scene: what the iterative solver must meet at a tight tolerance"""
    return B.adjust(big_scene(), num_iterations=num_iterations)
