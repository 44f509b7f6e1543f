"""Numpy restatement of the absolute-pose estimator's definition (include/lightglue_amd.h, lg_abspose_estimate), float64: correspondences, centring, bearings,
the P3P solver, the reprojection test, the selection rule, the Gauss-Newton refinement and the pooling of a query's pairs into one problem.  The SOLVER is a
formulation of its own, not the kernels': the two law-of-cosines equations left after eliminating s1 are quadratics in u whose coefficients are polynomials in
v; their resultant (polynomial arithmetic through np.polymul) is a quartic whose roots come from np.roots; u is the common root of the two quadratics, s1
comes from the b-equation, and (R, t') is the rigid alignment of the three world points to the three camera points through the SVD.  Only the root order
(ascending v) and the validity rules are the header's.  `grunert` holds the header's closed-form coefficients; tests/test_abspose_cpu.py compares the two.
`dtype` float64 is the ideal (nothing rounded: exact centroid, float64 bearings, candidates and test); float32 rounds what the definition rounds — the centroid
and X' = X - c, the bearings' two quotients, the candidate, the test in float32 with fmaf emulated through float64, t = t' - R c — with the solver still in
float64.  Also the scenes and the case tables shared by tests/test_abspose_cpu.py and tests/test_gpu_abspose.py.  No GPU, no torch."""
import functools

import numpy as np

from twoview_oracle import sample, _fma      # noqa: F401  (the shared sampling definition; fmaf through float64)
import twoview_oracle as TV

SAMPLE, REFINE_MIN, ROOTS, GN_STEPS, EPS = 3, 4, 4, 5, 1e-12


# ---------------------------------------------------------------------- correspondences, centring, bearings
def correspondences(kpts0, points3d1, matches0, num0=None, num1=None):
    """(rows [S], corr [S, 5] float64 holding the float32 (x, y, X, Y, Z)): row i counts unless matches0[i] < 0, i >= num0, matches0[i] >= n1 or >= num1, or
    the point has a non-finite coordinate"""
    kpts0, pts, matches0 = np.asarray(kpts0, np.float32), np.asarray(points3d1, np.float32), np.asarray(matches0, np.int64)
    live0 = len(kpts0) if num0 is None else min(max(int(num0), 0), len(kpts0))
    live1 = len(pts) if num1 is None else min(max(int(num1), 0), len(pts))
    i = np.arange(len(matches0))
    take = (i < live0) & (matches0 >= 0) & (matches0 < live1)
    take[take] = np.isfinite(pts[matches0[take]]).all(1)
    rows = i[take]
    return rows, np.concatenate([kpts0[rows], pts[matches0[rows]]], 1).astype(np.float64).reshape(-1, 5)


def centre(corr, dtype=np.float64):
    """(c [3], the list with X' = X - c): float64: the exact mean; float32: the mean (sum times 1 / S) rounded to float32 and one float32 subtraction"""
    if len(corr) == 0:
        return np.zeros(3), corr.copy()
    c = corr[:, 2:].sum(0) * (1.0 / len(corr))
    out = corr.copy()
    if np.dtype(dtype) == np.float32:
        c = c.astype(np.float32)
        out[:, 2:] = (corr[:, 2:].astype(np.float32) - c).astype(np.float64)
        return c.astype(np.float64), out
    out[:, 2:] = corr[:, 2:] - c
    return c, out


def camera_ok(cam):
    cam = np.asarray(cam, np.float64)
    return bool(np.isfinite(cam).all() and (cam[:2] > 0).all())


def bearings(xy, cam, dtype=np.float64):
    """[S, 3] float64 unit vectors; dtype float32: the two quotients formed in float32 as the definition says, then widened"""
    dt = np.dtype(dtype)
    p, c = np.asarray(xy).astype(dt), np.asarray(cam, np.float32).astype(dt)
    b = np.stack([(p[:, 0] - c[2]) / c[0], (p[:, 1] - c[3]) / c[1], np.ones(len(p), dt)], 1).astype(np.float64)
    return b / np.linalg.norm(b, axis=1, keepdims=True)


# ---------------------------------------------------------------------- the P3P solver (its own formulation)
def triangle(f, P):
    """(a2, b2, c2, cos A, cos B, cos G) of three bearings f [3, 3] and three world points P [3, 3]"""
    return (((P[1] - P[2]) ** 2).sum(), ((P[0] - P[2]) ** 2).sum(), ((P[0] - P[1]) ** 2).sum(), f[1] @ f[2], f[0] @ f[2], f[0] @ f[1])


def grunert(f, P):
    """the header's closed-form coefficients [A4, A3, A2, A1, A0] (Grunert 1841 as in Haralick et al. 1994)"""
    a2, b2, c2, ca, cb, cg = triangle(f, P)
    k, m = (a2 - c2) / b2, (a2 + c2) / b2
    return np.array([(k - 1) ** 2 - 4 * c2 / b2 * ca ** 2,
                     4 * (k * (1 - k) * cb - (1 - m) * ca * cg + 2 * c2 / b2 * ca ** 2 * cb),
                     2 * (k ** 2 - 1 + 2 * k ** 2 * cb ** 2 + 2 * (b2 - c2) / b2 * ca ** 2 - 4 * m * ca * cb * cg + 2 * (b2 - a2) / b2 * cg ** 2),
                     4 * (-k * (1 + k) * cb + 2 * a2 / b2 * cg ** 2 * cb - (1 - m) * ca * cg),
                     (1 + k) ** 2 - 4 * a2 / b2 * cg ** 2])


def resultant(f, P):
    """(quartic [5] descending in v, D0 [3], D1 [2]): with s2 = u s1, s3 = v s1 and w(v) = 1 + v^2 - 2 v cos B, the a- and c-equations divided by the
    b-equation are u^2 + p1 u + p0 = 0 and u^2 + q1 u + q0 = 0 with p1 = -2 cos A v, p0 = v^2 - (a2 / b2) w, q1 = -2 cos G, q0 = 1 - (c2 / b2) w.  Their
    difference gives u = -D0 / D1 (D0 = p0 - q0, D1 = p1 - q1); put into the second: D0^2 - q1 D0 D1 + q0 D1^2 = 0"""
    a2, b2, c2, ca, cb, cg = triangle(f, P)
    w = np.array([1.0, -2 * cb, 1.0])
    p0, q0 = np.array([1.0, 0, 0]) - a2 / b2 * w, np.array([0, 0, 1.0]) - c2 / b2 * w
    D0, D1 = p0 - q0, np.array([-2 * ca, 2 * cg])
    quartic = np.polyadd(np.polysub(np.polymul(D0, D0), -2 * cg * np.polymul(D0, D1)), np.polymul(q0, np.polymul(D1, D1)))
    return quartic, D0, D1


def align(P, C):
    """(R, t) with C_k = R P_k + t for two congruent triangles: Kabsch through the SVD"""
    mp, mc = P.mean(0), C.mean(0)
    U, _, Vt = np.linalg.svd((C - mc).T @ (P - mp))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    R = U @ D @ Vt
    return R, mc - R @ mp


def p3p(f, P):
    """the candidates of ONE sample: (poses [4, 12] float64 (R | t') row-major, zero where there is none; valid [4]; v [4]), root index ascending in v over the
    real roots of the quartic"""
    poses, valid, vs = np.zeros((ROOTS, 12)), np.zeros(ROOTS, bool), np.zeros(ROOTS)
    a2, b2, c2, ca, cb, cg = triangle(f, P)
    with np.errstate(all="ignore"):
        if not b2 > 0 or not np.linalg.norm(np.cross(P[1] - P[0], P[2] - P[0])) > EPS * np.sqrt(b2) * np.sqrt(c2):
            return poses, valid, vs
        quartic, D0, D1 = resultant(f, P)
        if not np.isfinite(quartic).all() or quartic[0] == 0:
            return poses, valid, vs
        z = np.roots(quartic)
        real = np.sort(z.real[abs(z.imag) <= 1e-9 * (1 + abs(z.real))])
        for r, v in enumerate(real[:ROOTS]):
            vs[r] = v
            den = cg - v * ca
            if not (v > 0 and abs(den) > EPS):
                continue
            u = -np.polyval(D0, v) / np.polyval(D1, v)
            if not (u > 0 and 1 + u * u - 2 * u * cg > 0):
                continue
            s1 = np.sqrt(b2 / (1 + v * v - 2 * v * cb))
            R, t = align(P, np.stack([s1 * f[0], u * s1 * f[1], v * s1 * f[2]]))
            pose = np.concatenate([R, t[:, None]], 1).reshape(12)
            if np.isfinite(pose).all():
                poses[r], valid[r] = pose, True
    return poses, valid, vs


def candidates(corr_c, cam, picks, dtype=np.float64):
    """(poses [H, 4, 12] in dtype: (R | t') of the centred list `corr_c`, zero where there is none; valid [H, 4]) of the samples `picks`"""
    dt = np.dtype(dtype)
    f = bearings(corr_c[:, :2], cam, dt)
    out, valid = np.zeros((len(picks), ROOTS, 12)), np.zeros((len(picks), ROOTS), bool)
    for h, pk in enumerate(picks):
        out[h], valid[h], _ = p3p(f[pk], corr_c[pk, 2:])
    out = out.astype(dt)
    valid &= np.isfinite(out).all(-1)
    return np.where(valid[..., None], out, 0).astype(dt), valid


# ---------------------------------------------------------------------- the inlier test
def residual_terms(m, corr_c, cam):
    """(lhs, rhs, pz) [..., S] in m's dtype, division-free: inlier iff pz > 0 and lhs <= t^2 rhs; m [..., 12]"""
    dt = m.dtype
    p, c = corr_c.astype(dt), np.asarray(cam, np.float32).astype(dt)
    x, y, X, Y, Z = (p[:, i] for i in range(5))
    e = [m[..., i, None] for i in range(12)]
    with np.errstate(all="ignore"):
        px, py, pz = (_fma(e[4 * i], X, _fma(e[4 * i + 1], Y, _fma(e[4 * i + 2], Z, e[4 * i + 3]))) for i in range(3))
        ex, ey = _fma(np.full_like(px, c[0]), px, (c[2] - x) * pz), _fma(np.full_like(py, c[1]), py, (c[3] - y) * pz)
        return _fma(ex, ex, ey * ey), pz * pz, pz


def inliers(m, corr_c, cam, t):
    """[..., S] bool in m's dtype"""
    lhs, rhs, pz = residual_terms(m, corr_c, cam)
    t2 = m.dtype.type(t) * m.dtype.type(t)
    with np.errstate(all="ignore"):
        return (pz > 0) & (lhs <= t2 * rhs)


def distances(m, corr_c, cam):
    """[S] float64: the reprojection error in pixels under ONE pose (R | t') of the list it is centred for (inf behind the camera)"""
    m, cam = np.asarray(m, np.float64).reshape(3, 4), np.asarray(cam, np.float64)
    p = corr_c[:, 2:] @ m[:, :3].T + m[:, 3]
    with np.errstate(all="ignore"):
        d = np.hypot(cam[0] * p[:, 0] / p[:, 2] + cam[2] - corr_c[:, 0], cam[1] * p[:, 1] / p[:, 2] + cam[3] - corr_c[:, 1])
    return np.where(p[:, 2] > 0, d, np.inf)


# ---------------------------------------------------------------------- frames
def to_world(m, c, dtype=np.float64):
    """(R | t) of (R | t'): t = t' - R c in float64, rounded to dtype"""
    m = np.asarray(m, np.float64).reshape(m.shape[:-1] + (3, 4)).copy()
    m[..., 3] = m[..., 3] - m[..., :3] @ c
    return m.reshape(m.shape[:-2] + (12,)).astype(dtype)


def to_centred(m, c, dtype=np.float64):
    """(R | t') of (R | t): t' = t + R c in float64, rounded to dtype"""
    m = np.asarray(m, np.float64).reshape(m.shape[:-1] + (3, 4)).copy()
    m[..., 3] = m[..., 3] + m[..., :3] @ c
    return m.reshape(m.shape[:-2] + (12,)).astype(dtype)


# ---------------------------------------------------------------------- refinement
def rodrigues(w):
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def refine(corr_c, mask, start, cam):
    """five Gauss-Newton steps from `start` [12] (widened) over the inliers `mask`; -> (R | t') [12] float64, or None if a step is abandoned"""
    cam = np.asarray(cam, np.float64)
    fx, fy, cx, cy = cam
    m = np.asarray(start, np.float64).reshape(3, 4).copy()
    c = corr_c[mask]
    for _ in range(GN_STEPS):
        p = c[:, 2:] @ m[:, :3].T + m[:, 3]
        ok = p[:, 2] > 0
        p, q = p[ok], c[ok]
        iz = 1.0 / p[:, 2]
        r = np.concatenate([fx * p[:, 0] * iz + cx - q[:, 0], fy * p[:, 1] * iz + cy - q[:, 1]])
        zero = np.zeros(len(p))
        dpi0 = np.stack([fx * iz, zero, -fx * p[:, 0] * iz * iz], 1)
        dpi1 = np.stack([zero, fy * iz, -fy * p[:, 1] * iz * iz], 1)
        skew = np.zeros((len(p), 3, 3))                                                      # -[p]x
        skew[:, 0, 1], skew[:, 0, 2], skew[:, 1, 0], skew[:, 1, 2], skew[:, 2, 0], skew[:, 2, 1] = p[:, 2], -p[:, 1], -p[:, 2], p[:, 0], p[:, 1], -p[:, 0]
        T = np.concatenate([skew, np.broadcast_to(np.eye(3), (len(p), 3, 3))], 2)            # [n, 3, 6]
        J = np.concatenate([np.einsum("ni,nij->nj", dpi0, T), np.einsum("ni,nij->nj", dpi1, T)])
        A, g = J.T @ J, J.T @ r
        # the definition abandons on a small pivot of its elimination; here: the smallest eigenvalue against the same bar (either says: rank deficient)
        if not np.isfinite(A).all() or np.linalg.eigvalsh(A)[0] <= EPS * A.diagonal().max():
            return None
        x = np.linalg.solve(A, -g)
        Q = rodrigues(x[:3])
        m = np.concatenate([Q @ m[:, :3], (Q @ m[:, 3] + x[3:])[:, None]], 1)
    return m.reshape(12) if np.isfinite(m).all() else None


# ---------------------------------------------------------------------- the whole definition for one problem
def verify(corr, cam, t, hyps, seed=0, refine_on=False, dtype=np.float64, given=None):
    """corr [S, 5] (x, y, X, Y, Z), the problem's list -> dict(pose [12] (R | t) in the world frame, mask [S], count, best_hypothesis, root, counts [hyps, 4],
    valid, picks, models [hyps, 4, 12] (R | t') of the centred list, c [3], centred [S, 5], winner_mask).  given [H, 12]: LG_ABSPOSE_GIVEN_POSES"""
    dt = np.dtype(dtype)
    S = len(corr)
    c, cc = centre(corr, dt)
    empty = dict(pose=np.zeros(12), mask=np.zeros(S, bool), count=0, best_hypothesis=-1, root=-1, counts=None, valid=None, picks=None, models=None, c=c, centred=cc,
                 winner_mask=np.zeros(S, bool))
    if S < (1 if given is not None else SAMPLE) or not camera_ok(cam):
        return empty
    if given is not None:
        g = np.asarray(given, np.float32).reshape(-1, 12)
        hyps = len(g)
        models, valid, picks = np.zeros((hyps, ROOTS, 12), dt), np.zeros((hyps, ROOTS), bool), None
        with np.errstate(all="ignore"):
            models[:, 0] = to_centred(g, c, dt)
        valid[:, 0] = np.isfinite(g).all(1) & (g != 0).any(1) & np.isfinite(models[:, 0]).all(1)
        models[~valid] = 0
    else:
        picks = sample(seed, hyps, S, SAMPLE)
        models, valid = candidates(cc, cam, picks, dt)
    counts = np.where(valid, inliers(models, cc, cam, t).sum(-1), 0)
    key = np.where(counts > 0, (counts.astype(np.int64) << 20) | ((0xFFFF - np.arange(hyps))[:, None] << 4) | (15 - np.arange(ROOTS))[None, :], 0)
    best = int(key.max())
    out = dict(empty, counts=counts, valid=valid, picks=picks, models=models)
    if best == 0:
        return out
    h, r = 0xFFFF - ((best >> 4) & 0xFFFF), 15 - (best & 15)
    model = models[h, r]
    mask = winner_mask = inliers(model, cc, cam, t)
    if refine_on and mask.sum() >= REFINE_MIN:
        again = refine(cc, mask, model, cam)
        if again is not None:
            again = again.astype(np.float32).astype(dt) if dt == np.float32 else again
            mask2 = inliers(again, cc, cam, t)
            if np.isfinite(again).all() and mask2.sum() >= mask.sum():
                model, mask = again, mask2
    # what comes back is the mask of the RETURNED pose, re-centred as a given pose is (float64: nothing is rounded, the same mask)
    world = to_world(model, c, dt)
    mask = inliers(to_centred(world, c, dt), cc, cam, t)
    if mask.sum() == 0:
        return out
    return dict(out, pose=world.astype(np.float64), mask=mask, count=int(mask.sum()), best_hypothesis=h, root=r, winner_mask=winner_mask)


# ---------------------------------------------------------------------- scenes: 640 x 480 frame, world points in a box far from the origin, noise 0.5 on the inliers
T, N0, N1, HYPS, SEED, TILE = TV.T, TV.N0, TV.N1, TV.HYPS, TV.SEED, TV.TILE
FRAME, SIGMA = TV.FRAME, TV.SIGMA
CAM = (500.0, 500.0, 320.0, 240.0)
BOX_CENTRE, BOX_HALF = np.array([100.0, -50.0, 20.0]), np.array([2.0, 1.5, 1.5])


def true_pose(seed=0):
    """(R, t): a camera about 5 units in front of the box, turned a little; X_cam = R X_world + t.  One pose per seed"""
    rng = np.random.default_rng(1000 + seed)
    R = rodrigues(rng.uniform(-0.15, 0.15, 3))
    centre_cam = np.array([0.0, 0.0, 5.0]) + rng.uniform(-0.3, 0.3, 3)                      # where the box centre lies in the camera frame
    return R, centre_cam - R @ BOX_CENTRE


def scene(S, share, seed):
    """S 2-D - 3-D correspondences, round(share * S) of them planted under true_pose(seed) with noise SIGMA on the pixel, the rest a uniform pixel against a
    uniform point of the box.  -> dict(x [S, 2] float32, X [S, 3] float32, planted [S] bool); the order is shuffled."""
    rng = np.random.default_rng(seed)
    R, t = true_pose(seed)
    n_in = int(round(share * S))
    X = (BOX_CENTRE + rng.uniform(-BOX_HALF, BOX_HALF, (8 * n_in + 64, 3))).astype(np.float32)
    p = X.astype(np.float64) @ R.T + t
    x = np.stack([CAM[0] * p[:, 0] / p[:, 2] + CAM[2], CAM[1] * p[:, 1] / p[:, 2] + CAM[3]], 1)
    keep = TV._inside(x) & (p[:, 2] > 0)
    X, x = X[keep][:n_in], x[keep][:n_in] + rng.normal(0, SIGMA, (n_in, 2))
    assert len(X) == n_in
    Xo = (BOX_CENTRE + rng.uniform(-BOX_HALF, BOX_HALF, (S - n_in, 3))).astype(np.float32)
    xo = rng.uniform([0, 0], FRAME, (S - n_in, 2))
    order = rng.permutation(S)
    return dict(x=np.concatenate([x, xo])[order].astype(np.float32), X=np.concatenate([X, Xo])[order], planted=(np.arange(S) < n_in)[order])


def pair_inputs(sc, n1, seed, nan_matched=8):
    """The database side of a scene as a model leaves it: points3d1 [n1, 3] float32 (NaN where a row has no point: a third of
    the unmatched rows, and `nan_matched` rows that matches0 DOES point at, from image-0 rows outside the scene); -> (points, the scene's rows of image 1, the rows without a point to match onto)"""
    rng = np.random.default_rng(seed)
    S = len(sc["x"])
    rows1 = rng.permutation(n1)
    pts = (BOX_CENTRE + rng.uniform(-BOX_HALF, BOX_HALF, (n1, 3))).astype(np.float32)
    pts[rows1[:S]] = sc["X"]
    spare = rows1[S:]
    pts[spare[: len(spare) // 3]] = np.nan
    pts[spare[0], 1:] = 5.0                                # one coordinate alone is enough
    pts[spare[1]] = (np.inf, 1.0, 1.0)
    return pts, rows1[:S], spare[:nan_matched]


# ---------------------------------------------------------------------- the per-pair cases of tests/test_gpu_abspose.py (and of the tolerance derivation)
SIZES = (3, 6, 65, TILE - 1, TILE, TILE + 1, 1000)
SHARE = {3: 1.0, 6: 1.0}       # every correspondence planted: at share 0.5 these sizes have too few all-inlier samples
# the scene of every case: the first seed on which the float64 oracle recovers the planted pose and the 2 % condition holds (tests/test_abspose_cpu.py asserts both)
SCENE_SEED = {}


@functools.lru_cache(maxsize=None)
def case(S, seed=None):
    """One pair of the GPU tests: dict(kpts0 [N0, 2], points [N1, 3], matches0 [N0], rows [S], corr [S, 5], planted [S] in the oracle's order, R, t, cam)"""
    seed = SCENE_SEED.get(S, 0) if seed is None else seed
    sc = scene(S, SHARE.get(S, 0.5), seed)
    rng = np.random.default_rng(seed + 2000)
    perm = rng.permutation(N0)
    rows0, extra0 = np.sort(perm[:S]), perm[S:S + 8]
    kpts0 = rng.uniform([0, 0], FRAME, (N0, 2)).astype(np.float32)
    kpts0[rows0] = sc["x"]
    pts, rows1, nan1 = pair_inputs(sc, N1, seed + 3000)
    matches0 = np.full(N0, -1, np.int64)
    matches0[rows0] = rows1
    matches0[extra0] = nan1                                # matches onto rows without a point: unmatched by the definition
    rows, corr = correspondences(kpts0, pts, matches0)
    assert (rows == rows0).all()
    R, t = true_pose(seed)
    return dict(kpts0=kpts0, points=pts, matches0=matches0, rows=rows, corr=corr, planted=sc["planted"], R=R, t=t, cam=np.asarray(CAM, np.float32))


@functools.lru_cache(maxsize=None)
def case_oracle(S, hyps, refine_on, dtype="float64"):
    """The definition's answer for a case (shared by the tests; treat as read-only)"""
    c = case(S)
    return verify(c["corr"], c["cam"], T, hyps, SEED, refine_on, np.dtype(dtype))


def all_inlier_of(planted, S, hyps):
    """[hyps] bool: the hypotheses of a problem of S correspondences whose whole sample is planted"""
    return planted[sample(SEED, hyps, S, SAMPLE)].all(1) if S >= SAMPLE else np.zeros(hyps, bool)


def all_inlier(S, hyps):
    """[hyps] bool: the hypotheses of a case whose whole sample is planted"""
    c = case(S)
    return all_inlier_of(c["planted"], len(c["corr"]), hyps)


# ---------------------------------------------------------------------- the pooled cases: five queries over nine database images
POOL_CAMS = [CAM, CAM, CAM, CAM, (0.0, 500.0, 320.0, 240.0)]
POOL_SIZES = {0: (100, 100, 100), 1: (65,), 2: (0, 0), 3: (65, 40), 4: (65,)}      # correspondences per pair of query q; q3's second pair gets a bad index
POOL_SEED = {}


@functools.lru_cache(maxsize=None)
def pooled():
    """dict(kpts0 [5, N0, 2], points [9, N1, 3], cams [5, 4], pairs [P, 2] (query, database) in an order that interleaves the queries, matches0 [P, N0],
    bad [P] bool (the pair whose database index is to be set outside the store), problems {q: dict(corr [S, 5] in the problem's order, planted, place [S]
    (the pair's position inside the problem), rows [S], R, t)}).  Query 0: three database images of 100 correspondences each on ascending blocks of image-0
    rows, so the pooled list is in ascending row order too and crosses a tile edge though no pair does; query 1: one image; query 2: two pairs without a
    match; query 3: two pairs, the second with an index outside the store; query 4: a camera without a focal length."""
    kpts0, points, pairs, m0, bad, problems = [], [], [], [], [], {}
    db = 0
    for q, sizes in POOL_SIZES.items():
        S = sum(sizes)
        seed = POOL_SEED.get(q, 0) + 50 + q
        sc = scene(S, 0.5, seed) if S else dict(x=np.zeros((0, 2), np.float32), X=np.zeros((0, 3), np.float32), planted=np.zeros(0, bool))
        rng = np.random.default_rng(seed + 2000)
        rows0 = np.sort(rng.permutation(N0)[:S])
        k0 = rng.uniform([0, 0], FRAME, (N0, 2)).astype(np.float32)
        k0[rows0] = sc["x"]
        kpts0.append(k0)
        at, corr, place, keep = 0, [], [], []
        for j, n in enumerate(sizes):
            part = dict(x=sc["x"][at:at + n], X=sc["X"][at:at + n])
            pts, rows1, _ = pair_inputs(part, N1, seed + 3000 + j)
            row = np.full(N0, -1, np.int64)
            row[rows0[at:at + n]] = rows1
            is_bad = q == 3 and j == 1
            points.append(pts)
            pairs.append((q, db))
            m0.append(row)
            bad.append(is_bad)
            if not is_bad:
                corr.append(correspondences(k0, pts, row)[1])
                place += [j] * n
                keep += list(range(at, at + n))
            db += 1
            at += n
        keep = np.asarray(keep, int)
        R, t = true_pose(seed)
        problems[q] = dict(corr=np.concatenate(corr) if corr else np.zeros((0, 5)), planted=sc["planted"][keep], place=np.asarray(place, int), rows=rows0[keep], R=R, t=t)
    order = [0, 3, 4, 1, 6, 5, 2, 8, 7]                    # the list's order: queries interleaved, a problem's pairs in their own order
    assert sorted(order) == list(range(len(pairs))) and all(order.index(a) < order.index(b) for a, b in ((0, 1), (1, 2), (4, 5), (6, 7)))
    return dict(kpts0=np.stack(kpts0), points=np.stack(points), cams=np.asarray(POOL_CAMS, np.float32), pairs=np.asarray([pairs[i] for i in order]),
                matches0=np.stack([m0[i] for i in order]), bad=np.asarray([bad[i] for i in order]), problems=problems)


@functools.lru_cache(maxsize=None)
def pooled_oracle(q, hyps, refine_on, dtype="float64"):
    pr = pooled()
    return verify(pr["problems"][q]["corr"], pr["cams"][q], T, hyps, SEED, refine_on, np.dtype(dtype))


# ---------------------------------------------------------------------- what the float32 roundings of the definition cost
SEPARATION, MAX_DERIVED = 1e-4, 64


def separation(world, valid):
    """[H, 4]: the distance (largest entry difference of R) of every valid candidate to the nearest OTHER valid candidate of its hypothesis (inf without one)"""
    R = world.reshape(world.shape[:-1] + (3, 4))[..., :3].reshape(world.shape[:-1] + (9,))
    d = abs(R[:, :, None, :] - R[:, None, :, :]).max(-1)
    d = np.where(valid[:, :, None] & valid[:, None, :] & ~np.eye(ROOTS, dtype=bool)[None], d, np.inf)
    return d.min(-1)


def solver_roots_to_compare(r64, allin, min_sep):
    """([(h, r, world pose [12])], their number, the number skipped): the valid candidates of the float64 run over the first MAX_DERIVED hypotheses of `allin`
    whose nearest other candidate is at least min_sep away — what the GPU's solver stage is compared with"""
    if r64["valid"] is None:
        return [], 0, 0
    w64 = to_world(r64["models"], r64["c"])
    sep = separation(w64, r64["valid"])
    out, skipped = [], 0
    for h in np.nonzero(allin)[0][:MAX_DERIVED]:
        for r in np.nonzero(r64["valid"][h])[0]:
            if sep[h, r] < min_sep:
                skipped += 1
            else:
                out.append((int(h), int(r), w64[h, r]))
    return out, len(out), skipped


def pose_difference(a, b):
    """(largest entry difference of R, of t) between poses [..., 12]"""
    d = abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).reshape(np.broadcast(a, b).shape[:-1] + (3, 4))
    return d[..., :3].max((-1, -2)), d[..., 3].max(-1)


def fp32_discrepancy(r32, r64, cam, allin):
    """Over the hypotheses `allin` (the first MAX_DERIVED), every candidate of the float64 run whose nearest other candidate is at least SEPARATION away is
    paired with the nearest candidate of the float32 run (by R): (the largest |d32 - d64| / T over the correspondences with d64 <= 2 T, d32 from the float32
    run's own float32 test terms; the largest entry difference of R and of t in the world frame; the number of candidates paired)"""
    if r64["valid"] is None:
        return 0.0, 0.0, 0.0, 0
    w32, w64 = to_world(r32["models"], r32["c"], np.float32).astype(np.float64), to_world(r64["models"], r64["c"])
    sep = separation(w64, r64["valid"])
    q1 = q2 = q3 = 0.0
    n = 0
    for h in np.nonzero(allin)[0][:MAX_DERIVED]:
        for r in np.nonzero(r64["valid"][h] & (sep[h] >= SEPARATION))[0]:
            dR, dt = pose_difference(w32[h], w64[h, r])
            dR[~r32["valid"][h]] = np.inf
            k = int(np.argmin(dR))
            lhs, rhs, pz = residual_terms(r32["models"][h, k], r32["centred"], cam)
            with np.errstate(all="ignore"):
                d32 = np.where(pz > 0, np.sqrt(lhs.astype(np.float64) / rhs.astype(np.float64)), np.inf)
            d64 = distances(r64["models"][h, r], r64["centred"], cam)
            near = d64 <= 2 * T
            if near.any():
                q1 = max(q1, float(abs(d32[near] - d64[near]).max()) / T)      # inf where the float32 run has the point behind the camera: a failure, not hidden
            q2, q3, n = max(q2, float(dR[k])), max(q3, float(dt[k])), n + 1
    return q1, q2, q3, n


def refine_sensitivity(r32, cam):
    """(dR, dt): the largest change of the refined pose in the world frame (float64, unrounded) when one entry of the float32 starting pose moves by one ulp
    either way, plus half a float32 ulp of the largest entry of R (1) and of t: the rounding of the output.  (0, 0) where nothing is refined"""
    if r32["best_hypothesis"] < 0 or r32["winner_mask"].sum() < REFINE_MIN:
        return 0.0, 0.0
    start = r32["models"][r32["best_hypothesis"], r32["root"]].astype(np.float32)
    base = refine(r32["centred"], r32["winner_mask"], start, cam)
    if base is None:
        return 0.0, 0.0
    w0 = to_world(base, r32["c"])
    dR = dt = 0.0
    for i in range(12):
        for way in (np.float32(np.inf), np.float32(-np.inf)):
            s = start.copy()
            s[i] = np.nextafter(s[i], way)
            again = refine(r32["centred"], r32["winner_mask"], s, cam)
            a, b = pose_difference(to_world(again, r32["c"]), w0)
            dR, dt = max(dR, float(a)), max(dt, float(b))
    return dR + 2.0 ** -24, dt + float(np.spacing(np.float32(abs(w0.reshape(3, 4)[:, 3]).max()))) / 2


def problems():
    """every problem of the GPU tests: (name, corr, cam, planted, oracle(hyps, refine, dtype))"""
    out = [(("pair", S), case(S)["corr"], case(S)["cam"], case(S)["planted"], functools.partial(case_oracle, S)) for S in SIZES]
    pr = pooled()
    return out + [(("pool", q), pr["problems"][q]["corr"], pr["cams"][q], pr["problems"][q]["planted"], functools.partial(pooled_oracle, q)) for q in (0, 1, 3)]
