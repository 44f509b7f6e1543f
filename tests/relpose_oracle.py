"""Numpy restatement of the relative-pose estimator's definition (include/lightglue_amd.h, lg_relpose_estimate), float64: bearings, the 5-point solver, the
pixel-space candidate, the selection rule, the refit on the essential manifold, the decomposition and the cheirality count.  The SOLVER is a formulation of its
own, not the kernels': an orthonormal null space from the SVD, the ten cubic constraints as a 10 x 20 system in graded order, and the eigenvectors of the
10 x 10 action matrix of multiplication by x (Stewenius, Engels, Nister 2006) through np.linalg.eig; the decomposition goes through np.linalg.svd.  It defines
the SET of real solutions of a sample; root order is the kernels' own and is not compared.  `dtype` float64 is the ideal (nothing rounded); float32 rounds what
the definition rounds — the bearings are formed in float32, the candidate is rounded to float32 and tested in float32 — with the solver still in float64.
Also the scenes and the case table shared by tests/test_relpose_cpu.py and tests/test_gpu_relpose.py.  No GPU, no torch."""
import functools
import itertools

import numpy as np

from twoview_oracle import hash3, sample, correspondences, scene, pair_inputs, distances, inlier_mask, output_form      # noqa: F401  (the shared definition)
import twoview_oracle as TV

KIND = "fundamental"           # the inlier test of every candidate
SAMPLE, REFIT_MIN, ROOTS = 5, 8, 10


# ---------------------------------------------------------------------- cameras and bearings
def K_of(cam):
    fx, fy, cx, cy = (float(v) for v in cam)
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])


def bearings(corr, cam0, cam1, dtype=np.float64):
    """[S, 4] float64 (x0h, y0h, x1h, y1h); dtype float32: formed in float32 as the definition says (one subtraction, one division), then widened"""
    dt = np.dtype(dtype)
    c = np.asarray(corr).astype(dt)
    cam = np.concatenate([np.asarray(cam0, np.float32), np.asarray(cam1, np.float32)]).astype(dt)
    out = np.stack([(c[:, 0] - cam[2]) / cam[0], (c[:, 1] - cam[3]) / cam[1], (c[:, 2] - cam[6]) / cam[4], (c[:, 3] - cam[7]) / cam[5]], 1)
    return out.astype(np.float64)


def pixel_f(E, cam0, cam1):
    """F = K1^-T E K0^-1 on [..., 9]"""
    Ki0, Ki1 = np.linalg.inv(K_of(cam0)), np.linalg.inv(K_of(cam1))
    return (Ki1.T @ E.reshape(E.shape[:-1] + (3, 3)) @ Ki0).reshape(E.shape)


def essential_of(F, cam0, cam1):
    """K1^T F K0 of ONE pixel-space F, Frobenius norm 1, output form, float64"""
    E = K_of(cam1).T @ np.asarray(F, np.float64).reshape(3, 3) @ K_of(cam0)
    return output_form((E / np.linalg.norm(E)).reshape(9))


# ---------------------------------------------------------------------- the 5-point solver (its own formulation)
_EXP = [e for d in range(4) for e in itertools.product(range(4), repeat=3) if sum(e) == d]      # exponents (x, y, z) up to degree 3
_SUP = {d: [e for e in _EXP if sum(e) <= d] for d in (1, 2, 3)}
# graded order: the ten cubics first, then x2 xy xz y2 yz z2 x y z 1
_ORDER = [(3, 0, 0), (2, 1, 0), (2, 0, 1), (1, 2, 0), (1, 1, 1), (1, 0, 2), (0, 3, 0), (0, 2, 1), (0, 1, 2), (0, 0, 3),
          (2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0), (0, 1, 1), (0, 0, 2), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]


def _pmul(a, da, b, db):
    """product of two polynomials held as dicts exponent -> [H] arrays, of degrees da, db"""
    out = {}
    for ea in _SUP[da]:
        for eb in _SUP[db]:
            e = (ea[0] + eb[0], ea[1] + eb[1], ea[2] + eb[2])
            out[e] = out.get(e, 0) + a[ea] * b[eb]
    return out


def _padd(a, b, s=1.0):
    out = dict(a)
    for e, v in b.items():
        out[e] = out.get(e, 0) + s * v
    return out


def five_point(q):
    """q [H, 5, 4] bearing correspondences -> (E [H, 10, 9] float64, each of Frobenius norm 1, real [H, 10] bool): the real solutions of every sample"""
    H = len(q)
    x, y, u, v = q[:, :, 0], q[:, :, 1], q[:, :, 2], q[:, :, 3]
    A = np.stack([u * x, u * y, u, v * x, v * y, v, x, y, np.ones_like(x)], -1)                # [H, 5, 9]
    B = np.linalg.svd(A, full_matrices=True)[2][:, 5:, :]                                     # [H, 4, 9]: an orthonormal null space
    e = [{(1, 0, 0): B[:, 0, k], (0, 1, 0): B[:, 1, k], (0, 0, 1): B[:, 2, k], (0, 0, 0): B[:, 3, k]} for k in range(9)]
    EEt = [[functools.reduce(_padd, [_pmul(e[3 * i + k], 1, e[3 * j + k], 1) for k in range(3)]) for j in range(3)] for i in range(3)]
    tr = _padd(_padd(EEt[0][0], EEt[1][1]), EEt[2][2])
    rows = []
    for i in range(3):
        for j in range(3):                                                                    # (2 E E^T E - tr(E E^T) E)_ij
            p = functools.reduce(_padd, [_pmul(EEt[i][k], 2, e[3 * k + j], 1) for k in range(3)])
            rows.append(_padd({k_: 2 * v_ for k_, v_ in p.items()}, _pmul(tr, 2, e[3 * i + j], 1), -1.0))
    m0 = _padd(_pmul(e[4], 1, e[8], 1), _pmul(e[5], 1, e[7], 1), -1.0)
    m1 = _padd(_pmul(e[3], 1, e[8], 1), _pmul(e[5], 1, e[6], 1), -1.0)
    m2 = _padd(_pmul(e[3], 1, e[7], 1), _pmul(e[4], 1, e[6], 1), -1.0)
    rows.append(_padd(_padd(_pmul(m0, 2, e[0], 1), _pmul(m1, 2, e[1], 1), -1.0), _pmul(m2, 2, e[2], 1)))
    M = np.stack([np.stack([r[m] * np.ones(H) for m in _ORDER], -1) for r in rows], 1)        # [H, 10, 20]
    E = np.zeros((H, ROOTS, 9))
    real = np.zeros((H, ROOTS), bool)
    for h in range(H):
        try:
            R = np.linalg.solve(M[h, :, :10], M[h, :, 10:])
        except np.linalg.LinAlgError:
            continue
        if not np.isfinite(R).all():
            continue
        Ax = np.zeros((10, 10))
        Ax[:6] = -R[:6]                                                                       # x * (x2 xy xz y2 yz z2) are the first six cubics
        Ax[6, 0] = Ax[7, 1] = Ax[8, 2] = Ax[9, 6] = 1.0                                       # x * (x y z 1) = x2 xy xz x
        lam, vec = np.linalg.eig(Ax)
        for r in range(ROOTS):
            if lam[r].imag == 0 and vec[9, r].real != 0:
                w = vec[6:9, r].real / vec[9, r].real
                Es = w[0] * B[h, 0] + w[1] * B[h, 1] + w[2] * B[h, 2] + B[h, 3]
                if np.isfinite(Es).all() and np.linalg.norm(Es) > 0:
                    E[h, r], real[h, r] = Es / np.linalg.norm(Es), True
    return E, real


def candidates(corr, cam0, cam1, picks, dtype=np.float64):
    """(F [H, 10, 9] in dtype: pixel space, unit norm, output form, zero where there is no solution; valid [H, 10]; E [H, 10, 9] float64) of the samples `picks`"""
    dt = np.dtype(dtype)
    E, real = five_point(bearings(corr, cam0, cam1, dt)[picks])
    F = pixel_f(E, cam0, cam1).astype(dt)
    with np.errstate(all="ignore"):
        F, ok = TV.unit(F)
    valid = real & ok
    return np.where(valid[..., None], F, 0).astype(dt), valid, E


# ---------------------------------------------------------------------- refit, decomposition, cheirality
def refit(corr, inl, cam0, cam1, dtype=np.float32):
    """least squares for E over the inliers in Hartley-normalised bearings (normalised over ALL bearings of the pair), projected onto the essential manifold;
    -> the candidate F [9] in dtype"""
    b = bearings(corr, cam0, cam1, dtype)
    nrm = TV.normalisation(b)
    cx0, cy0, s0, cx1, cy1, s1 = (np.float64(v) for v in nrm)
    c = b[inl]
    x, y, u, v = (c[:, 0] - cx0) * s0, (c[:, 1] - cy0) * s0, (c[:, 2] - cx1) * s1, (c[:, 3] - cy1) * s1
    A = np.stack([u * x, u * y, u, v * x, v * y, v, x, y, np.ones_like(x)], 1)
    f = np.linalg.eigh(A.T @ A)[1][:, 0]
    E = TV.denormalise(KIND, f, nrm).reshape(3, 3)
    U, _, Vt = np.linalg.svd(E)
    E = U @ np.diag([1.0, 1.0, 0.0]) @ Vt
    with np.errstate(all="ignore"):
        return TV.unit(pixel_f(E.reshape(9), cam0, cam1).astype(np.dtype(dtype)))[0]


def decompositions(E):
    """the four (R, t) of an essential matrix (any scale, any sign), through the SVD; their order is this function's own"""
    U, _, Vt = np.linalg.svd(np.asarray(E, np.float64).reshape(3, 3))
    U, Vt = U * np.sign(np.linalg.det(U)), Vt * np.sign(np.linalg.det(Vt))
    W = np.array([[0, -1.0, 0], [1.0, 0, 0], [0, 0, 1.0]])
    return [(R, s * U[:, 2]) for R in (U @ W @ Vt, U @ W.T @ Vt) for s in (1.0, -1.0)]


def in_front(R, t, b):
    """[S] bool: both depths of the midpoint triangulation positive, X1 = R X0 + t; b [S, 4] bearings"""
    b0, b1 = np.concatenate([b[:, :2], np.ones((len(b), 1))], 1), np.concatenate([b[:, 2:], np.ones((len(b), 1))], 1)
    a = b0 @ R.T
    aa, ab, bb, at, bt = (a * a).sum(1), (a * b1).sum(1), (b1 * b1).sum(1), a @ t, b1 @ t
    return (ab * bt - bb * at > 0) & (aa * bt - ab * at > 0)


def pose(E, corr, mask, cam0, cam1):
    """(R [3, 3], t [3], num_in_front, counts of the four) of ONE essential matrix over the inliers `mask`; bearings formed in float32 as the definition says"""
    b = bearings(corr, cam0, cam1, np.float32)[mask]
    four = decompositions(E)
    counts = [int(in_front(R, t, b).sum()) for R, t in four]
    k = int(np.argmax(counts))
    return four[k][0], four[k][1], counts[k], sorted(counts)


# ---------------------------------------------------------------------- the whole definition for one pair
def verify(corr, cam0, cam1, t, hyps, seed=0, refine=False, dtype=np.float64):
    """corr [S, 4] -> dict(model [9] (pixel F), mask [S], count, best_hypothesis, root, counts [hyps, 10], valid, picks, models, E [9], R, t, num_in_front)"""
    dt = np.dtype(dtype)
    S = len(corr)
    empty = dict(model=np.zeros(9, dt), mask=np.zeros(S, bool), count=0, best_hypothesis=-1, root=-1, counts=None, valid=None, picks=None, models=None,
                 E=np.zeros(9), R=np.zeros((3, 3)), t=np.zeros(3), num_in_front=0)
    cams = np.concatenate([np.asarray(cam0, np.float64), np.asarray(cam1, np.float64)])
    if S < SAMPLE or not (np.isfinite(cams).all() and (cams[[0, 1, 4, 5]] > 0).all()):
        return empty
    picks = sample(seed, hyps, S, SAMPLE)
    models, valid, _ = candidates(corr, cam0, cam1, picks, dt)
    counts = np.where(valid, TV.count(KIND, models, corr, t)[0], 0)
    key = np.where(counts > 0, (counts.astype(np.int64) << 20) | ((0xFFFF - np.arange(hyps))[:, None] << 4) | (15 - np.arange(ROOTS))[None, :], 0)
    best = int(key.max())
    out = dict(empty, counts=counts, valid=valid, picks=picks, models=models)
    if best == 0:
        return out
    h, r = 0xFFFF - ((best >> 4) & 0xFFFF), 15 - (best & 15)
    model = models[h, r]
    mask = inlier_mask(KIND, model, corr, t)
    if refine and mask.sum() >= REFIT_MIN:
        again = refit(corr, mask, cam0, cam1, np.float32 if dt == np.float32 else np.float64).astype(np.float32).astype(dt)
        if np.isfinite(again).all() and (again != 0).any():
            mask2 = inlier_mask(KIND, again, corr, t)
            if mask2.sum() >= mask.sum():
                model, mask = again, mask2
    if mask.sum() == 0:
        return out
    E = essential_of(model, cam0, cam1)
    R, tr, nif, _ = pose(E, corr, mask, cam0, cam1)
    return dict(out, model=model, mask=mask, count=int(mask.sum()), best_hypothesis=h, root=r, E=E, R=R, t=tr, num_in_front=nif)


# ---------------------------------------------------------------------- the cases of tests/test_gpu_relpose.py (and of the tolerance derivation)
T, N0, N1, HYPS, SEED = TV.T, TV.N0, TV.N1, TV.HYPS, TV.SEED
CAM0 = (500.0, 500.0, 320.0, 240.0)
CAMS1 = {"same": (500.0, 500.0, 320.0, 240.0), "other": (400.0, 400.0, 300.0, 250.0)}
SIZES = (5, 8, 65, TV.TILE - 1, TV.TILE, TV.TILE + 1, 1000)
SHARE = {5: 1.0, 8: 1.0}       # every correspondence planted: at share 0.5 these sizes have no all-inlier sample
VARIANTS = tuple(CAMS1)
CASES = [(S, v) for v in VARIANTS for S in SIZES]
# the scene of every case: the first seed on which the float64 oracle recovers the planted model and the 2 % condition holds (tests/test_relpose_cpu.py asserts both)
SCENE_SEED = {(8, "same"): 1}


def true_pose():
    _, R, tr, _ = TV._f_true()
    return R, tr / np.linalg.norm(tr)


@functools.lru_cache(maxsize=None)
def case(S, variant, seed=None):
    """One pair of the GPU tests: dict(kpts0 [N0, 2], kpts1 [N1, 2], matches0 [N0], rows [S], corr [S, 4], planted [S] in the oracle's order, true [9] (pixel F,
    unit norm), cam0, cam1).  `other`: the image-1 points re-projected through the second camera, so that K0 != K1"""
    seed = SCENE_SEED.get((S, variant), 0) if seed is None else seed
    sc = scene(KIND, S, SHARE.get(S, 0.5), seed)
    cam1 = CAMS1[variant]
    if variant != "same":
        x1 = (sc["x1"].astype(np.float64) - CAM0[2:]) / CAM0[:2] * cam1[:2] + cam1[2:]
        sc = dict(sc, x1=x1.astype(np.float32))
    kpts0, kpts1, matches0, order = pair_inputs(sc, N0, N1, seed + 1000)
    rows, corr = correspondences(kpts0, kpts1, matches0)
    R, tr = true_pose()
    tx = np.array([[0, -tr[2], tr[1]], [tr[2], 0, -tr[0]], [-tr[1], tr[0], 0]])
    true = pixel_f((tx @ R).reshape(9), CAM0, cam1)
    return dict(kpts0=kpts0, kpts1=kpts1, matches0=matches0, rows=rows, corr=corr, planted=sc["planted"][order], true=true / np.linalg.norm(true),
                cam0=np.asarray(CAM0, np.float32), cam1=np.asarray(cam1, np.float32))


@functools.lru_cache(maxsize=None)
def case_oracle(S, variant, hyps, refine, dtype="float64"):
    """The definition's answer for a case (shared by the tests; treat as read-only)"""
    c = case(S, variant)
    return verify(c["corr"], c["cam0"], c["cam1"], T, hyps, SEED, refine, np.dtype(dtype))


def all_inlier(S, variant, hyps):
    """[hyps] bool: the hypotheses of a case whose whole sample is planted"""
    c = case(S, variant)
    return c["planted"][sample(SEED, hyps, len(c["corr"]), SAMPLE)].all(1)


@functools.lru_cache(maxsize=None)
def pose_sensitivity(S, variant):
    """(dR, dt): the largest change of the oracle's R and t over a case's results when one entry of the float32 E moves by one float32 ulp either way"""
    c = case(S, variant)
    dR = dt = 0.0
    for hyps, refine in itertools.product(HYPS, (False, True)):
        r = case_oracle(S, variant, hyps, refine)
        E32 = r["E"].astype(np.float32)
        R0, t0, _, _ = pose(E32, c["corr"], r["mask"], c["cam0"], c["cam1"])
        for i in range(9):
            for way in (np.float32(np.inf), np.float32(-np.inf)):
                Ep = E32.copy()
                Ep[i] = np.nextafter(Ep[i], way)
                R1, t1, _, _ = pose(Ep, c["corr"], r["mask"], c["cam0"], c["cam1"])
                dR, dt = max(dR, float(abs(R1 - R0).max())), max(dt, float(abs(t1 - t0).max()))
    return dR, dt


SEPARATION, MAX_DERIVED = 5e-3, 64


def separation(models, valid):
    """[H, 10]: the distance (largest entry difference) of every valid solution to the nearest OTHER valid solution of its hypothesis (inf without one)"""
    d = abs(models[:, :, None, :] - models[:, None, :, :]).max(-1)
    d = np.where(valid[:, :, None] & valid[:, None, :] & ~np.eye(ROOTS, dtype=bool)[None], d, np.inf)
    return d.min(-1)


@functools.lru_cache(maxsize=None)
def fp32_discrepancy(S, variant, hyps=max(HYPS)):
    """What the float32 roundings of the definition cost on a case, over the hypotheses whose sample is all planted inliers (the first MAX_DERIVED of them):
    every solution of the float64 run whose nearest other solution is at least SEPARATION away — a pair of roots closer than that may merge and vanish under
    a rounding — is paired with the nearest solution of the float32 run: (the largest |d32 - d64| / T over the correspondences with d64 <= 2 T, d32 from the
    float32 run's own float32 test terms; the largest entry difference of the two models).  (0, 0) without such a hypothesis."""
    c = case(S, variant)
    r32, r64 = case_oracle(S, variant, hyps, False, "float32"), case_oracle(S, variant, hyps, False, "float64")
    if r64["valid"] is None:
        return 0.0, 0.0
    q1 = q2 = 0.0
    sep = separation(r64["models"], r64["valid"])
    for h in np.nonzero(all_inlier(S, variant, hyps))[0][:MAX_DERIVED]:
        for r in np.nonzero(r64["valid"][h] & (sep[h] >= SEPARATION))[0]:
            m64 = r64["models"][h, r]
            diff = abs(r32["models"][h].astype(np.float64) - m64).max(-1)
            diff[~r32["valid"][h]] = np.inf
            m32 = r32["models"][h, int(np.argmin(diff))]
            lhs, rhs, _ = TV.residual_terms(KIND, m32, c["corr"])
            with np.errstate(all="ignore"):
                d32 = np.sqrt(lhs.astype(np.float64) / rhs.astype(np.float64))
            d64 = distances(KIND, m64, c["corr"])
            near = d64 <= 2 * T
            if near.any():
                q1 = max(q1, float(np.nanmax(abs(d32 - d64)[near])) / T)
            q2 = max(q2, float(diff.min()))
    return q1, q2
