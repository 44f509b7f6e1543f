"""Numpy restatement of the two-view verifier's definition (include/lightglue_amd.h, lg_twoview_verify): the sampling hash, both minimal solvers, both residual
tests, the selection rule and the refit, vectorised over the hypotheses of one pair.  `dtype` chooses the arithmetic of the solvers and the tests: float64 is
the definition, float32 what fp32 arithmetic can deliver (the same operations in the same order as the kernels; fmaf is emulated through float64).  Also the
scene builders and the case table shared by tests/test_twoview_cpu.py and tests/test_gpu_twoview.py.  No GPU, no torch."""
import functools

import numpy as np

EPS_H, EPS_F, EPS_CUBIC, EPS_ROOT = 1e-3, 1e-4, 1e-8, 1e-2
SAMPLE = {"homography": 4, "fundamental": 7}
REFIT_MIN = {"homography": 4, "fundamental": 8}
M32 = np.uint64(0xFFFFFFFF)


# ---------------------------------------------------------------------- sampling
def mix(x):
    x = np.asarray(x, np.uint64) & M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x85EBCA6B)) & M32
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xC2B2AE35)) & M32
    x ^= x >> np.uint64(16)
    return x


def hash3(seed, hyp, slot):
    """hash(seed, hypothesis, slot) = mix(mix(seed + 0x9E3779B9 * (hypothesis + 1)) + 0x85EBCA6B * (slot + 1)), uint32 arithmetic"""
    hyp = np.asarray(hyp, np.uint64)
    inner = mix((np.uint64(seed) + np.uint64(0x9E3779B9) * (hyp + np.uint64(1))) & M32)
    return mix((inner + np.uint64(0x85EBCA6B) * np.uint64(slot + 1)) & M32)


def sample(seed, hyps, S, m):
    """[hyps, m] distinct indices below S: slot s draws hash mod (S - s) and skips past the earlier picks in ascending order"""
    picks = np.zeros((hyps, m), np.int64)
    for s in range(m):
        d = (hash3(seed, np.arange(hyps), s) % np.uint64(S - s)).astype(np.int64)
        srt = np.sort(picks[:, :s], axis=1)
        for e in range(s):
            d += d >= srt[:, e]
        picks[:, s] = d
    return picks


# ---------------------------------------------------------------------- correspondences and their normalisation
def correspondences(kpts0, kpts1, matches0, num0=None, num1=None):
    """(rows [S], corr [S, 4] float64 holding the float32 keypoints): row i counts unless matches0[i] < 0, i >= num0, matches0[i] >= n1 or >= num1"""
    kpts0, kpts1, matches0 = np.asarray(kpts0, np.float32), np.asarray(kpts1, np.float32), np.asarray(matches0, np.int64)
    live0 = len(kpts0) if num0 is None else min(max(int(num0), 0), len(kpts0))
    live1 = len(kpts1) if num1 is None else min(max(int(num1), 0), len(kpts1))
    i = np.arange(len(matches0))
    take = (i < live0) & (matches0 >= 0) & (matches0 < live1)
    rows = i[take]
    return rows, np.concatenate([kpts0[rows], kpts1[matches0[rows]]], 1).astype(np.float64).reshape(-1, 4)


def normalisation(corr):
    """(cx0, cy0, s0, cx1, cy1, s1) as float32 values: centroid and sqrt(2) / mean distance of either side (scale 1 where that distance is 0), sums in float64"""
    out = []
    for side in (corr[:, :2], corr[:, 2:]):
        c = side.mean(0) if len(side) else np.zeros(2)
        d = np.sqrt(((side - c) ** 2).sum(1)).mean() if len(side) else 0.0
        out += [c[0], c[1], np.sqrt(2.0) / d if d > 0 else 1.0]
    return np.asarray(out, np.float32)


# ---------------------------------------------------------------------- solvers (q: [hyps, m, 4] normalised, dtype arithmetic)
def _basis(x, y):
    c, lam = [], []
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        ci = (y[:, j] - y[:, k], x[:, k] - x[:, j], x[:, j] * y[:, k] - y[:, j] * x[:, k])
        c.append(ci)
        lam.append((ci[0] * x[:, 3] + ci[1] * y[:, 3]) + ci[2])
    det = (c[0][0] * x[:, 0] + c[0][1] * y[:, 0]) + c[0][2]
    ok = np.minimum(np.minimum(abs(lam[0]), abs(lam[1])), np.minimum(abs(lam[2]), abs(det))) > EPS_H
    return c, lam, ok


def solve_h(q):
    cs, ls, ok0 = _basis(q[:, :, 0], q[:, :, 1])
    cd, ld, ok1 = _basis(q[:, :, 2], q[:, :, 3])
    h = np.zeros((q.shape[0], 9), q.dtype)
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        w = ld[i] * (ls[j] * ls[k])
        b = (w * q[:, i, 2], w * q[:, i, 3], w)
        for r in range(3):
            for col in range(3):
                h[:, 3 * r + col] = h[:, 3 * r + col] + b[r] * cs[i][col]
    return h, ok0 & ok1


def _det3(r0, r1, r2):
    return (r0[:, 0] * (r1[:, 1] * r2[:, 2] - r1[:, 2] * r2[:, 1]) - r0[:, 1] * (r1[:, 0] * r2[:, 2] - r1[:, 2] * r2[:, 0])) + r0[:, 2] * (r1[:, 0] * r2[:, 1] - r1[:, 1] * r2[:, 0])


def solve_f(q):
    """(n1, n2 [hyps, 9], z [hyps, 3], roots [hyps], well [hyps, 3]): the null space N1 + z N2 of the 7 x 9 system, the real roots of det = 0 (roots = 0 for an
    invalid sample) and which of them are well conditioned: |p'(z)| > EPS_ROOT (|3 z^2| + |2 A z| + |B|) on the monic cubic p"""
    dt = q.dtype
    x, y, u, v = q[:, :, 0], q[:, :, 1], q[:, :, 2], q[:, :, 3]
    a = np.stack([u * x, u * y, u, v * x, v * y, v, x, y, np.ones_like(x)], -1)      # [hyps, 7, 9]
    ok = np.ones(len(q), bool)
    for k in range(7):
        for i in range(k + 1, 7):
            sw = abs(a[:, i, k]) > abs(a[:, k, k])
            rk, ri = a[:, k].copy(), a[:, i].copy()
            a[:, k] = np.where(sw[:, None], ri, rk)
            a[:, i] = np.where(sw[:, None], rk, ri)
        ok &= abs(a[:, k, k]) > EPS_F
        a[:, k, k:] = a[:, k, k:] / a[:, k, k:k + 1].copy()
        for i in range(7):
            if i != k:
                f = a[:, i, k:k + 1].copy()
                a[:, i, k:] = a[:, i, k:] - f * a[:, k, k:]
    n1, n2 = np.zeros((len(q), 9), dt), np.zeros((len(q), 9), dt)
    n1[:, :7], n2[:, :7] = -a[:, :, 7], -a[:, :, 8]
    n1[:, 7] = 1
    n2[:, 8] = 1
    A1, A2, A3, B1, B2, B3 = n1[:, 0:3], n1[:, 3:6], n1[:, 6:9], n2[:, 0:3], n2[:, 3:6], n2[:, 6:9]
    c0, c3 = _det3(A1, A2, A3), _det3(B1, B2, B3)
    c1 = (_det3(B1, A2, A3) + _det3(A1, B2, A3)) + _det3(A1, A2, B3)
    c2 = (_det3(A1, B2, B3) + _det3(B1, A2, B3)) + _det3(B1, B2, A3)
    ok &= abs(c3) > EPS_CUBIC
    A, B, C = c2 / c3, c1 / c3, c0 / c3
    Q = (A * A - 3 * B) / 9
    R = ((2 * A * A * A - 9 * A * B) + 27 * C) / 54
    Q3, R2 = Q * Q * Q, R * R
    three = R2 < Q3
    th = np.arccos(np.minimum(np.maximum(R / np.sqrt(Q3), -1), 1))
    sq = -2 * np.sqrt(Q)
    z3 = np.stack([sq * np.cos((th + dt.type(6.2831853071795865) * dt.type(k)) / 3) - A / 3 for k in range(3)], -1)
    e = -np.copysign(np.cbrt(abs(R) + np.sqrt(R2 - Q3)), R)
    g = np.where(e != 0, Q / np.where(e != 0, e, 1), 0).astype(dt)
    z1 = np.stack([(e + g) - A / 3, np.zeros_like(e), np.zeros_like(e)], -1)
    z = np.where(three[:, None], z3, z1).astype(dt)
    for _ in range(2):
        p = ((z + A[:, None]) * z + B[:, None]) * z + C[:, None]
        dp = (3 * z + 2 * A[:, None]) * z + B[:, None]
        z = np.where(abs(dp) > 1e-20, z - p / np.where(dp != 0, dp, 1), z).astype(dt)
    dp = (3 * z + 2 * A[:, None]) * z + B[:, None]
    well = abs(dp) > EPS_ROOT * ((abs((3 * z) * z) + abs((2 * A[:, None]) * z)) + abs(B[:, None]))      # a (nearly) double root is lost to rounding
    return n1, n2, z, np.where(ok, np.where(three, 3, 1), 0), well


def denormalise(kind, m, nrm):
    """H = T1^-1 Hn T0, F = T1^T Fn T0 on [..., 9] models, in m's dtype, the kernels' operation order"""
    cx0, cy0, s0, cx1, cy1, s1 = (m.dtype.type(v) for v in nrm)
    m = m.copy()
    for r in range(3):
        a, b = m[..., 3 * r] * s0, m[..., 3 * r + 1] * s0
        m[..., 3 * r + 2] = (m[..., 3 * r + 2] - a * cx0) - b * cy0
        m[..., 3 * r], m[..., 3 * r + 1] = a, b
    for c in range(3):
        if kind == "homography":
            m[..., c] = m[..., c] / s1 + cx1 * m[..., 6 + c]
            m[..., 3 + c] = m[..., 3 + c] / s1 + cy1 * m[..., 6 + c]
        else:
            a, b = m[..., c] * s1, m[..., 3 + c] * s1
            m[..., 6 + c] = (m[..., 6 + c] - a * cx1) - b * cy1
            m[..., c], m[..., 3 + c] = a, b
    return m


def output_form(m):
    """the entry of largest magnitude (the first one among equals) positive; m [..., 9].  Every model is scored in this form, so that "+H" means one matrix"""
    big = np.take_along_axis(m, np.argmax(abs(m), -1)[..., None], -1)
    return np.where(big < 0, -m, m)


def unit(m):
    """(m / |m|_F in output form, valid): invalid (and all zero) where the norm is 0 or anything is non-finite"""
    sq = np.zeros(m.shape[:-1], m.dtype)
    for i in range(9):
        sq = sq + m[..., i] * m[..., i]
    nrm = np.sqrt(sq)
    out = m / np.where(nrm != 0, nrm, 1)[..., None]
    ok = (nrm > 0) & np.isfinite(nrm) & np.isfinite(out).all(-1)
    return output_form(np.where(ok[..., None], out, 0).astype(m.dtype)), ok


def hypotheses(kind, corr, nrm, seed, hyps, dtype):
    """(models [hyps, 3, 9] denormalised and of unit norm, valid [hyps, 3], picks [hyps, m]) of one pair"""
    dt = np.dtype(dtype)
    S, m = len(corr), SAMPLE[kind]
    picks = sample(seed, hyps, S, m)
    c = corr.astype(dt)[picks]                                       # [hyps, m, 4]
    cx0, cy0, s0, cx1, cy1, s1 = (dt.type(v) for v in nrm)
    q = np.stack([(c[..., 0] - cx0) * s0, (c[..., 1] - cy0) * s0, (c[..., 2] - cx1) * s1, (c[..., 3] - cy1) * s1], -1)
    with np.errstate(all="ignore"):
        if kind == "homography":
            h, ok = solve_h(q)
            mod, fin = unit(denormalise(kind, h, nrm))
            models = np.zeros((hyps, 3, 9), dt)
            models[:, 0] = mod
            valid = np.zeros((hyps, 3), bool)
            valid[:, 0] = ok & fin
        else:
            n1, n2, z, roots, well = solve_f(q)
            raw = n1[:, None, :] + z[:, :, None] * n2[:, None, :]
            models, fin = unit(denormalise(kind, raw, nrm))
            valid = fin & well & (np.arange(3)[None, :] < roots[:, None])
    return models, valid, picks


# ---------------------------------------------------------------------- the inlier test
def _fma(a, b, c):
    if a.dtype == np.float32:
        return (a.astype(np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)
    return a * b + c


def residual_terms(kind, m, corr):
    """(lhs, rhs, w) [..., S] in m's dtype, division-free: the test is lhs <= t^2 rhs; w is the homography's third coordinate (ones for F); m [..., 9]"""
    dt = m.dtype
    p = corr.astype(dt)
    x, y, u, v = p[:, 0], p[:, 1], p[:, 2], p[:, 3]
    e = [m[..., i, None] for i in range(9)]
    with np.errstate(all="ignore"):
        l0, l1, l2 = _fma(e[0], x, _fma(e[1], y, e[2])), _fma(e[3], x, _fma(e[4], y, e[5])), _fma(e[6], x, _fma(e[7], y, e[8]))
        if kind == "homography":
            dx, dy = _fma(u, l2, -l0), _fma(v, l2, -l1)
            return _fma(dx, dx, dy * dy), l2 * l2, l2
        r = _fma(u, l0, _fma(v, l1, l2))
        g0, g1 = _fma(e[0], u, _fma(e[3], v, e[6])), _fma(e[1], u, _fma(e[4], v, e[7]))
        return r * r, _fma(l0, l0, _fma(l1, l1, _fma(g0, g0, g1 * g1))), np.ones_like(r)


def classify(kind, m, corr, t):
    """[..., S] int: 0 outside, +1 inside (H: with w > 0), -1 inside with w < 0 (H only); m [..., 9], in m's dtype"""
    lhs, rhs, w = residual_terms(kind, m, corr)
    t2 = m.dtype.type(t) * m.dtype.type(t)
    with np.errstate(all="ignore"):
        return np.where(lhs <= t2 * rhs, np.sign(w), 0).astype(np.int64)


def count(kind, m, corr, t):
    """(count [...], sign [...]) of models m [..., 9] in output form: H under the sign with more inliers, + on a tie"""
    inside = classify(kind, m, corr, t)
    pos, neg = (inside > 0).sum(-1), (inside < 0).sum(-1)
    return np.maximum(pos, neg), np.where(pos >= neg, 1, -1)


def inlier_mask(kind, m, corr, t):
    """[S] bool: the inliers of ONE model (any sign: it is put in output form) in its own dtype"""
    inside = classify(kind, output_form(m), corr, t)
    pos, neg = (inside > 0).sum(), (inside < 0).sum()
    return inside == (1 if pos >= neg else -1)


def distances(kind, m, corr):
    """[S] float64: reprojection error (H) / Sampson distance (F) under one model, the quantity the threshold is compared with"""
    m = np.asarray(m, np.float64).reshape(3, 3)
    x0 = np.concatenate([corr[:, :2], np.ones((len(corr), 1))], 1)
    x1 = np.concatenate([corr[:, 2:], np.ones((len(corr), 1))], 1)
    l = x0 @ m.T
    with np.errstate(all="ignore"):
        if kind == "homography":
            return np.sqrt(((x1[:, :2] - l[:, :2] / l[:, 2:]) ** 2).sum(1))
        g = x1 @ m
        return abs((x1 * l).sum(1)) / np.sqrt(l[:, 0] ** 2 + l[:, 1] ** 2 + g[:, 0] ** 2 + g[:, 1] ** 2)


# ---------------------------------------------------------------------- refit and output form
def refit(kind, corr, inl, nrm):
    """least squares over the inliers in the pair's normalised coordinates, float64: smallest eigenvector of the 9 x 9 normal matrix; F forced to rank 2"""
    cx0, cy0, s0, cx1, cy1, s1 = (np.float64(v) for v in nrm)
    c = corr[inl]
    x, y, u, v = (c[:, 0] - cx0) * s0, (c[:, 1] - cy0) * s0, (c[:, 2] - cx1) * s1, (c[:, 3] - cy1) * s1
    o, z = np.ones_like(x), np.zeros_like(x)
    if kind == "homography":
        A = np.concatenate([np.stack([-x, -y, -o, z, z, z, u * x, u * y, u], 1), np.stack([z, z, z, -x, -y, -o, v * x, v * y, v], 1)])
    else:
        A = np.stack([u * x, u * y, u, v * x, v * y, v, x, y, o], 1)
    f = np.linalg.eigh(A.T @ A)[1][:, 0]
    if kind == "fundamental":
        F = f.reshape(3, 3)
        v3 = np.linalg.eigh(F.T @ F)[1][:, 0]
        f = (F - np.outer(F @ v3, v3)).reshape(9)
    return unit(denormalise(kind, f, nrm))[0]


# ---------------------------------------------------------------------- the whole definition for one pair
def verify(kind, corr, t, hyps, seed=0, refine=False, dtype=np.float64, given=None):
    """corr [S, 4] -> dict(model [9], mask [S], count, best_hypothesis, root, counts [hyps, 3], valid, picks, models)"""
    dt = np.dtype(dtype)
    S = len(corr)
    empty = dict(model=np.zeros(9, dt), mask=np.zeros(S, bool), count=0, best_hypothesis=-1, root=-1, counts=None, valid=None, picks=None, models=None)
    if S < (1 if given is not None else SAMPLE[kind]):
        return empty
    nrm = normalisation(corr)
    if given is not None:
        g = np.asarray(given, np.float32).reshape(-1, 9).astype(dt)
        models, valid, picks = np.zeros((len(g), 3, 9), dt), np.zeros((len(g), 3), bool), None
        models[:, 0], valid[:, 0] = output_form(g), np.isfinite(g).all(1) & (g != 0).any(1)
        hyps = len(g)
    else:
        models, valid, picks = hypotheses(kind, corr, nrm, seed, hyps, dt)
    counts = np.where(valid, count(kind, models, corr, t)[0], 0)
    key = np.where(counts > 0, (counts << 18) | ((0xFFFF - np.arange(hyps))[:, None] << 2) | (3 - np.arange(3))[None, :], 0)
    best = int(key.max())
    out = dict(empty, counts=counts, valid=valid, picks=picks, models=models)
    if best == 0:
        return out
    h, r = 0xFFFF - ((best >> 2) & 0xFFFF), 3 - (best & 3)
    model = models[h, r]
    mask = inlier_mask(kind, model, corr, t)
    if refine and mask.sum() >= REFIT_MIN[kind]:
        again = refit(kind, corr, mask, nrm).astype(np.float32).astype(dt)
        if np.isfinite(again).all() and (again != 0).any():
            mask2 = inlier_mask(kind, again, corr, t)
            if mask2.sum() >= mask.sum():
                model, mask = again, mask2
    if mask.sum() == 0:
        return out
    return dict(out, model=model, mask=mask, count=int(mask.sum()), best_hypothesis=h, root=r)


# ---------------------------------------------------------------------- scenes: 640 x 480 frame, Gaussian noise 0.5 on the inliers, uniform outliers
FRAME, SIGMA, T = (640.0, 480.0), 0.5, 3.0
H_TRUE = np.array([[0.92, -0.11, 38.0], [0.13, 0.95, -21.0], [1.1e-4, -6e-5, 1.0]])


def _f_true():
    K = np.array([[500.0, 0, 320.0], [0, 500.0, 240.0], [0, 0, 1.0]])
    a, b = 0.12, -0.06
    Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    R, tr = Ry @ Rx, np.array([-0.6, 0.08, 0.15])
    tx = np.array([[0, -tr[2], tr[1]], [tr[2], 0, -tr[0]], [-tr[1], tr[0], 0]])
    Ki = np.linalg.inv(K)
    return K, R, tr, Ki.T @ tx @ R @ Ki


def _inside(p):
    return (p[:, 0] >= 0) & (p[:, 0] <= FRAME[0]) & (p[:, 1] >= 0) & (p[:, 1] <= FRAME[1])


def scene(kind, S, share, seed):
    """S correspondences, round(share * S) of them planted under a known model (a plane under H_TRUE / a 3-D point cloud under two known cameras) with noise
    SIGMA on the image-1 point, the rest uniform outliers.  -> dict(x0 [S, 2] float32, x1 [S, 2] float32, planted [S] bool, true [9]); the order is shuffled."""
    rng = np.random.default_rng(seed)
    n_in = int(round(share * S))
    if kind == "homography":
        x0 = rng.uniform([0, 0], FRAME, (8 * n_in + 64, 2))
        xh = np.concatenate([x0, np.ones((len(x0), 1))], 1) @ H_TRUE.T
        x1, true = xh[:, :2] / xh[:, 2:], H_TRUE
    else:
        K, R, tr, true = _f_true()
        X = rng.uniform([-3.0, -2.2, 4.0], [3.0, 2.2, 9.0], (8 * n_in + 64, 3))
        p0, p1 = X @ K.T, (X @ R.T + tr) @ K.T
        x0, x1 = p0[:, :2] / p0[:, 2:], p1[:, :2] / p1[:, 2:]
    keep = _inside(x0) & _inside(x1)
    x0, x1 = x0[keep][:n_in], x1[keep][:n_in] + rng.normal(0, SIGMA, (n_in, 2))
    assert len(x0) == n_in
    o0, o1 = rng.uniform([0, 0], FRAME, (S - n_in, 2)), rng.uniform([0, 0], FRAME, (S - n_in, 2))
    order = rng.permutation(S)
    planted = (np.arange(S) < n_in)[order]
    return dict(x0=np.concatenate([x0, o0])[order].astype(np.float32), x1=np.concatenate([x1, o1])[order].astype(np.float32), planted=planted,
                true=(true / np.linalg.norm(true)).reshape(9))


def pair_inputs(sc, n0, n1, seed):
    """The scene as a matcher leaves it: kpts0 [n0, 2], kpts1 [n1, 2] float32 and matches0 [n0] int64 (-1 on the n0 - S unmatched rows, which hold uniform
    keypoints).  Correspondence k of the oracle is the k-th matched row in ascending order; `order` [S] maps it back to the scene's index."""
    rng = np.random.default_rng(seed)
    S = len(sc["x0"])
    assert n0 >= S and n1 >= S
    rows0, rows1 = np.sort(rng.permutation(n0)[:S]), rng.permutation(n1)[:S]
    kpts0 = rng.uniform([0, 0], FRAME, (n0, 2)).astype(np.float32)
    kpts1 = rng.uniform([0, 0], FRAME, (n1, 2)).astype(np.float32)
    order = rng.permutation(S)
    kpts0[rows0], kpts1[rows1] = sc["x0"][order], sc["x1"][order]
    matches0 = np.full(n0, -1, np.int64)
    matches0[rows0] = rows1
    return kpts0, kpts1, matches0, order


# ---------------------------------------------------------------------- the cases of tests/test_gpu_twoview.py (and of the tolerance derivation)
TILE = 256                     # LG_TWOVIEW_TILE (tests/test_twoview_cpu.py checks it against the binding)
SHARE = {"homography": 0.3, "fundamental": 0.5}
N0, N1 = 1100, 1050            # n0 is not a multiple of 64
HYPS = (256, 512)
SEED = 0


# the scene of every case: the first seed on which the float64 oracle recovers the planted model (tests/test_twoview_cpu.py asserts that it does)
SCENE_SEED = {("homography", 255): 4, ("fundamental", 8): 1, ("fundamental", 65): 1, ("fundamental", 255): 1, ("fundamental", 256): 1, ("fundamental", 257): 2, ("fundamental", 1000): 2}


def case_sizes(kind):
    return (SAMPLE[kind], 8, 65, TILE - 1, TILE, TILE + 1, 1000)


@functools.lru_cache(maxsize=None)
def case(kind, S):
    """One pair of the GPU tests: dict(kpts0 [N0, 2], kpts1 [N1, 2], matches0 [N0], rows [S], corr [S, 4], planted [S] in the oracle's order, true [9])"""
    seed = SCENE_SEED.get((kind, S), 0)
    sc = scene(kind, S, SHARE[kind], seed)
    kpts0, kpts1, matches0, order = pair_inputs(sc, N0, N1, seed + 1000)
    rows, corr = correspondences(kpts0, kpts1, matches0)
    return dict(kpts0=kpts0, kpts1=kpts1, matches0=matches0, rows=rows, corr=corr, planted=sc["planted"][order], true=sc["true"])


@functools.lru_cache(maxsize=None)
def case_oracle(kind, S, hyps, refine, dtype="float64"):
    """The definition's answer for a case (shared by the tests; treat as read-only)"""
    return verify(kind, case(kind, S)["corr"], T, hyps, SEED, refine, np.dtype(dtype))


def all_inlier(kind, S, hyps):
    """[hyps] bool: the hypotheses of a case whose whole sample is planted"""
    c = case(kind, S)
    return c["planted"][sample(SEED, hyps, len(c["corr"]), SAMPLE[kind])].all(1)


@functools.lru_cache(maxsize=None)
def fp32_discrepancy(kind, S, hyps=max(HYPS)):
    """What fp32 arithmetic costs on a case, over the hypotheses whose sample is all planted inliers and the roots valid in both runs: (the largest
    |d32 - d64| / T, d32 = sqrt(lhs / rhs) of the float32 run's own test terms, d64 the float64 run's distance, over the correspondences with d64 <= 2 T: the
    ones a discrepancy could move across the threshold; the largest entry difference between the two runs' models in output form).  (0, 0) without such a hypothesis."""
    c = case(kind, S)
    r32, r64 = case_oracle(kind, S, hyps, False, "float32"), case_oracle(kind, S, hyps, False, "float64")
    if r64["valid"] is None:
        return 0.0, 0.0
    q1 = q2 = 0.0
    for h in np.nonzero(all_inlier(kind, S, hyps))[0]:
        for r in range(3):
            if r32["valid"][h, r] and r64["valid"][h, r]:
                m32, m64 = r32["models"][h, r], r64["models"][h, r]
                lhs, rhs, _ = residual_terms(kind, m32, c["corr"])
                with np.errstate(all="ignore"):
                    d32 = np.sqrt(lhs.astype(np.float64) / rhs.astype(np.float64))
                d64 = distances(kind, m64, c["corr"])
                near = d64 <= 2 * T
                if near.any():
                    q1 = max(q1, float(np.nanmax(abs(d32 - d64)[near])) / T)
                q2 = max(q2, float(abs(output_form(m32).astype(np.float64) - output_form(m64)).max()))
    return q1, q2


# ---------------------------------------------------------------------- the candidate models of the scoring-alone test (LG_TWOVIEW_GIVEN_MODELS)
PLANTED_AT, TWIN_AT, GIVEN = 5, 9, 256


@functools.lru_cache(maxsize=None)
def scoring_models(kind, S):
    """[GIVEN, 9] float32 candidates for a case: random models, the planted model at PLANTED_AT and an identical copy at TWIN_AT (the lower index must win),
    and perturbed copies of it in between (the planted model with its third column, F: third row too, scaled by 1 + 0.1 k: a shift that grows with k)"""
    rng = np.random.default_rng(100 + S)
    m = rng.standard_normal((GIVEN, 9))
    true = case(kind, S)["true"]
    for k, at in enumerate(range(16, 48), 1):
        p = true.reshape(3, 3).copy()
        p[:2, 2] *= 1 + 0.1 * k
        if kind == "fundamental":
            p[2, :2] *= 1 + 0.1 * k
        m[at] = p.reshape(9)
    m[PLANTED_AT] = m[TWIN_AT] = true
    return (m / np.linalg.norm(m, axis=1, keepdims=True)).astype(np.float32)
