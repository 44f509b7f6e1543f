"""The nearest-neighbour matcher's definition (include/lightglue_amd.h, lg_nn_match) restated in numpy float64: the yardstick of tests/test_nn_matcher_cpu.py and
tests/test_gpu_nn_matcher.py.  Besides the outputs it returns, per row, the MARGIN of every decision the row's result rests on, so that a test can tell a wrong
answer from a decision the float64 definition itself takes within fp32 round-off of a boundary:
    s1 - s2                 the arg-max (rows with exact duplicates among the columns excepted: there the tie rule, lowest index, decides in any precision —
                            `duplicates_ok` — provided the duplicate columns give bit-identical similarities, which they do: same operands, same order)
    |d1 - ratio^2 d2|       the ratio test
    |d1 - distance^2|       the distance test
and, with the mutual check, the same three of the partner's column, whose arg-max decides whether the match is kept."""
import numpy as np


def rootsift(x, eps=1e-6):
    """ref sift.py:53-56 on float64 rows"""
    x = np.asarray(x, np.float64)
    r = x / np.maximum(np.abs(x).sum(-1, keepdims=True), eps)
    r = np.sqrt(np.maximum(r, eps))
    return r / np.maximum(np.linalg.norm(r, axis=-1, keepdims=True), eps)


def normalised(desc, transform=None):
    """rows as they enter the similarity: widened, RootSIFT where the store asks for it, x / max(|x|_2, 1e-12)"""
    x = np.asarray(desc).astype(np.float64)
    if transform == "rootsift":
        x = rootsift(x)
    return x / np.maximum(np.linalg.norm(x, axis=-1, keepdims=True), 1e-12)


def similarity(desc0, desc1, transform0=None, transform1=None):
    return normalised(desc0, transform0) @ normalised(desc1, transform1).T


def _direction(sim, ratio, distance, duplicates_ok):
    """rows of `sim` against its columns -> raw [n] (-1: rejected), s1 [n], margin [n]"""
    n, m = sim.shape
    if m == 0:
        return np.full(n, -1, np.int64), np.zeros(n), np.full(n, np.inf)
    order = np.argsort(-sim, axis=1, kind="stable")          # equal values: the lowest index first
    rows = np.arange(n)
    j1 = order[:, 0]
    s1 = sim[rows, j1]
    s2 = sim[rows, order[:, 1]] if m >= 2 else np.full(n, -np.inf)
    d1, d2 = np.maximum(2.0 * (1.0 - s1), 0.0), np.maximum(2.0 * (1.0 - s2), 0.0)
    keep = np.ones(n, bool)
    margin = s1 - s2
    if duplicates_ok:
        margin = np.where(s1 == s2, np.inf, margin)
    if ratio is not None and m >= 2:
        keep &= d1 <= ratio * ratio * d2
        margin = np.minimum(margin, np.abs(d1 - ratio * ratio * d2))
    if distance is not None:
        keep &= d1 <= distance * distance
        margin = np.minimum(margin, np.abs(d1 - distance * distance))
    return np.where(keep, j1, -1).astype(np.int64), s1, margin


def match(sim, mutual=True, ratio=None, distance=None, duplicates_ok=False):
    """One pair from its float64 similarity matrix [n0, n1] -> the matcher's outputs for it (no batch dimension) + margin0 [n0], margin1 [n1]."""
    sim = np.asarray(sim, np.float64)
    n0, n1 = sim.shape
    raw0, s0, g0 = _direction(sim, ratio, distance, duplicates_ok)
    raw1, s1, g1 = _direction(sim.T, ratio, distance, duplicates_ok)

    def side(raw, other, s, g, g_other):
        m, margin = raw.copy(), g.copy()
        has = raw >= 0
        if mutual and has.any():
            idx = np.where(has)[0]
            back = other[raw[idx]] == idx
            m[idx[~back]] = -1
            margin[idx] = np.minimum(margin[idx], g_other[raw[idx]])
        return m, np.where(m > -1, (s + 1.0) / 2.0, 0.0), margin
    m0, sc0, margin0 = side(raw0, raw1, s0, g0, g1)
    m1, sc1, margin1 = side(raw1, raw0, s1, g1, g0)
    idx = np.where(m0 > -1)[0]
    return {"matches0": m0, "matches1": m1, "matching_scores0": sc0, "matching_scores1": sc1,
            "matches": np.stack([idx, m0[idx]], -1).reshape(-1, 2), "scores": sc0[idx], "raw0": raw0, "raw1": raw1,
            "margin0": margin0, "margin1": margin1}


def match_store(desc0, pairs, desc1=None, num0=None, num1=None, transform0=None, transform1=None, **kw):
    """A pair list over stores [K, N, D] -> one `match` dict per pair, padded to [N] with -1 / 0 (margins +inf) as the matcher returns them."""
    desc1 = desc0 if desc1 is None else desc1
    num1 = num0 if (num1 is None and desc1 is desc0) else num1
    out = []
    for i, j in pairs:
        n0 = desc0.shape[1] if num0 is None else int(num0[i])
        n1 = desc1.shape[1] if num1 is None else int(num1[j])
        r = match(similarity(desc0[i, :n0], desc1[j, :n1], transform0, transform1), **kw)
        for side, n, N in ((0, n0, desc0.shape[1]), (1, n1, desc1.shape[1])):
            for key, fill in ((f"matches{side}", -1), (f"matching_scores{side}", 0.0), (f"margin{side}", np.inf), (f"raw{side}", -1)):
                r[key] = np.concatenate([r[key], np.full(N - n, fill, r[key].dtype)])
        out.append(r)
    return out
