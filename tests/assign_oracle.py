"""The matcher's assignment head (lg_gemm.hip sim_kernel / lg_sim.hip, the 256 -> 1 heads of lg_tail.hip / lg_pointwise.hip, lg_assign.hip) restated in numpy,
stage by stage: the yardstick of tests/test_assign_oracle_cpu.py and tests/test_gpu_assign_stages.py.  Every function takes ONE stage's input arrays of one
pair and returns that stage's outputs, so that a GPU test can feed each stage the device's own input and see that stage's error alone.  float64 throughout,
except `scores_f32`: the score expression has no multiplication and the build has no fast-math, so the device's float32 result is defined bit for bit.
`ref :A-B` = lightglue/lightglue.py lines A..B of the reference, as in oracle/lightglue_oracle.py."""
import numpy as np


def sim(md0, md1):
    """ref :292: the projected descriptors' inner products, [n0, 256] x [n1, 256] -> [n0, n1]"""
    return np.asarray(md0, np.float64) @ np.asarray(md1, np.float64).T


def sim_scale(md0, md1):
    """sum_k |a_k| |b_k| per entry of `sim`: the unit in which a dot product's rounding error is bounded"""
    return np.abs(np.asarray(md0, np.float64)) @ np.abs(np.asarray(md1, np.float64)).T


def _sigmoid(z):
    e = np.exp(-np.abs(z))                       # never overflows
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def _logsigmoid(z):
    return np.minimum(z, 0.0) - np.log1p(np.exp(-np.abs(z)))


def heads(x, w, b):
    """A 256 -> 1 head (ref :89-94 token confidence, :293-299 matchability) on rows x [n, 256]: z = x . w + b, sigmoid(z), logsigmoid(z), logsigmoid(-z)"""
    z = np.asarray(x, np.float64) @ np.asarray(w, np.float64).reshape(-1) + float(np.asarray(b, np.float64).reshape(-1)[0])
    return z, _sigmoid(z), _logsigmoid(z), _logsigmoid(-z)


def _lse(s, axis):
    s = np.asarray(s, np.float64)
    m = s.max(axis=axis, keepdims=True)
    e = np.sort(np.exp(s - m), axis=axis)        # sorted: rows with the same entries in any order sum to the same bits
    return np.squeeze(m, axis) + np.log(e.sum(axis=axis))


def lse_rows(s):
    """log sum_b exp(sim[a, b]) (the normaliser of ref :270 log_softmax(sim, 2)) -> [n0]"""
    return _lse(s, 1)


def lse_cols(s):
    """log sum_a exp(sim[a, b]) (ref :271) -> [n1]"""
    return _lse(s, 0)


def scores_f32(s, lse_r, lse_c, ls0, ls1):
    """lg_assign.hip score_of in numpy float32, in ITS order: ((sim - lr) + (sim - lc)) + (l0 + l1)  (ref :270-274)"""
    f = np.float32
    s, lr, lc = np.asarray(s, f), np.asarray(lse_r, f)[:, None], np.asarray(lse_c, f)[None, :]
    cert = np.asarray(ls0, f)[:, None] + np.asarray(ls1, f)[None, :]
    out = ((s - lr) + (s - lc)) + cert
    assert out.dtype == np.float32
    return out


def argmax_first(scores):
    """ref :304-306 (torch.max: first index among equals) -> max0 [n0], arg0 [n0], max1 [n1], arg1 [n1]"""
    scores = np.asarray(scores)
    return scores.max(1), scores.argmax(1), scores.max(0), scores.argmax(0)


def finalize(max0, arg0, arg1, ind0, ind1, n0, n1, threshold):
    """ref :302-318 behind the argmax + :593-614: mutual check, exp, threshold, un-pruning through the index sets.  max0 / arg0 [len0], arg1 [len1] in live
    (pruned) index space; ind0 [len0], ind1 [len1] map it to the original one of n0 / n1 rows.  The threshold is compared as the matcher compares it: on
    float32 scores.  Returns a dict: matches0 [n0], matches1 [n1] (-1: no match / not live), scores0 [n0], scores1 [n1] (float64 exp of the float32 maximum;
    0: not mutual / not live), matches [k, 2] sorted by image-0 row, match_scores [k], n_matches."""
    arg0, arg1, ind0, ind1 = (np.asarray(v, np.int64) for v in (arg0, arg1, ind0, ind1))
    len0, len1 = len(arg0), len(arg1)
    out = {"matches0": np.full(n0, -1, np.int64), "matches1": np.full(n1, -1, np.int64), "scores0": np.zeros(n0), "scores1": np.zeros(n1)}
    if len0 == 0 or len1 == 0:
        return {**out, "matches": np.zeros((0, 2), np.int64), "match_scores": np.zeros(0), "n_matches": 0}
    mutual0 = np.arange(len0) == arg1[arg0]                                      # ref :308
    mutual1 = np.arange(len1) == arg0[arg1]                                      # ref :309
    ms0 = np.where(mutual0, np.exp(np.asarray(max0, np.float32).astype(np.float64)), 0.0)   # ref :310-312
    ms1 = np.where(mutual1, ms0[arg1], 0.0)                                      # ref :313
    valid0 = mutual0 & (ms0.astype(np.float32) > np.float32(threshold))          # ref :314
    valid1 = mutual1 & valid0[arg1]                                              # ref :315
    out["matches0"][ind0] = np.where(valid0, ind1[arg0], -1)                     # ref :316, :608
    out["matches1"][ind1] = np.where(valid1, ind0[arg1], -1)                     # ref :317, :609
    out["scores0"][ind0], out["scores1"][ind1] = ms0, ms1                        # ref :612-613
    rows = np.where(valid0)[0]                                                   # ref :595-602: ascending live row = ascending original row (ind is sorted)
    return {**out, "matches": np.stack([ind0[rows], ind1[arg0[rows]]], -1).reshape(-1, 2), "match_scores": ms0[rows], "n_matches": len(rows)}
