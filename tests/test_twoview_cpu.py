"""The two-view verifier without a GPU: the float64 definition (tests/twoview_oracle.py) recovers the planted model on every scene, the binding mirrors the
header, lg_twoview_verify refuses what lies outside its envelope before it touches a GPU, the sampling hash gives distinct indices, and the tolerances of
tests/test_gpu_twoview.py are derived here — from the oracle's float32 run against its float64 run on that file's own inputs — and compared with the constants
in its header."""
import ctypes as C
import itertools
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import twoview_oracle as O
import test_gpu_twoview as G
from lightglue_amd import TwoViewVerifier, _cabi

HEADER = (Path(__file__).resolve().parent.parent / "include" / "lightglue_amd.h").read_text()
CASES = [(kind, S) for kind in G.KINDS for S in O.case_sizes(kind)]


@pytest.mark.parametrize("kind,S", CASES)
def test_oracle_recovers_the_planted_model(kind, S):
    """a condition on the scenes, not a measurement: at least 95 % of the planted inliers lie inside t under the model the float64 definition returns"""
    c = O.case(kind, S)
    assert len(c["corr"]) == S and c["planted"].sum() == round(O.SHARE[kind] * S) and len(c["kpts0"]) % 64
    assert (O.distances(kind, c["true"], c["corr"])[c["planted"]] <= O.T).mean() >= 0.99       # the scene is what it says: noise 0.5 against t = 3
    for hyps, refine in itertools.product(O.HYPS, (False, True)):
        r = O.case_oracle(kind, S, hyps, refine)
        assert r["count"] > 0 and r["count"] == r["mask"].sum()       # (4 arbitrary points may map with w of both signs: fewer than 4 inliers)
        d = O.distances(kind, r["model"], c["corr"])
        assert (d[c["planted"]] <= O.T).mean() >= 0.95, (hyps, refine, (d[c["planted"]] <= O.T).mean())
        assert abs(np.linalg.norm(r["model"]) - 1) < 1e-6 and r["model"][np.argmax(abs(r["model"]))] > 0
    assert O.case_oracle(kind, S, 512, True)["count"] >= O.case_oracle(kind, S, 512, False)["count"]


def test_oracle_definitions_on_known_geometry():
    # exact data: the 4-point and 7-point solvers return the planted model (F: among their roots), and the refit returns it too
    for kind in G.KINDS:
        sc = O.scene(kind, 40, 1.0, 3)
        x0 = sc["x0"].astype(np.float64)
        if kind == "homography":
            xh = np.concatenate([x0, np.ones((40, 1))], 1) @ O.H_TRUE.T
            x1 = xh[:, :2] / xh[:, 2:]
        else:
            x1 = sc["x1"].astype(np.float64)
        corr = np.concatenate([x0, x1], 1)
        nrm = O.normalisation(corr)
        models, valid, picks = O.hypotheses(kind, corr, nrm, 0, 256, np.float64)
        assert valid.any(1).mean() > 0.5
        if kind == "homography":
            err = np.array([abs(O.output_form(m[0]) - O.output_form(sc["true"])).max() for m, ok in zip(models, valid) if ok[0]])
            assert err.max() < 1e-6
            assert abs(O.output_form(O.refit(kind, corr, np.ones(40, bool), nrm)) - O.output_form(sc["true"])).max() < 1e-9
        else:       # image-1 points carry noise 0.5: every valid root of a sample explains its own 7 points, to rounding
            for h in np.nonzero(valid.any(1))[0][:50]:
                for r in np.nonzero(valid[h])[0]:
                    assert O.distances(kind, models[h, r], corr[picks[h]]).max() < 1e-6
                    assert abs(np.linalg.det(models[h, r].reshape(3, 3))) < 1e-9
            F = O.refit(kind, corr, np.ones(40, bool), nrm).reshape(3, 3)
            assert np.linalg.svd(F)[1][2] < 1e-12 and np.median(O.distances(kind, F, corr)) < 1.0
    # the sign of a homography matrix carries no meaning: -H has the same inliers
    c = O.case("homography", 65)
    m = O.case_oracle("homography", 65, 256, False)["model"]
    assert (O.inlier_mask("homography", m, c["corr"], O.T) == O.inlier_mask("homography", -m, c["corr"], O.T)).all()
    # the selection rule on given models: most inliers, then the lowest index
    g = O.scoring_models("homography", 65)
    r = O.verify("homography", c["corr"], O.T, 256, given=g)
    assert r["best_hypothesis"] == O.PLANTED_AT and (r["counts"][O.PLANTED_AT] == r["counts"][O.TWIN_AT]).all()
    # unmatched entries
    rows, corr = O.correspondences(np.zeros((5, 2)), np.ones((4, 2)), [0, -1, 4, 3, 2], num0=4, num1=3)
    assert rows.tolist() == [0] and corr.tolist() == [[0, 0, 1, 1]]
    assert O.verify("fundamental", np.zeros((6, 4)), O.T, 256)["count"] == 0 and O.verify("homography", np.ones((30, 4)), O.T, 256)["count"] == 0


@pytest.mark.parametrize("S", (4, 7, 8, 65))
def test_hash_gives_distinct_indices(S):
    for m in (4, 7):
        if S >= m:
            picks = O.sample(12345, 4096, S, m)
            assert picks.min() >= 0 and picks.max() < S
            assert all(len(set(row)) == m for row in picks.tolist())
            assert len(np.unique(picks[:, 0])) == min(S, 4096)           # every index is drawn
            if S == m:
                assert (np.sort(picks, 1) == np.arange(S)).all()
    assert not (O.sample(1, 64, 65, 4) == O.sample(2, 64, 65, 4)).all()
    # the formula, once by hand: mix and hash in plain Python integers
    def mix(x):
        x ^= x >> 16; x = x * 0x85EBCA6B % 2 ** 32; x ^= x >> 13; x = x * 0xC2B2AE35 % 2 ** 32; return x ^ x >> 16
    want = mix((mix((7 + 0x9E3779B9 * (11 + 1)) % 2 ** 32) + 0x85EBCA6B * (2 + 1)) % 2 ** 32)
    assert int(O.hash3(7, np.array([11]), 2)[0]) == want


def typed_fields_of(struct_name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct_name, struct_name), HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        parts = [p.strip() for p in decl.split(",")]
        first = re.fullmatch(r"(.*?)(\w+)", parts[0])
        ctype = first.group(1).replace("const", "").replace("*", "").strip()
        out.append((first.group(2), ctype, "*" in first.group(1)))
        out += [(p.lstrip("* "), ctype, p.startswith("*")) for p in parts[1:]]
    return out


def test_binding_mirrors_the_header():
    scalars = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "float": C.c_float}
    want = [(name, C.c_void_p if pointer else scalars[ctype]) for name, ctype, pointer in typed_fields_of("lg_twoview_io")]
    assert want == list(_cabi.LgTwoViewIO._fields_)
    for name in ("LG_TWOVIEW_HOMOGRAPHY", "LG_TWOVIEW_FUNDAMENTAL", "LG_TWOVIEW_REFINE", "LG_TWOVIEW_GIVEN_MODELS"):
        assert int(re.search(r"#define %s (\d+)u" % name, HEADER).group(1)) == getattr(_cabi, name)
    bits = [_cabi.LG_TWOVIEW_HOMOGRAPHY, _cabi.LG_TWOVIEW_FUNDAMENTAL, _cabi.LG_TWOVIEW_REFINE, _cabi.LG_TWOVIEW_GIVEN_MODELS, _cabi.LG_FLAG_INDEXED, _cabi.LG_FLAG_NN_MUTUAL]
    assert all(b & (b - 1) == 0 for b in bits) and len(set(bits)) == len(bits)
    assert int(re.search(r"#define LG_TWOVIEW_TILE (\d+)", HEADER).group(1)) == _cabi.LG_TWOVIEW_TILE == O.TILE
    lib = _cabi.load()
    assert lib.lg_version().decode() == "lightglue_amd 0.6 (gfx950)"
    assert lib.lg_twoview_verify.argtypes == [C.POINTER(_cabi.LgTwoViewIO), C.c_void_p]
    # the sampling hash is written in the header as a formula: the constants there are the oracle's
    for const in ("0x85EBCA6B", "0xC2B2AE35", "0x9E3779B9"):
        assert const in HEADER


def good_io(**over):
    H = _cabi.LG_TWOVIEW_HOMOGRAPHY
    io = _cabi.LgTwoViewIO(pairs=2, n0=100, n1=90, images0=3, images1=3, flags=H, threshold=3.0, num_hypotheses=256, seed=0, kpts0=256, kpts1=256, matches0=256,
                           workspace=256, workspace_bytes=1 << 40, models=256, inliers0=256, num_inliers=256, status=256)
    for k, v in over.items():
        setattr(io, k, v)
    return io


def test_envelope_is_refused_without_touching_a_gpu():
    """every pointer is a fake non-null value: a refusal that came after anything was dereferenced or launched would have crashed"""
    lib = _cabi.load()
    H, F, R, G_, X = _cabi.LG_TWOVIEW_HOMOGRAPHY, _cabi.LG_TWOVIEW_FUNDAMENTAL, _cabi.LG_TWOVIEW_REFINE, _cabi.LG_TWOVIEW_GIVEN_MODELS, _cabi.LG_FLAG_INDEXED
    inv = _cabi.LG_ERR_INVALID
    assert lib.lg_twoview_verify(None, None) == inv and b"null io" in lib.lg_last_error()
    refused = [
        (dict(flags=H | 1), b"flag"), (dict(flags=H | 1 << 31), b"flag"), (dict(flags=H | _cabi.LG_FLAG_NN_MUTUAL), b"flag"),
        (dict(flags=H | F), b"exactly one"), (dict(flags=R), b"exactly one"), (dict(flags=0), b"exactly one"),
        (dict(n0=-1), b"LG_MAX_KEYPOINTS"), (dict(n0=8193), b"LG_MAX_KEYPOINTS"), (dict(n1=-1), b"LG_MAX_KEYPOINTS"), (dict(n1=8193), b"LG_MAX_KEYPOINTS"),
        (dict(pairs=-1), b"pair count"),
        (dict(num_hypotheses=0), b"num_hypotheses"), (dict(num_hypotheses=255), b"num_hypotheses"), (dict(num_hypotheses=300), b"num_hypotheses"),
        (dict(num_hypotheses=65536 + 256), b"num_hypotheses"),
        (dict(threshold=0.0), b"threshold"), (dict(threshold=-1.0), b"threshold"), (dict(threshold=float("nan")), b"threshold"), (dict(threshold=float("inf")), b"threshold"),
        (dict(workspace_bytes=1000), b"workspace holds"), (dict(workspace=None), b"null workspace"), (dict(workspace=128), b"256-byte aligned"),
        (dict(kpts0=None), b"null pointer"), (dict(kpts1=None), b"null pointer"), (dict(matches0=None), b"null pointer"), (dict(models=None), b"null pointer"),
        (dict(inliers0=None), b"null pointer"), (dict(num_inliers=None), b"null pointer"), (dict(status=None), b"null pointer"),
        (dict(flags=H | G_), b"null pointer"),                               # LG_TWOVIEW_GIVEN_MODELS without models_in
        (dict(flags=H | X), b"LG_FLAG_INDEXED"), (dict(flags=H | X, index0=256, index1=256, images0=0), b"LG_FLAG_INDEXED"),
    ]
    for over, word in refused:
        assert lib.lg_twoview_verify(C.byref(good_io(**over)), None) == inv, over
        assert word in lib.lg_last_error() and b"lg_twoview_verify" in lib.lg_last_error(), (over, lib.lg_last_error())
    assert lib.lg_twoview_verify(C.byref(good_io(pairs=0)), None) == _cabi.LG_OK            # nothing to do, nothing touched
    # the workspace: the correspondence list and its rows per pair, one 32-byte record per pair; -1 outside the envelope
    up = lambda b: (b + 255) // 256 * 256
    for pairs, n0 in ((1, 0), (1, 1), (7, 1100), (120, 2048), (100000, 8192)):
        assert lib.lg_twoview_workspace_bytes(pairs, n0, F) == up(32 * pairs) + up(16 * pairs * n0) + up(4 * pairs * n0)
    assert lib.lg_twoview_workspace_bytes(1, 8193, F) == -1 and lib.lg_twoview_workspace_bytes(1, 10, H | F) == -1 and lib.lg_twoview_workspace_bytes(-1, 10, H) == -1
    # the Python class: configuration errors and the device check
    for bad in (dict(model="essential"), dict(threshold=0), dict(num_hypotheses=100), dict(num_hypotheses=2 ** 17), dict(seed=-1)):
        with pytest.raises(ValueError):
            TwoViewVerifier(**bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        TwoViewVerifier()({"image0": {"keypoints": torch.zeros(1, 8, 2)}, "image1": {"keypoints": torch.zeros(1, 8, 2)}}, torch.full((1, 8), -1))


# ---------------------------------------------------------------------- the tolerances of tests/test_gpu_twoview.py
def test_gpu_tolerances_are_the_derived_ones():
    """Q_RESIDUAL and Q_MODEL of the GPU file's header are the largest fp32-against-fp64 discrepancies of the oracle over that file's inputs (rounded up in the
    third digit); the margins are 8 x these."""
    q = np.array([O.fp32_discrepancy(kind, S) for kind, S in CASES])
    assert (q[:, 0] > 0).sum() >= 8                                     # the figures rest on cases that have all-inlier hypotheses
    q1, q2 = q.max(0)
    print("derived: Q_RESIDUAL %.4e Q_MODEL %.4e" % (q1, q2))
    assert q1 <= G.Q_RESIDUAL <= q1 * 1.01, (q1, G.Q_RESIDUAL)
    assert q2 <= G.Q_MODEL <= q2 * 1.01, (q2, G.Q_MODEL)
    assert G.MARGIN == 8 * G.Q_RESIDUAL and G.MODEL_MARGIN == 8 * G.Q_MODEL and G.MAX_EXCLUDED == 0.02
    doc = G.__doc__
    assert "Q_RESIDUAL %.2e" % G.Q_RESIDUAL in doc and "Q_MODEL    %.2e" % G.Q_MODEL in doc


@pytest.mark.parametrize("kind,S", CASES)
def test_at_most_two_percent_lie_within_the_margin(kind, S):
    """decided by the oracle alone: under its best model, the share of a pair's correspondences whose float64 residual lies within MARGIN t of t"""
    c = O.case(kind, S)
    for hyps, refine in itertools.product(O.HYPS, (False, True)):
        d = O.distances(kind, O.case_oracle(kind, S, hyps, refine)["model"], c["corr"])
        assert (abs(d - O.T) <= G.MARGIN * O.T).mean() <= G.MAX_EXCLUDED, (hyps, refine)
    if S in (65, 1000):                                                 # the scoring-alone test: the planted model, and its lead over every other candidate
        g = O.scoring_models(kind, S)
        d = O.distances(kind, g[O.PLANTED_AT], c["corr"])
        assert (abs(d - O.T) <= G.MARGIN * O.T).mean() <= G.MAX_EXCLUDED
        low = O.verify(kind, c["corr"], O.T * (1 - G.MARGIN), O.GIVEN, given=g)["counts"][:, 0]
        high = O.verify(kind, c["corr"], O.T * (1 + G.MARGIN), O.GIVEN, given=g)["counts"][:, 0]
        assert (g[O.PLANTED_AT] == g[O.TWIN_AT]).all() and low[O.PLANTED_AT] > np.delete(high, [O.PLANTED_AT, O.TWIN_AT]).max()
