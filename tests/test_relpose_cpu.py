"""The relative-pose estimator without a GPU: the float64 definition (tests/relpose_oracle.py) solves, decomposes and recovers the planted model on every scene,
the binding mirrors the header, lg_relpose_estimate refuses what lies outside its envelope before it touches a GPU, and the tolerances of
tests/test_gpu_relpose.py are derived here — from the oracle alone on that file's own inputs — and compared with the constants in its header."""
import ctypes as C
import itertools
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import relpose_oracle as P
import twoview_oracle as TV
import test_gpu_relpose as G
from lightglue_amd import RelativePoseEstimator, TwoViewVerifier, _cabi
from lightglue_amd._readers import as_cameras
from test_twoview_cpu import typed_fields_of

HEADER = (Path(__file__).resolve().parent.parent / "include" / "lightglue_amd.h").read_text()


def exact_scene(n=40, seed=3):
    """noise-free correspondences of the scenes' true motion, float64 pixels"""
    K, R, tr, _ = TV._f_true()
    X = np.random.default_rng(seed).uniform([-3.0, -2.2, 4.0], [3.0, 2.2, 9.0], (n, 3))
    p0, p1 = X @ K.T, (X @ R.T + tr) @ K.T
    return np.concatenate([p0[:, :2] / p0[:, 2:], p1[:, :2] / p1[:, 2:]], 1), R, tr / np.linalg.norm(tr)


# ---------------------------------------------------------------------- solver and decomposition
def test_solver_satisfies_its_equations_and_finds_the_true_matrix():
    worst = 0.0
    for S, variant in ((65, "same"), (P.TV.TILE + 1, "other"), (1000, "same")):
        c = P.case(S, variant)
        allin = np.nonzero(P.all_inlier(S, variant, 512))[0]
        picks = P.sample(P.SEED, 512, S, P.SAMPLE)[allin]
        b = P.bearings(c["corr"], c["cam0"], c["cam1"])
        E, real = P.five_point(b[picks])
        assert real.any(1).all() and real.sum(1).max() <= 10
        for h in range(len(picks)):
            q = b[picks[h]]
            x0, x1 = np.c_[q[:, :2], np.ones(5)], np.c_[q[:, 2:], np.ones(5)]
            scale = (np.linalg.norm(x0, axis=1) * np.linalg.norm(x1, axis=1)).max()
            for r in np.nonzero(real[h])[0]:
                Em = E[h, r].reshape(3, 3)                         # Frobenius norm 1: the bars are relative to it
                worst = max(worst, abs(((x1 @ Em) * x0).sum(1)).max() / scale, abs(np.linalg.det(Em)), abs(2 * Em @ Em.T @ Em - np.trace(Em @ Em.T) * Em).max())
                s = np.linalg.svd(Em)[1]
                assert abs(s[0] - s[1]) < 1e-9 and s[2] < 1e-9
    assert worst < 1e-9, worst
    corr, R, t = exact_scene()
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    true = P.output_form((tx @ R / np.linalg.norm(tx @ R)).reshape(9))
    E, real = P.five_point(P.bearings(corr, P.CAM0, P.CAM0)[P.sample(0, 64, len(corr), 5)])
    for h in range(64):
        assert min(abs(P.output_form(E[h, r]) - true).max() for r in np.nonzero(real[h])[0]) < 1e-9, h


def test_decomposition_returns_the_true_pose_on_exact_data():
    corr, R, t = exact_scene()
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    for sign in (1.0, -1.0):
        for scale in (1.0, 0.37):
            gotR, gott, nif, counts = P.pose(sign * scale * (tx @ R).reshape(9), corr, np.ones(len(corr), bool), P.CAM0, P.CAM0)
            assert abs(gotR - R).max() < 1e-12 and abs(gott - t).max() < 1e-12 and nif == len(corr) and counts[-2] == 0
    four = P.decompositions(tx @ R)
    assert all(abs(Rk @ Rk.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(Rk) - 1) < 1e-12 and abs(np.linalg.norm(tk) - 1) < 1e-12 for Rk, tk in four)
    # the refit on exact data returns the true matrix, on the essential manifold
    F = P.refit(corr, np.ones(len(corr), bool), P.CAM0, P.CAM0, np.float64)
    E = P.essential_of(F, P.CAM0, P.CAM0).reshape(3, 3)
    s = np.linalg.svd(E)[1]
    assert abs(s[0] - s[1]) < 1e-9 and s[2] < 1e-9 and abs(P.output_form(E.reshape(9)) - P.output_form((tx @ R / np.linalg.norm(tx @ R)).reshape(9))).max() < 1e-9
    # cameras that the definition refuses, and too few correspondences
    for cam in ((0.0, 500, 320, 240), (500, -1.0, 320, 240), (np.nan, 500, 320, 240), (np.inf, 500, 320, 240)):
        assert P.verify(corr, cam, P.CAM0, P.T, 256)["count"] == 0 and P.verify(corr, P.CAM0, cam, P.T, 256)["count"] == 0
    assert P.verify(corr[:4], P.CAM0, P.CAM0, P.T, 256)["count"] == 0


@pytest.mark.parametrize("S,variant", P.CASES)
def test_oracle_recovers_the_planted_model(S, variant):
    """a condition on the scenes, not a measurement: at least 95 % of the planted inliers lie inside t under the model the float64 definition returns"""
    c = P.case(S, variant)
    assert len(c["corr"]) == S and c["planted"].sum() == round(P.SHARE.get(S, 0.5) * S) and len(c["kpts0"]) % 64
    assert (P.distances(P.KIND, c["true"], c["corr"])[c["planted"]] <= P.T).mean() >= 0.99       # the scene is what it says: noise 0.5 against t = 3
    assert P.all_inlier(S, variant, min(P.HYPS)).sum() >= 5
    for hyps, refine in itertools.product(P.HYPS, (False, True)):
        r = P.case_oracle(S, variant, hyps, refine)
        assert r["count"] >= P.SAMPLE and r["count"] == r["mask"].sum()
        d = P.distances(P.KIND, r["model"], c["corr"])
        assert (d[c["planted"]] <= P.T).mean() >= 0.95, (hyps, refine, (d[c["planted"]] <= P.T).mean())
        assert abs(np.linalg.norm(r["model"]) - 1) < 1e-6 and r["model"][np.argmax(abs(r["model"]))] > 0
        assert abs(np.linalg.det(r["R"]) - 1) < 1e-9 and 0 < r["num_in_front"] <= r["count"]
    assert P.case_oracle(S, variant, 512, True)["count"] >= P.case_oracle(S, variant, 512, False)["count"]
    seed = P.SCENE_SEED.get((S, variant), 0)
    assert (variant == "other") == (tuple(c["cam0"]) != tuple(c["cam1"])) and seed >= 0


# ---------------------------------------------------------------------- binding, refusals, workspace
def test_binding_mirrors_the_header():
    scalars = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "float": C.c_float}
    want = [(name, C.c_void_p if pointer else scalars[ctype]) for name, ctype, pointer in typed_fields_of("lg_relpose_io")]
    assert want == list(_cabi.LgRelPoseIO._fields_)
    assert int(re.search(r"#define LG_RELPOSE_REFINE (\d+)u", HEADER).group(1)) == _cabi.LG_RELPOSE_REFINE
    assert int(re.search(r"#define LG_RELPOSE_ROOTS (\d+)", HEADER).group(1)) == _cabi.LG_RELPOSE_ROOTS == P.ROOTS
    assert int(re.search(r"#define LG_ERR_CAMERA (\d+)", HEADER).group(1)) == _cabi.LG_ERR_CAMERA
    bits = [_cabi.LG_RELPOSE_REFINE, _cabi.LG_TWOVIEW_HOMOGRAPHY, _cabi.LG_TWOVIEW_FUNDAMENTAL, _cabi.LG_TWOVIEW_REFINE, _cabi.LG_TWOVIEW_GIVEN_MODELS, _cabi.LG_FLAG_INDEXED,
            _cabi.LG_FLAG_NN_MUTUAL]
    assert all(b & (b - 1) == 0 for b in bits) and len(set(bits)) == len(bits)
    codes = [_cabi.LG_OK, _cabi.LG_ERR_INVALID, _cabi.LG_ERR_HIP, _cabi.LG_ERR_STATE, _cabi.LG_ERR_RANGE, _cabi.LG_ERR_DEVICE, _cabi.LG_ERR_INDEX, _cabi.LG_ERR_CAMERA]
    assert len(set(codes)) == len(codes)
    lib = _cabi.load()
    assert lib.lg_relpose_estimate.argtypes == [C.POINTER(_cabi.LgRelPoseIO), C.c_void_p]
    assert "lg_relpose_estimate" in _cabi.EXPORTED_SYMBOLS and "lg_relpose_workspace_bytes" in _cabi.EXPORTED_SYMBOLS
    assert lib.lg_version().decode() == "lightglue_amd 0.6 (gfx950)" and "backward compatible" in HEADER


def good_io(**over):
    io = _cabi.LgRelPoseIO(pairs=2, n0=100, n1=90, images0=3, images1=3, flags=0, threshold=3.0, num_hypotheses=256, seed=0, kpts0=256, kpts1=256, matches0=256,
                           cameras0=256, cameras1=256, workspace=256, workspace_bytes=1 << 40, rotations=256, translations=256, essentials=256, models=256,
                           inliers0=256, num_inliers=256, num_in_front=256, status=256)
    for k, v in over.items():
        setattr(io, k, v)
    return io


def test_envelope_is_refused_without_touching_a_gpu():
    """every pointer is a fake non-null value: a refusal that came after anything was dereferenced or launched would have crashed"""
    lib = _cabi.load()
    R, X = _cabi.LG_RELPOSE_REFINE, _cabi.LG_FLAG_INDEXED
    inv = _cabi.LG_ERR_INVALID
    assert lib.lg_relpose_estimate(None, None) == inv and b"null io" in lib.lg_last_error()
    refused = [
        (dict(flags=1), b"flag"), (dict(flags=R | 1 << 31), b"flag"), (dict(flags=_cabi.LG_FLAG_NN_MUTUAL), b"flag"),
        (dict(flags=_cabi.LG_TWOVIEW_FUNDAMENTAL), b"flag"), (dict(flags=_cabi.LG_TWOVIEW_REFINE), b"flag"), (dict(flags=_cabi.LG_TWOVIEW_GIVEN_MODELS), b"flag"),
        (dict(n0=-1), b"LG_MAX_KEYPOINTS"), (dict(n0=8193), b"LG_MAX_KEYPOINTS"), (dict(n1=-1), b"LG_MAX_KEYPOINTS"), (dict(n1=8193), b"LG_MAX_KEYPOINTS"),
        (dict(pairs=-1), b"pair count"),
        (dict(num_hypotheses=0), b"num_hypotheses"), (dict(num_hypotheses=255), b"num_hypotheses"), (dict(num_hypotheses=300), b"num_hypotheses"),
        (dict(num_hypotheses=65536 + 256), b"num_hypotheses"), (dict(num_hypotheses=-256), b"num_hypotheses"),
        (dict(threshold=0.0), b"threshold"), (dict(threshold=-1.0), b"threshold"), (dict(threshold=float("nan")), b"threshold"), (dict(threshold=float("inf")), b"threshold"),
        (dict(workspace_bytes=1000), b"workspace holds"), (dict(workspace=None), b"null workspace"), (dict(workspace=128), b"256-byte aligned"),
        (dict(kpts0=None), b"null pointer"), (dict(kpts1=None), b"null pointer"), (dict(matches0=None), b"null pointer"), (dict(models=None), b"null pointer"),
        (dict(cameras0=None), b"null pointer"), (dict(cameras1=None), b"null pointer"),
        (dict(rotations=None), b"null pointer"), (dict(translations=None), b"null pointer"), (dict(essentials=None), b"null pointer"),
        (dict(inliers0=None), b"null pointer"), (dict(num_inliers=None), b"null pointer"), (dict(num_in_front=None), b"null pointer"), (dict(status=None), b"null pointer"),
        (dict(flags=X), b"LG_FLAG_INDEXED"), (dict(flags=R | X, index0=256, index1=256, images0=0), b"LG_FLAG_INDEXED"),
    ]
    for over, word in refused:
        assert lib.lg_relpose_estimate(C.byref(good_io(**over)), None) == inv, over
        assert word in lib.lg_last_error() and b"lg_relpose_estimate" in lib.lg_last_error(), (over, lib.lg_last_error())
    assert lib.lg_relpose_estimate(C.byref(good_io(pairs=0)), None) == _cabi.LG_OK            # nothing to do, nothing touched
    assert lib.lg_relpose_estimate(C.byref(good_io(pairs=0, flags=R)), None) == _cabi.LG_OK
    # the workspace: the verifier's three pieces, one 48-byte record per pair and 360 bytes per hypothesis and pair; -1 outside the envelope
    up = lambda b: (b + 255) // 256 * 256
    for pairs, n0, hyps in ((1, 0, 256), (1, 1, 256), (7, 1100, 512), (120, 2048, 4096), (1000, 8192, 65536)):
        want = up(32 * pairs) + up(48 * pairs) + up(16 * pairs * n0) + up(4 * pairs * n0) + up(360 * pairs * hyps)
        assert lib.lg_relpose_workspace_bytes(pairs, n0, hyps, R) == want == lib.lg_relpose_workspace_bytes(pairs, n0, hyps, X)
        assert want - up(48 * pairs) - up(360 * pairs * hyps) == lib.lg_twoview_workspace_bytes(pairs, n0, _cabi.LG_TWOVIEW_FUNDAMENTAL)
    for bad in ((1, 8193, 256, 0), (-1, 10, 256, 0), (1, 10, 100, 0), (1, 10, 256, 4096), (1, 10, 131072, 0)):
        assert lib.lg_relpose_workspace_bytes(*bad) == -1, bad


def test_python_configuration_errors():
    for bad in (dict(threshold=0), dict(threshold=-2.0), dict(num_hypotheses=100), dict(num_hypotheses=2 ** 17), dict(seed=-1), dict(seed=2 ** 32)):
        with pytest.raises(ValueError):
            RelativePoseEstimator(**bad)
    with pytest.raises(ValueError):
        TwoViewVerifier(model="essential")                        # the calibrated case is a class of its own
    est = RelativePoseEstimator()
    assert (est.threshold, est.num_hypotheses, est.refine, est.seed) == (3.0, 1024, True, 0)
    data = {"image0": {"keypoints": torch.zeros(1, 8, 2)}, "image1": {"keypoints": torch.zeros(1, 8, 2)}}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        est(data, torch.full((1, 8), -1), torch.tensor([P.CAM0]), torch.tensor([P.CAM0]))
    # cameras: [K, 4] as it stands, [K, 3, 3] checked
    K = torch.tensor([[[500.0, 0, 320], [0, 510, 240], [0, 0, 1]]])
    assert as_cameras(K, 1, "cpu").tolist() == [[500.0, 510.0, 320.0, 240.0]] and as_cameras([P.CAM0], 1, "cpu").dtype is torch.float32
    for i, j, v in ((0, 1, 0.5), (1, 0, 1e-3), (2, 0, 1.0), (2, 1, -1.0), (2, 2, 2.0)):
        bad = K.clone()
        bad[0, i, j] = v
        with pytest.raises(ValueError, match="zero skew"):
            as_cameras(bad, 1, "cpu")
    for shape in ((2, 4), (1, 3), (1, 4, 4), (4,)):
        with pytest.raises(ValueError, match="must have shape"):
            as_cameras(torch.ones(shape), 1, "cpu")


# ---------------------------------------------------------------------- the tolerances of tests/test_gpu_relpose.py
def test_gpu_tolerances_are_the_derived_ones():
    """Q_RESIDUAL, Q_MODEL, Q_POSE_R and Q_POSE_T of the GPU file's header are the oracle's own figures over that file's inputs (rounded up in the third digit);
    the margins are 8 x these."""
    q = np.array([P.fp32_discrepancy(S, v) for S, v in P.CASES])
    assert (q[:, 0] > 0).all()                                          # every case has all-inlier hypotheses
    q1, q2 = q.max(0)
    s1, s2 = np.array([P.pose_sensitivity(S, v) for S, v in P.CASES]).max(0)
    print("derived: Q_RESIDUAL %.4e Q_MODEL %.4e Q_POSE_R %.4e Q_POSE_T %.4e" % (q1, q2, s1, s2))
    for got, want in ((G.Q_RESIDUAL, q1), (G.Q_MODEL, q2), (G.Q_POSE_R, s1), (G.Q_POSE_T, s2)):
        assert want <= got <= want * 1.01, (want, got)
    assert G.MARGIN == 8 * G.Q_RESIDUAL and G.MODEL_MARGIN == 8 * G.Q_MODEL and G.MAX_EXCLUDED == 0.02
    assert G.POSE_MARGIN_R == 8 * G.Q_POSE_R and G.POSE_MARGIN_T == 8 * G.Q_POSE_T
    assert 10 * G.MODEL_MARGIN >= P.SEPARATION      # the solver test skips every solution the derivation skipped
    doc = G.__doc__
    assert "Q_RESIDUAL %.2e" % G.Q_RESIDUAL in doc and "Q_MODEL    %.2e" % G.Q_MODEL in doc and "Q_POSE_R   %.2e" % G.Q_POSE_R in doc and "Q_POSE_T   %.2e" % G.Q_POSE_T in doc


@pytest.mark.parametrize("S,variant", P.CASES)
def test_at_most_two_percent_lie_within_the_margin(S, variant):
    """decided by the oracle alone: under its best model, the share of a pair's correspondences whose float64 residual lies within MARGIN t of t"""
    c = P.case(S, variant)
    for hyps, refine in itertools.product(P.HYPS, (False, True)):
        d = P.distances(P.KIND, P.case_oracle(S, variant, hyps, refine)["model"], c["corr"])
        assert (abs(d - P.T) <= G.MARGIN * P.T).mean() <= G.MAX_EXCLUDED, (hyps, refine)
