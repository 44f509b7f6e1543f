"""The absolute-pose estimator without a GPU: the float64 definition (tests/abspose_oracle.py) solves P3P, refines and recovers the planted pose on every scene,
the header's Grunert coefficients agree with the oracle's own elimination, the binding mirrors the header, lg_abspose_estimate refuses what lies outside its
envelope before it touches a GPU, and the tolerances of tests/test_gpu_abspose.py are derived here — from the oracle alone on that file's own inputs — and
compared with the constants in its header."""
import ctypes as C
import itertools
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import abspose_oracle as A
import test_gpu_abspose as G
from lightglue_amd import AbsolutePoseEstimator, _cabi
from lightglue_amd.abspose import group_by_query
from test_twoview_cpu import typed_fields_of

HEADER = (Path(__file__).resolve().parent.parent / "include" / "lightglue_amd.h").read_text()
PROBLEMS = A.problems()
NAMES = [p[0] for p in PROBLEMS]


def exact_sample(rng):
    """three noise-free correspondences of true_pose(0): (unit bearings [3, 3], centred world points [3, 3], the centroid, the true (R | t') [12])"""
    R, t = A.true_pose(0)
    X = A.BOX_CENTRE + rng.uniform(-A.BOX_HALF, A.BOX_HALF, (3, 3))
    c = X.mean(0)
    p = X @ R.T + t
    return p / np.linalg.norm(p, axis=1, keepdims=True), X - c, c, np.concatenate([R, (t + R @ c)[:, None]], 1).reshape(12)


# ---------------------------------------------------------------------- solver
def test_solver_satisfies_its_equations_and_finds_the_true_pose():
    rng = np.random.default_rng(5)
    worst_eq = worst_true = 0.0
    seen = np.zeros(5, int)
    for _ in range(300):
        f, P, _, true = exact_sample(rng)
        poses, valid, v = A.p3p(f, P)
        assert valid.any() and (np.diff(v[: int((v != 0).sum())]) > 0).all()            # ascending v over the real roots
        seen[valid.sum()] += 1
        a2, b2, c2, ca, cb, cg = A.triangle(f, P)
        for r in np.nonzero(valid)[0]:
            m = poses[r].reshape(3, 4)
            cam_pts = P @ m[:, :3].T + m[:, 3]
            s = np.linalg.norm(cam_pts, axis=1)
            assert abs(m[:, :3] @ m[:, :3].T - np.eye(3)).max() < 1e-9 and np.linalg.det(m[:, :3]) > 0 and (s > 0).all()
            # the three law-of-cosines equations on the depths, and the three sample points reprojected onto their bearings
            eqs = (s[1] ** 2 + s[2] ** 2 - 2 * s[1] * s[2] * ca - a2, s[0] ** 2 + s[2] ** 2 - 2 * s[0] * s[2] * cb - b2, s[0] ** 2 + s[1] ** 2 - 2 * s[0] * s[1] * cg - c2)
            worst_eq = max(worst_eq, max(abs(e) for e in eqs) / max(a2, b2, c2), abs(cam_pts / s[:, None] - f).max())
            assert abs(s[2] / s[0] - v[r]) < 1e-6 * v[r]
        worst_true = max(worst_true, abs(poses[valid] - true).max(1).min())
    # a root next to a double root keeps half of float64's digits (sqrt(2.2e-16) = 1.5e-8), times the growth through u, s1 and the alignment
    assert worst_eq < 1e-6 and worst_true < 1e-6, (worst_eq, worst_true)
    assert seen[2] > 150 and seen[0] == 0 and seen.sum() == 300, seen               # most triangles have two solutions in front of the camera


def test_grunert_coefficients_agree_with_the_oracles_elimination():
    """the header's closed form against the resultant of the two quadratics in u, up to scale, at random triangles — and both vanish at the true v"""
    rng = np.random.default_rng(6)
    for _ in range(300):
        f, P, _, true = exact_sample(rng)
        g, (q, _, _) = A.grunert(f, P), A.resultant(f, P)
        assert abs(g / g[0] - q / q[0]).max() <= 1e-8 * abs(g / g[0]).max()
        m = true.reshape(3, 4)
        s = np.linalg.norm(P @ m[:, :3].T + m[:, 3], axis=1)
        v = s[2] / s[0]
        assert abs(np.polyval(g, v)) <= 1e-9 * (abs(g) * v ** np.arange(4, -1, -1)).sum()


def test_gauss_newton_converges_to_the_true_pose_on_exact_data():
    rng = np.random.default_rng(7)
    R, t = A.true_pose(0)
    X = (A.BOX_CENTRE + rng.uniform(-A.BOX_HALF, A.BOX_HALF, (40, 3))).astype(np.float32).astype(np.float64)
    p = X @ R.T + t
    corr = np.concatenate([np.stack([A.CAM[0] * p[:, 0] / p[:, 2] + A.CAM[2], A.CAM[1] * p[:, 1] / p[:, 2] + A.CAM[3]], 1), X], 1)
    c, cc = A.centre(corr)
    r = A.verify(corr, A.CAM, A.T, 256, 0, False)
    assert r["count"] == 40
    win = r["models"][r["best_hypothesis"], r["root"]].reshape(3, 4)
    Q = A.rodrigues(2e-3 * rng.standard_normal(3))                   # the winner, pushed off the solution by a twist
    start = np.concatenate([Q @ win[:, :3], (Q @ win[:, 3] + 5e-3 * rng.standard_normal(3))[:, None]], 1).reshape(12)
    assert A.distances(start, cc, A.CAM).max() > 0.5
    got = A.refine(cc, np.ones(40, bool), start, A.CAM)
    world = A.to_world(got, c).reshape(3, 4)
    assert abs(world[:, :3] - R).max() < 1e-9 and abs(world[:, 3] - t).max() < 1e-7
    assert A.distances(got, cc, A.CAM).max() < 1e-7
    # too few or degenerate inliers: abandoned; cameras the definition refuses and too few correspondences: empty
    assert A.refine(cc, np.arange(40) < 2, start, A.CAM) is None
    for cam in ((0.0, 500, 320, 240), (500, -1.0, 320, 240), (np.nan, 500, 320, 240), (500, 500, np.inf, 240)):
        assert A.verify(corr, cam, A.T, 256)["count"] == 0
    assert A.verify(corr[:2], A.CAM, A.T, 256)["count"] == 0 and A.verify(corr[:1], A.CAM, A.T, 256, given=r["pose"][None])["count"] == 1
    # a given pose: the world-frame pose scores what its centred candidate scored
    g = A.verify(corr, A.CAM, A.T, 256, given=np.stack([np.zeros(12), r["pose"], r["pose"]]))
    assert g["best_hypothesis"] == 1 and g["count"] == 40


@pytest.mark.parametrize("name", NAMES)
def test_oracle_recovers_the_planted_pose(name):
    """a condition on the scenes, not a measurement: at least 95 % of the planted correspondences lie inside t under the pose the float64 definition returns"""
    _, corr, cam, planted, oracle = PROBLEMS[NAMES.index(name)]
    assert A.all_inlier_of(planted, len(corr), min(A.HYPS)).sum() >= 5
    for hyps, refine in itertools.product(A.HYPS, (False, True)):
        r = oracle(hyps, refine)
        assert r["count"] >= A.SAMPLE and r["count"] == r["mask"].sum()
        m = r["pose"].reshape(3, 4)
        d = A.distances(r["pose"], corr, cam)                        # a world-frame pose against the list as it is
        assert (d[planted] <= A.T).mean() >= 0.95, (hyps, refine, (d[planted] <= A.T).mean())
        assert abs(m[:, :3] @ m[:, :3].T - np.eye(3)).max() < 1e-9 and np.linalg.det(m[:, :3]) > 0
    assert oracle(512, True)["count"] >= oracle(512, False)["count"]


def test_the_cases_are_what_they_say():
    for S in A.SIZES:
        c = A.case(S)
        assert len(c["corr"]) == S and c["planted"].sum() == round(A.SHARE.get(S, 0.5) * S) and len(c["kpts0"]) % 64
        assert (c["matches0"] >= 0).sum() == S + 8 and not np.isfinite(c["points"][c["matches0"][c["matches0"] >= 0]]).all(1).all()      # matches onto rows without a point
        true = np.concatenate([c["R"], c["t"][:, None]], 1).reshape(12)
        assert (A.distances(true, c["corr"], c["cam"])[c["planted"]] <= A.T).mean() >= 0.99       # noise 0.5 against t = 3
        assert abs(c["corr"][:, 2:].mean(0) - A.BOX_CENTRE).max() < 1.5 and 3 < (c["corr"][:, 2:] @ c["R"].T + c["t"])[:, 2].mean() < 7
    pr = A.pooled()
    sizes = {q: len(p["corr"]) for q, p in pr["problems"].items()}
    assert sizes == {0: 300, 1: 65, 2: 0, 3: 65, 4: 65} and max(A.POOL_SIZES[0]) < A.TILE < sizes[0]
    assert pr["bad"].sum() == 1 and (np.diff(pr["problems"][0]["rows"]) > 0).all()
    assert [int(q) for q in pr["pairs"][:, 0]] != sorted(int(q) for q in pr["pairs"][:, 0])      # the list interleaves the queries
    offsets, order, queries, inverse = group_by_query(pr["pairs"][:, 0])
    assert queries.tolist() == [0, 1, 2, 3, 4] and offsets.tolist() == [0, 3, 4, 6, 8, 9] and sorted(order.tolist()) == list(range(9))
    for g in range(5):
        members = order[offsets[g]:offsets[g + 1]].tolist()
        assert members == sorted(members) and all(pr["pairs"][p, 0] == g and inverse[p] == g for p in members)      # stable: the list's order inside a problem


# ---------------------------------------------------------------------- binding, refusals, workspace
def test_binding_mirrors_the_header():
    scalars = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "float": C.c_float}
    want = [(name, C.c_void_p if pointer else scalars[ctype]) for name, ctype, pointer in typed_fields_of("lg_abspose_io")]
    assert want == list(_cabi.LgAbsposeIO._fields_)
    for name in ("LG_ABSPOSE_REFINE", "LG_ABSPOSE_GROUPED", "LG_ABSPOSE_GIVEN_POSES"):
        assert int(re.search(r"#define %s (\d+)u" % name, HEADER).group(1)) == getattr(_cabi, name)
    assert int(re.search(r"#define LG_ABSPOSE_ROOTS (\d+)", HEADER).group(1)) == _cabi.LG_ABSPOSE_ROOTS == A.ROOTS
    bits = [_cabi.LG_ABSPOSE_REFINE, _cabi.LG_ABSPOSE_GROUPED, _cabi.LG_ABSPOSE_GIVEN_POSES, _cabi.LG_RELPOSE_REFINE, _cabi.LG_TWOVIEW_HOMOGRAPHY, _cabi.LG_TWOVIEW_FUNDAMENTAL,
            _cabi.LG_TWOVIEW_REFINE, _cabi.LG_TWOVIEW_GIVEN_MODELS, _cabi.LG_FLAG_INDEXED, _cabi.LG_FLAG_NN_MUTUAL]
    assert all(b & (b - 1) == 0 for b in bits) and len(set(bits)) == len(bits)
    assert [_cabi.LG_ABSPOSE_REFINE, _cabi.LG_ABSPOSE_GROUPED, _cabi.LG_ABSPOSE_GIVEN_POSES] == [2 * _cabi.LG_RELPOSE_REFINE, 4 * _cabi.LG_RELPOSE_REFINE, 8 * _cabi.LG_RELPOSE_REFINE]
    lib = _cabi.load()
    assert lib.lg_abspose_estimate.argtypes == [C.POINTER(_cabi.LgAbsposeIO), C.c_void_p]
    assert "lg_abspose_estimate" in _cabi.EXPORTED_SYMBOLS and "lg_abspose_workspace_bytes" in _cabi.EXPORTED_SYMBOLS
    assert lib.lg_version().decode() == "lightglue_amd 0.6 (gfx950)" and HEADER.count("backward compatible") >= 2
    assert A.TILE == _cabi.LG_TWOVIEW_TILE


def good_io(**over):
    io = _cabi.LgAbsposeIO(pairs=4, n0=100, n1=90, images0=3, images1=3, groups=2, flags=0, threshold=3.0, num_hypotheses=256, seed=0, kpts0=256, points3d1=256,
                           matches0=256, cameras0=256, workspace=256, workspace_bytes=1 << 40, rotations=256, translations=256, num_inliers=256, inliers0=256,
                           pair_num_inliers=256, status=256)
    for k, v in over.items():
        setattr(io, k, v)
    return io


def test_envelope_is_refused_without_touching_a_gpu():
    """every pointer is a fake non-null value: a refusal that came after anything was dereferenced or launched would have crashed"""
    lib = _cabi.load()
    R, X, Gr, Gi = _cabi.LG_ABSPOSE_REFINE, _cabi.LG_FLAG_INDEXED, _cabi.LG_ABSPOSE_GROUPED, _cabi.LG_ABSPOSE_GIVEN_POSES
    inv = _cabi.LG_ERR_INVALID
    assert lib.lg_abspose_estimate(None, None) == inv and b"null io" in lib.lg_last_error()
    grouped = dict(flags=Gr, group_offsets=256, group_pairs=256)
    refused = [
        (dict(flags=1), b"flag"), (dict(flags=R | 1 << 31), b"flag"), (dict(flags=_cabi.LG_FLAG_NN_MUTUAL), b"flag"), (dict(flags=_cabi.LG_RELPOSE_REFINE), b"flag"),
        (dict(flags=_cabi.LG_TWOVIEW_FUNDAMENTAL), b"flag"), (dict(flags=_cabi.LG_TWOVIEW_REFINE), b"flag"), (dict(flags=_cabi.LG_TWOVIEW_GIVEN_MODELS), b"flag"),
        (dict(flags=8 * Gi), b"flag"),
        (dict(n0=-1), b"LG_MAX_KEYPOINTS"), (dict(n0=8193), b"LG_MAX_KEYPOINTS"), (dict(n1=-1), b"LG_MAX_KEYPOINTS"), (dict(n1=8193), b"LG_MAX_KEYPOINTS"),
        (dict(pairs=-1), b"pair count"),
        (dict(num_hypotheses=0), b"num_hypotheses"), (dict(num_hypotheses=255), b"num_hypotheses"), (dict(num_hypotheses=300), b"num_hypotheses"),
        (dict(num_hypotheses=65536 + 256), b"num_hypotheses"), (dict(num_hypotheses=-256), b"num_hypotheses"),
        (dict(threshold=0.0), b"threshold"), (dict(threshold=-1.0), b"threshold"), (dict(threshold=float("nan")), b"threshold"), (dict(threshold=float("inf")), b"threshold"),
        (dict(workspace_bytes=1000), b"workspace holds"), (dict(workspace=None), b"null workspace"), (dict(workspace=128), b"256-byte aligned"),
        (dict(kpts0=None), b"null pointer"), (dict(points3d1=None), b"null pointer"), (dict(matches0=None), b"null pointer"), (dict(cameras0=None), b"null pointer"),
        (dict(rotations=None), b"null pointer"), (dict(translations=None), b"null pointer"), (dict(num_inliers=None), b"null pointer"),
        (dict(inliers0=None), b"null pointer"), (dict(pair_num_inliers=None), b"null pointer"), (dict(status=None), b"null pointer"),
        (dict(flags=Gi), b"null pointer"),                                                             # poses_in
        (dict(flags=X), b"LG_FLAG_INDEXED"), (dict(flags=R | X, index0=256, index1=256, images0=0), b"LG_FLAG_INDEXED"),
        (dict(flags=Gr), b"null pointer"), (dict(flags=Gr, group_offsets=256), b"null pointer"), (dict(flags=Gr, group_pairs=256), b"null pointer"),
        (dict(grouped, groups=0), b"groups"), (dict(grouped, groups=5), b"groups"), (dict(grouped, groups=-1), b"groups"),
        (dict(grouped, groups=1, pairs=1025, n0=2048), b"LG_MAX_ROWS"), (dict(grouped, groups=1, pairs=257, n0=8192), b"LG_MAX_ROWS"),
    ]
    for over, word in refused:
        assert lib.lg_abspose_estimate(C.byref(good_io(**over)), None) == inv, over
        assert word in lib.lg_last_error() and b"lg_abspose_estimate" in lib.lg_last_error(), (over, lib.lg_last_error())
    assert lib.lg_abspose_estimate(C.byref(good_io(pairs=0)), None) == _cabi.LG_OK            # nothing to do, nothing touched
    assert lib.lg_abspose_estimate(C.byref(good_io(pairs=0, flags=R | Gr, group_offsets=256, group_pairs=256, groups=0)), None) == _cabi.LG_OK
    # the workspace: a 64-byte record per pair and 16 + 8 + 4 bytes per row of matches0; -1 outside the envelope
    up = lambda b: (b + 255) // 256 * 256
    for pairs, n0, hyps in ((1, 0, 256), (1, 1, 256), (7, 1100, 512), (120, 2048, 4096), (1000, 8192, 65536)):
        want = up(64 * pairs) + up(16 * pairs * n0) + up(8 * pairs * n0) + up(4 * pairs * n0)
        assert lib.lg_abspose_workspace_bytes(pairs, n0, hyps, R) == want == lib.lg_abspose_workspace_bytes(pairs, n0, hyps, X | Gi)
    assert lib.lg_abspose_workspace_bytes(1024, 2048, 256, Gr) > 0
    for bad in ((1, 8193, 256, 0), (-1, 10, 256, 0), (1, 10, 100, 0), (1, 10, 256, _cabi.LG_RELPOSE_REFINE), (1, 10, 131072, 0), (1025, 2048, 256, Gr)):
        assert lib.lg_abspose_workspace_bytes(*bad) == -1, bad


def test_python_configuration_errors():
    for bad in (dict(threshold=0), dict(threshold=-2.0), dict(num_hypotheses=100), dict(num_hypotheses=2 ** 17), dict(seed=-1), dict(seed=2 ** 32)):
        with pytest.raises(ValueError):
            AbsolutePoseEstimator(**bad)
    est = AbsolutePoseEstimator()
    assert (est.threshold, est.num_hypotheses, est.refine, est.seed) == (3.0, 1024, True, 0)
    data = {"image0": {"keypoints": torch.zeros(1, 8, 2)}}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        est(data, torch.full((1, 8), -1), torch.tensor([A.CAM]), torch.zeros(1, 8, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        est.estimate_pairs(data["image0"], [(0, 0)], torch.full((1, 8), -1), torch.tensor([A.CAM]), torch.zeros(1, 8, 3))


# ---------------------------------------------------------------------- the tolerances of tests/test_gpu_abspose.py
@pytest.fixture(scope="module")
def derived():
    H = max(A.HYPS)
    rows, compared = [], 0
    for name, corr, cam, planted, oracle in PROBLEMS:
        allin = A.all_inlier_of(planted, len(corr), H)
        q = A.fp32_discrepancy(oracle(H, False, "float32"), oracle(H, False, "float64"), cam, allin)
        s = np.max([A.refine_sensitivity(oracle(hyps, True, "float32"), cam) for hyps in A.HYPS], 0)
        rows.append(list(q[:3]) + list(s))
        assert q[3] >= 5, name                                           # every problem has all-inlier hypotheses whose candidates are compared
        compared += A.solver_roots_to_compare(oracle(H, False, "float64"), allin, 10 * G.POSE_MARGIN_R)[1]
    return np.asarray(rows).max(0), compared


def test_gpu_tolerances_are_the_derived_ones(derived):
    """Q_RESIDUAL, Q_POSE_R, Q_POSE_T, Q_REFINE_R and Q_REFINE_T of the GPU file's header are the oracle's own figures over that file's inputs (rounded up in
    the third digit); the margins are 8 x these; the floor of the solver test is the oracle's own count."""
    q, compared = derived
    print("derived: Q_RESIDUAL %.4e Q_POSE_R %.4e Q_POSE_T %.4e Q_REFINE_R %.4e Q_REFINE_T %.4e, solver roots to compare %d" % (*q, compared))
    for got, want in zip((G.Q_RESIDUAL, G.Q_POSE_R, G.Q_POSE_T, G.Q_REFINE_R, G.Q_REFINE_T), q):
        assert want <= got <= want * 1.01, (want, got)
    assert G.MARGIN == 8 * G.Q_RESIDUAL and G.POSE_MARGIN_R == 8 * G.Q_POSE_R and G.POSE_MARGIN_T == 8 * G.Q_POSE_T and G.MAX_EXCLUDED == 0.02
    assert G.REFINE_MARGIN_R == 8 * G.Q_REFINE_R and G.REFINE_MARGIN_T == 8 * G.Q_REFINE_T
    assert 10 * G.POSE_MARGIN_R >= A.SEPARATION      # the solver test skips every candidate the derivation skipped
    assert G.SOLVER_FLOOR == compared and compared >= 500
    doc = G.__doc__
    for k in ("Q_RESIDUAL", "Q_POSE_R", "Q_POSE_T", "Q_REFINE_R", "Q_REFINE_T"):
        assert "%-10s %.2e" % (k, getattr(G, k)) in doc, k


@pytest.mark.parametrize("name", NAMES)
def test_at_most_two_percent_lie_within_the_margin(name):
    """decided by the oracle alone: under its returned pose, the share of a problem's correspondences whose float64 reprojection error lies within MARGIN t of t"""
    _, corr, cam, _, oracle = PROBLEMS[NAMES.index(name)]
    for hyps, refine in itertools.product(A.HYPS, (False, True)):
        d = A.distances(oracle(hyps, refine)["pose"], corr, cam)
        assert (abs(d - A.T) <= G.MARGIN * A.T).mean() <= G.MAX_EXCLUDED, (hyps, refine)
