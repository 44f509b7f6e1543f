"""The global positioner without a GPU: the float64 definition (tests/positioning_oracle.py) against planted scenes, the host API's refusals and the C ABI's
envelope.  What is asserted and where each bar comes from is said at the test; every measured figure is printed before it is asserted."""
import ctypes

import numpy as np
import pytest
import torch

import positioning_oracle as P
import posegraph_oracle as G
import triangulate_oracle as O
import lightglue_amd
from lightglue_amd import GlobalPositioner, _cabi, positioning

# the exact scene: the oracle's worst centre and point error against the truth, both about 100 units from the origin.  Measured 4.7e-13 and 2.6e-13 (the
# centres stop moving at a step below 1e-12 and the points follow them); asserted one order above, as tests/test_posegraph_cpu.py does with its 3e-11
EXACT_BAR = 5e-12
NOISE_LEVELS, NOISE_SEEDS = (0.5, 1.0, 2.0), 5


def chain_tracks():
    sc = G.chain_scene()
    tr = O.triangulate(dict(kpts=sc["kpts"], num=None, pairs=sc["pairs"], matches0=sc["matches0"], cams=sc["cams"], poses=sc["poses"]), tracks_only=True)
    return sc, tr["track_id"], tr["num_tracks"]


def noisy_relative(sc, pairs, noise, seed):
    """exact relative poses of the chain scene with `scene()`'s noise model: every R_ab and t_ab turned by 0.2 .. 1 x `noise` degrees about a random axis"""
    rng = np.random.default_rng(100 * seed + int(10 * noise))
    Rab, t = G.relative(*G.in_gauge(sc["poses"], 0, 1), pairs)
    for p in range(len(Rab)):
        Rab[p] = G.random_rotation(rng, rng.uniform(0.2, 1.0) * noise) @ Rab[p]
        t[p] = G.random_rotation(rng, rng.uniform(0.2, 1.0) * noise) @ t[p]
    return Rab.astype(np.float32), t.astype(np.float32)


def positioned(sc, tid, T, est):
    held = np.zeros(len(sc["poses"]), bool)
    held[[est["origin"], est["baseline"]]] = True
    return P.solve(dict(kpts=sc["kpts"], num=None, track_id=tid, T=T, cams=sc["cams"], poses=est["poses64"].astype(np.float32), held=held))


# ---------------------------------------------------------------------- 1. the definition on planted scenes
def test_exact_scene_returns_the_truth_to_rounding():
    """exact pixels, orthonormal float64 rotations, float64 inputs as they are (`wide`): the oracle returns the held-gauge truth to rounding"""
    sc = P.scene(8, 32, 60, seed=1, exact=True)
    poses = sc["poses"].astype(np.float64)
    U, _, Vt = np.linalg.svd(poses[:, :, :3])
    poses[:, :, :3] = U @ Vt
    centres = -np.einsum("kji,kj->ki", poses[:, :, :3], poses[:, :, 3])
    X, cams, kpts = sc["planted"]["X"], sc["cams"].astype(np.float64), sc["kpts"].astype(np.float64)
    for j, at in enumerate(sc["planted"]["rows"]):
        for k, r in at.items():
            p = poses[k, :, :3] @ X[j] + poses[k, :, 3]
            kpts[k, r] = (cams[k, 0] * p[0] / p[2] + cams[k, 2], cams[k, 1] * p[1] / p[2] + cams[k, 3])
    out = P.solve(dict(P.oracle_input(sc), kpts=kpts, poses=poses, cams=cams, wide=True))
    dc, dx = abs(out["centres64"] - centres).max(), abs(out["xyz64"] - X).max()
    print("exact scene: centres %.3g, points %.3g off the truth after %d iterations, largest angle %.3g degrees" % (dc, dx, out["iterations"], np.nanmax(out["angle_error64"])))
    assert out["positions_ok"] and out["num_posed"] == 8 and out["num_points"] == 60 and out["num_outliers"] == 0
    assert (out["image_state"] == [P.HELD] + [P.POSED] * 6 + [P.HELD]).all() and (out["node_state"][sc["track_id"] >= 0] == P.INLIER).all()
    assert dc < EXACT_BAR and dx < EXACT_BAR, (dc, dx)


def test_positions_from_tracks_beat_direction_averaging():
    """posegraph_oracle.chain_scene() (K = 6, 110 tracks, 499 observations), relative poses with 0.5, 1 and 2 degrees of `scene()`-style noise, rotations and the
    two held centres from posegraph_oracle.estimate.  With four free centres a single draw of the pair noise decides little (three of the fifteen draws below
    go the other way for the centres and one is a tie), so the centre error is compared as the mean over NOISE_SEEDS draws per level; the median reprojection error is lower
    in every single draw.  Orderings only.  Measured (centre error / extent after similarity alignment, averaging -> positioned, mean of five; median
    reprojection error in pixels, mean of five; the worst single max):
      0.5 degrees   0.0023 -> 0.0018     1.06 -> 0.51     max 3.8 -> 1.9
      1.0 degrees   0.0044 -> 0.0035     2.34 -> 0.67     max 6.4 -> 3.1
      2.0 degrees   0.0129 -> 0.0053     4.78 -> 0.83     max 16.4 -> 8.1
    Zero noise is not asserted: averaging is exact there and the tracks carry the planted 0.5 px (positioning gives 0.0010 of the extent)."""
    sc, tid, T = chain_tracks()
    K, cams = len(sc["poses"]), sc["cams"].astype(np.float64)
    for noise in NOISE_LEVELS:
        rows = []
        for seed in range(NOISE_SEEDS):
            R, t = noisy_relative(sc, sc["pairs"], noise, seed)
            est = G.estimate(sc["pairs"], R, t, K)
            assert est["num_posed"] == K
            out = positioned(sc, tid, T, est)
            assert out["positions_ok"] and out["num_posed"] == K and out["iterations"] <= 12
            _, cg = G.in_gauge(sc["poses"], est["origin"], est["baseline"])
            before = P.reprojection(sc["kpts"], tid, cams, est["poses64"], P.triangulated(sc["kpts"], tid, T, sc["cams"], est["poses64"].astype(np.float32)))
            after = P.reprojection(sc["kpts"], out["track_id"], cams, out["poses64"], out["xyz64"])
            rows.append((P.centre_error(est["centres64"], cg), P.centre_error(out["centres64"], cg), np.median(before), np.median(after), before.max(), after.max()))
            assert rows[-1][3] < rows[-1][2], (noise, seed, rows[-1])
        m = np.mean(rows, 0)
        print("noise %.1f: centre error %.4f -> %.4f, median reprojection %.2f -> %.2f px (means of %d draws), worst max %.1f -> %.1f; per draw %s" % (
            noise, m[0], m[1], m[2], m[3], NOISE_SEEDS, max(r[4] for r in rows), max(r[5] for r in rows), ["%.4f -> %.4f" % r[:2] for r in rows]))
        assert m[1] < m[0], (noise, rows)


def test_an_image_on_one_pair_gets_its_centre_from_its_tracks():
    """image 5 of the chain scene joined to the view graph by ONE pair: averaging gives it a rotation and no position; the positioner places it from its tracks.
    The bar is the ordering's: the worst centre error of all six images after similarity alignment, image 5 among them, is no larger than what averaging leaves
    on the FULL graph, where it can place every image, at the same noise and draw (0.5 degrees).  Measured: 0.0025 of the extent against 0.0042"""
    sc, tid, T = chain_tracks()
    K = len(sc["poses"])
    pairs = np.asarray([p for p in sc["pairs"].tolist() if 5 not in p or p == [4, 5]])
    R, t = noisy_relative(sc, pairs, 0.5, 0)
    est = G.estimate(pairs, R, t, K)
    assert est["image_state"][5] == G.ROTATION_ONLY and est["num_posed"] == K - 1 and np.isnan(est["poses64"][5, :, 3]).all()
    out = positioned(sc, tid, T, est)
    assert out["image_state"][5] == P.POSED and out["num_posed"] == K and out["positions_ok"]
    _, cg = G.in_gauge(sc["poses"], est["origin"], est["baseline"])
    full = G.estimate(sc["pairs"], *noisy_relative(sc, sc["pairs"], 0.5, 0), K)
    bar = P.centre_error(full["centres64"], G.in_gauge(sc["poses"], full["origin"], full["baseline"])[1])
    err = P.centre_error(out["centres64"], cg)
    print("all six centres with image 5 from its tracks: %.4f of the extent after similarity alignment; averaging on the full graph: %.4f" % (err, bar))
    assert err <= bar


def test_stray_observations_come_out_as_outliers():
    """ten observations of tracks with four or more views moved by 30 .. 60 px (tests/triangulate_robust_oracle.py moves rows the same way): exactly those are
    outliers, and the centres stay near the clean run's.  Measured: centre error 0.0021 of the extent with them, 0.00067 without (3.1 x: the strays pull
    while the scale is wide, and no solve follows the classification); the largest inlier angle 0.29 degrees, the smallest planted one 3.7.  Asserted with a
    2 x margin on the ratio: 6.3 x the clean run's error"""
    bad, clean, planted, sc = P.stray_scene()
    got, ref = P.solve(bad), P.solve(clean)
    e1, e0 = P.centre_error(got["centres64"], sc["cg"]), P.centre_error(ref["centres64"], sc["cg"])
    inl = np.nanmax(np.where(planted, np.nan, got["angle_error64"]))
    print("stray observations: %d outliers of %d planted; centre error %.5f against %.5f clean (%.2f x); largest inlier angle %.3f, smallest planted %.3f degrees" % (
        got["num_outliers"], planted.sum(), e1, e0, e1 / e0, inl, np.nanmin(got["angle_error64"][planted])))
    assert ref["num_outliers"] == 0 and planted.sum() == 10
    assert ((got["node_state"] == P.OUTLIER) == planted).all() and got["num_outliers"] == 10
    assert (got["track_id"][planted] == -1).all() and np.isnan(got["points3d64"][planted]).all() and got["num_points"] == ref["num_points"]
    assert e1 <= 6.3 * e0


def test_degenerate_inputs():
    e = P.edge_scene()
    w = e["what"]
    out = P.solve(P.oracle_input(e))
    rows = w["rows"]
    assert out["positions_ok"] and (out["image_state"] == [P.HELD, P.POSED, P.POSED, P.POSED, P.HELD, P.TOO_FEW_TRACKS, 3, 3, 3]).all()
    # parallel rays: the 3 x 3 pivot fails, the track is out, everything else is solved
    assert all(out["node_state"][k, r] == P.DEGENERATE for k, r in rows[w["parallel"]].items()) and np.isnan(out["xyz64"][w["parallel"]]).all()
    # an image with one track is peeled; the track lives on in its other two images
    assert out["node_state"][5, rows[w["one"]][5]] == P.PEELED and out["node_state"][1, rows[w["one"]][1]] == P.INLIER and np.isfinite(out["xyz64"][w["one"]]).all()
    assert np.isfinite(out["poses64"][5, :, :3]).all() and np.isnan(out["poses64"][5, :, 3]).all()
    # the island
    for j in w["island"]:
        assert all(out["node_state"][k, r] == P.NOT_CONNECTED for k, r in rows[j].items()) and np.isnan(out["xyz64"][j]).all()
    assert out["node_state"][w["short"]] == P.PEELED and (out["node_state"][3, -2:] == P.NONE).all()
    assert out["num_posed"] == 5 and out["num_points"] == 31 and out["num_outliers"] == 0
    _, counts = np.unique(out["node_state"], return_counts=True)
    print("edge scene: node states", dict(zip(*np.unique(out["node_state"], return_counts=True))), "image states", out["image_state"].tolist())
    # held images at one centre
    poses = e["poses"].copy()
    poses[4] = poses[0]
    with pytest.raises(ValueError):
        P.solve(dict(P.oracle_input(e), poses=poses))


def test_a_bad_camera_leaves_everything_else_bit_for_bit():
    sc = P.scene(8, 32, 60, seed=1)
    inp = P.oracle_input(sc)
    cams, poses, tid = sc["cams"].copy(), sc["poses"].copy(), sc["track_id"].copy()
    cams[2, 0], poses[5, 1, 1] = 0.0, np.nan
    tid[[2, 5]] = -1
    got, ref = P.solve_once(dict(inp, cams=cams, poses=poses)), P.solve_once(dict(inp, track_id=tid))
    assert (got["status"] == [0, 0, 7, 0, 0, 7, 0, 0]).all() and (got["image_state"][[2, 5]] == P.IMG_BAD).all() and np.isnan(got["poses64"][[2, 5]]).all()
    assert (got["node_state"][[2, 5]][sc["track_id"][[2, 5]] >= 0] == P.BAD_IMAGE).all()
    rest = [0, 1, 3, 4, 6, 7]
    for k in ("poses64", "centres64", "points3d64", "track_id", "node_state", "angle_error64", "image_state"):
        assert np.array_equal(got[k][rest], ref[k][rest], equal_nan=True), k
    assert np.array_equal(got["xyz64"], ref["xyz64"], equal_nan=True) and got["iterations"] == ref["iterations"] and got["num_points"] == ref["num_points"]


# ---------------------------------------------------------------------- 2. the host API
def host_call(**kw):
    sc = P.scene(6, 32, 40)
    args = dict(feats={"keypoints": torch.from_numpy(sc["kpts"])}, tracks=(torch.from_numpy(sc["track_id"]), sc["T"]), cameras=torch.from_numpy(sc["cams"]),
                poses=torch.from_numpy(sc["poses"]), constant_pose=[0, 5])
    args.update(kw)
    return GlobalPositioner().solve(**args), sc


def test_constructor_refusals():
    for kw in (dict(num_iterations=5), dict(num_iterations=101), dict(num_iterations=7.5), dict(num_iterations=True), dict(angle_scale=0.0),
               dict(angle_scale=float("inf")), dict(angle_scale=float("nan")), dict(max_angle_error=-1.0), dict(max_angle_error=float("nan"))):
        with pytest.raises(ValueError, match=next(iter(kw))):
            GlobalPositioner(**kw)
    pos = GlobalPositioner(num_iterations=6, angle_scale=0.5, max_angle_error=3)
    assert (pos.num_iterations, pos.angle_scale, pos.max_angle_error) == (6, 0.5, 3.0)
    assert len(positioning.STATES) == 10 and positioning.STATES[P.OUTLIER] == "outlier" and positioning.STATES[P.INLIER] == "inlier"
    assert len(positioning.IMAGE_STATES) == 6 and positioning.IMAGE_STATES[P.POSED] == "posed" and positioning.IMAGE_STATES[P.IMG_NOT_CONNECTED] == "not_connected"
    assert lightglue_amd.GlobalPositioner is GlobalPositioner and "position_from_tracks" in lightglue_amd.__all__ and "GlobalPositioner" in lightglue_amd.__all__


def test_call_refusals_need_no_gpu():
    sc = P.scene(6, 32, 40)
    poses, tid = torch.from_numpy(sc["poses"]), torch.from_numpy(sc["track_id"])
    same = poses.clone()
    same[5] = same[0]
    nan_t = poses.clone()
    nan_t[5, 0, 3] = float("nan")
    for kw, word in ((dict(constant_pose=None), "at least two"), (dict(constant_pose=[0]), "at least two"), (dict(constant_pose=[]), "holds no image"),
                     (dict(constant_pose=[0, 6]), "outside"), (dict(constant_pose=torch.ones(5, dtype=torch.bool)), "shape"),
                     (dict(poses=same), "distinct centres"), (dict(poses=nan_t), "finite poses"), (dict(poses=poses[:5]), "poses must have shape"),
                     (dict(poses=(poses[:, :, :3], poses[:, :2, 3])), "poses"), (dict(tracks=(tid[:, :31], 40)), "track_id must have shape"),
                     (dict(tracks=(tid.float(), 40)), "integers"), (dict(tracks=(tid, 97)), "number of tracks"), (dict(tracks=(tid, -1)), "number of tracks"),
                     (dict(tracks=(tid, 2.5)), "number of tracks"), (dict(tracks=tid), "tracks must be"), (dict(tracks={"track_id": tid}), "num_tracks"),
                     (dict(poses={"poses": poses, "origin": 0}), "baseline"), (dict(poses={"poses": poses, "origin": 0, "baseline": None}, constant_pose=None), "baseline"),
                     (dict(cameras=torch.from_numpy(sc["cams"][:5])), "cameras")):
        with pytest.raises(ValueError, match=word):
            host_call(**kw)
    with pytest.raises(ValueError, match="between 2 and"):
        host_call(feats={"keypoints": torch.zeros(1, 32, 2)})
    # everything in order: the call reaches the device check, and there is no other path
    with pytest.raises(RuntimeError, match="MI355X"):
        host_call()
    with pytest.raises(RuntimeError, match="MI355X"):
        host_call(tracks={"track_id": tid, "num_tracks": 40}, poses=(poses[:, :, :3], poses[:, :, 3]), constant_pose=torch.tensor([True, False, False, False, False, True]))
    with pytest.raises(RuntimeError, match="MI355X"):
        lightglue_amd.position_from_tracks(GlobalPositioner(), (tid, 40), {"keypoints": torch.from_numpy(sc["kpts"])}, torch.from_numpy(sc["cams"]), poses, [0, 5])


def test_the_pose_estimators_dict_names_the_held_images():
    """constant_pose defaults to [origin, baseline] of GlobalPoseEstimator's dict: with those two at one centre the gauge is refused, with any other value of
    constant_pose it is not; with distinct centres the call goes through to the device check"""
    sc = P.scene(6, 32, 40)
    poses = torch.from_numpy(sc["poses"]).clone()
    poses[3] = poses[1]
    est = {"poses": poses, "origin": 1, "baseline": 3}
    with pytest.raises(ValueError, match="distinct centres"):
        host_call(poses=est, constant_pose=None)
    with pytest.raises(RuntimeError, match="MI355X"):
        host_call(poses=est, constant_pose=[0, 5])
    with pytest.raises(RuntimeError, match="MI355X"):
        host_call(poses=dict(est, baseline=4), constant_pose=None)


# ---------------------------------------------------------------------- 3. the C ABI
def test_workspace_bytes_and_the_envelope():
    lib = _cabi.load()
    size = lib.lg_positioning_workspace_bytes
    assert size(6, 128, 384, 0) > 0 and size(6, 128, 384, 0) % 256 == 0 and size(256, 8192, 2 ** 20, 0) > 0
    for args in ((1, 128, 10, 0), (257, 16, 10, 0), (6, 128, 385, 0), (6, 128, -1, 0), (6, 8193, 10, 0), (6, -1, 0, 0), (256, 8192 + 1, 10, 0), (6, 128, 10, 1),
                 (6, 128, 10, 1 << 31)):
        assert size(*args) == -1, args
    assert size(255, 8192, 10, 0) > 0 and size(256, 8192, 10, 0) > 0                # 2^21 rows: the cap itself
    for name in ("lg_positioning_workspace_bytes", "lg_positioning_solve"):
        assert name in _cabi.EXPORTED_SYMBOLS and getattr(lib, name) is not None
    assert lib.lg_positioning_solve.argtypes == [ctypes.POINTER(_cabi.LgPositioningIO), ctypes.c_void_p]


def test_solve_refuses_before_the_gpu_is_touched():
    """every pointer is a fake non-null value: a refusal that came later would have crashed"""
    lib = _cabi.load()
    inv = _cabi.LG_ERR_INVALID

    def io(**kw):
        need = lib.lg_positioning_workspace_bytes(6, 32, 40, 0)
        fields = dict(n=32, images=6, tracks=40, flags=0, num_iterations=12, angle_scale=1.0, max_angle_error=2.0, workspace=256, workspace_bytes=need)
        fields.update({k: 256 for k in ("kpts", "track_id", "cameras", "poses", "constant_pose", "poses_out", "xyz", "points3d", "track_id_out", "node_state",
                                         "image_state", "angle_error", "summary", "status")})
        fields.update(kw)
        return _cabi.LgPositioningIO(**fields)
    assert lib.lg_positioning_solve(None, None) == inv and b"lg_positioning_solve: null io" in lib.lg_last_error()
    for kw, word in ((dict(flags=1), b"flag"), (dict(images=1), b"images"), (dict(images=257), b"images"), (dict(tracks=97), b"tracks"), (dict(n=8193), b"LG_MAX_KEYPOINTS"),
                     (dict(num_iterations=5), b"num_iterations"), (dict(num_iterations=101), b"num_iterations"), (dict(angle_scale=0.0), b"angle_scale"),
                     (dict(max_angle_error=float("nan")), b"max_angle_error"), (dict(angle_scale=float("inf")), b"angle_scale"), (dict(track_id_out=None), b"null pointer"),
                     (dict(image_state=None), b"null pointer"), (dict(workspace=None), b"null workspace"), (dict(workspace_bytes=1024), b"lg_positioning_workspace_bytes"),
                     (dict(workspace=264), b"256-byte aligned")):
        assert lib.lg_positioning_solve(ctypes.byref(io(**kw)), None) == inv, kw
        assert word in lib.lg_last_error() and b"lg_positioning_solve" in lib.lg_last_error(), (kw, lib.lg_last_error())
