"""The global pose estimator without a GPU: what the definition (tests/posegraph_oracle.py) is worth against the truth, the host layer's refusals, the C ABI's
mirror and envelope.  Scenes: cameras on an arc around a box (tests/triangulate_oracle.py), a ring plus 3 K random chords, weights 40 .. 400."""
import ctypes
import re

import numpy as np
import pytest
import torch

import posegraph_oracle as G
import lightglue_amd
from lightglue_amd import GlobalPoseEstimator, _cabi
from test_cabi_symbols import HEADER, typed_fields_of

SCALARS = {"int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double}

# noise 0.5 degrees on every pair, 25 % of the chords replaced by random poses: (K, seed) -> the oracle's worst rotation error in degrees and worst centre
# error as a fraction of the scene's extent after a similarity alignment, as measured; asserted with a 2 x margin.  Seeds on which the ring leaves every
# image two good pairs and the oracle poses all of them ((60, 0), (100, 1) and (100, 2) are not: an image is left with rotation only there)
MEASURED = {(6, 0): (0.3498, 0.00399), (20, 0): (0.4236, 0.00311), (20, 1): (0.5863, 0.03201), (40, 0): (0.5135, 0.00592), (60, 1): (0.4422, 0.00709)}


# ---------------------------------------------------------------------- the definition against the truth
@pytest.mark.parametrize("K", [3, 6, 16, 49, 100])
def test_exact_inputs_give_the_true_poses(K):
    sc = G.scene(K)
    out = G.run(sc, exact=True)
    assert out["num_posed"] == K and out["positions_ok"] and out["baseline"] == sc["baseline"] and (out["pair_state"] == G.USED).all()
    dR, dc = abs(out["poses64"][:, :, :3] - sc["Rg"]).max(), abs(out["centres64"] - sc["cg"]).max()
    print("K = %d: rotations %.2e, centres %.2e off the truth" % (K, dR, dc))          # measured: 4.3e-15 and 3.2e-11 at worst (K = 100, K = 49)
    assert dR < 1e-9 and dc < 1e-9
    t = -np.einsum("kij,kj->ki", sc["Rg"], sc["cg"])
    assert abs(out["poses64"][:, :, 3] - t).max() < 1e-9
    assert np.nanmax(out["rotation_error64"]) < 1e-9 and np.nanmax(out["direction_error64"]) < 1e-6
    assert out["rotation_iterations"] == 8                  # the scale is final from iteration 7 on; nothing moves on exact inputs


@pytest.mark.parametrize("K,seed", sorted(MEASURED))
def test_noise_and_outliers(K, seed):
    sc = G.scene(K, seed=seed, noise=0.5, outliers=0.25)
    out = G.run(sc)
    assert sc["planted"].sum() >= 2 and (out["pair_state"][sc["planted"]] == G.ROTATION_OUTLIER).all()
    assert (out["pair_state"][~sc["planted"]] == G.USED).all()
    assert out["num_posed"] == K and out["positions_ok"] and (out["image_state"] == G.POSED).all()
    rot, centre = G.against_truth(out, sc)
    print("K = %d, seed %d: %.4f degrees, %.5f of the extent" % (K, seed, rot, centre))
    assert rot <= 2.0 * MEASURED[K, seed][0] and centre <= 2.0 * MEASURED[K, seed][1]
    assert np.nanmin(out["rotation_error64"][sc["planted"]]) > 15.0 > np.nanmax(out["rotation_error64"][~sc["planted"]])


def test_edges_of_the_definition():
    bad, clean, what = G.edge_scene()
    a = G.estimate(bad["pairs"], bad["R"], bad["t"], 12, weights=bad["weights"])
    b = G.estimate(clean["pairs"], clean["R"], clean["t"], 12, weights=clean["weights"])
    assert np.array_equal(a["poses64"], b["poses64"], equal_nan=True) and (a["image_state"] == b["image_state"]).all()
    assert a["image_state"].tolist() == [0] * 7 + [G.ROTATION_ONLY] + [G.NOT_CONNECTED] * 4
    for p, st in enumerate(what["states"]):
        assert st is None or a["pair_state"][p] == st
    assert sorted(set(b["pair_state"].tolist())) == [G.USED, G.OUTSIDE, G.NO_POSITION]
    co = G.collinear_scene()
    c = G.estimate(co["pairs"], co["R"], co["t"], 5, weights=co["weights"])
    assert not c["positions_ok"] and c["num_posed"] == 0 and (c["image_state"] == G.ROTATION_ONLY).all() and np.isnan(c["poses64"][:, :, 3]).all()
    assert np.isfinite(c["poses64"][:, :, :3]).all() and (c["pair_state"] == G.USED).all()
    # too few inliers: no model
    sc = G.scene(6)
    inl = np.full(len(sc["pairs"]), 100)
    inl[4] = 14
    d = G.estimate(sc["pairs"], sc["R"], sc["t"], 6, num_inliers=inl)
    assert d["pair_state"][4] == G.NO_MODEL and (np.delete(d["pair_state"], 4) == G.USED).all() and np.isnan(d["rotation_error64"][4])


# ---------------------------------------------------------------------- the host layer
def test_constructor_and_shape_checks():
    assert "GlobalPoseEstimator" in lightglue_amd.__all__ and "estimate_global_poses" in lightglue_amd.__all__ and callable(lightglue_amd.estimate_global_poses)
    est = GlobalPoseEstimator()
    assert (est.num_iterations, est.rotation_scale, est.max_rotation_error, est.direction_scale, est.min_inliers) == (12, 5.0, 15.0, 5.0, 15)
    assert GlobalPoseEstimator.forward is GlobalPoseEstimator.estimate
    for bad in (dict(num_iterations=5), dict(num_iterations=101), dict(num_iterations=7.5), dict(rotation_scale=0.0), dict(rotation_scale=float("nan")),
                dict(max_rotation_error=float("inf")), dict(max_rotation_error=-1.0), dict(direction_scale=0.0), dict(min_inliers=-1), dict(min_inliers=2.5)):
        with pytest.raises(ValueError):
            GlobalPoseEstimator(**bad)
    sc = G.scene(6)
    pairs, R, t = (torch.from_numpy(np.ascontiguousarray(sc[k])) for k in ("pairs", "R", "t"))
    P = len(pairs)
    rel = {"R": R, "t": t, "num_inliers": torch.full((P,), 50)}
    for args, kw, word in (((pairs[:, :1], (R, t), 6), {}, "pairs"), ((pairs.float(), (R, t), 6), {}, "pairs"), ((pairs, (R[:-1], t), 6), {}, "R must"),
                           ((pairs, (R, t[:, :2]), 6), {}, "t must"), ((pairs, R, 6), {}, "relative"), ((pairs, {"R": R, "t": t}, 6), {}, "num_inliers"),
                           ((pairs, dict(rel, num_inliers=torch.ones(P)), 6), {}, "integers"), ((pairs, (R, t), 1), {}, "num_images"),
                           ((pairs, (R, t), 257), {}, "num_images"), ((pairs[:0], (R[:0], t[:0]), 6), {}, "pair list"), ((pairs, (R, t), 6), dict(origin=6), "origin"),
                           ((pairs, (R, t), 6), dict(baseline=0), "baseline"), ((pairs, (R, t), 6), dict(baseline=9), "baseline"),
                           ((pairs, (R, t), 6), dict(weights=torch.ones(P - 1)), "weights"), ((pairs, (R, t), 6), dict(weights=torch.ones(P).long()), "weights")):
        with pytest.raises(ValueError, match=word):
            est.estimate(*args, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # every check passed: the device is refused, nothing else runs
        est.estimate(pairs, rel, 6, origin=1, baseline=2, weights=torch.ones(P))


def test_mirror_symbols_and_constants_match_the_header():
    want = [(f, ctypes.c_void_p if ptr else SCALARS[t]) for f, t, ptr in typed_fields_of("lg_posegraph_io")]
    assert want == list(_cabi.LgPosegraphIO._fields_)
    assert {"lg_posegraph_workspace_bytes", "lg_posegraph_solve"} <= set(_cabi.EXPORTED_SYMBOLS)
    assert int(re.search(r"#define LG_PG_MIN_ITERATIONS (\d+)", HEADER).group(1)) == _cabi.LG_PG_MIN_ITERATIONS == 6
    assert re.search(r"\bint lg_posegraph_solve\(const lg_posegraph_io\* io, void\* hip_stream\);", HEADER)
    assert re.search(r"\bint64_t lg_posegraph_workspace_bytes\(int64_t images, int64_t pairs, uint32_t flags\);", HEADER)


def _io(**over):
    """a well-formed io, every pointer a fake non-null value: a refusal comes before anything is dereferenced"""
    lib = _cabi.load()
    K, P = 6, 15
    fields = dict(images=K, pairs=P, flags=0, num_iterations=12, origin=0, baseline=-1, min_inliers=15, rotation_scale=5.0, max_rotation_error=15.0,
                  direction_scale=5.0, workspace=256, workspace_bytes=lib.lg_posegraph_workspace_bytes(K, P, 0))
    fields.update({f: 256 for f, t in _cabi.LgPosegraphIO._fields_ if t is ctypes.c_void_p and f not in ("workspace", "num_inliers")})
    fields.update(over)
    return _cabi.LgPosegraphIO(**fields)


def test_envelope_is_refused_without_touching_a_gpu():
    lib = _cabi.load()
    size = lib.lg_posegraph_workspace_bytes
    assert size(6, 15, 0) > 0 and size(256, 2 ** 20, 0) > 769 * 768 * 8 + 52 * 2 ** 20 and size(2, 1, 0) > 0
    for args in ((1, 15, 0), (0, 15, 0), (257, 15, 0), (6, 0, 0), (6, -1, 0), (6, 2 ** 20 + 1, 0), (6, 15, 1), (6, 15, 1 << 31)):
        assert size(*args) == -1, args
    assert size(7, 15, 0) > size(6, 15, 0) and size(6, 150, 0) > size(6, 15, 0)
    inv = _cabi.LG_ERR_INVALID
    assert lib.lg_posegraph_solve(None, None) == inv and b"null io" in lib.lg_last_error()
    need = size(6, 15, 0)
    for over, word in ((dict(flags=1), b"flag"), (dict(images=257), b"LG_BA_MAX_IMAGES"), (dict(images=1), b"images"), (dict(pairs=0), b"pairs"),
                       (dict(pairs=2 ** 20 + 1), b"pairs"), (dict(num_iterations=5), b"num_iterations"), (dict(num_iterations=101), b"num_iterations"),
                       (dict(origin=6), b"origin"), (dict(origin=-1), b"origin"), (dict(baseline=0), b"baseline"), (dict(baseline=6), b"baseline"),
                       (dict(baseline=-2), b"baseline"), (dict(rotation_scale=0.0), b"rotation_scale"), (dict(max_rotation_error=float("nan")), b"max_rotation_error"),
                       (dict(direction_scale=float("inf")), b"direction_scale"), (dict(pair_index=None), b"null pointer"), (dict(rotations=None), b"null pointer"),
                       (dict(weights=None), b"null pointer"), (dict(poses=None), b"null pointer"), (dict(summary=None), b"null pointer"),
                       (dict(direction_error=None), b"null pointer"), (dict(workspace=None), b"null workspace"), (dict(workspace=264), b"aligned"),
                       (dict(workspace_bytes=need - 1), b"lg_posegraph_workspace_bytes")):
        io = _io(**over)
        assert lib.lg_posegraph_solve(ctypes.byref(io), None) == inv, over
        assert word in lib.lg_last_error() and b"lg_posegraph_solve" in lib.lg_last_error(), (over, lib.lg_last_error())
