"""The bundle adjuster without a GPU: what the definition's fixed choices are worth on the inputs of tests/test_gpu_bundle.py (the precondition of its one-ulp
bar), that no decision of the oracle lies near its bar there, the cost's behaviour on the main scene, and the host layer (constructor, shape checks, the ctypes
mirror against the header, the envelope refusals of the C entry points)."""
import ctypes
import re

import numpy as np
import pytest
import torch

import bundle_oracle as B
import triangulate_oracle as O
import lightglue_amd
from lightglue_amd import BundleAdjuster, _cabi
from test_cabi_symbols import HEADER, typed_fields_of
from test_gpu_bundle import Q_POINT, Q_R, Q_T

SCALARS = {"int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double}


# ---------------------------------------------------------------------- the oracle
def spread(name):
    """the largest difference between the oracle's variants on one scene, in float32 ulps of the scale: (points, t, R)"""
    inp, ref = B.GPU_SCENES[name](), B.answer(name)
    track, image = B.scales(inp, ref)
    pu, tu = np.array([O.ulp32(s) for s in track]), np.array([O.ulp32(s) for s in image])
    worst = np.zeros(3)
    for solver in ("schur", "full"):
        for order in ("ascending", "descending"):
            out = B.answer(name, solver=solver, order=order)
            for k in ("num_iterations", "num_accepted", "converged", "num_observations"):
                assert out[k] == ref[k], (name, solver, order, k)
            assert (out["node_state"] == ref["node_state"]).all() and abs(out["final_cost"] - ref["final_cost"]) <= 1e-9 * ref["final_cost"]
            adj = ref["adjusted"]
            worst = np.maximum(worst, [(abs(out["xyz64"] - ref["xyz64"]).max(1)[adj] / pu[adj]).max(),
                                       (abs(out["poses64"][:, :, 3] - ref["poses64"][:, :, 3]).max(1) / tu).max(),
                                       abs(out["poses64"][:, :, :3] - ref["poses64"][:, :, :3]).max() / O.ulp32(1.0)])
    return worst


def test_oracle_sensitivity_is_far_below_one_ulp():
    worst = np.max([spread(name) for name in B.GPU_SCENES], 0)
    print("oracle spread in float32 ulps: points %.2e, t %.2e, R %.2e" % tuple(worst))
    assert (worst < 1e-3).all(), worst
    # the figures in the GPU test's docstring are these (other BLAS builds sum in other orders: a factor, not an order of magnitude)
    assert (worst <= 4 * np.array([Q_POINT, Q_T, Q_R])).all() and (np.array([Q_POINT, Q_T, Q_R]) < 1e-3).all(), worst


def test_no_decision_is_near_its_bar():
    for name in B.GPU_SCENES:
        for order in ("ascending", "descending"):
            assert B.answer(name, order=order)["near"] == [], (name, order)
    assert B.answer("main", num_iterations=1)["near"] == []
    slow = B.adjust(B.GPU_SCENES["main"](), initial_damping=B.SLOW_DAMPING)
    assert slow["near"] == [] and slow["num_iterations"] == 10 and not slow["converged"]


def test_cost_behaviour_on_the_main_scene():
    sc = B.main_scene()
    inp, out = B.oracle_input(sc), B.answer("main")
    costs = out["costs"]
    assert out["num_observations"] > 150 and out["free"].tolist() == [False, False, True, True, True, True]
    assert all(b < a for a, b in zip(costs, costs[1:])) and costs[0] == out["initial_cost"] and costs[-1] == out["final_cost"] and len(costs) == out["num_accepted"] + 1
    assert out["converged"] and out["num_iterations"] < 10 and out["final_cost"] < 0.05 * out["initial_cost"]
    long = B.adjust(inp, num_iterations=50, function_tolerance=1e-300)
    assert abs(out["final_cost"] - long["final_cost"]) <= 1e-6 * long["final_cost"], (out["final_cost"], long["final_cost"])
    adj = out["adjusted"]
    before = np.linalg.norm(inp["xyz"].astype(np.float64) - sc["truth"], axis=1)[adj]
    after = np.linalg.norm(out["xyz64"] - sc["truth"], axis=1)[adj]
    assert after.mean() < 0.5 * before.mean(), (before.mean(), after.mean())
    # the constant images come back as they went in; one iteration is one accepted step here
    assert (out["poses64"][:2] == inp["poses"][:2].astype(np.float64)).all()
    one = B.answer("main", num_iterations=1)
    assert one["num_iterations"] == 1 and one["num_accepted"] == 1 and not one["converged"] and one["final_cost"] == costs[1]


def test_the_edge_scene_holds_every_edge():
    bad, clean, what = B.edge_scene()
    out, ref = B.answer("edge"), B.answer("edge clean")
    st = out["node_state"]
    assert set(np.unique(st).tolist()) == {B.NONE, B.ACTIVE, B.BAD_IMAGE, B.NON_FINITE, B.BEHIND, B.SHORT}
    assert (st[3][bad["track_id"][3] >= 0] == B.BAD_IMAGE).all() and out["status"].tolist() == [0, 0, 0, B.LG_ERR_CAMERA, 0, 0, 0]
    assert not out["free"][what["empty_image"]] and (st[what["empty_image"]] == B.NONE).all()
    rows = what["rows"]
    assert st[2, rows[what["behind"]][2]] == B.BEHIND and st[5, rows[what["behind"]][5]] == B.SHORT
    assert all(st[k, i] == B.NON_FINITE for k, i in rows[what["nan"]].items() if k != 3)
    assert out["adjusted"][what["constant_only"]] and out["adjusted"][what["pair"]] and (st == B.ACTIVE)[:, :].sum() == out["num_observations"]
    assert sorted(k for k, i in rows[what["full"]].items() if st[k, i] == B.ACTIVE) == [0, 1, 2, 4, 5]
    # what the bad entries leave untouched is what the call without them gives, bit for bit
    assert np.array_equal(out["poses64"], ref["poses64"]) and np.array_equal(out["xyz64"], ref["xyz64"], equal_nan=True)
    assert out["final_cost"] == ref["final_cost"] and out["num_observations"] == ref["num_observations"]


def test_the_far_and_long_scenes_hold_what_they_are_for():
    far = B.answer("far")
    assert far["num_iterations"] - far["num_accepted"] >= 2 and far["converged"] and far["costs"][-1] < 1e-4 * far["costs"][0]
    assert all(b < a for a, b in zip(far["costs"], far["costs"][1:]))
    inp, clean = B.long_scene()
    out, ref = B.answer("long"), B.answer("long clean")
    T = len(inp["xyz"]) - 2
    assert (out["node_state"] == B.TOO_LONG).sum() == 1148 and not out["adjusted"][T] and out["adjusted"][T + 1] and out["xyz64"][T].tolist() == inp["xyz"][T].tolist()
    assert (out["node_state"][2, 100:102] == B.ACTIVE).all()              # two observations of one image in one track
    assert np.array_equal(out["poses64"], ref["poses64"]) and np.array_equal(out["xyz64"], ref["xyz64"]) and out["final_cost"] == ref["final_cost"]


# ---------------------------------------------------------------------- the host layer
def test_constructor_and_shape_checks():
    assert "BundleAdjuster" in lightglue_amd.__all__ and "bundle_adjust" in lightglue_amd.__all__ and callable(lightglue_amd.bundle_adjust)
    ba = BundleAdjuster()
    assert (ba.num_iterations, ba.initial_damping, ba.function_tolerance) == (10, 1e-4, 1e-6)
    for bad in (dict(num_iterations=0), dict(num_iterations=101), dict(num_iterations=2.5), dict(initial_damping=0.0), dict(initial_damping=float("nan")),
                dict(initial_damping=float("inf")), dict(function_tolerance=-1.0), dict(function_tolerance=float("inf"))):
        with pytest.raises(ValueError):
            BundleAdjuster(**bad)
    inp = B.oracle_input(B.main_scene())
    feats = {"keypoints": torch.from_numpy(inp["kpts"])}
    tid, xyz, cams, poses = (torch.from_numpy(np.ascontiguousarray(inp[k])) for k in ("track_id", "xyz", "cams", "poses"))
    const = torch.from_numpy(inp["constant"])
    with pytest.raises(ValueError, match="no image"):
        ba.adjust(feats, (tid, xyz), cams, poses, torch.zeros(O.K, dtype=torch.bool))
    with pytest.raises(ValueError, match="no image"):
        ba.adjust(feats, (tid, xyz), cams, poses, [])
    for args, word in ((((tid[:, :-1], xyz), cams, poses, const), "track_id"), (((tid.float(), xyz), cams, poses, const), "integers"),
                       (((tid, xyz[:, :2]), cams, poses, const), "xyz"), (((tid, xyz), cams[:-1], poses, const), "cameras"),
                       (((tid, xyz), cams, poses[:, :2], const), "poses"), (((tid, xyz), cams, poses, const[:-1]), "constant_pose"),
                       (((tid, xyz), cams, poses, [0, 9]), "outside"), ((tid, cams, poses, const), "tracks"),
                       (((tid, torch.zeros(O.K * O.N, 3)), cams, poses, const), "more than")):
        with pytest.raises(ValueError, match=word):
            ba.adjust(feats, *args)
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # every check passed: the device is refused, nothing else runs
        ba.adjust(feats, {"track_id": tid, "xyz": xyz}, cams, poses, [0, 1])


def test_mirror_symbols_and_constants_match_the_header():
    want = [(f, ctypes.c_void_p if ptr else SCALARS[t]) for f, t, ptr in typed_fields_of("lg_bundle_io")]
    assert want == list(_cabi.LgBundleIO._fields_)
    assert {"lg_bundle_workspace_bytes", "lg_bundle_adjust"} <= set(_cabi.EXPORTED_SYMBOLS)
    for name in ("LG_BA_MAX_IMAGES", "LG_BA_MAX_ITERATIONS", "LG_BA_MAX_TRACK_LENGTH", "LG_BA_CHOLESKY_BLOCK"):
        assert int(re.search(r"#define %s (\d+)" % name, HEADER).group(1)) == getattr(_cabi, name), name
    assert re.search(r"\bint lg_bundle_adjust\(const lg_bundle_io\* io, void\* hip_stream\);", HEADER)


def _io(**over):
    """a well-formed io, every pointer a fake non-null value: a refusal comes before anything is dereferenced"""
    lib = _cabi.load()
    K, N, T = 6, 96, 50
    fields = dict(n=N, images=K, tracks=T, flags=0, num_iterations=10, initial_damping=1e-4, function_tolerance=1e-6, workspace=256,
                  workspace_bytes=lib.lg_bundle_workspace_bytes(K, N, T, 0))
    fields.update({f: 256 for f, t in _cabi.LgBundleIO._fields_ if t is ctypes.c_void_p and f not in ("workspace", "num")})
    fields.update(over)
    return _cabi.LgBundleIO(**fields)


def test_envelope_is_refused_without_touching_a_gpu():
    lib = _cabi.load()
    size = lib.lg_bundle_workspace_bytes
    assert size(6, 96, 50, 0) > 0 and size(256, 8192, 2 ** 20, 0) > 256 * 6 * 256 * 6 * 8
    for args in ((0, 96, 0, 0), (257, 8, 4, 0), (6, 8193, 4, 0), (6, -1, 0, 0), (256, 8192 + 1, 4, 0), (6, 96, 289, 0), (6, 96, -1, 0), (6, 96, 50, 1),
                 (6, 96, 50, 1 << 21), (6, 96, 50, 1 << 31)):
        assert size(*args) == -1, args
    # the layout grows with every count (pieces are rounded to 256 bytes)
    assert size(6, 96, 250, 0) > size(6, 96, 50, 0) and size(7, 96, 50, 0) > size(6, 96, 50, 0) and size(6, 128, 50, 0) > size(6, 96, 50, 0)
    inv = _cabi.LG_ERR_INVALID
    assert lib.lg_bundle_adjust(None, None) == inv and b"null io" in lib.lg_last_error()
    need = size(6, 96, 50, 0)
    for over, word in ((dict(flags=2), b"flag"), (dict(images=257), b"LG_BA_MAX_IMAGES"), (dict(images=0), b"images"), (dict(n=8193), b"LG_MAX_KEYPOINTS"),
                       (dict(tracks=289), b"tracks"), (dict(tracks=-1), b"tracks"), (dict(num_iterations=0), b"num_iterations"),
                       (dict(num_iterations=101), b"num_iterations"), (dict(initial_damping=0.0), b"initial_damping"),
                       (dict(initial_damping=float("nan")), b"initial_damping"), (dict(function_tolerance=float("inf")), b"function_tolerance"),
                       (dict(function_tolerance=-1e-6), b"function_tolerance"), (dict(kpts=None), b"null pointer"), (dict(track_id=None), b"null pointer"),
                       (dict(xyz=None), b"null pointer"), (dict(constant_pose=None), b"null pointer"), (dict(summary=None), b"null pointer"),
                       (dict(observation_error=None), b"null pointer"), (dict(workspace=None), b"null workspace"), (dict(workspace=264), b"aligned"),
                       (dict(workspace_bytes=need - 1), b"lg_bundle_workspace_bytes")):
        io = _io(**over)
        assert lib.lg_bundle_adjust(ctypes.byref(io), None) == inv, over
        assert word in lib.lg_last_error() and b"lg_bundle_adjust" in lib.lg_last_error(), (over, lib.lg_last_error())
