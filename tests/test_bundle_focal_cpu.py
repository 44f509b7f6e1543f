"""The bundle adjuster with focal lengths refined, without a GPU: what the float64 definition (tests/bundle_focal_oracle.py) is for on scenes with wrong
focal lengths, where it coincides with tests/bundle_robust_oracle.py, that no decision of the oracle lies near its bar on the inputs of
tests/test_gpu_bundle_focal.py (the exceptions are named), and the host layer (constructor, constant_camera, the ctypes mirror, the C entry's refusals)."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import bundle_focal_oracle as F
import bundle_oracle as B
import bundle_robust_oracle as R
from lightglue_amd import BundleAdjuster, _cabi, bundle_adjust

HEADER = (Path(__file__).resolve().parents[1] / "include" / "lightglue_amd.h").read_text()


# ---------------------------------------------------------------------- 1. recovery
def test_exact_observations_return_the_true_focal_lengths():
    """Six images of 64 rows, 60 tracks of 3 .. 6 views in a box (not planar), exact observations (rounded to float32), the true poses with images 0 and 1
    held, every focal length off by a factor of its own in [0.92, 1.08] (2.3 % .. 6.2 % here), the points triangulated linearly under the wrong cameras.
    The oracle reaches a relative focal error of 2.2e-7 in every image (the keypoints are float32: 6e-8 of 500 pixels at a lever of a few hundred pixels)
    and a final cost of 1.9e-8 in 5 iterations; with the cameras held it stops at 42.8.  Bars, with a margin of about 40 on each figure the oracle
    reaches: relative focal error <= 1e-5 after; final cost with the focal lengths refined <= 1e-6 of the final cost with them held (oracle: 4.4e-10)."""
    inp, truth = F.recovery_scene()
    before = F.focal_error(inp["cams"], truth)
    assert 0.02 < before.min() and before.max() < 0.08
    out = F.adjust(inp)
    held = R.adjust(inp)
    after = F.focal_error(out["cameras64"], truth)
    print("focal error before %s\nafter %s\nfinal cost %.4g refined, %.4g held, %d iterations" % (before, after, out["final_cost"], held["final_cost"], out["num_iterations"]))
    assert out["converged"] and out["near"] == [] and out["num_free_cameras"] == F.RECOVERY_K and out["free"].sum() == 4
    assert after.max() <= 1e-5
    assert out["final_cost"] <= 1e-6 * held["final_cost"]
    # with refine_focal = False nothing can move a camera: the call ends far above the noise (here: zero) with the cameras it was given
    assert held["final_cost"] > 10.0 and np.sqrt(held["final_cost"] / held["num_observations"]) > 0.2
    assert np.array_equal(out["cameras64"][:, 2:], inp["cams"][:, 2:].astype(np.float64))
    # the held poses are the input's, their cameras moved
    assert np.array_equal(out["poses64"][:2], inp["poses"][:2].astype(np.float64)) and after[:2].max() <= 1e-5


def test_all_cameras_held_is_the_robust_mode():
    """every camera held: the seventh columns are identity and the call is tests/bundle_robust_oracle.py's, up to the two solvers' rounding"""
    inp = F.SCENES["all held"]()
    out, want = F.answer("all held"), R.adjust(F.SCENES["main"]())
    assert out["num_free_cameras"] == 0 and np.array_equal(out["cameras64"], inp["cams"].astype(np.float64))
    for k in ("num_iterations", "num_accepted", "converged", "num_observations"):
        assert out[k] == want[k], k
    assert (out["node_state"] == want["node_state"]).all()
    assert abs(out["final_cost"] - want["final_cost"]) <= 1e-9 * want["final_cost"]
    assert abs(out["poses64"] - want["poses64"]).max() < 1e-9 and abs(out["xyz64"] - want["xyz64"]).max() < 1e-9


# ---------------------------------------------------------------------- 2. noise
def test_half_a_pixel_of_noise():
    """The recovery scene with 0.5 pixels of noise on every observation.  Recorded from the oracle: the focal error falls from (3.1, 2.3, 5.9, 6.2, 2.5,
    5.7) % to (0.08, 0.06, 1.9, 0.57, 1.5, 1.3) %: closer to the truth in every image; the median reprojection error ends at 0.41 pixels (the noise: sigma
    = 0.5 per axis has a median radius of 0.59; the fit takes its share), the final cost is 74.4 over 268 observations"""
    inp, truth = F.recovery_scene(0.5)
    out = F.adjust(inp)
    before, after = F.focal_error(inp["cams"], truth), F.focal_error(out["cameras64"], truth)
    median = float(np.nanmedian(out["error64"]))
    print("focal error before %s\nafter %s\nmedian reprojection error %.3f, final cost %.4g over %d" % (before, after, median, out["final_cost"], out["num_observations"]))
    assert (after < before).all() and out["converged"]
    assert 0.2 < median < 0.59 * 1.2                         # at the noise level: not above the noise's own median radius (with 20 % for 268 samples)
    held = R.adjust(inp)                                     # the free poses and the points bend around the wrong cameras: a higher cost, the same cameras
    print("cameras held: median %.3f, final cost %.4g" % (float(np.nanmedian(held["error64"])), held["final_cost"]))
    assert held["final_cost"] > out["final_cost"] and float(np.nanmedian(held["error64"])) > median


# ---------------------------------------------------------------------- 3. no decision near its bar on the GPU test's scenes
NEAR = {"main": ["accept"], "K = 9": ["accept"], "camera held": ["accept"], "all held": ["accept"]}


def test_no_decision_is_near_its_bar_on_the_gpu_test_inputs():
    """The exceptions, one kind: the last accepted step of four calls lowers the cost by 1.4e-10 .. 7.5e-10 of it (6e-9 .. 6e-8 absolute: main 2.1e-10,
    K = 9 2.8e-10, camera held 1.4e-10, all held 7.5e-10), five orders above the fp64 noise of a sum of 200 terms.  The GPU test asserts those decisions
    equal like all others"""
    for name in F.SCENES:
        out = F.answer(name)
        assert out["near"] == NEAR.get(name, []), (name, out["near"])
        if out["near"]:
            c = out["costs"]
            assert 1e-10 < (c[-2] - c[-1]) / c[-2] < 1e-9 and c[-2] - c[-1] > 1e-9, name


def test_scenes_are_what_the_gpu_test_takes_them_for():
    assert len(F.SCENES["K = 7"]()["cams"]) == 7 and F.D * 7 == _cabi.LG_BA_CHOLESKY_BLOCK + 1             # one column past the first panel
    assert F.D * 9 > _cabi.LG_BA_CHOLESKY_BLOCK + F.D
    planted = F.answer("planted")
    assert sorted(map(tuple, np.argwhere(planted["node_state"] == R.FILTERED).tolist())) == R.planted_scene()[1] and planted["num_filtered"] == 12
    long = F.answer("long")
    assert (long["node_state"][2, 100:102] == B.ACTIVE).all() and abs(long["error64"][2, 100] - long["error64"][2, 101]) > 1e-3
    main, held = F.answer("main"), F.answer("camera held")
    inp = F.SCENES["main"]()
    # a pose-held image with a free camera: images 0 and 1 of the main scene
    assert not main["free"][:2].any() and main["free_camera"][:2].all() and (main["cameras64"][:2, :2] != inp["cams"][:2, :2]).all()
    assert np.array_equal(main["poses64"][:2], inp["poses"][:2].astype(np.float64))
    # a pose-free image with a held camera: images 3 and 4
    assert held["free"][3:5].all() and not held["free_camera"][3:5].any() and held["num_free_cameras"] == 4
    assert np.array_equal(held["cameras64"][3:5], inp["cams"][3:5].astype(np.float64)) and (held["poses64"][3:5] != inp["poses"][3:5]).any()
    edge, clean = F.answer("edge"), F.answer("edge clean")
    assert edge["status"].tolist() == [0, 0, 0, B.LG_ERR_CAMERA, 0, 0, 0] and np.array_equal(edge["cameras64"][3], F.SCENES["edge"]()["cams"][3].astype(np.float64))
    for k in ("poses64", "xyz64", "final_cost"):
        assert np.array_equal(edge[k], clean[k], equal_nan=True), k
    assert np.array_equal(np.delete(edge["cameras64"], 3, 0), np.delete(clean["cameras64"], 3, 0))


# ---------------------------------------------------------------------- 4. the host layer
def _call(ba, constant_pose=(0, 1), **kw):
    inp = B.oracle_input(B.main_scene())
    feats = {"keypoints": torch.from_numpy(inp["kpts"])}
    return ba.adjust(feats, (torch.from_numpy(inp["track_id"]), torch.from_numpy(inp["xyz"])), torch.from_numpy(inp["cams"]), torch.from_numpy(inp["poses"]),
                     list(constant_pose), **kw)


def test_constructor_and_constant_camera_are_validated_on_the_host():
    assert BundleAdjuster().refine_focal is False and BundleAdjuster(refine_focal=True).refine_focal is True
    ba = BundleAdjuster(refine_focal=True, loss="cauchy", loss_scale=3.0, filter_rounds=2, max_reproj_error=2.5)
    assert (ba.loss, ba.loss_scale, ba.filter_rounds, ba.max_reproj_error, ba.refine_focal) == ("cauchy", 3.0, 2, 2.5, True)
    ba.robust_entry = True
    assert ba.refine_focal is True                             # the tests' switch between the two older entry points leaves it alone
    for bad, word in ((dict(refine_focal=1), "refine_focal"), (dict(refine_focal="yes"), "refine_focal"), (dict(refine_focal=True, loss="l1"), "loss"),
                      (dict(refine_focal=True, loss="huber", loss_scale=0.0), "loss_scale"), (dict(refine_focal=True, filter_rounds=5), "filter_rounds"),
                      (dict(refine_focal=True, filter_rounds=1, max_reproj_error=0.0), "max_reproj_error"), (dict(refine_focal=True, num_iterations=0), "num_iterations")):
        with pytest.raises(ValueError, match=word):
            BundleAdjuster(**bad)
    # without refine_focal a camera cannot be named
    for held in ([0], np.zeros(6, bool), []):
        with pytest.raises(ValueError, match="constant_camera needs refine_focal"):
            _call(BundleAdjuster(), constant_camera=held)
    with pytest.raises(ValueError, match="constant_camera needs refine_focal"):
        bundle_adjust(BundleAdjuster(loss="cauchy"), (torch.zeros((6, 96), dtype=torch.int64), torch.zeros((4, 3))), {"keypoints": torch.zeros((6, 96, 2))},
                      torch.ones((6, 4)), torch.zeros((6, 3, 4)), [0], constant_camera=[1])
    # with it: constant_pose's parsing and messages under the argument's own name; the gauge rule is about poses alone
    focal = BundleAdjuster(refine_focal=True)
    for held, word in (([6], r"constant_camera names an image outside \[0, 6\)"), ([-1], "constant_camera names an image outside"),
                       (np.zeros(5, bool), r"constant_camera must have shape \[6\]"), ([0.5], "constant_camera must be a \\[K\\] bool mask or a sequence of image indices"),
                       (np.zeros((6, 1), np.int64), "constant_camera must be")):
        with pytest.raises(ValueError, match=word):
            _call(focal, constant_camera=held)
    with pytest.raises(ValueError, match="constant_pose holds no image"):
        _call(focal, constant_pose=[], constant_camera=[0, 1])
    # every host check passes, no camera held, an empty list or all of them: the call then asks for a GPU (this process has none to give a CPU tensor)
    for held in (None, [], np.zeros(6, bool), np.ones(6, bool), [0, 5]):
        with pytest.raises(Exception) as err:
            _call(focal, constant_camera=held)
        assert not isinstance(err.value, (ValueError, TypeError)) or "constant" not in str(err.value), (held, err.value)


def fields_of(name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [re.match(r"(?:const )?(\w+) ?(\*?)(\w+)$", d.strip()).groups() for d in body.split(";") if d.strip()]


def test_mirror_and_symbols_match_the_header():
    want = [(f, _cabi.LgBundleRobustIO if t == "lg_bundle_robust_io" else ctypes.c_void_p) for t, ptr, f in fields_of("lg_bundle_focal_io")]
    assert want == list(_cabi.LgBundleFocalIO._fields_) and [f for f, _ in want] == ["base", "constant_camera", "cameras_out"]
    assert {"lg_bundle_focal_workspace_bytes", "lg_bundle_adjust_focal"} <= set(_cabi.EXPORTED_SYMBOLS)
    assert re.search(r"\bint lg_bundle_adjust_focal\(const lg_bundle_focal_io\* io, void\* hip_stream\);", HEADER)
    assert re.search(r"\bint64_t lg_bundle_focal_workspace_bytes\(int64_t images, int32_t n, int64_t tracks, uint32_t flags\);", HEADER)
    # the two older entry points are what they were
    assert re.search(r"\bint lg_bundle_adjust\(const lg_bundle_io\* io, void\* hip_stream\);", HEADER)
    assert re.search(r"\bint lg_bundle_adjust_robust\(const lg_bundle_robust_io\* io, void\* hip_stream\);", HEADER)


def _io(base=None, robust=None, **over):
    """a well-formed io, every pointer a fake non-null value: a refusal comes before anything is dereferenced"""
    lib = _cabi.load()
    K, N, T = 6, 96, 50
    fields = dict(n=N, images=K, tracks=T, flags=0, num_iterations=10, initial_damping=1e-4, function_tolerance=1e-6, workspace=256,
                  workspace_bytes=lib.lg_bundle_focal_workspace_bytes(K, N, T, 0))
    fields.update({f: 256 for f, t in _cabi.LgBundleIO._fields_ if t is ctypes.c_void_p and f not in ("workspace", "num")})
    fields.update(base or {})
    mid = dict(loss=2, loss_scale=2.0, filter_rounds=1, max_reproj_error=4.0)
    mid.update(robust or {})
    top = dict(constant_camera=256, cameras_out=256)
    top.update(over)
    return _cabi.LgBundleFocalIO(base=_cabi.LgBundleRobustIO(base=_cabi.LgBundleIO(**fields), **mid), **top)


def test_envelope_is_refused_without_touching_a_gpu():
    lib = _cabi.load()
    size, robust = lib.lg_bundle_focal_workspace_bytes, lib.lg_bundle_robust_workspace_bytes
    # 7 unknowns per image: the step grows by 8 bytes per image, S from (6 K + 1) 6 K to (7 K + 1) 7 K fp64, and the camera state is 64 bytes per image
    up = lambda b: (b + 255) // 256 * 256
    for K in (6, 7, 256):
        grown = up(K * 56) - up(K * 48) + up((7 * K + 1) * 7 * K * 8) - up((6 * K + 1) * 6 * K * 8) + up(K * 64)
        assert size(K, 96, 50, 0) == robust(K, 96, 50, 0) + grown, K
    assert (7 * 256 + 1) * 7 * 256 * 8 == 25704448             # 25.7 MB at 256 images
    for args in ((0, 96, 0, 0), (257, 8, 4, 0), (6, 8193, 4, 0), (6, 96, 289, 0), (6, 96, -1, 0), (6, 96, 50, 1), (6, 96, 50, 1 << 31)):
        assert size(*args) == -1, args
    inv, name = _cabi.LG_ERR_INVALID, b"lg_bundle_adjust_focal"
    assert lib.lg_bundle_adjust_focal(None, None) == inv and b"null io" in lib.lg_last_error() and name in lib.lg_last_error()
    need = size(6, 96, 50, 0)
    nan, inf = float("nan"), float("inf")
    cases = [(dict(), dict(loss=-1), dict(), b"loss must"), (dict(), dict(loss=3), dict(), b"loss must"), (dict(), dict(loss=1, loss_scale=0.0), dict(), b"loss_scale"),
             (dict(), dict(loss=2, loss_scale=nan), dict(), b"loss_scale"), (dict(), dict(filter_rounds=-1), dict(), b"filter_rounds"),
             (dict(), dict(filter_rounds=5), dict(), b"filter_rounds"), (dict(), dict(filter_rounds=1, max_reproj_error=0.0), dict(), b"max_reproj_error"),
             (dict(), dict(filter_rounds=2, max_reproj_error=inf), dict(), b"max_reproj_error"),
             (dict(flags=1), dict(), dict(), b"flag"), (dict(flags=1 << 31), dict(), dict(), b"flag"),
             (dict(images=257), dict(), dict(), b"LG_BA_MAX_IMAGES"), (dict(images=0), dict(), dict(), b"images"), (dict(n=8193), dict(), dict(), b"LG_MAX_KEYPOINTS"),
             (dict(tracks=289), dict(), dict(), b"tracks"), (dict(num_iterations=0), dict(), dict(), b"num_iterations"), (dict(num_iterations=101), dict(), dict(), b"num_iterations"),
             (dict(initial_damping=nan), dict(), dict(), b"initial_damping"), (dict(function_tolerance=-1e-6), dict(), dict(), b"function_tolerance"),
             (dict(), dict(), dict(cameras_out=None), b"cameras_out"),
             (dict(kpts=None), dict(), dict(), b"null pointer"), (dict(summary=None), dict(), dict(), b"null pointer"), (dict(constant_pose=None), dict(), dict(), b"null pointer"),
             (dict(workspace=None), dict(), dict(), b"null workspace"), (dict(workspace=264), dict(), dict(), b"aligned"),
             (dict(workspace_bytes=need - 1), dict(), dict(), b"lg_bundle_focal_workspace_bytes"),
             (dict(workspace_bytes=robust(6, 96, 50, 0)), dict(), dict(), b"lg_bundle_focal_workspace_bytes")]
    for base, mid, over, word in cases:
        io = _io(base, mid, **over)
        assert lib.lg_bundle_adjust_focal(ctypes.byref(io), None) == inv, (base, mid, over)
        assert word in lib.lg_last_error() and name in lib.lg_last_error(), (base, mid, over, lib.lg_last_error())
    # the order: the layout, the robust settings, cameras_out, then lg_bundle_adjust's list
    io = _io(dict(num_iterations=0, flags=1), dict(loss=7), cameras_out=None)
    assert lib.lg_bundle_adjust_focal(ctypes.byref(io), None) == inv and b"flag" in lib.lg_last_error()
    io = _io(dict(num_iterations=0), dict(loss=7), cameras_out=None)
    assert lib.lg_bundle_adjust_focal(ctypes.byref(io), None) == inv and b"loss must" in lib.lg_last_error()
    io = _io(dict(num_iterations=0), cameras_out=None)
    assert lib.lg_bundle_adjust_focal(ctypes.byref(io), None) == inv and b"cameras_out" in lib.lg_last_error()
    # a null constant_camera holds no camera and is not refused: the refusal that follows is the next in line (here the workspace)
    io = _io(dict(workspace_bytes=0), constant_camera=None)
    assert lib.lg_bundle_adjust_focal(ctypes.byref(io), None) == inv and b"workspace" in lib.lg_last_error()
    # the older entry points refuse under their own names, as before
    io = _io(dict(flags=2))
    assert lib.lg_bundle_adjust_robust(ctypes.byref(io.base), None) == inv and b"lg_bundle_adjust_robust:" in lib.lg_last_error()
    assert lib.lg_bundle_adjust(ctypes.byref(io.base.base), None) == inv and b"lg_bundle_adjust:" in lib.lg_last_error()
