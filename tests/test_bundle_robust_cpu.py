"""The bundle adjuster's robust mode without a GPU: the float64 definition (tests/bundle_robust_oracle.py) against tests/bundle_oracle.py where the two must
coincide, what the loss and the filter are for on the planted scene, the filter's edges, that no decision of the oracle lies near its bar on the inputs of
tests/test_gpu_bundle_robust.py, and the host layer (constructor, the ctypes mirror against the header, the refusals of the C entry point)."""
import ctypes
import re

import numpy as np
import pytest

import bundle_oracle as B
import bundle_robust_oracle as R
from lightglue_amd import BundleAdjuster, _cabi, bundle
from test_cabi_symbols import HEADER, typed_fields_of

OUTPUTS = ("poses64", "xyz64", "points3d64", "node_state", "error64", "initial_cost", "final_cost", "num_iterations", "num_accepted", "converged",
           "num_observations", "status", "free", "adjusted", "costs")


def same(a, b, what):
    for k in OUTPUTS:
        assert np.array_equal(a[k], b[k], equal_nan=True) if isinstance(a[k], np.ndarray) else a[k] == b[k], (what, k)


def filtered(out):
    return sorted(map(tuple, np.argwhere(out["node_state"] == R.FILTERED).tolist()))


# ---------------------------------------------------------------------- where the two definitions coincide
@pytest.mark.parametrize("name", ["main", "edge", "far", "long"])
def test_squared_loss_without_filter_is_the_plain_adjuster(name):
    inp = B.GPU_SCENES[name]()
    out = R.adjust(inp)
    same(out, B.answer(name), name)
    assert out["num_filtered"] == 0 and out["num_filter_stages"] == 0 and out["near"] == B.answer(name)["near"]


def test_huber_with_a_huge_scale_is_the_squared_loss_in_every_bit():
    for name in ("main", "long"):                   # long: two observations of one image in one track
        inp = B.GPU_SCENES[name]()
        same(R.adjust(inp, loss="huber", loss_scale=1e6), B.answer(name), name)
    inp = R.planted_scene()[0]
    same(R.adjust(inp, loss="huber", loss_scale=1e6, **R.ONE_ROUND), R.adjust(inp, **R.ONE_ROUND), "planted, one round")


def test_a_filter_that_removes_nothing_is_the_longer_single_stage_call():
    inp = B.GPU_SCENES["main"]()
    for conf, iterations, rounds in ((R.CAUCHY, 3, 1), (R.CAUCHY, 2, 2), (R.HUBER, 10, 1), (dict(loss="squared"), 1, 3)):
        staged = R.adjust(inp, **conf, filter_rounds=rounds, max_reproj_error=50.0, num_iterations=iterations)
        single = R.adjust(inp, **conf, num_iterations=iterations * (rounds + 1))
        assert staged["num_filtered"] == 0 and staged["num_filter_stages"] == 0 and staged["near"] == single["near"]
        same(staged, single, (conf, iterations, rounds))
    assert R.adjust(inp, **R.CAUCHY, num_iterations=6)["num_iterations"] == 6          # the identity above crosses a stage boundary before it converges


# ---------------------------------------------------------------------- what the feature is for: the planted scene
def test_planted_scene_is_the_recipe():
    inp, planted, _ = R.planted_scene()
    clean = B.GPU_SCENES["main"]()
    assert len(planted) == 12 and (B.answer("main")["node_state"] == B.ACTIVE).sum() == 212
    tracks = [int(inp["track_id"][n]) for n in planted]
    assert len(set(tracks)) == 12 and all((inp["track_id"] == j).sum() >= 3 for j in tracks)
    moved = np.linalg.norm(inp["kpts"].astype(np.float64) - clean["kpts"], axis=2)
    assert sorted(map(tuple, np.argwhere(moved > 0).tolist())) == planted and all(19.99 < moved[n] < 80.01 for n in planted)
    assert len(R.planted_scene(30)[1]) == 23


def test_cauchy_and_one_filter_round_take_exactly_the_planted_observations():
    inp, planted, truth = R.planted_scene()
    out = R.answer("planted", **R.CAUCHY, **R.ONE_ROUND)
    assert filtered(out) == planted and out["num_filtered"] == 12 and out["num_filter_stages"] == 1 and out["num_observations"] == 200
    assert out["near"] == [] and out["converged"]
    squared = R.answer("planted")
    robust, plain = np.median(R.point_errors(inp, out, truth)), np.median(R.point_errors(inp, squared, truth))
    print("median point error: %.4f with Cauchy and one round, %.4f with the squared loss" % (robust, plain))
    assert robust < plain and robust < 0.1 * plain
    assert np.nanmax(out["error64"]) < 4.0 and (np.nan_to_num(squared["error64"]) > 4.0).sum() > 60          # squared: 63 clean observations above the bar
    assert np.isnan(out["points3d64"][tuple(np.array(planted).T)]).all() and np.isnan(out["error64"][tuple(np.array(planted).T)]).all()
    # without the filter the loss alone already singles them out; a second round finds nothing more
    for conf in (R.CAUCHY, R.HUBER, dict(loss="cauchy", loss_scale=4.0)):
        alone = R.answer("planted", **conf)
        assert alone["near"] == [] and sorted(map(tuple, np.argwhere(np.nan_to_num(alone["error64"]) > 4.0).tolist())) == planted, conf
        assert np.median(R.point_errors(inp, alone, truth)) < plain
    twice = R.answer("planted", **R.CAUCHY, filter_rounds=2, max_reproj_error=4.0)
    assert filtered(twice) == planted and twice["num_filter_stages"] == 1 and twice["near"] == []
    for k in ("poses64", "xyz64", "node_state"):
        assert np.array_equal(twice[k], out[k], equal_nan=True), k
    # Huber and the wider Cauchy with a round: the same twelve.  Huber's last accepted step lowers the cost by 5.9e-10 of it (3e-8 absolute): the one
    # decision within NEAR of a bar on these inputs
    for conf, near in ((R.HUBER, ["accept"]), (dict(loss="cauchy", loss_scale=4.0), [])):
        other = R.answer("planted", **conf, **R.ONE_ROUND)
        assert filtered(other) == planted and other["near"] == near, conf


def test_cauchy_holds_at_twice_the_contamination():
    inp, planted, truth = R.planted_scene(30)
    out = R.answer("planted 23", **R.CAUCHY, **R.ONE_ROUND)
    assert len(planted) == 23 and filtered(out) == planted and out["near"] == []
    assert np.median(R.point_errors(inp, out, truth)) < np.median(R.point_errors(inp, R.adjust(inp), truth))


# ---------------------------------------------------------------------- the filter's edges
def test_filter_shortens_a_track_to_one_observation():
    inp, moved, alone, j = R.short_scene()
    out = R.answer("short", **R.CAUCHY, **R.ONE_ROUND)
    assert out["near"] == [] and filtered(out) == [moved] and out["node_state"][alone] == B.SHORT
    assert out["adjusted"][j] and not out["adjusted_end"][j] and np.isnan(out["points3d64"][alone]).all()
    # the track comes back where its last accepted step left it, not as the bits that went in
    assert abs(out["xyz64"][j] - inp["xyz"][j].astype(np.float64)).max() > 1e-3
    assert out["num_observations"] == (out["first_state"] == B.ACTIVE).sum() - 2


def test_filter_takes_the_last_observations_of_a_free_image():
    inp, nodes = R.last_observation_scene()
    out = R.answer("last", **R.LAST)
    assert out["near"] == [] and filtered(out) == nodes and out["num_iterations"] == 2
    assert out["free"][R.LAST_IMAGE] and not out["free_end"][R.LAST_IMAGE] and out["free_end"][2:5].all()
    assert abs(out["poses64"][R.LAST_IMAGE] - inp["poses"][R.LAST_IMAGE].astype(np.float64)).max() > 1e-3          # its last accepted pose
    one = R.adjust(inp, **R.CAUCHY, num_iterations=1)
    assert np.array_equal(out["poses64"][R.LAST_IMAGE], one["poses64"][R.LAST_IMAGE])                              # which the second stage left alone
    assert out["adjusted_end"][[int(inp["track_id"][n]) for n in nodes]].all()                                     # their tracks go on without them


def test_no_decision_is_near_its_bar_on_the_gpu_test_inputs():
    for name, conf in (("planted", R.CAUCHY), ("planted", R.HUBER), ("planted", dict(R.CAUCHY, **R.ONE_ROUND)), ("short", dict(R.CAUCHY, **R.ONE_ROUND)),
                       ("last", R.LAST), ("K = 9", R.CAUCHY), ("edge", dict(R.CAUCHY, **R.ONE_ROUND)), ("edge clean", dict(R.CAUCHY, **R.ONE_ROUND)), ("long", R.CAUCHY)):
        assert R.answer(name, **conf)["near"] == [], (name, conf)


# ---------------------------------------------------------------------- the host layer
def test_constructor_validates_like_the_c_side():
    ba = BundleAdjuster()
    assert (ba.loss, ba.loss_scale, ba.filter_rounds, ba.max_reproj_error) == ("squared", 2.0, 0, 4.0)
    assert bundle.STATES[7] == "filtered" and len(bundle.STATES) == 8 and bundle.STATES[:7] == ("none", "active", "bad_image", "non_finite_point", "behind",
                                                                                               "short_track", "too_long")
    ok = BundleAdjuster(loss="cauchy", loss_scale=3.0, filter_rounds=4, max_reproj_error=2.5)
    assert (ok.loss, ok.loss_scale, ok.filter_rounds, ok.max_reproj_error) == ("cauchy", 3.0, 4, 2.5)
    for bad, word in ((dict(loss="l1"), "loss"), (dict(loss=1), "loss"), (dict(loss="huber", loss_scale=0.0), "loss_scale"),
                      (dict(loss="cauchy", loss_scale=float("nan")), "loss_scale"), (dict(loss="cauchy", loss_scale=float("inf")), "loss_scale"),
                      (dict(filter_rounds=-1), "filter_rounds"), (dict(filter_rounds=5), "filter_rounds"), (dict(filter_rounds=1.5), "filter_rounds"),
                      (dict(filter_rounds=1, max_reproj_error=0.0), "max_reproj_error"), (dict(filter_rounds=2, max_reproj_error=float("nan")), "max_reproj_error")):
        with pytest.raises(ValueError, match=word):
            BundleAdjuster(**bad)
    # what the C side does not read is not refused
    BundleAdjuster(loss="squared", loss_scale=0.0)
    BundleAdjuster(loss="huber", filter_rounds=0, max_reproj_error=-1.0)


def test_mirror_symbols_and_constants_match_the_header():
    scalars = {"int32_t": ctypes.c_int32, "double": ctypes.c_double, "lg_bundle_io": _cabi.LgBundleIO}
    want = [(f, scalars[t]) for f, t, ptr in typed_fields_of("lg_bundle_robust_io") if not ptr]
    assert want == list(_cabi.LgBundleRobustIO._fields_)
    assert {"lg_bundle_robust_workspace_bytes", "lg_bundle_adjust_robust"} <= set(_cabi.EXPORTED_SYMBOLS)
    for name, value in (("LG_BA_LOSS_SQUARED", _cabi.LG_BA_LOSS["squared"]), ("LG_BA_LOSS_HUBER", _cabi.LG_BA_LOSS["huber"]),
                        ("LG_BA_LOSS_CAUCHY", _cabi.LG_BA_LOSS["cauchy"]), ("LG_BA_MAX_FILTER_ROUNDS", _cabi.LG_BA_MAX_FILTER_ROUNDS)):
        assert int(re.search(r"#define %s (\d+)" % name, HEADER).group(1)) == value, name
    assert R.MAX_FILTER_ROUNDS == _cabi.LG_BA_MAX_FILTER_ROUNDS and list(R.LOSSES) == sorted(_cabi.LG_BA_LOSS, key=_cabi.LG_BA_LOSS.get)
    assert re.search(r"\bint lg_bundle_adjust_robust\(const lg_bundle_robust_io\* io, void\* hip_stream\);", HEADER)


def _io(base=None, **over):
    """a well-formed io, every pointer a fake non-null value: a refusal comes before anything is dereferenced"""
    lib = _cabi.load()
    K, N, T = 6, 96, 50
    fields = dict(n=N, images=K, tracks=T, flags=0, num_iterations=10, initial_damping=1e-4, function_tolerance=1e-6, workspace=256,
                  workspace_bytes=lib.lg_bundle_robust_workspace_bytes(K, N, T, 0))
    fields.update({f: 256 for f, t in _cabi.LgBundleIO._fields_ if t is ctypes.c_void_p and f not in ("workspace", "num")})
    fields.update(base or {})
    top = dict(loss=2, loss_scale=2.0, filter_rounds=1, max_reproj_error=4.0)
    top.update(over)
    return _cabi.LgBundleRobustIO(base=_cabi.LgBundleIO(**fields), **top)


def test_envelope_is_refused_without_touching_a_gpu():
    lib = _cabi.load()
    size, plain = lib.lg_bundle_robust_workspace_bytes, lib.lg_bundle_workspace_bytes
    assert size(6, 96, 50, 0) == plain(6, 96, 50, 0) + 256 and size(6, 96, 0, 0) == plain(6, 96, 0, 0)          # one int32 per track, rounded to 256 bytes
    for args in ((0, 96, 0, 0), (257, 8, 4, 0), (6, 8193, 4, 0), (6, 96, 289, 0), (6, 96, -1, 0), (6, 96, 50, 1), (6, 96, 50, 2), (6, 96, 50, 1 << 31)):
        assert size(*args) == -1, args
    inv, name = _cabi.LG_ERR_INVALID, b"lg_bundle_adjust_robust"
    assert lib.lg_bundle_adjust_robust(None, None) == inv and b"null io" in lib.lg_last_error() and name in lib.lg_last_error()
    need = size(6, 96, 50, 0)
    nan, inf = float("nan"), float("inf")
    cases = [(dict(), dict(loss=-1), b"loss must"), (dict(), dict(loss=3), b"loss must"), (dict(), dict(loss=1, loss_scale=0.0), b"loss_scale"),
             (dict(), dict(loss=2, loss_scale=-2.0), b"loss_scale"), (dict(), dict(loss=2, loss_scale=nan), b"loss_scale"), (dict(), dict(loss=1, loss_scale=inf), b"loss_scale"),
             (dict(), dict(filter_rounds=-1), b"filter_rounds"), (dict(), dict(filter_rounds=5), b"filter_rounds"),
             (dict(), dict(filter_rounds=1, max_reproj_error=0.0), b"max_reproj_error"), (dict(), dict(filter_rounds=4, max_reproj_error=nan), b"max_reproj_error"),
             (dict(), dict(filter_rounds=2, max_reproj_error=inf), b"max_reproj_error"), (dict(), dict(filter_rounds=1, max_reproj_error=-4.0), b"max_reproj_error"),
             (dict(flags=1), dict(), b"flag"), (dict(flags=2), dict(), b"flag"), (dict(flags=1 << 31), dict(), b"flag"),
             # the envelope of lg_bundle_adjust, under this entry point's name
             (dict(images=257), dict(), b"LG_BA_MAX_IMAGES"), (dict(images=0), dict(), b"images"), (dict(n=8193), dict(), b"LG_MAX_KEYPOINTS"),
             (dict(tracks=289), dict(), b"tracks"), (dict(num_iterations=0), dict(), b"num_iterations"), (dict(num_iterations=101), dict(), b"num_iterations"),
             (dict(initial_damping=nan), dict(), b"initial_damping"), (dict(function_tolerance=-1e-6), dict(), b"function_tolerance"),
             (dict(kpts=None), dict(), b"null pointer"), (dict(summary=None), dict(), b"null pointer"), (dict(workspace=None), dict(), b"null workspace"),
             (dict(workspace=264), dict(), b"aligned"), (dict(workspace_bytes=need - 1), dict(), b"lg_bundle_robust_workspace_bytes"),
             (dict(workspace_bytes=lib.lg_bundle_workspace_bytes(6, 96, 50, 0)), dict(), b"lg_bundle_robust_workspace_bytes")]
    for base, over, word in cases:
        io = _io(base, **over)
        assert lib.lg_bundle_adjust_robust(ctypes.byref(io), None) == inv, (base, over)
        assert word in lib.lg_last_error() and name in lib.lg_last_error(), (base, over, lib.lg_last_error())
    # a field the call does not read is not refused: the refusal that follows is the next one in line (here the workspace)
    for over in (dict(loss=0, loss_scale=0.0), dict(filter_rounds=0, max_reproj_error=nan)):
        io = _io(dict(workspace_bytes=0), **over)
        assert lib.lg_bundle_adjust_robust(ctypes.byref(io), None) == inv and b"workspace" in lib.lg_last_error(), over
    # lg_bundle_adjust still refuses any flag bit, under its own name
    io = _io(dict(flags=2))
    assert lib.lg_bundle_adjust(ctypes.byref(io.base), None) == inv and b"lg_bundle_adjust:" in lib.lg_last_error() and b"flag" in lib.lg_last_error()
