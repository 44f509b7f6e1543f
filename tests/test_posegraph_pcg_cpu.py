"""The global pose estimator's iterative solver without a GPU: the preconditions of the bars of tests/test_gpu_posegraph_pcg.py from the float64 definitions
alone (tests/posegraph_pcg_oracle.py, tests/posegraph_oracle.py) on every call that file makes, and the host layer (constructor, the ctypes mirror against
the header, the workspace formula, the refusals of the C entry point in their stated order).
  (a) at cg_tolerance = 1e-13 the iterative and the dense definition take the same decisions on every scene compared with the dense definition and differ
      by at most 1e-3 of a float32 ulp of the scale on R and t;
  (b) on every call the solves whose solver-iteration count moves with the accumulation order (`moving`) are at most a quarter of the solves, and none at
      the default tolerance;
  (c) no call's oracle run places p.q > 0, a block pivot or the solver's stop within a relative 1e-9 of its bar;
  (d) every budget leaves a quarter above the oracle's largest count, except where a test sets 1.
The figures are printed; the largest are in the docstring of tests/test_gpu_posegraph_pcg.py."""
import ctypes
import re

import numpy as np
import pytest
import torch

import posegraph_oracle as G
import posegraph_pcg_oracle as P
import triangulate_oracle as O
from lightglue_amd import GlobalPoseEstimator, _cabi
from test_cabi_symbols import HEADER, typed_fields_of

DECISIONS = ("origin", "baseline", "num_posed", "positions_ok")


def ulps(got, want):
    """the largest difference of two answers in float32 ulps of the scale: (R, t)"""
    dr = np.nan_to_num(abs(got["poses64"][:, :, :3] - want["poses64"][:, :, :3])).max() / O.ulp32(1.0)
    posed = want["image_state"] == G.POSED
    if not posed.any():
        return float(dr), 0.0
    scale = np.maximum(abs(want["poses64"][posed, :, 3]).max(1), abs(want["centres64"][posed]).max(1))
    dt = abs(got["poses64"][posed, :, 3] - want["poses64"][posed, :, 3]).max(1) / np.array([O.ulp32(s) for s in scale])
    return float(dr), float(dt.max())


# ---------------------------------------------------------------------- (a) the tight solve is the dense definition
@pytest.mark.parametrize("name", P.DENSE)
def test_tight_tolerance_meets_the_dense_definition(name):
    got, want = P.answer(name), P.dense_answer(name)
    for k in DECISIONS:
        assert got[k] == want[k], (name, k, got[k], want[k])
    assert (got["pair_state"] == want["pair_state"]).all() and (got["image_state"] == want["image_state"]).all(), name
    for stage in ("rotation", "position"):                  # a stage either definition marks as decided by rounding has no count to compare
        if stage not in got["near"] and stage not in want["near"]:
            assert got[stage + "_iterations"] == want[stage + "_iterations"], (name, stage)
    q = ulps(got, want)
    print("%s: iterative against dense, / ulp: R %.3g, t %.3g; iterations %d + %d (dense %d + %d); solver iterations at most %d / %d" % (
        (name,) + q + (got["rotation_iterations"], got["position_iterations"], want["rotation_iterations"], want["position_iterations"],
                       max(got["cg_counts"]["rotation"]), max(got["cg_counts"]["position"]))))
    assert max(q) <= 1e-3, (name, q)
    assert got["rotation_cg_unconverged"] == 0 and got["position_cg_unconverged"] == 0 and got["cg_failures"] == 0


# ---------------------------------------------------------------------- (b), (c), (d) on every call of the GPU file
@pytest.mark.parametrize("name", sorted(P.CALLS))
def test_preconditions_of_the_gpu_bars(name):
    conf, got = P.CALLS[name][1], P.answer(name)
    solves = len(got["cg_counts"]["rotation"]) + len(got["cg_counts"]["position"])
    print("%s: %d solves, %d moving %s, near %s, margins %s, largest counts %s / %s" % (
        name, solves, len(got["moving"]), got["moving"], got["near"], {k: "%.3g" % v for k, v in got["margins"].items()},
        max(got["cg_counts"]["rotation"] or [0]), max(got["cg_counts"]["position"] or [0])))
    assert 4 * len(got["moving"]) <= solves, (name, got["moving"])
    if conf.get("cg_tolerance", P.CG_TOLERANCE) == P.CG_TOLERANCE:
        assert got["moving"] == [], (name, got["moving"])
    assert min(got["margins"].values()) > 1e-9, (name, got["margins"])
    for stage, default in (("rotation", P.ROTATION_CG_ITERATIONS), ("position", P.POSITION_CG_ITERATIONS)):
        budget = conf.get(stage + "_cg_iterations", default)
        for run in (got, got["other"]):
            if budget > 1:
                assert 1.25 * max(run["cg_counts"][stage] or [0]) <= budget and run[stage + "_cg_unconverged"] == 0, (name, stage, run["cg_counts"][stage])
            else:
                assert run["cg_counts"][stage] == [1] * run[stage + "_iterations"] == [1] * 12 and run[stage + "_cg_unconverged"] == 12
    assert 12 * (conf.get("rotation_cg_iterations", 64) + conf.get("position_cg_iterations", 800)) <= P.MAX_SOLVER_ITERATIONS


def test_issue_counts_and_the_big_scene():
    """the solver-iteration counts the issue measured, and the 1 100-image scene against the truth"""
    assert (max(P.answer("K16 default")["cg_counts"]["rotation"]), max(P.answer("K16 default")["cg_counts"]["position"])) == (12, 41)
    assert (max(P.answer("K16 tight")["cg_counts"]["rotation"]), max(P.answer("K16 tight")["cg_counts"]["position"])) == (15, 42)
    assert (max(P.answer("K49 tight")["cg_counts"]["rotation"]), max(P.answer("K49 tight")["cg_counts"]["position"])) == (30, 130)
    big, sc = P.answer("big"), P.CALLS["big"][0]()
    assert len(sc["pairs"]) == 8800 and big["num_posed"] == 1100 and big["positions_ok"] and (big["pair_state"] == G.USED).all()
    assert (max(big["cg_counts"]["rotation"]), max(big["cg_counts"]["position"])) == (18, 401)
    rot, centre = G.against_truth(big, sc)
    print("K = 1100: rotation %.3f degrees, centres %.4f of the extent off the truth" % (rot, centre))      # measured: 0.17 degrees, 0.25 %
    assert rot < 1.0 and centre < 0.01
    hub = P.CALLS["hub tight"][0]()
    lengths = np.bincount(hub["pairs"].ravel(), minlength=300)
    assert lengths[hub["hub"]] == 300 and len({tuple(sorted(p)) for p in hub["pairs"].tolist()}) == len(hub["pairs"]) - 1
    edge = P.answer("no baseline")
    assert edge["baseline"] == -1 and not edge["positions_ok"] and edge["position_iterations"] == 0 and edge["position_cg_iterations"] == 0
    co = P.answer("collinear")
    assert not co["positions_ok"] and (co["image_state"] == G.ROTATION_ONLY).all() and co["cg_failures"] == 1


# ---------------------------------------------------------------------- the host layer
def test_constructor_validates_like_the_c_side():
    est = GlobalPoseEstimator()
    assert (est.solver, est.rotation_cg_iterations, est.position_cg_iterations, est.cg_tolerance) == ("cholesky", None, None, None)
    GlobalPoseEstimator(solver="cholesky", rotation_cg_iterations=0, position_cg_iterations=-3, cg_tolerance=7.0)        # read with "pcg" only
    ok = GlobalPoseEstimator(solver="pcg")
    assert (ok.solver, ok.rotation_cg_iterations, ok.position_cg_iterations, ok.cg_tolerance) == ("pcg", 64, 800, 1e-6)
    assert (P.ROTATION_CG_ITERATIONS, P.POSITION_CG_ITERATIONS, P.CG_TOLERANCE) == (64, 800, 1e-6)
    nan = float("nan")
    for bad, word in ((dict(solver="cg"), "solver"), (dict(solver=None), "solver"), (dict(solver="pcg", rotation_cg_iterations=0), "rotation_cg_iterations"),
                      (dict(solver="pcg", rotation_cg_iterations=1001), "rotation_cg_iterations"), (dict(solver="pcg", position_cg_iterations=0), "position_cg_iterations"),
                      (dict(solver="pcg", position_cg_iterations=1001), "position_cg_iterations"), (dict(solver="pcg", position_cg_iterations=2.5), "position_cg_iterations"),
                      (dict(solver="pcg", rotation_cg_iterations=True), "rotation_cg_iterations"), (dict(solver="pcg", cg_tolerance=0.0), "cg_tolerance"),
                      (dict(solver="pcg", cg_tolerance=1.0), "cg_tolerance"), (dict(solver="pcg", cg_tolerance=nan), "cg_tolerance"),
                      (dict(solver="pcg", cg_tolerance=-1e-6), "cg_tolerance"), (dict(solver="pcg", cg_tolerance="loose"), "cg_tolerance"),
                      (dict(solver="pcg", cg_tolerance=None), "cg_tolerance"), (dict(solver="pcg", num_iterations=24), "20000"),       # 24 x 864 = 20 736
                      (dict(solver="pcg", num_iterations=100, rotation_cg_iterations=100, position_cg_iterations=101), "20000"),
                      (dict(solver="pcg", num_iterations=5), "num_iterations")):
        with pytest.raises(ValueError, match=word):
            GlobalPoseEstimator(**bad)
    GlobalPoseEstimator(solver="pcg", num_iterations=100, rotation_cg_iterations=100, position_cg_iterations=100)           # 20 000 exactly
    GlobalPoseEstimator(solver="pcg", num_iterations=23)                                                                    # 19 872


def test_num_images_bound_follows_the_solver():
    sc = G.scene(6)
    pairs, R, t = (torch.from_numpy(np.ascontiguousarray(sc[k])) for k in ("pairs", "R", "t"))
    # the dense solver's refusal keeps its words (tests/test_geometry_call_cpu.py compares them whole): it names LG_BA_MAX_IMAGES by its value
    dense, wide = r"num_images must be an integer in \[2, %d\]" % _cabi.LG_BA_MAX_IMAGES, r"num_images must be an integer in \[2, %d\]" % _cabi.LG_BA_PCG_MAX_IMAGES
    with pytest.raises(ValueError, match=dense + ", got 300"):
        GlobalPoseEstimator(solver="cholesky").estimate(pairs, (R, t), 300)
    with pytest.raises(ValueError, match=dense + ", got 257"):
        GlobalPoseEstimator().estimate(pairs, (R, t), 257)
    with pytest.raises(ValueError, match=wide + ", got 4097"):
        GlobalPoseEstimator(solver="pcg").estimate(pairs, (R, t), 4097)
    for K in (300, 4096):                                   # every check passes: the device is refused, nothing else runs
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            GlobalPoseEstimator(solver="pcg").estimate(pairs, (R, t), K)


def test_mirror_symbols_and_constants_match_the_header():
    scalars = {"int32_t": ctypes.c_int32, "double": ctypes.c_double, "lg_posegraph_io": _cabi.LgPosegraphIO}
    want = [(f, scalars[t]) for f, t, ptr in typed_fields_of("lg_posegraph_pcg_io") if not ptr]
    assert want == list(_cabi.LgPosegraphPcgIO._fields_)
    assert [f for f, _ in want] == ["base", "rotation_cg_iterations", "position_cg_iterations", "cg_tolerance"]
    assert {"lg_posegraph_pcg_workspace_bytes", "lg_posegraph_solve_pcg"} <= set(_cabi.EXPORTED_SYMBOLS)
    assert (P.MAX_IMAGES, P.MAX_CG, P.MAX_SOLVER_ITERATIONS) == (_cabi.LG_BA_PCG_MAX_IMAGES, _cabi.LG_BA_PCG_MAX_CG_ITERATIONS, _cabi.LG_BA_PCG_MAX_SOLVER_ITERATIONS)
    assert re.search(r"\bint lg_posegraph_solve_pcg\(const lg_posegraph_pcg_io\* io, void\* hip_stream\);", HEADER)
    assert re.search(r"\bint64_t lg_posegraph_pcg_workspace_bytes\(int64_t images, int64_t pairs, uint32_t flags\);", HEADER)
    assert ctypes.sizeof(_cabi.LgPosegraphPcgIO) == ctypes.sizeof(_cabi.LgPosegraphIO) + 16


def header_workspace_bytes(K, P_):
    """the header's words: lg_posegraph_solve's workspace without the dense system, a 256-byte record, 48 bytes per pair, 256 bytes per image in nine
    pieces; every piece rounded up to 256 bytes"""
    up = lambda b: (b + 255) // 256 * 256
    dense_without_S = 256 + up(K * 72) + up(K * 24) + 4 * up(K * 4) + up((K + 1) * 4) + up(P_ * 4) + up(P_ * 8) + up(P_ * 24) + up(P_ * 16)
    if K <= 256:
        assert dense_without_S == _cabi.load().lg_posegraph_workspace_bytes(K, P_, 0) - up((3 * K + 1) * 3 * K * 8)
    return dense_without_S + 256 + up(P_ * 48) + 5 * up(K * 24) + up(K * 48) + up(K * 72) + 2 * up(K * 8)


def test_workspace_is_the_headers_formula():
    size = _cabi.load().lg_posegraph_pcg_workspace_bytes
    for K, P_ in ((6, 15), (2, 1), (256, 1024), (300, 1200), (1100, 8800), (4096, 2 ** 20), (4096, 1)):
        assert size(K, P_, 0) == header_workspace_bytes(K, P_), (K, P_)
        assert abs(size(K, P_, 0) - (512 + 372 * K + 4 + 100 * P_)) <= 22 * 256                            # the sum before the rounding of its 22 pieces
    assert size(4096, 2 ** 20, 0) < 2 ** 27                                                                # no dense system: 3 x 4096 unknowns would be 1.2 GB
    for args in ((1, 15, 0), (0, 15, 0), (4097, 15, 0), (6, 0, 0), (6, -1, 0), (6, 2 ** 20 + 1, 0), (6, 15, 1), (6, 15, 1 << 31)):
        assert size(*args) == -1, args
    dense = _cabi.load().lg_posegraph_workspace_bytes
    assert dense(257, 15, 0) == -1 and size(257, 15, 0) > 0                                                # the dense bound stays where it was


def _io(base=None, **over):
    """a well-formed io, every pointer a fake non-null value: a refusal comes before anything is dereferenced"""
    lib = _cabi.load()
    K, P_ = 6, 15
    fields = dict(images=K, pairs=P_, flags=0, num_iterations=12, origin=0, baseline=-1, min_inliers=15, rotation_scale=5.0, max_rotation_error=15.0,
                  direction_scale=5.0, workspace=256, workspace_bytes=lib.lg_posegraph_pcg_workspace_bytes(K, P_, 0))
    fields.update({f: 256 for f, t in _cabi.LgPosegraphIO._fields_ if t is ctypes.c_void_p and f not in ("workspace", "num_inliers")})
    fields.update(base or {})
    top = dict(rotation_cg_iterations=64, position_cg_iterations=800, cg_tolerance=1e-6)
    top.update(over)
    return _cabi.LgPosegraphPcgIO(base=_cabi.LgPosegraphIO(**fields), **top)


def test_envelope_is_refused_in_the_stated_order_without_touching_a_gpu():
    lib = _cabi.load()
    inv, name = _cabi.LG_ERR_INVALID, b"lg_posegraph_solve_pcg"
    assert lib.lg_posegraph_solve_pcg(None, None) == inv and b"null io" in lib.lg_last_error() and name in lib.lg_last_error()
    need = lib.lg_posegraph_pcg_workspace_bytes(6, 15, 0)
    nan, inf = float("nan"), float("inf")
    cases = [(dict(flags=1), dict(), b"flag"), (dict(images=4097), dict(), b"LG_BA_PCG_MAX_IMAGES"), (dict(images=1), dict(), b"images"),
             (dict(pairs=0), dict(), b"pairs"), (dict(pairs=2 ** 20 + 1), dict(), b"pairs"), (dict(num_iterations=5), dict(), b"num_iterations"),
             (dict(num_iterations=101), dict(rotation_cg_iterations=1, position_cg_iterations=1), b"num_iterations"), (dict(origin=6), dict(), b"origin"),
             (dict(baseline=0), dict(), b"baseline"), (dict(rotation_scale=0.0), dict(), b"rotation_scale"), (dict(max_rotation_error=nan), dict(), b"max_rotation_error"),
             (dict(direction_scale=inf), dict(), b"direction_scale"),
             (dict(), dict(rotation_cg_iterations=0), b"rotation_cg_iterations"), (dict(), dict(rotation_cg_iterations=1001), b"rotation_cg_iterations"),
             (dict(), dict(position_cg_iterations=0), b"position_cg_iterations"), (dict(), dict(position_cg_iterations=-1), b"position_cg_iterations"),
             (dict(), dict(position_cg_iterations=1001), b"position_cg_iterations"),
             (dict(), dict(cg_tolerance=0.0), b"cg_tolerance"), (dict(), dict(cg_tolerance=1.0), b"cg_tolerance"), (dict(), dict(cg_tolerance=nan), b"cg_tolerance"),
             (dict(), dict(cg_tolerance=inf), b"cg_tolerance"), (dict(), dict(cg_tolerance=-1e-6), b"cg_tolerance"),
             (dict(num_iterations=24), dict(), b"LG_BA_PCG_MAX_SOLVER_ITERATIONS"),                                                # 24 x 864 = 20 736
             (dict(num_iterations=100), dict(rotation_cg_iterations=100, position_cg_iterations=101), b"LG_BA_PCG_MAX_SOLVER_ITERATIONS"),
             (dict(pair_index=None), dict(), b"null pointer"), (dict(summary=None), dict(), b"null pointer"), (dict(workspace=None), dict(), b"null workspace"),
             (dict(workspace=264), dict(), b"aligned"), (dict(workspace_bytes=need - 1), dict(), b"lg_posegraph_pcg_workspace_bytes"),
             # the stated order: of two faults the earlier one is named
             (dict(flags=1, images=4097), dict(), b"flag"), (dict(images=4097, pairs=0), dict(), b"LG_BA_PCG_MAX_IMAGES"), (dict(pairs=0, num_iterations=5), dict(), b"pairs"),
             (dict(direction_scale=0.0), dict(rotation_cg_iterations=0), b"direction_scale"),
             (dict(), dict(rotation_cg_iterations=0, position_cg_iterations=0), b"rotation_cg_iterations"),
             (dict(), dict(position_cg_iterations=0, cg_tolerance=0.0), b"position_cg_iterations"),
             (dict(num_iterations=24), dict(cg_tolerance=2.0), b"cg_tolerance"), (dict(num_iterations=24, poses=None), dict(), b"LG_BA_PCG_MAX_SOLVER_ITERATIONS"),
             (dict(poses=None, workspace=None), dict(), b"null pointer")]
    for base, over, word in cases:
        io = _io(base, **over)
        assert lib.lg_posegraph_solve_pcg(ctypes.byref(io), None) == inv, (base, over)
        assert word in lib.lg_last_error() and name in lib.lg_last_error(), (base, over, lib.lg_last_error())
    # 20 000 solver iterations exactly and 4 096 images pass every check up to the workspace
    for base, over in ((dict(num_iterations=100, workspace_bytes=0), dict(rotation_cg_iterations=100, position_cg_iterations=100)),
                       (dict(images=4096, workspace_bytes=0), dict()), (dict(images=257, workspace_bytes=0), dict())):
        io = _io(base, **over)
        assert lib.lg_posegraph_solve_pcg(ctypes.byref(io), None) == inv and b"workspace holds" in lib.lg_last_error(), (base, over, lib.lg_last_error())
    # the dense entry point keeps its bound and its words
    io = _io(dict(images=257))
    assert lib.lg_posegraph_solve(ctypes.byref(io.base), None) == inv and lib.lg_last_error() == b"lg_posegraph_solve: images must lie in [2, LG_BA_MAX_IMAGES]"


def test_cholesky_builds_the_io_it_always_built(monkeypatch):
    """solver="cholesky" reaches the entry point a call without the argument reaches, with the same struct and an 8-entry summary; "pcg" wraps it once more"""
    from lightglue_amd import _call
    seen = []

    def device_call(device, entry, sizer, size_args, make_io, **kw):
        io = make_io(256, 0)
        seen.append((entry, sizer, size_args, type(io), bytes(io)))
        raise RuntimeError("stop before the device")
    monkeypatch.setattr(_call, "device_call", device_call)
    monkeypatch.setattr(_call, "require_gpu", lambda *a, **k: None)
    sc = G.scene(6)
    pairs, R, t = (torch.from_numpy(np.ascontiguousarray(sc[k])) for k in ("pairs", "R", "t"))
    for conf in (dict(), dict(solver="cholesky"), dict(solver="pcg", rotation_cg_iterations=7, position_cg_iterations=9, cg_tolerance=1e-9)):
        with pytest.raises(RuntimeError, match="stop before"):
            GlobalPoseEstimator(**conf).estimate(pairs, (R, t), 6)
    plain, chol, pcg = seen
    assert plain[:4] == chol[:4] == ("lg_posegraph_solve", "lg_posegraph_workspace_bytes", (6, 15, 0), _cabi.LgPosegraphIO)
    assert pcg[:4] == ("lg_posegraph_solve_pcg", "lg_posegraph_pcg_workspace_bytes", (6, 15, 0), _cabi.LgPosegraphPcgIO)
    head = _cabi.LgPosegraphIO.pair_index.offset             # the settings in front of the first pointer are the same bytes
    assert plain[4][:head] == chol[4][:head] == pcg[4][:head]
    io = _cabi.LgPosegraphPcgIO.from_buffer_copy(pcg[4])
    assert (io.rotation_cg_iterations, io.position_cg_iterations, io.cg_tolerance, io.base.num_iterations) == (7, 9, 1e-9, 12)
