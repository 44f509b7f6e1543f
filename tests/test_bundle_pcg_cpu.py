"""The bundle adjuster's iterative solver without a GPU: the preconditions of the bars of tests/test_gpu_bundle_pcg.py from the float64 definition alone
(tests/bundle_pcg_oracle.py) on every scene that file uses, and the host layer (constructor, the ctypes mirror against the header, the workspace formula, the
refusals of the C entry point).
  (a) at cg_tolerance = 1e-13, under a budget the oracle never hits, the iterative and the dense definition (Schur complement + Cholesky) agree on every
      integer and decision and differ by less than 1e-3 of the one-float32-ulp scale on points, t and R;
  (b) at the default tolerance the iterative oracle moves by less than 1e-3 of that ulp between ascending and descending accumulation, and marks no
      decision within a relative 1e-9 of its bar.
The figures are printed; the largest are in the docstring of tests/test_gpu_bundle_pcg.py."""
import ctypes
import re

import numpy as np
import pytest

import bundle_oracle as B
import bundle_pcg_oracle as P
import bundle_robust_oracle as R
import triangulate_oracle as O
from lightglue_amd import BundleAdjuster, _cabi
from test_cabi_symbols import HEADER, typed_fields_of

DECISIONS = ("num_observations", "num_iterations", "num_accepted", "converged")


def ulps(name, inp, a, b):
    """the largest difference of two answers in float32 ulps of the scale: (points, t, R)"""
    track, image = (R.scales if "first_state" in b else B.scales)(inp, b)
    pu, tu = np.array([O.ulp32(s) for s in track]), np.array([O.ulp32(s) for s in image])
    adj = b["adjusted"]
    dx = abs(a["xyz64"] - b["xyz64"]).max(1)
    dt = abs(a["poses64"][:, :, 3] - b["poses64"][:, :, 3]).max(1)
    dr = abs(a["poses64"][:, :, :3] - b["poses64"][:, :, :3]).max()
    return float((dx[adj] / pu[adj]).max()), float((dt / tu).max()), float(dr / O.ulp32(1.0))


def same_decisions(a, b, what):
    for k in DECISIONS:
        assert a[k] == b[k], (what, k, a[k], b[k])
    assert (a["node_state"] == b["node_state"]).all() and (a["status"] == b["status"]).all() and (a["free"] == b["free"]).all(), what
    assert (a["adjusted"] == b["adjusted"]).all() and len(a["costs"]) == len(b["costs"]), what
    for k in ("num_filtered", "num_filter_stages"):
        assert a.get(k, 0) == b.get(k, 0), (what, k)


# ---------------------------------------------------------------------- (a) the tight solve is the dense definition
@pytest.mark.parametrize("name", sorted(P.TIGHT_CALLS))
def test_tight_tolerance_meets_the_dense_definition(name):
    conf, inp = P.TIGHT_CALLS[name], P.SCENES[name]()
    got, want = P.answer(name, **conf), P.dense_answer(name)
    assert got["near"] == [] and want["near"] == [], (name, got["near"], want["near"])
    same_decisions(got, want, name)
    assert abs(got["final_cost"] - want["final_cost"]) <= 1e-9 * want["final_cost"]
    q = ulps(name, inp, got, want)
    print("%s: iterative against dense, / ulp: points %.3g, t %.3g, R %.3g; solver iterations %s" % ((name,) + q + (got["cg_counts"],)))
    assert max(q) < 1e-3, (name, q)
    # the budget is never hit, with a quarter to spare, and the recorded count is the oracle's
    assert got["cg_unconverged"] == 0 and max(got["cg_counts"]) == P.COUNTS["tight"][name] and 1.25 * max(got["cg_counts"]) <= conf["max_cg_iterations"], got["cg_counts"]
    assert got["cg_iterations"] == sum(got["cg_counts"]) and len(got["cg_counts"]) == got["num_iterations"]
    # not a precondition, a figure: at 1e-13 a solve ends near the rounding floor of its recurrences, where the residual stalls for a few iterations, so the
    # other accumulation order may stop a solve some iterations earlier or later (the 300-image scene: 107 instead of 103 in its second solve) while the
    # answers stay within the figures above.  The counts of tests/test_gpu_bundle_pcg.py at 1e-13 are therefore those of the definition's own order, which
    # tests/bundle_pcg_oracle.py follows operation by operation
    print("%s: solver iterations with descending accumulation %s" % (name, P.answer(name, order="descending", **conf)["cg_counts"]))


# ---------------------------------------------------------------------- (b) the default tolerance: the orders are worth nothing, no decision is near its bar
@pytest.mark.parametrize("name", sorted(P.DEFAULT_CALLS))
def test_default_tolerance_does_not_depend_on_the_order(name):
    conf, inp = P.DEFAULT_CALLS[name], P.SCENES[name]()
    up, down = P.answer(name, **conf), P.answer(name, order="descending", **conf)
    assert up["near"] == [] and down["near"] == [], (name, up["near"], down["near"])
    same_decisions(up, down, name)
    assert up["accepts"] == down["accepts"] and up["cg_counts"] == down["cg_counts"], (name, up["cg_counts"], down["cg_counts"])
    q = ulps(name, inp, down, up)
    print("%s: descending against ascending, / ulp: points %.3g, t %.3g, R %.3g; solver iterations %s" % ((name,) + q + (up["cg_counts"],)))
    assert max(q) < 1e-3, (name, q)
    budget = conf.get("max_cg_iterations", P.MAX_CG_ITERATIONS)
    assert up["cg_unconverged"] == 0 and max(up["cg_counts"]) == P.COUNTS["default"][name] and 1.25 * max(up["cg_counts"]) <= budget
    # the looser solve takes fewer solver iterations than the tight one and still ends at the dense definition's cost
    tight = P.answer(name, **P.TIGHT_CALLS[name])
    assert up["cg_iterations"] < tight["cg_iterations"] and abs(up["final_cost"] - tight["final_cost"]) <= 1e-6 * tight["final_cost"]


def test_a_budget_of_one_is_counted_and_still_descends():
    one = P.answer("main", max_cg_iterations=1)
    assert one["near"] == [] and one["cg_counts"] == [1] * one["num_iterations"] and one["cg_unconverged"] == one["num_iterations"] == 10
    assert all(one["accepts"]) and one["final_cost"] < 0.02 * one["initial_cost"] and np.isfinite(one["poses64"]).all() and np.isfinite(one["xyz64"]).all()
    # precondition (b) of the one-ulp bar for this call too
    down = P.answer("main", max_cg_iterations=1, order="descending")
    assert down["near"] == [] and down["accepts"] == one["accepts"] and down["cg_counts"] == one["cg_counts"]
    same_decisions(one, down, "main, one solver iteration")
    q = ulps("main", P.SCENES["main"](), down, one)
    print("main, one solver iteration: descending against ascending, / ulp: points %.3g, t %.3g, R %.3g" % q)
    assert max(q) < 1e-3, q


def test_big_scene_is_the_recipe():
    inp, want = P.big_scene(), P.dense_big()
    assert inp["kpts"].shape[:2] == (300, 32) and len(inp["xyz"]) == 1200 and 300 > _cabi.LG_BA_MAX_IMAGES
    assert want["num_observations"] == 4171 and int(want["free"].sum()) == 298 and want["num_accepted"] == 4
    per_image = (want["node_state"] == B.ACTIVE).sum(1)
    assert per_image.min() == 4 and per_image.max() == 22
    assert 106467 < want["initial_cost"] < 106468 and 744 < want["final_cost"] < 746


# ---------------------------------------------------------------------- the host layer
def test_constructor_validates_like_the_c_side():
    ba = BundleAdjuster()
    assert (ba.solver, ba.max_cg_iterations, ba.cg_tolerance) == ("cholesky", None, None)
    assert BundleAdjuster(solver="cholesky").robust == ba.robust and BundleAdjuster(solver="cholesky", max_cg_iterations=0, cg_tolerance=7.0).robust == ba.robust
    ok = BundleAdjuster(solver="pcg")
    assert (ok.solver, ok.max_cg_iterations, ok.cg_tolerance) == ("pcg", 100, 1e-6) == ("pcg", P.MAX_CG_ITERATIONS, P.CG_TOLERANCE)
    ok = BundleAdjuster(solver="pcg", max_cg_iterations=1000, cg_tolerance=1e-13, loss="cauchy", filter_rounds=1, num_iterations=10)
    assert (ok.max_cg_iterations, ok.cg_tolerance, ok.loss, ok.filter_rounds) == (1000, 1e-13, "cauchy", 1)
    nan = float("nan")
    for bad, word in ((dict(solver="cg"), "solver"), (dict(solver=None), "solver"), (dict(solver="pcg", max_cg_iterations=0), "max_cg_iterations"),
                      (dict(solver="pcg", max_cg_iterations=1001), "max_cg_iterations"), (dict(solver="pcg", max_cg_iterations=2.5), "max_cg_iterations"),
                      (dict(solver="pcg", max_cg_iterations=True), "max_cg_iterations"), (dict(solver="pcg", cg_tolerance=0.0), "cg_tolerance"),
                      (dict(solver="pcg", cg_tolerance=1.0), "cg_tolerance"), (dict(solver="pcg", cg_tolerance=nan), "cg_tolerance"),
                      (dict(solver="pcg", cg_tolerance=-1e-6), "cg_tolerance"), (dict(solver="pcg", refine_focal=True), "refine_focal"),
                      (dict(solver="pcg", num_iterations=100, max_cg_iterations=201), "20000"),
                      (dict(solver="pcg", num_iterations=59, filter_rounds=2, max_reproj_error=4.0, max_cg_iterations=113), "20000"),        # 20 001
                      (dict(solver="pcg", cg_tolerance="loose"), "cg_tolerance"), (dict(solver="pcg", cg_tolerance=None), "cg_tolerance"),
                      (dict(solver="pcg", num_iterations=100, filter_rounds=1, max_reproj_error=4.0, max_cg_iterations=101), "20000")):
        with pytest.raises(ValueError, match=word):
            BundleAdjuster(**bad)
    BundleAdjuster(solver="pcg", num_iterations=100, max_cg_iterations=200)             # 20 000 exactly


def test_mirror_symbols_and_constants_match_the_header():
    scalars = {"int32_t": ctypes.c_int32, "double": ctypes.c_double, "lg_bundle_robust_io": _cabi.LgBundleRobustIO}
    want = [(f, scalars[t]) for f, t, ptr in typed_fields_of("lg_bundle_pcg_io") if not ptr]
    assert want == list(_cabi.LgBundlePcgIO._fields_) and [f for f, _ in want] == ["base", "max_cg_iterations", "pad", "cg_tolerance"]
    assert {"lg_bundle_pcg_workspace_bytes", "lg_bundle_adjust_pcg"} <= set(_cabi.EXPORTED_SYMBOLS)
    for name, value in (("LG_BA_PCG_MAX_IMAGES", _cabi.LG_BA_PCG_MAX_IMAGES), ("LG_BA_PCG_MAX_CG_ITERATIONS", _cabi.LG_BA_PCG_MAX_CG_ITERATIONS),
                        ("LG_BA_PCG_MAX_SOLVER_ITERATIONS", _cabi.LG_BA_PCG_MAX_SOLVER_ITERATIONS), ("LG_BA_MAX_IMAGES", _cabi.LG_BA_MAX_IMAGES)):
        assert int(re.search(r"#define %s (\d+)" % name, HEADER).group(1)) == value, name
    assert (P.MAX_IMAGES, P.MAX_CG, P.MAX_SOLVER_ITERATIONS) == (4096, 1000, 20000) == (_cabi.LG_BA_PCG_MAX_IMAGES, _cabi.LG_BA_PCG_MAX_CG_ITERATIONS,
                                                                                       _cabi.LG_BA_PCG_MAX_SOLVER_ITERATIONS)
    assert re.search(r"\bint lg_bundle_adjust_pcg\(const lg_bundle_pcg_io\* io, void\* hip_stream\);", HEADER)
    assert ctypes.sizeof(_cabi.LgBundlePcgIO) == ctypes.sizeof(_cabi.LgBundleRobustIO) + 16


def header_workspace_bytes(K, N, T):
    """the header's words: lg_bundle_adjust_robust's workspace without S, a 256-byte record, 784 bytes per image in eight pieces, 24 bytes per track; every
    piece rounded up to 256 bytes"""
    up = lambda b: (b + 255) // 256 * 256
    lib = _cabi.load()
    robust_without_S = lib.lg_bundle_robust_workspace_bytes(min(K, 256), N, T, 0) - up((6 * min(K, 256) + 1) * 6 * min(K, 256) * 8) if K <= 256 else None
    pieces = (256 + up(K * 64) + up(K * 192) + up(K * 48) + up(K * 8) + 2 * up(K * N * 4) + 3 * up(T * 4) + up(T * 48) + up(T * 72) + up(T * 24) + up(T * 4))
    assert robust_without_S is None or robust_without_S == pieces
    return pieces + 256 + 4 * up(K * 48) + 2 * up(K * 288) + 2 * up(K * 8) + up(T * 24)


def _io(base=None, **over):
    """a well-formed io, every pointer a fake non-null value: a refusal comes before anything is dereferenced"""
    lib = _cabi.load()
    K, N, T = 6, 96, 50
    fields = dict(n=N, images=K, tracks=T, flags=0, num_iterations=10, initial_damping=1e-4, function_tolerance=1e-6, workspace=256,
                  workspace_bytes=lib.lg_bundle_pcg_workspace_bytes(K, N, T, 0))
    fields.update({f: 256 for f, t in _cabi.LgBundleIO._fields_ if t is ctypes.c_void_p and f not in ("workspace", "num")})
    fields.update(base or {})
    top = dict(max_cg_iterations=100, pad=0, cg_tolerance=1e-6, loss=2, loss_scale=2.0, filter_rounds=1, max_reproj_error=4.0)
    top.update(over)
    robust = {k: top.pop(k) for k in ("loss", "loss_scale", "filter_rounds", "max_reproj_error")}
    return _cabi.LgBundlePcgIO(base=_cabi.LgBundleRobustIO(base=_cabi.LgBundleIO(**fields), **robust), **top)


def test_workspace_is_the_headers_formula():
    size = _cabi.load().lg_bundle_pcg_workspace_bytes
    for K, N, T in ((6, 96, 50), (1, 0, 0), (256, 32, 1000), (300, 32, 1200), (4096, 512, 100000), (4096, 1, 0)):
        assert size(K, N, T, 0) == header_workspace_bytes(K, N, T), (K, N, T)
    assert size(4096, 512, 100000, 0) < 2 ** 27                                          # no S: 6 x 4096 unknowns would be 4.8 GB dense
    for args in ((0, 96, 0, 0), (4097, 8, 4, 0), (4096, 513, 4, 0), (6, 8193, 4, 0), (6, 96, 289, 0), (6, 96, -1, 0), (6, 96, 50, 1), (6, 96, 50, 1 << 31)):
        assert size(*args) == -1, args
    dense = _cabi.load().lg_bundle_robust_workspace_bytes
    assert dense(257, 8, 4, 0) == -1 and size(257, 8, 4, 0) > 0                          # the dense bound stays where it was


def test_envelope_is_refused_without_touching_a_gpu():
    lib = _cabi.load()
    inv, name = _cabi.LG_ERR_INVALID, b"lg_bundle_adjust_pcg"
    assert lib.lg_bundle_adjust_pcg(None, None) == inv and b"null io" in lib.lg_last_error() and name in lib.lg_last_error()
    need = lib.lg_bundle_pcg_workspace_bytes(6, 96, 50, 0)
    nan, inf = float("nan"), float("inf")
    cases = [(dict(images=4097, n=8, tracks=4), dict(), b"LG_BA_PCG_MAX_IMAGES"), (dict(images=0), dict(), b"images"),
             (dict(images=4096, n=513, tracks=4), dict(), b"LG_MAX_ROWS"),
             (dict(), dict(max_cg_iterations=0), b"max_cg_iterations"), (dict(), dict(max_cg_iterations=1001), b"max_cg_iterations"),
             (dict(), dict(max_cg_iterations=-1), b"max_cg_iterations"),
             (dict(num_iterations=100), dict(filter_rounds=0, max_cg_iterations=201), b"LG_BA_PCG_MAX_SOLVER_ITERATIONS"),           # 20 100
             (dict(num_iterations=67), dict(filter_rounds=2, max_cg_iterations=100), b"LG_BA_PCG_MAX_SOLVER_ITERATIONS"),            # 20 100
             (dict(num_iterations=59), dict(filter_rounds=2, max_cg_iterations=113), b"LG_BA_PCG_MAX_SOLVER_ITERATIONS"),            # 59 x 3 x 113 = 20 001
             (dict(num_iterations=1), dict(filter_rounds=0, max_cg_iterations=1000, cg_tolerance=0.0), b"cg_tolerance"),
             (dict(), dict(cg_tolerance=0.0), b"cg_tolerance"), (dict(), dict(cg_tolerance=1.0), b"cg_tolerance"), (dict(), dict(cg_tolerance=nan), b"cg_tolerance"),
             (dict(), dict(cg_tolerance=inf), b"cg_tolerance"), (dict(), dict(cg_tolerance=-1e-6), b"cg_tolerance"),
             (dict(), dict(pad=1), b"pad"), (dict(), dict(pad=-1), b"pad"),
             # the envelope of lg_bundle_adjust_robust, under this entry point's name
             (dict(), dict(loss=3), b"loss must"), (dict(), dict(filter_rounds=5), b"filter_rounds"), (dict(flags=1), dict(), b"flag"),
             (dict(n=8193), dict(), b"LG_MAX_KEYPOINTS"), (dict(tracks=289), dict(), b"tracks"), (dict(num_iterations=0), dict(), b"num_iterations"),
             (dict(num_iterations=101), dict(max_cg_iterations=1), b"num_iterations"), (dict(initial_damping=nan), dict(), b"initial_damping"),
             (dict(kpts=None), dict(), b"null pointer"), (dict(workspace=None), dict(), b"null workspace"), (dict(workspace=264), dict(), b"aligned"),
             (dict(workspace_bytes=need - 1), dict(), b"lg_bundle_pcg_workspace_bytes")]
    for base, over, word in cases:
        io = _io(base, **over)
        assert lib.lg_bundle_adjust_pcg(ctypes.byref(io), None) == inv, (base, over)
        assert word in lib.lg_last_error() and name in lib.lg_last_error(), (base, over, lib.lg_last_error())
    # 20 000 solver iterations exactly and 257 images pass every check up to the workspace
    for base, over in ((dict(num_iterations=100, workspace_bytes=0), dict(filter_rounds=0, max_cg_iterations=200)),
                       (dict(images=257, n=8, tracks=4, workspace_bytes=0), dict())):
        io = _io(base, **over)
        assert lib.lg_bundle_adjust_pcg(ctypes.byref(io), None) == inv and b"workspace holds" in lib.lg_last_error(), (base, over, lib.lg_last_error())
    # the three dense entry points keep their bound and their words
    io = _io(dict(images=257, n=8, tracks=4))
    for call, arg, word in ((lib.lg_bundle_adjust, io.base.base, b"lg_bundle_adjust: images must lie in [1, LG_BA_MAX_IMAGES]"),
                            (lib.lg_bundle_adjust_robust, io.base, b"lg_bundle_adjust_robust: images must lie in [1, LG_BA_MAX_IMAGES]")):
        assert call(ctypes.byref(arg), None) == inv and lib.lg_last_error() == word, lib.lg_last_error()
    focal = _cabi.LgBundleFocalIO(base=io.base, constant_camera=None, cameras_out=256)
    assert lib.lg_bundle_adjust_focal(ctypes.byref(focal), None) == inv and lib.lg_last_error() == b"lg_bundle_adjust_focal: images must lie in [1, LG_BA_MAX_IMAGES]"


def test_cholesky_builds_the_io_it_always_built(monkeypatch):
    """solver="cholesky" reaches the entry points a call without the argument reaches, with the same struct, and "pcg" wraps the robust struct once more"""
    import torch

    from lightglue_amd import _call
    seen = []

    def device_call(device, entry, sizer, size_args, make_io, **kw):
        io = make_io(256, 0)
        seen.append((entry, sizer, size_args, type(io), bytes(io)))
        raise RuntimeError("stop before the device")
    monkeypatch.setattr(_call, "device_call", device_call)
    monkeypatch.setattr(_call, "require_gpu", lambda *a, **k: None)
    monkeypatch.setattr(_call, "summary_status", lambda n, K, device: (torch.zeros(K, dtype=torch.int32), 512, 768, lambda: None))
    inp = B.GPU_SCENES["main"]()
    feats = {"keypoints": torch.from_numpy(inp["kpts"]), "num_keypoints": torch.as_tensor(np.asarray(inp["num"]), dtype=torch.int32)}
    for conf in (dict(), dict(solver="cholesky"), dict(loss="cauchy"), dict(loss="cauchy", solver="cholesky"), dict(solver="pcg", loss="cauchy", max_cg_iterations=7)):
        with pytest.raises(RuntimeError, match="stop before"):
            BundleAdjuster(**conf).adjust(feats, (torch.from_numpy(inp["track_id"]), torch.from_numpy(inp["xyz"])), torch.from_numpy(inp["cams"]),
                                          torch.from_numpy(inp["poses"]), torch.from_numpy(inp["constant"]))
    plain, chol, robust, robust_chol, pcg = seen
    assert plain[:4] == chol[:4] == ("lg_bundle_adjust", "lg_bundle_workspace_bytes", (6, 96, 50, 0), _cabi.LgBundleIO)
    assert robust[:4] == robust_chol[:4] == ("lg_bundle_adjust_robust", "lg_bundle_robust_workspace_bytes", (6, 96, 50, 0), _cabi.LgBundleRobustIO)
    assert pcg[:4] == ("lg_bundle_adjust_pcg", "lg_bundle_pcg_workspace_bytes", (6, 96, 50, 0), _cabi.LgBundlePcgIO)
    # the structs hold addresses of fresh output tensors; the settings in front of the first pointer and behind the last are the same bytes
    head, tail = _cabi.LgBundleIO.kpts.offset, ctypes.sizeof(_cabi.LgBundleIO)
    assert plain[4][:head] == chol[4][:head] and robust[4][:head] == robust_chol[4][:head] and robust[4][tail:] == robust_chol[4][tail:]
    assert pcg[4][tail:ctypes.sizeof(_cabi.LgBundleRobustIO)] == robust[4][tail:]
    io = _cabi.LgBundlePcgIO.from_buffer_copy(pcg[4])
    assert (io.max_cg_iterations, io.pad, io.cg_tolerance, io.base.loss) == (7, 0, 1e-6, 2)
