"""BundleAdjuster(solver="pcg") on the GPU against the float64 definitions: the dense one (tests/bundle_oracle.py, tests/bundle_robust_oracle.py: Schur
complement + Cholesky) at a tight solver tolerance, the iterative one (tests/bundle_pcg_oracle.py) at the tight and at the default tolerance, and itself.

The bars are those of tests/test_gpu_bundle.py, unchanged: observations, node states, iterations run, steps accepted, `converged`, the filter's counters and
the per-image status equal the oracle's exactly; a pose entry, a point and a row of points3d may differ from the oracle's fp64 value by ONE float32 ulp of
the scale (for a point the largest coordinate magnitude among the point and the centres of the cameras that see it, for t the same over the image's centre
and t, for R 1); costs agree within 1e-9 relative; observation_error within one float32 ulp of the error.  Against the iterative oracle the solver's two
counters, cg_iterations and cg_unconverged, are integers too and equal the oracle's.
Preconditions, asserted without a GPU by tests/test_bundle_pcg_cpu.py on every call of this file (each figure the largest over the calls, in float32 ulps of
the scale):
  (a) at cg_tolerance = 1e-13 the iterative and the dense definition take the same decisions and differ by at most
      Q_POINT    3.35e-08  on points
      Q_T        7.19e-07  on t
      Q_R        4.15e-07  on R
  (b) at the default tolerance (1e-6) the iterative definition moves between ascending and descending accumulation by at most
      Q_POINT    1.47e-06  on points
      Q_T        7.53e-05  on t
      Q_R        3.86e-05  on R
  all below 1e-3, and no call's oracle run places a decision (accept / reject, convergence, a pivot, pz = 0, the solver's stop, p.q > 0) within a relative
  1e-9 of its bar.
Budgets: the oracle's largest count of solver iterations in one Levenberg-Marquardt iteration, at 1e-13 / 1e-6: main 22 / 16, K = 9 34, K = 24 60, edge 18,
far 22 / 16, planted (Cauchy, one round) 22, long (squared and Cauchy) 22, the 300-image scene 110 / 83.  Every max_cg_iterations (bundle_pcg_oracle.TIGHT_CALLS, DEFAULT_CALLS) leaves at
least a quarter above its count, so no solve of these calls ends on the budget, except where a test sets a budget of 1 to see exactly that.
At 1e-13 a solve ends near the rounding floor of its recurrences and its count can move by a few iterations with the last bits (the CPU test prints what the
other accumulation order does: 107 instead of 103 in the second solve of the 300-image scene); cg_iterations is compared all the same, which holds because
the oracle follows the definition's order of operations one by one, and fp64 without fused multiply-add is the same arithmetic on both sides.
That equality also rests on sqrt, the division and the sine and cosine of the trial pose being the same bits in numpy on the host and in the device library:
after a change of the toolchain or of numpy, a cg_iterations mismatch at 1e-13 with every answer inside its bar is the first thing to suspect, and the place
to look is a solve whose residual stalls within a few tenths of the bar (the counts at the default tolerance do not move with either order).
The scenes are those of tests/bundle_oracle.py and tests/bundle_robust_oracle.py plus bundle_pcg_oracle.big_scene: 300 images of 32 rows, 4 171 observations,
298 free images, 1 200 tracks, which the dense solver refuses (more than LG_BA_MAX_IMAGES = 256 images)."""
import numpy as np
import pytest

import bundle_oracle as B
import bundle_pcg_oracle as P
import bundle_robust_oracle as R
import lightglue_amd
from test_gpu_bundle import same_bits
from test_gpu_bundle_robust import ALL_BITS, check, filtered, run

pytestmark = pytest.mark.gpu

PCG_BITS = ALL_BITS + ("cg_iterations", "cg_unconverged")


def pcg(name, **conf):
    return run(P.SCENES[name](), solver="pcg", **conf)


def check_dense(got, name, what):
    """against the dense definition: tests/test_gpu_bundle.py's bars (a plain answer has no filter counters: they are 0)"""
    want = dict(P.dense_answer(name))
    want.setdefault("num_filtered", 0), want.setdefault("num_filter_stages", 0), want.setdefault("first_state", want["node_state"])
    check(got, want, P.SCENES[name](), what + " against the dense definition")


def check_iterative(got, want, name, what):
    check(got, want, P.SCENES[name](), what + " against the iterative definition")
    print("%s: solver iterations %d (oracle %d, per iteration %s), on the budget %d" % (what, got["cg_iterations"], want["cg_iterations"], want["cg_counts"],
                                                                                   got["cg_unconverged"]))
    assert (got["cg_iterations"], got["cg_unconverged"]) == (want["cg_iterations"], want["cg_unconverged"]), what


@pytest.fixture(scope="module")
def main_default():
    return pcg("main")


@pytest.fixture(scope="module")
def big_tight():
    return pcg("big", **P.TIGHT_CALLS["big"])


# ---------------------------------------------------------------------- 1. a tight solve is the dense definition
@pytest.mark.parametrize("name", ["main", "K = 9", "K = 24"])
def test_tight_solve_meets_the_dense_definition(name):
    conf = P.TIGHT_CALLS[name]
    got = pcg(name, **conf)
    check_dense(got, name, name)
    check_iterative(got, P.answer(name, **conf), name, name)
    assert got["cg_unconverged"] == 0


# ---------------------------------------------------------------------- 2. the default tolerance, and a budget of one
def test_default_tolerance_follows_the_iterative_definition(main_default):
    want = P.answer("main")
    check_iterative(main_default, want, "main", "main, default tolerance")
    assert main_default["num_accepted"] == sum(want["accepts"]) and main_default["cg_unconverged"] == 0
    one = pcg("main", max_cg_iterations=1)
    check_iterative(one, P.answer("main", max_cg_iterations=1), "main", "main, one solver iteration")
    assert one["cg_unconverged"] == one["num_iterations"] == one["cg_iterations"] == 10
    assert all(np.isfinite(one[k]).all() for k in ("poses", "xyz", "initial_cost", "final_cost")) and one["final_cost"] < 0.02 * one["initial_cost"]


# ---------------------------------------------------------------------- 3. every edge in one scene
def test_edge_inputs_leave_everything_else_untouched():
    bad, clean, what = B.edge_scene()
    conf = P.TIGHT_CALLS["edge"]
    got = run(bad, expect=("LG_ERR_CAMERA", "image %d" % what["bad_image"]), solver="pcg", **conf)
    check_dense(got, "edge", "edge")
    check_iterative(got, P.answer("edge", **conf), "edge", "edge")
    assert got["status"].tolist() == [0, 0, 0, B.LG_ERR_CAMERA, 0, 0, 0]
    assert set(np.unique(got["node_state"]).tolist()) == {B.NONE, B.ACTIVE, B.BAD_IMAGE, B.NON_FINITE, B.BEHIND, B.SHORT}
    alone = run(clean, solver="pcg", **conf)                             # the same call without the bad entries: no status, no error
    check_dense(alone, "edge clean", "edge clean")
    same_bits(got, alone, "edge against clean", tuple(k for k in PCG_BITS if k != "node_state"))
    assert ((got["node_state"] == B.ACTIVE) == (alone["node_state"] == B.ACTIVE)).all()
    # the two constant images, the image with a bad camera and the image without observations return the bits that went in
    for k in (0, 1, what["bad_image"], what["empty_image"]):
        assert np.array_equal(got["poses"][k], bad["poses"][k]), k
    assert (got["poses"][[2, 4, 5]] != bad["poses"][[2, 4, 5]]).any()


# ---------------------------------------------------------------------- 4. beyond the dense envelope
def test_more_images_than_the_dense_solver_takes(big_tight):
    inp = P.big_scene()
    assert inp["kpts"].shape[:2] == (P.BIG_K, P.BIG_N) and P.BIG_K > lightglue_amd._cabi.LG_BA_MAX_IMAGES
    with pytest.raises(AssertionError, match="LG_BA_MAX_IMAGES"):
        run(inp, solver="cholesky", num_iterations=P.BIG_ITERATIONS)
    check_dense(big_tight, "big", "300 images, tight")
    check_iterative(big_tight, P.answer("big", **P.TIGHT_CALLS["big"]), "big", "300 images, tight")
    assert big_tight["num_observations"] == 4171 and big_tight["num_accepted"] == 4 and big_tight["final_cost"] < 0.01 * big_tight["initial_cost"]
    loose = pcg("big", **P.DEFAULT_CALLS["big"])
    check_iterative(loose, P.answer("big", **P.DEFAULT_CALLS["big"]), "big", "300 images, default tolerance")
    assert loose["cg_iterations"] < big_tight["cg_iterations"] and loose["cg_unconverged"] == 0


# ---------------------------------------------------------------------- 5. the same bits from run to run and under a relabelling of the tracks
def test_outputs_are_the_same_bits(main_default, big_tight):
    same_bits(big_tight, pcg("big", **P.TIGHT_CALLS["big"]), "300 images again", PCG_BITS)
    inp = P.SCENES["main"]()
    same_bits(main_default, pcg("main"), "main again", PCG_BITS)
    moved, perm = B.relabel(inp, 5)
    other = run(moved, solver="pcg")
    same_bits(main_default, dict(other, xyz=other["xyz"][perm]), "tracks relabelled", PCG_BITS)


# ---------------------------------------------------------------------- 6. the robust mode, and rejected steps
def test_cauchy_with_one_filter_round():
    inp, planted, _ = R.planted_scene()
    conf = P.TIGHT_CALLS["planted"]
    got = pcg("planted", **conf)
    check_dense(got, "planted", "planted, cauchy, one round")
    check_iterative(got, P.answer("planted", **conf), "planted", "planted, cauchy, one round")
    assert filtered(got) == planted and got["num_filtered"] == 12 and got["num_filter_stages"] == 1 and got["num_observations"] == 200


def test_rejected_steps_follow_the_definition():
    want = P.answer("far")
    assert want["accepts"][:2] == [False, False] and want["converged"] and want["num_accepted"] <= want["num_iterations"] - 2
    got = pcg("far")
    check_iterative(got, want, "far", "far start, default tolerance")
    tight = pcg("far", **P.TIGHT_CALLS["far"])
    check_dense(tight, "far", "far start, tight")
    check_iterative(tight, P.answer("far", **P.TIGHT_CALLS["far"]), "far", "far start, tight")


# ---------------------------------------------------------------------- 6b. two observations of one track in one image: both E_aa branches of the setup kernel
@pytest.mark.parametrize("name", ["long", "long cauchy"])
def test_two_rows_of_one_image_in_one_track(name):
    """rows 100 and 101 of image 2 carry one track: with the squared loss the setup kernel adds the row's own term twice, with Cauchy its entry lanes
    linearise both observations again, each with its own weight"""
    inp, conf = P.SCENES[name](), P.TIGHT_CALLS[name]
    T = len(inp["xyz"]) - 2
    want = P.answer(name, **conf)
    assert (inp["track_id"][2, 100:102] == T + 1).all() and (want["node_state"][2, 100:102] == B.ACTIVE).all() and want["free"][2]
    got = pcg(name, **conf)
    check_dense(got, name, name)
    check_iterative(got, want, name, name)
    assert got["cg_unconverged"] == 0


# ---------------------------------------------------------------------- 7. the default solver is the call without the argument
def test_cholesky_is_the_call_without_the_argument():
    inp = P.SCENES["main"]()
    plain, named = run(inp), run(inp, solver="cholesky")
    assert set(plain) == set(named) and "cg_iterations" not in named
    same_bits(plain, named, "solver='cholesky'", ALL_BITS)
    robust, robust_named = run(R.planted_scene()[0], **R.CAUCHY, **R.ONE_ROUND), run(R.planted_scene()[0], solver="cholesky", **R.CAUCHY, **R.ONE_ROUND)
    same_bits(robust, robust_named, "solver='cholesky', robust", ALL_BITS)
