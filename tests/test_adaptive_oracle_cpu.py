"""tests/adaptive_oracle.py against the oracle it restates, and every tie of the adaptive step pinned by hand (no GPU).

The confidence-threshold tie (a token confidence EQUAL to the layer's threshold) is pinned here only: on the device the threshold is a fixed formula and
the confidence a sigmoid output, so the tie cannot be forced there (tests/test_gpu_adaptive_stages.py forces the two that can be)."""
import numpy as np
import pytest

import adaptive_oracle as A
import gpu_util
import test_gpu_adaptive_stages as G
from lightglue_amd import synthetic as synth
from oracle import lightglue_oracle as O

L5 = 5
# (seed, n0, n1, conf): mixed sizes, both adaptive mechanisms alone and together, thresholds at, below and above the sizes
REPLAY_CASES = [
    (1, 300, 200, dict(pruning_min_kpts=-1)),
    (2, 129, 333, dict(pruning_min_kpts=64)),
    (3, 65, 17, dict(pruning_min_kpts=16, depth_confidence=0.999)),
    (4, 40, 1, dict(pruning_min_kpts=16, depth_confidence=0.999)),
    (5, 200, 260, dict(pruning_min_kpts=-1, depth_confidence=-1)),
    (6, 150, 90, dict(width_confidence=-1)),
    (7, 64, 65, dict(pruning_min_kpts=64, depth_confidence=0.999)),
    (8, 120, 80, dict(pruning_min_kpts=-1, depth_confidence=-1, width_confidence=0.5)),
    (9, 90, 70, dict(pruning_min_kpts=-1, depth_confidence=-1, width_confidence=1e-9)),   # 1 - 1e-9 rounds to 1.0f: every row of both images dropped
]


def _replay(seed, n0, n1, kw):
    """forward_pair with its trace, and the step function applied layer by layer to the confidences in that trace"""
    sd = synth.make_state_dict(0, recipe="B", n_layers=L5)
    pair = synth.make_pair(seed, n0, n1)
    conf = O.make_conf(n_layers=L5, **kw)
    tr = {}
    out = O.forward_pair(sd, conf, pair["keypoints0"], pair["keypoints1"], pair["descriptors0"], pair["descriptors1"], pair["image_size0"], pair["image_size1"], trace=tr)
    length, active, final_layer = (n0, n1), 1, L5 - 1
    ind = (np.arange(n0), np.arange(n1))
    prune = [np.ones(n0, np.int64), np.ones(n1, np.int64)]
    steps = []
    for i in range(L5 - 1):
        if not active:
            break
        cf = (tr[f"l{i}_conf0"], tr[f"l{i}_conf1"]) if conf.depth_confidence > 0 else None
        st = A.step_pair(cf, (tr[f"l{i}_mscore0"], tr[f"l{i}_mscore1"]), length, (n0, n1), active, final_layer, ind, i, L5,
                         conf.depth_confidence, conf.width_confidence, conf.pruning_min_kpts)
        steps.append(st)
        if not st.stop and conf.width_confidence > 0:
            np.testing.assert_array_equal(st.ind[0], tr[f"l{i}_ind0"]); np.testing.assert_array_equal(st.ind[1], tr[f"l{i}_ind1"])
        for im in (0, 1):   # the step's own outputs agree with each other
            kept = np.where(st.keep[im])[0]
            np.testing.assert_array_equal(st.dst[im][kept], np.arange(len(kept)))
            assert (st.dst[im][~st.keep[im]] == -1).all() and st.len[im] == len(kept)
            np.testing.assert_array_equal(A.apply_step(st, im, np.asarray(ind[im]))[0], st.ind[im])
            prune[im] += st.prune_inc[im]
        length, active, final_layer, ind = st.len, st.active, st.final_layer, st.ind
    return out, steps, prune, final_layer


@pytest.mark.parametrize("seed,n0,n1,kw", REPLAY_CASES, ids=[str(c[0]) for c in REPLAY_CASES])
def test_step_function_replays_forward_pair(seed, n0, n1, kw):
    """Kept index sets (asserted per layer in _replay), the stop layer and the prune counters of a whole adaptive forward_pair."""
    out, steps, prune, final_layer = _replay(seed, n0, n1, kw)
    assert out["stop"] == final_layer + 1
    if kw.get("width_confidence", 0.99) > 0:
        np.testing.assert_array_equal(out["prune0"], prune[0]); np.testing.assert_array_equal(out["prune1"], prune[1])
    else:
        assert all(s.len_old == (-1, -1) and s.len == (n0, n1) for s in steps)


def test_replay_cases_cover_every_outcome():
    """The cases above would prove little if no pair stopped early, pruned twice, left an image unpruned or lost one altogether."""
    seen = set()
    for seed, n0, n1, kw in REPLAY_CASES:
        out, steps, _, final_layer = _replay(seed, n0, n1, kw)
        if any(s.stop for s in steps):
            seen.add("stopped")
        if final_layer == L5 - 1:
            seen.add("ran every layer")
        if sum(1 for s in steps if s.len_old[0] >= 0 and s.len[0] < s.len_old[0]) >= 2:
            seen.add("pruned twice")
        if any(s.len_old[0] >= 0 and s.len_old[1] < 0 for s in steps if not s.stop and s.active):
            seen.add("one image below the threshold")
        if any(not s.stop and not s.active for s in steps):
            seen.add("image emptied")
            assert out["stop"] == len(steps) + 1 and (out["matches0"] == -1).all()
    assert seen == {"stopped", "ran every layer", "pruned twice", "one image below the threshold", "image emptied"}, seen


def _f32(*v):
    return np.array(v, np.float32)


def test_confidence_equal_to_the_threshold_is_not_below_it_and_is_kept():
    L, layer = 9, 2
    thr = O.confidence_thresholds_f32(L)[layer]
    below, above = np.nextafter(thr, np.float32(0)), np.nextafter(thr, np.float32(2))
    conf = (_f32(thr, below, above, thr), _f32(below, thr))
    # ratio: two of six are below the threshold; the three AT it do not count
    assert A.stop_ratio(conf[0], conf[1], (4, 2), layer, L) == np.float32(1.0) - np.float32(2.0) / np.float32(6.0)
    ms = (_f32(0, 0, 0, 0), _f32(0, 0))   # nothing survives on matchability: conf <= thr alone decides
    st = A.step_pair(conf, ms, (4, 2), (4, 2), 1, L - 1, (np.arange(4), np.arange(2)), layer, L, 0.99, 0.99, -1)
    assert not st.stop
    assert st.keep[0].tolist() == [True, True, False, True] and st.keep[1].tolist() == [True, True]
    assert st.dst[0].tolist() == [0, 1, -1, 2] and st.ind[0].tolist() == [0, 1, 3] and st.len == (3, 2) and st.len_old == (4, 2)
    assert st.prune_inc[0].tolist() == [1, 1, 0, 1]


def test_matchability_equal_to_one_minus_width_confidence_is_dropped():
    wc = 0.75
    edge = np.float32(1.0 - wc)
    ms = (_f32(edge, np.nextafter(edge, np.float32(1)), np.nextafter(edge, np.float32(0))), _f32(1.0))
    st = A.step_pair(None, ms, (3, 1), (3, 1), 1, 8, (np.arange(3), np.arange(1)), 0, 9, -1, wc, -1)
    assert st.keep[0].tolist() == [False, True, False] and st.ind[0].tolist() == [1] and st.active == 1
    # a width_confidence that float32 cannot tell from 0 keeps nothing: one image lost every point -> the pair ends at the next layer's guard
    st = A.step_pair(None, (_f32(1.0, 0.5), _f32(1.0)), (2, 1), (2, 1), 1, 8, (np.arange(2), np.arange(1)), 3, 9, -1, 1e-9, -1)
    assert st.len == (0, 0) and st.active == 0 and st.final_layer == 4 and not st.stop


def test_ratio_equal_to_depth_confidence_does_not_stop():
    L, layer = 9, 0
    thr = O.confidence_thresholds_f32(L)[layer]
    conf = (np.where(np.arange(7) < 2, np.float32(0.1), np.float32(0.99)).astype(np.float32), _f32(0.99, 0.99, 0.1))   # 3 of 10 below
    ratio = A.stop_ratio(conf[0], conf[1], (7, 3), layer, L)
    assert ratio == np.float32(1.0) - np.float32(3.0) / np.float32(10.0) and thr > 0.1
    args = (conf, None, (7, 3), (7, 3), 1, L - 1, (np.arange(7), np.arange(3)), layer, L)
    st = A.step_pair(*args, float(ratio), -1, -1)
    assert not st.stop and st.active == 1 and st.final_layer == L - 1
    st = A.step_pair(*args, float(np.nextafter(ratio, np.float32(-np.inf))), -1, -1)
    assert st.stop and st.active == 0 and st.final_layer == layer and st.len_old == (-1, -1) and st.len == (7, 3)
    # the ratio is over the ORIGINAL counts: the same live rows of a pair that started with 20 points
    assert A.stop_ratio(conf[0], conf[1], (12, 8), layer, L) == np.float32(1.0) - np.float32(3.0) / np.float32(20.0)


def test_pruning_threshold_is_strict():
    ms = (np.zeros(17, np.float32), np.zeros(16, np.float32)); ms[0][5] = ms[1][5] = 1.0
    st = A.step_pair(None, ms, (17, 16), (17, 16), 1, 8, (np.arange(17), np.arange(16)), 0, 9, -1, 0.99, 16)
    assert st.len_old == (17, -1) and st.len == (1, 16) and st.ind[0].tolist() == [5] and st.keep[1].all()
    assert st.prune_inc[0].sum() == 1 and st.prune_inc[1].sum() == 0   # counters move only where the branch is taken (ref :558)


def test_an_ended_pair_is_left_alone():
    ms = (np.zeros(4, np.float32), np.zeros(4, np.float32))
    st = A.step_pair((ms[0], ms[1]), ms, (4, 4), (9, 9), 0, 2, (np.arange(4), np.arange(4)), 5, 9, 0.5, 0.99, -1)
    assert not st.stop and st.active == 0 and st.final_layer == 2 and st.len == (4, 4) and st.len_old == (-1, -1)


def test_layer_trace_is_the_loop_body_of_forward_pair():
    """layer_trace run on its own from the previous layer's output leaves exactly the keys and values forward_pair's loop leaves."""
    sd = synth.make_state_dict(3, recipe="A", n_layers=2)
    pair = synth.make_pair(11, 37, 21)
    conf = O.make_conf(n_layers=2, depth_confidence=-1, width_confidence=-1)
    tr = {"_full_layers": (0, 1)}
    O.forward_pair(sd, conf, pair["keypoints0"], pair["keypoints1"], pair["descriptors0"], pair["descriptors1"], pair["image_size0"], pair["image_size1"], trace=tr)
    own = {}
    p = {k: np.asarray(v, np.float32) for k, v in sd.items()}
    O.layer_trace(O.make_ctx(np.float32, None), p, 1, tr["desc0_l0"], tr["desc1_l0"], tr["cos0"], tr["sin0"], tr["cos1"], tr["sin1"], 4, 2, own)
    want = {k for k in tr if k.startswith("l1_") or k.endswith("_l1")}
    assert set(own) == want and len(want) > 30
    for k in want:
        np.testing.assert_array_equal(own[k], tr[k], err_msg=k)


def _oracle_steps(counts, data, conf_kw):
    """per pair: the oracle's output and its trace, on the pair's own rows of a ragged fixture of tests/test_gpu_adaptive_stages.py"""
    res = []
    for b, (c0, c1) in enumerate(counts):
        d0, d1 = data["image0"], data["image1"]
        tr = {}
        out = O.forward_pair(G.state_dict(conf_kw["n_layers"]), O.make_conf(**conf_kw), d0["keypoints"][b][:c0], d1["keypoints"][b][:c1], d0["descriptors"][b][:c0],
                             d1["descriptors"][b][:c1], d0["image_size"][b], d1["image_size"][b], trace=tr)
        res.append((out, tr))
    return res


def test_gpu_fixtures_exercise_what_they_are_meant_to():
    """What tests/test_gpu_adaptive_stages.py asserts on the device's masks holds on the oracle with a margin: the last pair of the main batch stops behind
    layer 0 and no other does, most segments above the threshold drop and keep rows there, segments are pruned again behind layer 1; every segment above the
    threshold of the layer fixture loses rows and every pair goes on.  Padding rows are NaN."""
    res = _oracle_steps(G.MAIN_COUNTS, G.main_batch(), G.MAIN_CONF)
    L, dc = G.MAIN_CONF["n_layers"], G.MAIN_CONF["depth_confidence"]
    assert {c for pair in G.MAIN_COUNTS[:-1] for c in pair} == {1, 63, 64, 65, 1023, 1024, 1025, 2049, 127, 128, 129, 257, G.PMIN, G.PMIN + 1}
    assert max(c[0] for c in G.MAIN_COUNTS) <= 2176 and max(c[1] for c in G.MAIN_COUNTS) <= 1152 and len(G.MAIN_COUNTS) <= 8
    both = above = again = 0
    for b, ((out, tr), (c0, c1)) in enumerate(zip(res, G.MAIN_COUNTS)):
        ratio = A.stop_ratio(tr["l0_conf0"], tr["l0_conf1"], (c0, c1), 0, L)
        last = b == len(G.MAIN_COUNTS) - 1
        assert (ratio > dc + 0.05) if last else (ratio < dc - 0.05), (b, ratio)   # a margin low-precision confidences will not cross
        assert out["stop"] == (1 if last else 3)
        if last:
            continue
        for im, n in ((0, c0), (1, c1)):
            kept0, kept1 = len(tr[f"l0_ind{im}"]), len(tr[f"l1_ind{im}"])
            above += n > G.PMIN
            both += n > G.PMIN and 0 < kept0 < n
            again += 0 < kept1 < kept0 < n
            assert n > G.PMIN or kept0 == n
    assert 2 * both >= above + 4 and again >= 4, (both, above, again)
    data = G.main_batch()
    assert np.isnan(data["image0"]["descriptors"][6, 17:]).all() and np.isfinite(data["image0"]["descriptors"][6, :17]).all()
    for (out, tr), (c0, c1) in zip(_oracle_steps(G.LAYER_COUNTS, G.layer_batch(), G.LAYER_CONF), G.LAYER_COUNTS):
        assert out["stop"] == 3
        for im, n in ((0, c0), (1, c1)):
            kept = len(tr[f"l0_ind{im}"])
            assert (0 < kept < n) if n > G.PMIN else kept == n, (c0, c1, im, kept)


def test_layer1_bounds_are_the_derived_ones():
    """The stages of test_layer_behind_a_pruning_step are held to the layer-0 bounds of tests/test_gpu_parity.py, but for four stages of "f16x3/fp16": the
    context of a segment with ONE key is that key's v at operand precision (one f16 plane), un-averaged, and out_proj / to_out inherit it.  Their bounds are
    twice LAYER1_QUANT_FLOOR, which is what the oracle's own quantised run shows against its float64 run on that fixture (rounded up in the third digit); every
    other stage of every precision keeps the imported bound, and the quantised run itself stays within it there."""
    floor = G.quantised_layer1_errors(O.FAST_ATTENTION_QUANT)
    print("derived:", {k: "%.4e" % v for k, v in floor.items()})
    derived = {stage for (precision, stage) in G.LAYER1_QUANT_FLOOR}
    assert derived == {"self.attn_ctx", "self.out_proj", "cross.attn_ctx", "cross.to_out"} and {p for p, _ in G.LAYER1_QUANT_FLOOR} == {"f16x3/fp16"}
    for stage, q in floor.items():
        if stage in derived:
            const = G.LAYER1_QUANT_FLOOR[("f16x3/fp16", stage)]
            assert q <= const <= 1.01 * q, (stage, q, const)
            assert G.layer1_bound("f16x3/fp16", stage) == 2 * const > G._STAGE_TOL["f16x3/fp16"]
            assert "%.2e" % const in G.test_layer_behind_a_pruning_step.__doc__
        else:
            tol = G._OPERAND_TOL["f16x3/fp16"] if stage in G._PROJ_STAGES else G._STAGE_TOL["f16x3/fp16"]
            assert G.layer1_bound("f16x3/fp16", stage) == tol and q <= tol, (stage, q, tol)
    for precision in G.PRECISIONS:
        if precision != "f16x3/fp16":
            assert all(G.layer1_bound(precision, stage) == (G._OPERAND_TOL if stage in G._PROJ_STAGES else G._STAGE_TOL)[precision] for stage in G.STAGE_KEYS)
    # the cause, not just the figure: with the one-key pair left out, the quantised run meets the imported bound at every stage
    state = G.oracle_state_behind_step13()
    assert state["LEN"][3, 1] == 1 and (state["LEN"][:3] >= 10).all()
    three = {**state, "rows": gpu_util.Rows(3, 0, 0, 384, 384), "LEN": state["LEN"][:3]}
    exact, rounded = G.layer1_traces(G.state_dict(), three, 3), G.layer1_traces(G.state_dict(), three, 3, np.float64, O.FAST_ATTENTION_QUANT)
    for stage in derived:
        key = G.STAGE_KEYS[stage]
        worst = max(gpu_util.err(q[key.format(im=im)], e[key.format(im=im)])[1] for e, q in zip(exact, rounded) for im in (0, 1))
        assert worst <= 2 * G._STAGE_TOL["f16x3/fp16"], (stage, worst)
