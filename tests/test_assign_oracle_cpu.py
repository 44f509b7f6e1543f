"""tests/assign_oracle.py against the oracle it restates, the properties of the fixtures that tests/test_gpu_assign_stages.py relies on, and the measured
floors behind that file's bounds.  No GPU."""
import math

import numpy as np
import pytest

import assign_oracle as A
import test_gpu_assign_stages as G
from lightglue_amd import synthetic as synth
from oracle import lightglue_oracle as O


def _composition(x0, x1, sd, n0, n1, ind0, ind1, threshold):
    """every assign_oracle stage in a row, in float64: (scores [len0, len1], dustbin column, dustbin row, finalize dict)"""
    w, b = G.head_weights(sd, "match", 0)
    wf, bf = sd["log_assignment.0.final_proj.weight"].astype(np.float64), sd["log_assignment.0.final_proj.bias"].astype(np.float64)
    md0, md1 = (x0 @ wf.T + bf) / 4.0, (x1 @ wf.T + bf) / 4.0           # 256 ** 0.25 == 4
    s = A.sim(md0, md1)
    h0, h1 = A.heads(x0, w, b), A.heads(x1, w, b)
    scores = ((s - A.lse_rows(s)[:, None]) + (s - A.lse_cols(s)[None, :])) + (h0[2][:, None] + h1[2][None, :])
    max0, arg0, _, arg1 = A.argmax_first(scores)
    return scores, h0[3], h1[3], max0, A.finalize(max0, arg0, arg1, ind0, ind1, n0, n1, threshold)


def _reference_outputs(scores_full, ind0, ind1, n0, n1, threshold):
    """ref :592-614 as oracle/lightglue_oracle.py forward_pair assembles them"""
    m0, m1, ms0, ms1 = O.filter_matches(scores_full, threshold)
    valid = m0 > -1
    matches = np.stack([ind0[np.where(valid)[0]], ind1[m0[valid]]], -1)
    M0, M1, S0, S1 = np.full(n0, -1, np.int64), np.full(n1, -1, np.int64), np.zeros(n0), np.zeros(n1)
    M0[ind0] = np.where(m0 == -1, -1, ind1[np.clip(m0, 0, None)])
    M1[ind1] = np.where(m1 == -1, -1, ind0[np.clip(m1, 0, None)])
    S0[ind0], S1[ind1] = ms0, ms1
    return M0, M1, S0, S1, matches, ms0[valid]


def _assert_same_outputs(got, ref):
    M0, M1, S0, S1, matches, mscores = ref
    np.testing.assert_array_equal(got["matches0"], M0)
    np.testing.assert_array_equal(got["matches1"], M1)
    np.testing.assert_array_equal(got["matches"], matches.reshape(-1, 2))
    assert got["n_matches"] == len(matches)
    # finalize takes exp of the float32 maximum, as the matcher does: 2^-24 |max| of relative difference
    np.testing.assert_allclose(got["scores0"], S0, rtol=2e-5, atol=0)
    np.testing.assert_allclose(got["scores1"], S1, rtol=2e-5, atol=0)
    np.testing.assert_allclose(got["match_scores"], mscores, rtol=2e-5, atol=0)


@pytest.mark.parametrize("seed,len0,len1,n0,n1", [(0, 70, 90, 70, 90), (1, 45, 33, 80, 64), (2, 1, 7, 3, 7), (3, 20, 1, 20, 5)])
def test_composition_equals_the_oracle(seed, len0, len1, n0, n1):
    """sim -> heads -> lse -> scores -> argmax -> finalize == O.log_assignment + O.filter_matches + the un-pruning of forward_pair, in float64, with
    identity and with pruned index sets."""
    rng = np.random.Generator(np.random.PCG64(seed))
    sd = {k: v.astype(np.float64) for k, v in synth.make_state_dict(seed, recipe="C", n_layers=1).items()}
    x0, x1 = rng.standard_normal((len0, 256)), rng.standard_normal((len1, 256))
    ind0, ind1 = np.sort(rng.permutation(n0)[:len0]), np.sort(rng.permutation(n1)[:len1])
    tr = {}
    full, s = O.log_assignment(O.make_ctx(np.float64, None), sd, 0, x0, x1, tr)
    scores, dust0, dust1, max0, got = _composition(x0, x1, sd, n0, n1, ind0, ind1, 0.1)
    np.testing.assert_allclose(A.sim(tr["md0"], tr["md1"]), s, rtol=0, atol=1e-12)
    np.testing.assert_allclose(A.heads(x0, *G.head_weights(sd, "match", 0))[0], tr["z0"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(scores, full[:-1, :-1], rtol=0, atol=1e-10)
    np.testing.assert_allclose(dust0, full[:-1, -1], rtol=0, atol=1e-12)
    np.testing.assert_allclose(dust1, full[-1, :-1], rtol=0, atol=1e-12)
    _assert_same_outputs(got, _reference_outputs(full, ind0, ind1, n0, n1, 0.1))
    assert got["n_matches"] > 0 or min(len0, len1) == 1
    # the float32 restatement of score_of is the same expression
    f32 = A.scores_f32(s, A.lse_rows(s), A.lse_cols(s), A.heads(x0, *G.head_weights(sd, "match", 0))[2], A.heads(x1, *G.head_weights(sd, "match", 0))[2])
    assert f32.dtype == np.float32 and np.abs(f32 - scores).max() <= 16 * 2.0 ** -24 * np.abs(scores).max()


def test_heads_are_stable_and_consistent():
    x = np.zeros((7, 256)); x[:, 0] = [-800.0, -40.0, -1.0, 0.0, 1.0, 40.0, 800.0]
    w = np.zeros(256); w[0] = 1.0
    z, sg, ls, lsneg = A.heads(x, w, np.zeros(1))
    assert np.isfinite(sg).all() and np.isfinite(ls).all() and np.isfinite(lsneg).all()
    np.testing.assert_array_equal(z, x[:, 0])
    np.testing.assert_allclose(ls[::-1], lsneg, rtol=0, atol=0)
    np.testing.assert_allclose(sg + sg[::-1], 1.0, rtol=0, atol=3e-16)
    np.testing.assert_allclose(ls[2:5], np.log(sg[2:5]), rtol=1e-14)
    assert ls[0] == -800.0 and lsneg[-1] == -800.0 and sg[0] == 0.0 and sg[-1] == 1.0
    tok = O.token_confidence(None, {"token_confidence.0.token.0.weight": w[None], "token_confidence.0.token.0.bias": np.zeros(1)}, 0, x)
    np.testing.assert_allclose(sg, tok, rtol=1e-15)


def test_first_index_tie_rule_on_a_hand_made_matrix():
    s = np.array([[1.0, 3.0, 3.0, 0.0],
                  [2.0, 2.0, 2.0, 2.0],
                  [1.0, 3.0, 0.0, 2.0]], np.float32)
    max0, arg0, max1, arg1 = A.argmax_first(s)
    assert arg0.tolist() == [1, 0, 1] and arg1.tolist() == [1, 0, 0, 1]
    assert max0.tolist() == [3.0, 2.0, 3.0] and max1.tolist() == [2.0, 3.0, 3.0, 2.0]
    got = A.finalize(max0 - 4, arg0, arg1, np.array([0, 2, 5]), np.array([1, 2, 3, 7]), 6, 8, 0.0)
    # row 0 <-> column 1 is mutual; row 2 also points at column 1 but loses the column's tie to row 0; row 1's column 0 prefers ... row 1: mutual
    assert got["matches"].tolist() == [[0, 2], [2, 1]] and got["n_matches"] == 2
    assert got["matches0"].tolist() == [2, -1, 1, -1, -1, -1] and got["matches1"].tolist() == [-1, 2, 0, -1, -1, -1, -1, -1]
    np.testing.assert_allclose(got["scores0"], [math.exp(-1), 0, math.exp(-2), 0, 0, 0])
    np.testing.assert_allclose(got["scores1"], [0, math.exp(-2), math.exp(-1), 0, 0, 0, 0, 0])
    # all equal: exactly one match, (0, 0)
    got = A.finalize(*(lambda r: (r[0], r[1], r[3]))(A.argmax_first(np.zeros((3, 5), np.float32))), np.arange(3), np.arange(5), 3, 5, 0.0)
    assert got["matches"].tolist() == [[0, 0]] and got["matches0"].tolist() == [0, -1, -1] and got["matches1"].tolist() == [0, -1, -1, -1, -1]
    # the threshold is strict (ref :314)
    got = A.finalize(np.zeros(1, np.float32), [0], [0], [0], [0], 1, 1, 1.0)
    assert got["n_matches"] == 0 and got["scores0"].tolist() == [1.0] and got["matches0"].tolist() == [-1] and got["matches1"].tolist() == [-1]
    assert A.finalize(np.zeros(1, np.float32), [0], [0], [0], [0], 1, 1, 0.999)["matches"].tolist() == [[0, 0]]
    empty = A.finalize(np.zeros(0, np.float32), [], [], [], [], 4, 2, 0.1)
    assert empty["n_matches"] == 0 and (empty["matches0"] == -1).all() and (empty["scores1"] == 0).all()


def _oracle_outputs_equal_finalize(name, dtype):
    fx = G.fixture(name)
    n0, n1 = fx.data["image0"]["keypoints"].shape[1], fx.data["image1"]["keypoints"].shape[1]
    res = []
    for out, tr in G.oracle_traces(name, dtype):
        if "scores_full" not in tr:
            assert len(out["matches"]) == 0
            res.append(None)
            continue
        max0, arg0, _, arg1 = A.argmax_first(tr["scores_full"][:-1, :-1])
        got = A.finalize(max0, arg0, arg1, tr["ind0"], tr["ind1"], len(out["matches0"]), len(out["matches1"]), fx.conf.get("filter_threshold", 0.1))
        _assert_same_outputs(got, (out["matches0"], out["matches1"], out["matching_scores0"], out["matching_scores1"], out["matches"], out["scores"]))
        res.append((got, tr))
    return res


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", ["tie-33x1025", "tie-1057x5"])
def test_all_tie_fixture_has_exactly_one_match(name, dtype):
    (got, tr), = _oracle_outputs_equal_finalize(name, dtype)
    assert got["matches"].tolist() == [[0, 0]]
    inner = tr["scores_full"][:-1, :-1]
    assert (inner == inner[0, 0]).all() and (tr["sim"] == tr["sim"][0, 0]).all()
    assert (inner.argmax(1) == 0).all() and (inner.argmax(0) == 0).all()


def test_duplicates_fixture_ties_are_exact_and_every_group_wins_somewhere():
    """Identical keypoints give bit-identical score rows and columns in the float64 oracle too — as long as its BLAS does not split the rows of a product
    over threads (a thread's remainder rows take another summation order; seen: 4e-14), so the oracle runs on one thread here."""
    import threadpoolctl
    _oracle_outputs_equal_finalize("dups", np.float64)
    with threadpoolctl.threadpool_limits(limits=1):
        (out, tr), = G.oracle_traces.__wrapped__("dups")
    inner = tr["scores_full"][:-1, :-1]
    arg0, arg1 = inner.argmax(1), inner.argmax(0)
    for g in G.DUP_COLS:
        for j in g[1:]:
            assert np.array_equal(inner[:, j], inner[:, g[0]]) and np.array_equal(tr["sim"][:, j], tr["sim"][:, g[0]]), (g[0], j)
        assert np.isin(arg0, g).any(), f"no row has its best column in {g}"
        assert (arg0[np.isin(arg0, g)] == min(g)).all()
    for g in G.DUP_ROWS:
        for i in g[1:]:
            assert np.array_equal(inner[i], inner[g[0]]) and np.array_equal(tr["sim"][i], tr["sim"][g[0]]), (g[0], i)
        assert np.isin(arg1, g).any(), f"no column has its best row in {g}"
        assert (arg1[np.isin(arg1, g)] == min(g)).all()
    # the groups sit where the kernels' tie rules are: one float4, two lanes of a wave, two waves of a pass, both passes; one tile, tiles of other / the same merge wave
    cols = {(a // 4 == b // 4, a // 256 == b // 256, a // 1024 == b // 1024) for g in G.DUP_COLS for a, b in zip(g, g[1:])}
    assert {(True, True, True), (False, True, True), (False, False, True), (False, False, False)} <= cols
    tiles = {(a // 32 == b // 32, (a // 32) % 4 == (b // 32) % 4) for g in G.DUP_ROWS for a, b in zip(g, g[1:])}
    assert {(True, True), (False, False), (False, True)} <= tiles


def test_shape_fixtures_reach_what_they_are_for():
    (got, tr), = _oracle_outputs_equal_finalize("600x1025", np.float64)
    blocks = np.bincount(got["matches"][:, 0] // 256, minlength=3).tolist()
    print(f"600 x 1025, filter_threshold 0: {got['n_matches']} matches, per 256-row block {blocks}")
    assert got["n_matches"] == 598 and blocks == [256, 255, 87]
    (got, tr), = _oracle_outputs_equal_finalize("300x1300", np.float64)
    arg0 = tr["scores_full"][:-1, :-1].argmax(1)
    print(f"300 x 1300: {int((arg0 >= 1024).sum())} rows have their best column in the second pass, {got['n_matches']} matches")
    assert (arg0 >= 1024).any() and (arg0 < 1024).any()
    for name in ("1x1025", "33x1021", "1057x5", "5x700"):
        (got, tr), = _oracle_outputs_equal_finalize(name, np.float64)
        assert tr["sim"].shape == G.SHAPES[name]
    ragged = _oracle_outputs_equal_finalize("ragged", np.float64)
    assert ragged[2] is None and [r[1]["sim"].shape for r in ragged[:2]] == [(300, 1300), (31, 1025)]
    assert all(np.isnan(G.fixture("ragged").data[k]["descriptors"][b, c:]).all() for k, cs in (("image0", G.RAGGED0), ("image1", G.RAGGED1)) for b, c in enumerate(cs))


def test_adaptive_fixture_prunes():
    (got, tr), = _oracle_outputs_equal_finalize("adaptive", np.float64)
    print(f"adaptive 600 x 520: live {len(tr['ind0'])} x {len(tr['ind1'])}, {got['n_matches']} matches")
    assert (len(tr["ind0"]), len(tr["ind1"]), got["n_matches"]) == (506, 453, 377)
    (got32, tr32), = _oracle_outputs_equal_finalize("adaptive", np.float32)
    assert np.array_equal(tr32["ind0"], tr["ind0"]) and np.array_equal(tr32["ind1"], tr["ind1"])


def test_head_fixture_keeps_every_point_and_both_signs():
    for shape in G.HEAD_SHAPES:
        fx = G.head_fixture(shape)
        for b in range(2):
            tr = {"_full_layers": (0, 1)}
            out = O.forward_pair(fx.sd, O.make_conf(**fx.conf), *G.pair_inputs(fx, b), dtype=np.float64, trace=tr)
            assert out["stop"] == 2 and (len(tr["ind0"]), len(tr["ind1"])) == shape
            for im in (0, 1):
                w, bias = G.head_weights(fx.sd, "match", 0)
                z, sg, ls, lsneg = A.heads(tr[f"desc{im}_l0"], w, bias)
                np.testing.assert_allclose(z, tr[f"l0_z{im}"], rtol=0, atol=1e-12)
                np.testing.assert_allclose(A.heads(tr[f"desc{im}_l0"], *G.head_weights(fx.sd, "token", 0))[1], tr[f"l0_tok{im}"], rtol=1e-13)
                assert "l1_tok0" not in tr and f"l1_z{im}" in tr
    z = np.concatenate([tr["l0_z0"], tr["l0_z1"]])
    assert (z > 0).any() and (z < 0).any()


# ------------------------------------------------------------------------------------------------ the floors behind the GPU bounds
def _lse_f32_sequential(s, axis):
    s = np.moveaxis(np.asarray(s, np.float32), axis, 0)
    m, acc = s.max(0), np.zeros(s.shape[1:], np.float32)
    for row in s:
        acc = acc + np.exp(row - m)
    assert acc.dtype == np.float32
    return m + np.log(acc)


def test_floors_behind_the_gpu_bounds():
    """What plain float32 evaluations of the same definitions show against float64 on the fixtures' own data.  The GPU tests' bounds are 4 x these floors
    (plus a derived term each); the constants there must be what is measured here, within the spread of BLAS builds (a factor of 2 either way)."""
    sim_floor = head_floor = lse_floor = seq_floor = 0.0
    for name in G.FIXTURES:
        for out, tr in G.oracle_traces(name):
            if "sim" not in tr:
                continue
            md0, md1 = tr["md0"], tr["md1"]
            f32 = np.matmul(md0.astype(np.float32), md1.astype(np.float32).T)
            exact = A.sim(md0.astype(np.float32), md1.astype(np.float32))
            sim_floor = max(sim_floor, float((np.abs(f32 - exact) / A.sim_scale(md0, md1)).max()))
            s = tr["sim"]
            for axis, want in ((1, A.lse_rows(s)), (0, A.lse_cols(s))):
                seq = np.abs(_lse_f32_sequential(s, axis) - A._lse(s.astype(np.float32), axis)).max()
                red = np.abs(np.logaddexp.reduce(s.astype(np.float32), axis=axis) - A._lse(s.astype(np.float32), axis)).max()
                lse_floor, seq_floor = max(lse_floor, float(seq), float(red)), max(seq_floor, float(seq))
    for shape in G.HEAD_SHAPES + ((300, 1300),):
        fx = G.head_fixture(shape)
        tr = {"_full_layers": (0,)}
        O.forward_pair(fx.sd, O.make_conf(**fx.conf), *G.pair_inputs(fx, 0), dtype=np.float64, trace=tr)
        for im in (0, 1):
            x = tr[f"desc{im}_l0"].astype(np.float32)
            for kind in ("token", "match"):
                w, b = G.head_weights(fx.sd, kind, 0)
                z = (x @ w.reshape(-1).astype(np.float32) + np.float32(b.reshape(-1)[0])).astype(np.float32)
                e = np.exp(-np.abs(z))
                f32 = (z, np.where(z >= 0, np.float32(1) / (np.float32(1) + e), e / (np.float32(1) + e)), np.minimum(z, 0) - np.log1p(e), np.minimum(-z, 0) - np.log1p(e))
                assert all(v.dtype == np.float32 for v in f32)
                for got, want in zip(f32, A.heads(x, w, b)):
                    head_floor = max(head_floor, float((np.abs(got - want) / G.head_scale(x, w, b)).max()))
    print(f"floors: SIM {sim_floor:.3e} (recorded {G.SIM_FLOOR:.1e})  heads {head_floor:.3e} (recorded {G.HEAD_FLOOR:.1e})  LSE {lse_floor:.3e} (recorded {G.LSE_FLOOR:.1e})  LSE, sequential sum alone {seq_floor:.3e} (recorded {G.LSE_SEQ_FLOOR:.1e})")
    assert G.LSE_SEQ_FLOOR <= G.LSE_FLOOR
    for measured, recorded in ((sim_floor, G.SIM_FLOOR), (head_floor, G.HEAD_FLOOR), (lse_floor, G.LSE_FLOOR), (seq_floor, G.LSE_SEQ_FLOOR)):
        assert recorded / 2 <= measured <= recorded * 2, (measured, recorded)
