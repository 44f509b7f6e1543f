"""The triangulator's robust mode on the GPU against the float64 definition (tests/triangulate_robust_oracle.py) and against itself.

Bars, as in tests/test_gpu_triangulate.py: tracks, states, lengths, ids, counts and statuses are integers and equal the oracle's exactly; a point may differ from
the oracle's by ONE float32 ulp of the largest coordinate magnitude among the point and its cameras' centres, track_error by one float32 ulp of the error.
The winner of a round is decided by integers (images that pass) and the consensus by comparisons of errors, so a component the oracle alone places within a
relative 1e-9 of such a decision (`near`) may come out either way and is left out; at most MAX_EXCLUDED = 1 % of a scene's components may be, and
tests/test_triangulate_robust_cpu.py asserts that the oracle leaves out NONE on the scenes of this file.
Scenes (tests/triangulate_robust_oracle.py): `stray` K = 8, N = 96, 60 tracks, 20 stray observations, 5 merged pairs of tracks; `wide` K = 12, 8 tracks of 15
nodes (Q = 105 index pairs > 64 hypotheses); `big` one component of 300 nodes (lists longer than a wave, four rounds); the main and bad-camera scenes of
tests/triangulate_oracle.py."""
import numpy as np
import pytest
import torch

import triangulate_oracle as O
import triangulate_robust_oracle as R
from lightglue_amd import AbsolutePoseEstimator, BundleAdjuster, Triangulator
from lightglue_amd._cabi import LightGlueAmdError
from test_gpu_triangulate import ALL_KEYS, check_integers, check_points, cuda, host, store

MAX_EXCLUDED = 0.01
STRAY_QUERY = R.STRAY_K - 1                                             # the image the chain test localises against the others

pytestmark = pytest.mark.gpu


def run(inp, expect=None, **conf):
    """one robust call (device outputs); expect: the words the call's error must hold (then the error's outputs come back)"""
    tri = Triangulator(robust=True, **conf)
    call = lambda: tri.triangulate(store(inp), torch.from_numpy(np.asarray(inp["pairs"])).cuda(), {"matches0": cuda(inp["matches0"])},
                                   torch.from_numpy(inp["cams"]), cuda(inp["poses"]), validate=False)
    if expect is None:
        return call()
    with pytest.raises(LightGlueAmdError) as err:
        call()
    for word in expect:
        assert word in str(err.value), (word, str(err.value))
    return err.value.outputs


def check(got, want, inp, what):
    """everything against the oracle; the components it calls near are left out of nothing here unless there are some (then only the cap is checked)"""
    near = [t for t in want["tracks"] if t[3]]
    assert len(near) <= MAX_EXCLUDED * max(len(want["tracks"]), 1), (what, len(near))
    if near:
        keep = np.ones(want["node_state"].size, bool)
        for t in near:
            keep[t[1]] = False
        assert (got["node_state"].reshape(-1)[keep] == want["node_state"].reshape(-1)[keep]).all(), what
        return
    check_integers(got, want, what)
    assert (got["num_outliers"], got["num_split"]) == (want["num_outliers"], want["num_split"]), (what, got["num_outliers"], got["num_split"])
    check_points(got, want, inp, what)


def same_bits(a, b, what):
    for k in ALL_KEYS:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)
    assert (a["num_tracks"], a["num_outliers"], a["num_split"], a["state_counts"]) == (b["num_tracks"], b["num_outliers"], b["num_split"], b["state_counts"]), what


# ---------------------------------------------------------------------- 1. the stray scene against the oracle
@pytest.mark.parametrize("num_hypotheses, max_tracks", [(64, 2), (64, 1), (16, 2), (16, 1)])
def test_stray_scene_equals_the_oracle(num_hypotheses, max_tracks):
    inp = O.oracle_input(R.stray_scene())
    want = R.answer("stray", num_hypotheses, max_tracks)
    got = host(run(inp, num_hypotheses=num_hypotheses, max_tracks=max_tracks))
    check(got, want, inp, (num_hypotheses, max_tracks))
    assert got["num_tracks"] == (60 if max_tracks == 2 else 55) and got["num_outliers"] == (20 if max_tracks == 2 else 44)
    assert set(np.unique(got["node_state"]).tolist()) == {0, 1, 8}
    if max_tracks == 2:
        assert sorted(np.flatnonzero(got["node_state"].reshape(-1) == R.OUTLIER).tolist()) == sorted(R.stray_scene()["strays"].tolist())
        assert got["num_split"] == R.MERGES


# ---------------------------------------------------------------------- 2. more hypotheses than lanes take at once, lists longer than a wave, four rounds
def test_hypothesis_stride_and_long_lists():
    inp = O.oracle_input(R.wide_scene())
    want = R.answer("wide")
    assert [len(t[1]) for t in want["tracks"]] == [15] * R.WIDE_TRACKS
    check(host(run(inp)), want, inp, "wide")
    check(host(run(inp, num_hypotheses=128)), R.answer("wide", 128), inp, "wide, every pair tried")
    big = O.big_component()
    want = R.answer("big")
    assert [len(t[1]) for t in want["tracks"]] == [O.BIG_NODES] and want["num_tracks"] >= 2
    got = host(run(big, max_track_length=1024, num_hypotheses=256, max_tracks=4))
    check(got, want, big, "big")
    short = host(run(big))                                              # the same component under max_track_length = 128: too long, as in the plain mode
    assert int((short["node_state"] == O.TOO_LONG).sum()) == O.BIG_NODES and short["num_tracks"] == 0 and short["state_counts"]["too_long"] == 1
    assert (short["num_outliers"], short["num_split"]) == (0, 0)


# ---------------------------------------------------------------------- 3. a whole consensus is the plain mode's track, bit for bit
def test_whole_consensus_has_the_plain_bits():
    inp = O.oracle_input(O.main_scene())
    words = ("LG_ERR_INDEX",)

    def plain():
        tri = Triangulator()
        with pytest.raises(LightGlueAmdError) as err:
            tri.triangulate(store(inp), torch.from_numpy(inp["pairs"]).cuda(), cuda(inp["matches0"]), torch.from_numpy(inp["cams"]), cuda(inp["poses"]), validate=False)
        return host(err.value.outputs)
    before, got, after = plain(), host(run(inp, expect=words)), plain()
    want = R.answer("main")
    check(got, want, inp, "main")
    whole = [t for t in want["tracks"] if t[4]]
    assert len(whole) >= 50 and got["num_split"] == 1                   # the one conflicted component comes apart into its two tracks
    for _, nodes, state, _, _ in whole:
        k, i = nodes // O.N, nodes % O.N
        assert (got["node_state"][k, i] == before["node_state"][k, i]).all() and state == O.DONE
        assert np.array_equal(got["points3d"][k, i], before["points3d"][k, i])
        a, b = got["track_id"][k[0], i[0]], before["track_id"][k[0], i[0]]
        assert got["track_error"][a] == before["track_error"][b] and got["track_length"][a] == before["track_length"][b] == len(nodes)
    check_integers(before, O.main_oracle(), "plain")
    assert set(before) == {"track_id", "node_state", "num_tracks", "track_length", "state_counts", "status", "points3d", "xyz", "track_error"}
    for k in ALL_KEYS:
        assert np.array_equal(before[k], after[k], equal_nan=True), k


# ---------------------------------------------------------------------- 4. the outputs are a function of the edge set
def test_outputs_do_not_depend_on_the_list():
    inp = O.oracle_input(R.stray_scene())
    first = host(run(inp))
    permuted, order = O.permute_pairs(inp, 3)
    both = dict(inp, pairs=np.concatenate([inp["pairs"], inp["pairs"][:1]]), matches0=np.concatenate([inp["matches0"], inp["matches0"][:1]]))
    for what, other in (("the same call again", inp), ("permuted", permuted), ("every pair reversed", O.reverse_pairs(inp)), ("a pair listed twice", both)):
        same_bits(first, host(run(other)), what)
    # a pair outside the store and a pair (a, a): flagged, and nothing else moves
    main = O.oracle_input(O.main_scene())
    regular = np.arange(len(O.PAIRS) - 2)
    flagged = host(run(main, expect=("LG_ERR_INDEX", "pair %d" % O.BAD_INDEX, "pair %d" % O.SELF_PAIR)))
    same_bits(flagged, host(run(dict(main, pairs=main["pairs"][regular], matches0=main["matches0"][regular]))), "bad index")
    assert flagged["status"].tolist() == [0] * len(regular) + [O.LG_ERR_INDEX] * 2
    # an image with a bad camera: its pairs are flagged, its rows are in no track, and every other track is what the list without those pairs gives
    bad, sub, keep = O.bad_camera_scene()
    got = host(run(bad, expect=("LG_ERR_CAMERA",)))
    check(got, R.answer("bad cameras"), bad, "bad cameras")
    assert (got["status"] == np.where(keep, 0, O.LG_ERR_CAMERA)).all()
    assert (got["node_state"][[2, 5]] == 0).all() and (got["track_id"][[2, 5]] == -1).all() and np.isnan(got["points3d"][[2, 5]]).all()
    same_bits(got, host(run(sub)), "bad cameras")


# ---------------------------------------------------------------------- 5. the chain: into the bundle adjuster and into the absolute pose
def test_robust_tracks_go_unchanged_into_the_adjuster_and_the_absolute_pose():
    sc = R.stray_scene()
    inp = O.oracle_input(sc)
    feats, cams, poses = store(inp), torch.from_numpy(inp["cams"]), cuda(inp["poses"])
    out = Triangulator(robust=True).triangulate(feats, inp["pairs"].tolist(), cuda(inp["matches0"]), cams, poses)
    done, outlier = out["node_state"] == 1, out["node_state"] == R.OUTLIER
    assert int(outlier.sum()) == out["num_outliers"] == R.STRAYS and bool(torch.isnan(out["points3d"][outlier]).all())
    ba = BundleAdjuster().adjust(feats, out, cams, poses, [0, 1])
    assert ba["num_observations"] == int(done.sum()) and bool((ba["node_state"][outlier] == 0).all())
    assert ba["final_cost"] <= ba["initial_cost"]
    # image 7 localised against the points of the others; its matches also lead to the outlier rows, whose points are NaN
    query = STRAY_QUERY
    pairs = [(query, j) for j in range(query)]
    qm0 = O.match_rows(pairs, sc["planted"]["rows"])
    for p, (_, j) in enumerate(pairs):
        free = np.flatnonzero(qm0[p] < 0)
        rows = (sc["strays"] % O.N)[sc["strays"] // O.N == j]
        qm0[p, free[:len(rows)]] = rows
    model = out["points3d"].clone()
    model[query] = float("nan")
    est = AbsolutePoseEstimator(threshold=3.0, num_hypotheses=512, refine=True, seed=0)
    a = est.estimate_pairs(feats, pairs, cuda(qm0), cams, model, pool=True)
    assert a["queries"].tolist() == [query]
    R7, t7 = a["R"][0].cpu().numpy().astype(np.float64), a["t"][0].cpu().numpy().astype(np.float64)
    pl = sc["planted"]
    seen = [j for j, at in enumerate(pl["rows"]) if query in at]
    px, pz = O.project_pixels(np.concatenate([R7, t7[:, None]], 1), inp["cams"][query], pl["X"][seen])
    clean = np.stack([pl["clean"][query, pl["rows"][j][query]] for j in seen])
    assert len(seen) >= 20 and int(a["num_inliers"][0]) >= len(seen) and (pz > 0).all() and np.hypot(*(px - clean).T).max() <= 3.0
