"""Triangulator on the GPU against the float64 definition (tests/triangulate_oracle.py) and against itself.

Bars and where they come from (tests/test_triangulate_cpu.py derives every figure without a GPU, from the oracle alone on the inputs of this file, and asserts
that the constants below are those figures):
  Tracks, states, lengths, ids and statuses are integers: they equal the oracle's exactly.
  A point may differ from the oracle's by ONE float32 ulp of the largest coordinate magnitude among the point and its cameras' centres (about 100 here: 7.6e-6).
  Both sides are fp64 under one accumulation order and one elimination, so only fused-multiply placement and the rounding of division and square root differ;
  the oracle itself moves by
  Q_POINT    1.50e-08  of that ulp at most between ascending and descending accumulation and between np.linalg.solve and the prescribed elimination
  Q_ERROR    5.90e-04  the same for track_error, in float32 ulps of the error
  and the CPU test asserts both are below 1e-3: the precondition of the one-ulp bar.
  A track the oracle alone places within a relative 1e-9 of a bar (a pivot, pz = 0, max_reproj_error, the cosine) may come out in either state and is excluded;
  at most 2 % of the tracks may be, and the CPU test asserts the oracle excludes NONE on these inputs.
The inputs are the scenes of tests/triangulate_oracle.py (640 x 480 images, camera (500, 500, 320, 240), six cameras about 6 units from a box of points
centred at (100, -50, 20), pixel noise 0.5, N = 96 rows per image, at most 17 pairs), built without a GPU."""
import numpy as np
import pytest
import torch

import triangulate_oracle as O
import lightglue_amd
from lightglue_amd import AbsolutePoseEstimator, NearestNeighborMatcher, Triangulator, TwoViewVerifier
from lightglue_amd._cabi import LightGlueAmdError
from test_gpu_abspose import MARGIN as ABSPOSE_MARGIN

Q_POINT, Q_ERROR = 1.50e-8, 5.90e-4
MAX_EXCLUDED = 0.02
INT_KEYS = ("track_id", "node_state", "track_length")
ALL_KEYS = INT_KEYS + ("points3d", "xyz", "track_error")

pytestmark = pytest.mark.gpu


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def store(inp):
    feats = {"keypoints": cuda(inp["kpts"])}
    if inp.get("num") is not None:
        feats["num_keypoints"] = torch.as_tensor(np.asarray(inp["num"]), dtype=torch.int32)
    return feats


def run(inp, tracks_only=False, pairs_on_device=True, expect=None, **conf):
    """one call; expect: the status codes the call must name in its error (then the error's outputs come back)"""
    tri = Triangulator(**conf)
    feats, pairs, m0 = store(inp), torch.from_numpy(np.asarray(inp["pairs"])), cuda(inp["matches0"])
    pairs = pairs.cuda() if pairs_on_device else pairs
    call = (lambda: tri.build_tracks(feats, pairs, m0, validate=False)) if tracks_only else \
        (lambda: tri.triangulate(feats, pairs, {"matches0": m0}, torch.from_numpy(inp["cams"]), cuda(inp["poses"]), validate=False))
    if expect is None:
        return call()
    with pytest.raises(LightGlueAmdError) as err:
        call()
    for word in expect:
        assert word in str(err.value), (word, str(err.value))
    return err.value.outputs


def host(out):
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}


def check_integers(got, want, what):
    assert got["num_tracks"] == want["num_tracks"], (what, got["num_tracks"], want["num_tracks"])
    for k in INT_KEYS:
        assert (got[k] == want[k]).all(), (what, k, int((got[k] != want[k]).sum()))
    assert list(got["state_counts"].values()) == want["state_counts"].tolist(), (what, got["state_counts"])
    assert (got["status"] == want["status"]).all(), (what, got["status"])


def check_points(got, want, inp, what):
    """every track the oracle triangulates: |dX| within one float32 ulp of the scale, track_error within one float32 ulp of the error; points3d is xyz
    scattered over the tracks' rows and NaN elsewhere"""
    scale = O.point_scale(inp, want)
    d = abs(got["xyz"].astype(np.float64) - want["xyz64"]).max(1)
    bar = np.array([O.ulp32(s) for s in scale])
    print("%s: %d tracks, worst |dX| / ulp %.3f" % (what, len(d), float((d / bar).max())))
    assert (d <= bar).all(), (what, float((d / bar).max()))
    de = abs(got["track_error"].astype(np.float64) - want["error64"])
    assert (de <= np.array([O.ulp32(e) for e in want["error64"]])).all(), what
    tid = got["track_id"]
    assert (got["points3d"][tid >= 0] == got["xyz"][tid[tid >= 0]]).all() and np.isnan(got["points3d"][tid < 0]).all(), what


def drop_near(got, want, what):
    """the tracks the oracle places within a relative 1e-9 of a bar are excluded (at most MAX_EXCLUDED of them): -> [K, N] bool, the nodes outside them"""
    near = [t for t in want["tracks"] if t[3]]
    assert len(near) <= MAX_EXCLUDED * max(len(want["tracks"]), 1), (what, len(near))
    keep = np.ones(want["node_state"].size, bool)
    for _, nodes, _, _ in near:
        keep[nodes] = False
    return keep.reshape(want["node_state"].shape)


@pytest.fixture(scope="module")
def main():
    """the main scene, each configuration run once: {name: host outputs}"""
    inp = O.oracle_input(O.main_scene())
    words = ("LG_ERR_INDEX", "pair %d" % O.BAD_INDEX, "pair %d" % O.SELF_PAIR)
    return {"tracks": host(run(inp, tracks_only=True, expect=words)), "full": host(run(inp, expect=words)),
            "start": host(run(inp, expect=words, refine=False))}


# ---------------------------------------------------------------------- 1. tracks are exact
def test_tracks_are_exact(main):
    for name, want in (("tracks", O.main_oracle(tracks_only=True)), ("full", O.main_oracle()), ("start", O.main_oracle(refine_on=False))):
        check_integers(main[name], want, name)
    got = main["tracks"]
    assert set(np.unique(got["node_state"]).tolist()) == {0, 1, 2} and "points3d" not in got and got["num_tracks"] == 51
    # ids follow the ascending order of the tracks' lowest nodes
    tid = got["track_id"].reshape(-1)
    first = [int(np.flatnonzero(tid == t)[0]) for t in range(got["num_tracks"])]
    assert first == sorted(first) == O.main_oracle(tracks_only=True)["names"].tolist()
    # too long: the same graph under max_track_length = 4
    inp = O.oracle_input(O.main_scene())
    short = host(run(inp, tracks_only=True, expect=("LG_ERR_INDEX",), max_track_length=4))
    want = O.main_oracle(tracks_only=True, max_len=4)
    check_integers(short, want, "max_track_length = 4")
    assert want["state_counts"][O.TOO_LONG] >= 10 and 3 in short["node_state"]
    # a pair list on the host, validated: the pair outside the store is a ValueError before anything runs
    with pytest.raises(ValueError, match="outside the feature stores"):
        Triangulator().build_tracks(store(inp), inp["pairs"].tolist(), cuda(inp["matches0"]))


# ---------------------------------------------------------------------- 2. one large component
def test_one_large_component_is_found_whole_and_reported_too_long():
    inp = O.big_component()
    want = O.triangulate(inp)
    assert [len(t[1]) for t in want["tracks"]] == [O.BIG_NODES] and want["state_counts"][O.TOO_LONG] == 1
    for tracks_only in (True, False):
        got = host(run(inp, tracks_only=tracks_only))
        check_integers(got, O.triangulate(inp, tracks_only=tracks_only), tracks_only)
        assert int((got["node_state"] == O.TOO_LONG).sum()) == O.BIG_NODES and got["num_tracks"] == 0 and (got["track_id"] == -1).all()
    # the same component within the longest track the triangulator takes on: sorted and found conflicted (300 nodes over 8 images)
    got = host(run(inp, tracks_only=True, max_track_length=1024))
    check_integers(got, O.triangulate(inp, tracks_only=True, max_len=1024), "1024")
    assert int((got["node_state"] == O.CONFLICT).sum()) == O.BIG_NODES


# ---------------------------------------------------------------------- 3. points
def test_points_lie_within_one_ulp_of_the_definition(main):
    inp = O.oracle_input(O.main_scene())
    check_points(main["full"], O.main_oracle(), inp, "refined")
    assert main["full"]["num_tracks"] == 51 and main["full"]["xyz"].shape == (51, 3)


# ---------------------------------------------------------------------- 4. every rejection state, planted
def test_every_rejection_state():
    sc = O.reject_scene()
    inp = O.oracle_input(sc)
    want = O.reject_oracle()
    got = host(run(inp, max_track_length=O.REJECT_MAX_LEN))
    keep = drop_near(got, want, "reject")
    assert (got["node_state"][keep] == want["node_state"][keep]).all(), np.flatnonzero(got["node_state"] != want["node_state"])
    state = got["node_state"].reshape(-1)
    for st, nodes in sc["want"].items():
        assert all(state[n] == st for n in nodes), (st, [state[n] for n in nodes])
    if keep.all():                                                       # nothing excluded (the CPU test asserts that for these inputs): everything is exact
        check_integers(got, want, "reject")
        check_points(got, want, inp, "reject")


# ---------------------------------------------------------------------- 5. determinism
def test_outputs_do_not_depend_on_the_list(main):
    inp = O.oracle_input(O.main_scene())
    words = ("LG_ERR_INDEX",)
    permuted, order = O.permute_pairs(inp, 3)
    again, moved, turned = host(run(inp, expect=words)), host(run(permuted, expect=words)), host(run(O.reverse_pairs(inp), expect=words))
    for k in ALL_KEYS:
        for what, other in (("the same call again", again), ("permuted", moved), ("every pair reversed", turned)):
            assert np.array_equal(main["full"][k], other[k], equal_nan=True), (what, k)
    assert (moved["status"] == main["full"]["status"][order]).all() and (turned["status"] == main["full"]["status"]).all()
    both = dict(inp, pairs=np.concatenate([inp["pairs"], inp["pairs"]]), matches0=np.concatenate([inp["matches0"], inp["matches0"]]))
    doubled = host(run(both, expect=words))
    for k in ALL_KEYS:
        assert np.array_equal(main["full"][k], doubled[k], equal_nan=True), ("the list twice", k)


# ---------------------------------------------------------------------- 6. refine=False; LG_ERR_CAMERA
def test_the_start_point_and_bad_cameras(main):
    inp = O.oracle_input(O.main_scene())
    check_points(main["start"], O.main_oracle(refine_on=False), inp, "start")
    moved = abs(main["start"]["xyz"] - main["full"]["xyz"]).max()
    assert 1e-4 < moved < 0.2, moved                                     # the refinement does something, and not much
    bad, sub, keep = O.bad_camera_scene()
    got = host(run(bad, expect=("LG_ERR_CAMERA",)))
    want = O.triangulate(bad)
    check_integers(got, want, "bad cameras")
    assert (got["status"] == np.where(keep, 0, O.LG_ERR_CAMERA)).all() and (~keep).sum() == 7
    assert (got["node_state"][[2, 5]] == 0).all() and (got["track_id"][[2, 5]] == -1).all() and np.isnan(got["points3d"][[2, 5]]).all()
    alone = host(run(sub))                                               # the same list without the flagged pairs: no status, no error
    for k in ALL_KEYS:
        assert np.array_equal(got[k], alone[k], equal_nan=True), k


# ---------------------------------------------------------------------- 7. the chain this feature exists for
def test_points3d_goes_unchanged_into_the_absolute_pose():
    sc = O.chain_scene()
    inp = O.oracle_input(sc)
    out = run(inp)
    want = O.triangulate(inp)
    check_integers(host(out), want, "chain")
    feats, cams = store(inp), torch.from_numpy(inp["cams"])
    est = AbsolutePoseEstimator(threshold=3.0, num_hypotheses=512, refine=True, seed=0)
    qm0 = cuda(sc["query_matches0"])
    a = est.estimate_pairs(feats, sc["query_pairs"].tolist(), qm0, cams, out["points3d"], pool=True)
    b = est.estimate_pairs(feats, sc["query_pairs"].tolist(), qm0, cams, cuda(want["points3d"]), pool=True)
    assert a["queries"].tolist() == [5] and int(a["num_inliers"][0]) >= 150
    # the two point sets differ by an ulp here and there: the counts may differ by the correspondences within the absolute pose's own margin of its threshold
    R, t = a["R"][0].cpu().numpy().astype(np.float64), a["t"][0].cpu().numpy().astype(np.float64)
    near = 0
    for p, (_, j) in enumerate(sc["query_pairs"]):
        rows = np.flatnonzero(sc["query_matches0"][p] >= 0)
        X = want["points3d"][j][sc["query_matches0"][p][rows]].astype(np.float64)
        px, pz = O.project_pixels(np.concatenate([R, t[:, None]], 1), inp["cams"][5], X)
        d = np.hypot(*(px - inp["kpts"][5][rows]).T)
        near += int((abs(d - 3.0) <= ABSPOSE_MARGIN * 3.0).sum())
    assert abs(int(a["num_inliers"][0]) - int(b["num_inliers"][0])) <= near, (int(a["num_inliers"][0]), int(b["num_inliers"][0]), near)
    # the recovered pose reprojects the planted points to where image 5 really sees them, within the estimator's threshold
    pl = sc["planted"]
    px, pz = O.project_pixels(np.concatenate([R, t[:, None]], 1), inp["cams"][5], pl["X"])
    clean = np.stack([pl["clean"][5, at[5]] for at in pl["rows"]])
    assert (pz > 0).all() and np.hypot(*(px - clean).T).max() <= 3.0


# ---------------------------------------------------------------------- 8. behind both matchers, with nothing copied to the host in between
def test_behind_the_matcher_and_the_verifier(monkeypatch):
    sc = O.chain_scene()
    inp = O.oracle_input(sc)
    rng = np.random.default_rng(41)
    desc = rng.standard_normal((O.K, O.N, 64))
    proto = rng.standard_normal((len(sc["planted"]["rows"]), 64))
    for j, at in enumerate(sc["planted"]["rows"]):
        for k, row in at.items():
            desc[k, row] = proto[j] + 0.05 * rng.standard_normal(64)       # descriptors follow the planted tracks
    feats = dict(store(inp), descriptors=cuda(desc.astype(np.float32)))
    pairs = inp["pairs"].tolist()
    matcher = NearestNeighborMatcher(mutual=True, distance_threshold=0.5)
    verifier = TwoViewVerifier(model="fundamental", threshold=3.0, num_hypotheses=512, refine=True, seed=0)
    tri = Triangulator()
    cams, poses = torch.from_numpy(inp["cams"]), cuda(inp["poses"])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        verified = verifier.verify_pairs(feats, pairs, matcher.match_pairs(feats, pairs, deferred=True))
        assert verified["matches0"].is_cuda and verified["matches0"].dtype is torch.int64 and verified["matches0"].is_contiguous()
        # from here to the outputs: one read of the host-side sizes, no copy of a tensor to the host
        calls = {"tolist": 0, "cpu": 0}
        for name in calls:
            real = getattr(torch.Tensor, name)
            monkeypatch.setattr(torch.Tensor, name, lambda self, *a, _real=real, _name=name, **k: (calls.__setitem__(_name, calls[_name] + 1), _real(self, *a, **k))[1])
        out = tri.triangulate(feats, pairs, verified, cams, poses, validate=False)       # (validation reads the pair list on the host: not what is counted)
        monkeypatch.undo()
        assert calls == {"tolist": 1, "cpu": 0}, calls
        same = lightglue_amd.triangulate_tracks(tri, verified["matches0"], feats, pairs, cams, poses)
    side.synchronize()
    for k in ALL_KEYS:
        assert torch.equal(out[k].nan_to_num(1e9), same[k].nan_to_num(1e9)), k
    # what the verifier kept is a subset of the planted matches, so every track is a part of a planted track; most are whole and their points are the planted ones
    got, v0 = host(out), verified["matches0"].cpu().numpy()
    assert ((v0 == inp["matches0"]) | (v0 == -1)).all() and (v0 >= 0).sum() >= 0.9 * (inp["matches0"] >= 0).sum()
    want = O.triangulate(dict(inp, matches0=v0))
    check_integers(got, want, "verified")
    check_points(got, want, inp, "verified")
    assert got["num_tracks"] >= 70
