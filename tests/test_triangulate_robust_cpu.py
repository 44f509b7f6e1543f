"""The triangulator's robust mode without a GPU: the float64 definition (tests/triangulate_robust_oracle.py) on the stray scene gives the counts the mode was
proposed with, recovers every planted track and names exactly the strays; the oracle alone leaves out no component of any scene of
tests/test_gpu_triangulate_robust.py (the near-bar cap); the binding mirrors the header; lg_triangulate_robust refuses what lies outside its envelope before
it touches a GPU; `Triangulator` checks the new configuration."""
import ctypes as C
import itertools
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import triangulate_oracle as O
import triangulate_robust_oracle as R
import test_gpu_triangulate_robust as G
from lightglue_amd import Triangulator, _cabi
from lightglue_amd.triangulate import ROBUST_STATES, STATES
from test_triangulate_cpu import good_io
from test_twoview_cpu import typed_fields_of

HEADER = (Path(__file__).resolve().parent.parent / "include" / "lightglue_amd.h").read_text()


# ---------------------------------------------------------------------- the definition on the stray scene
def test_stray_scene_counts_and_planted_points():
    """measured with the oracles alone: 55 components; lg_triangulate's definition keeps 30 (16 conflict, 9 reprojection); one round keeps 55 tracks and
    drops 44 nodes; two rounds give all 60 planted tracks, each within 0.02 units of its planted point (0.017 measured), with exactly the 20 strays left over"""
    sc = R.stray_scene()
    inp, pl = O.oracle_input(sc), sc["planted"]
    assert inp["kpts"].shape == (8, 96, 2) and len(inp["pairs"]) == 28 and len(pl["rows"]) == 60 and min(len(at) for at in pl["rows"]) >= 3
    assert len(set(sc["strays"].tolist())) == R.STRAYS == 20 and sc["merged"] == [(20, 21), (22, 23), (24, 25), (26, 27), (28, 29)]
    for row in inp["matches0"]:                                          # one-to-one, so that the reversed list holds the same edges
        live = row[row >= 0]
        assert len(set(live.tolist())) == len(live)
    plain = O.triangulate(inp)
    assert len(plain["tracks"]) == 55 and plain["state_counts"].tolist() == [0, 30, 16, 0, 0, 0, 9, 0]
    for nh in (64, 16):
        one = R.answer("stray", nh, 1)
        assert (one["num_tracks"], one["num_outliers"], one["num_split"]) == (55, 44, 0) and one["state_counts"].tolist() == [0, 55, 0, 0, 0, 0, 0, 0], nh
        two = R.answer("stray", nh, 2)
        assert (two["num_tracks"], two["num_outliers"], two["num_split"]) == (60, 20, 5) and two["state_counts"].tolist() == [0, 60, 0, 0, 0, 0, 0, 0], nh
        state, tid = two["node_state"].reshape(-1), two["track_id"].reshape(-1)
        assert sorted(np.flatnonzero(state == R.OUTLIER).tolist()) == sorted(sc["strays"].tolist()) and O.CONFLICT not in state
        assert (tid[state == R.OUTLIER] == -1).all() and np.isnan(two["points3d"].reshape(-1, 3)[state == R.OUTLIER]).all()
        node_of = {k * O.N + r: j for j, at in enumerate(pl["rows"]) for k, r in at.items()}
        found, worst = set(), 0.0
        for t in range(two["num_tracks"]):
            nodes = np.flatnonzero(tid == t)
            planted = {node_of[v] for v in nodes}
            assert len(planted) == 1 and len(nodes) == two["track_length"][t] == len(pl["rows"][min(planted)])       # a whole planted track, and only it
            j = planted.pop()
            found.add(j)
            worst = max(worst, float(np.linalg.norm(two["xyz64"][t] - pl["X"][j])))
        print("stray scene, %d hypotheses: worst distance to the planted point %.4f" % (nh, worst))
        assert len(found) == 60 and worst <= 0.02
        # ids are dense in ascending (component, round)
        first = [(int(two["names"][t]), t) for t in range(two["num_tracks"])]
        assert first == sorted(first)


def test_hypotheses_are_a_function_of_the_length_alone():
    for L, nh in ((2, 64), (8, 64), (11, 64), (12, 64), (15, 64), (8, 16), (300, 256), (1024, 4096)):
        Q = L * (L - 1) // 2
        got = R.hypotheses(L, nh)
        assert len(got) == min(Q, nh) and all(0 <= i < j < L for i, j in got) and got == sorted(got) and len(set(got)) == len(got)
        if Q <= nh:
            assert got == list(itertools.combinations(range(L), 2))
        else:                                                            # pair number floor(h Q / nh): by counting the pairs in front of it
            for h in (0, 1, nh // 2, nh - 1):
                i, j = got[h]
                assert i * (2 * L - i - 1) // 2 + (j - i - 1) == h * Q // nh
    assert R.hypotheses(8, 16)[-1] == (5, 7) and len(R.hypotheses(15, 64)) == 64 and len(R.hypotheses(15, 128)) == 105


def gpu_scenes():
    """(name, the oracle's answer) of every comparison of tests/test_gpu_triangulate_robust.py"""
    yield from ((("stray", nh, mt), R.answer("stray", nh, mt)) for nh in (64, 16) for mt in (2, 1))
    yield from ((("wide", nh), R.answer("wide", nh)) for nh in (64, 128))
    yield from ((name, R.answer(name)) for name in ("big", "main", "bad cameras"))
    yield "bad cameras, without", R.triangulate(O.bad_camera_scene()[1])


def test_the_oracle_stays_within_the_near_cap():
    """decided by the oracle alone: at most 1 % of a scene's components within a relative 1e-9 of a decision — and here none at all (0.5 px noise, a 4 px bar)"""
    assert G.MAX_EXCLUDED == 0.01 and O.NEAR == 1e-9
    for name, out in gpu_scenes():
        near = sum(bool(t[3]) for t in out["tracks"])
        assert near <= G.MAX_EXCLUDED * len(out["tracks"]) and near == 0, (name, near)
    # what the GPU tests count on
    wide, big, main = R.answer("wide"), R.answer("big"), R.answer("main")
    assert (wide["num_tracks"], wide["num_outliers"]) == (8, 24) and sorted(np.flatnonzero(wide["node_state"].reshape(-1) == 8).tolist()) == sorted(R.wide_scene()["strays"].tolist())
    assert big["num_tracks"] >= 2 and big["num_outliers"] == O.BIG_NODES - int(big["track_length"].sum()) and big["num_split"] == 1
    assert (main["num_tracks"], main["num_split"], main["num_outliers"]) == (53, 1, 0) and sum(t[4] for t in main["tracks"]) == 51


# ---------------------------------------------------------------------- binding, refusals, workspace
def test_binding_mirrors_the_header():
    fields = typed_fields_of("lg_triangulate_robust_io")
    assert fields == [("base", "lg_triangulate_io", False), ("num_hypotheses", "int32_t", False), ("max_tracks", "int32_t", False), ("outlier_counts", "int32_t", True)]
    assert list(_cabi.LgTriangulateRobustIO._fields_) == [("base", _cabi.LgTriangulateIO), ("num_hypotheses", C.c_int32), ("max_tracks", C.c_int32), ("outlier_counts", C.c_void_p)]
    for name in ("LG_TRI_MAX_HYPOTHESES", "LG_TRI_MAX_TRACKS"):
        assert int(re.search(r"#define %s (\d+)" % name, HEADER).group(1)) == getattr(_cabi, name)
    assert (_cabi.LG_TRI_MAX_HYPOTHESES, _cabi.LG_TRI_MAX_TRACKS) == (4096, 4)
    lib = _cabi.load()
    assert lib.lg_triangulate_robust.argtypes == [C.POINTER(_cabi.LgTriangulateRobustIO), C.c_void_p]
    assert lib.lg_triangulate_robust_workspace_bytes.argtypes == [C.c_int64, C.c_int32, C.c_int32] and lib.lg_triangulate_robust_workspace_bytes.restype is C.c_int64
    assert "lg_triangulate_robust" in _cabi.EXPORTED_SYMBOLS and "lg_triangulate_robust_workspace_bytes" in _cabi.EXPORTED_SYMBOLS
    assert STATES == ROBUST_STATES[:8] and ROBUST_STATES[R.OUTLIER] == "outlier" and len(ROBUST_STATES) == 9


def robust_io(num_hypotheses=64, max_tracks=2, outlier_counts=256, **over):
    return _cabi.LgTriangulateRobustIO(base=good_io(**over), num_hypotheses=num_hypotheses, max_tracks=max_tracks, outlier_counts=outlier_counts)


def test_envelope_is_refused_without_touching_a_gpu():
    """every pointer is a fake non-null value: a refusal that came after anything was dereferenced or launched would have crashed"""
    lib = _cabi.load()
    R_, T, inv = _cabi.LG_TRI_REFINE, _cabi.LG_TRI_TRACKS_ONLY, _cabi.LG_ERR_INVALID
    assert lib.lg_triangulate_robust(None, None) == inv and b"null io" in lib.lg_last_error()
    refused = [
        (dict(flags=T), b"LG_TRI_TRACKS_ONLY"), (dict(flags=R_ | T), b"LG_TRI_TRACKS_ONLY"), (dict(flags=1), b"flag"), (dict(flags=R_ | 1 << 31), b"flag"),
        (dict(num_hypotheses=0), b"num_hypotheses"), (dict(num_hypotheses=-1), b"num_hypotheses"), (dict(num_hypotheses=4097), b"num_hypotheses"),
        (dict(max_tracks=0), b"max_tracks"), (dict(max_tracks=5), b"max_tracks"), (dict(max_tracks=-2), b"max_tracks"),
        (dict(outlier_counts=None), b"outlier_counts"),
        # the existing envelope, unchanged
        (dict(n=-1), b"LG_MAX_KEYPOINTS"), (dict(n=8193), b"LG_MAX_KEYPOINTS"), (dict(images=-1), b"LG_MAX_ROWS"), (dict(images=257, n=8192), b"LG_MAX_ROWS"),
        (dict(pairs=-1), b"2^31"), (dict(pairs=2 ** 20, n=2048), b"2^31"),
        (dict(max_track_length=1), b"max_track_length"), (dict(max_track_length=1025), b"max_track_length"),
        (dict(max_reproj_error=0.0), b"max_reproj_error"), (dict(max_reproj_error=float("nan")), b"max_reproj_error"), (dict(max_reproj_error=float("inf")), b"max_reproj_error"),
        (dict(min_angle=-0.5), b"min_angle"), (dict(min_angle=180.0), b"min_angle"),
        (dict(workspace_bytes=1000), b"workspace holds"), (dict(workspace=None), b"null workspace"), (dict(workspace=128), b"256-byte aligned"),
    ]
    refused += [(dict({k: None}), b"null pointer") for k in ("kpts", "index0", "index1", "matches0", "cameras", "poses", "points3d", "track_id", "node_state", "xyz",
                                                             "track_length", "track_error", "counts", "status")]
    for over, word in refused:
        assert lib.lg_triangulate_robust(C.byref(robust_io(**over)), None) == inv, over
        assert word in lib.lg_last_error() and b"lg_triangulate_robust" in lib.lg_last_error(), (over, lib.lg_last_error())
    # a workspace of the plain call's size is too small for the robust one
    plain = lib.lg_triangulate_workspace_bytes(3, 100, R_)
    assert lib.lg_triangulate_robust(C.byref(robust_io(workspace_bytes=plain)), None) == inv and b"lg_triangulate_robust_workspace_bytes" in lib.lg_last_error()
    # the workspace: the plain one, two int32 per node, and per slot (possible track x max_tracks) three int32 and 16 bytes; -1 outside the envelope
    up = lambda b: (b + 255) // 256 * 256
    for images, n, mt in ((1, 0, 1), (1, 1, 4), (6, 96, 2), (8, 96, 1), (16, 2048, 2), (256, 8192, 4)):
        nodes = images * n
        slots = nodes // 2 * mt
        want = lib.lg_triangulate_workspace_bytes(images, n, R_) + 2 * up(4 * nodes) + 3 * up(4 * slots) + up(16 * slots)
        assert lib.lg_triangulate_robust_workspace_bytes(images, n, mt) == want, (images, n, mt)
    for bad in ((1, 8193, 2), (-1, 10, 2), (1, -1, 2), (6, 96, 0), (6, 96, 5), (257, 8192, 2)):
        assert lib.lg_triangulate_robust_workspace_bytes(*bad) == -1, bad


def test_python_configuration():
    for bad in (dict(num_hypotheses=0), dict(num_hypotheses=4097), dict(num_hypotheses=2.5), dict(max_tracks=0), dict(max_tracks=5), dict(max_tracks=1.5)):
        with pytest.raises(ValueError):
            Triangulator(robust=True, **bad)
    tri = Triangulator()
    assert (tri.robust, tri.num_hypotheses, tri.max_tracks) == (False, 64, 2) and (R.NUM_HYPOTHESES, R.MAX_TRACKS) == (64, 2)
    Triangulator(robust=True, num_hypotheses=1, max_tracks=1), Triangulator(robust=True, num_hypotheses=4096, max_tracks=4)
    feats = {"keypoints": torch.zeros(2, 8, 2)}
    with pytest.raises(ValueError, match="robust"):
        Triangulator(robust=True).build_tracks(feats, [(0, 1)], torch.full((1, 8), -1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Triangulator(robust=True).triangulate(feats, [(0, 1)], torch.full((1, 8), -1), torch.tensor([O.CAM, O.CAM]), torch.zeros(2, 3, 4))
