"""The triangulator without a GPU: the float64 definition (tests/triangulate_oracle.py) recovers the planted points within a bound derived from the noise and
the geometry, its scenes hold what they say, the binding mirrors the header, lg_triangulate refuses what lies outside its envelope before it touches a GPU,
`Triangulator` checks its configuration, and the constants of tests/test_gpu_triangulate.py are derived here — from the oracle alone on that file's own
inputs — and compared with the constants in its header."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import triangulate_oracle as O
import test_gpu_triangulate as G
from lightglue_amd import Triangulator, _cabi
from lightglue_amd._readers import as_poses
from lightglue_amd.triangulate import STATES
from test_twoview_cpu import typed_fields_of

HEADER = (Path(__file__).resolve().parent.parent / "include" / "lightglue_amd.h").read_text()


def observations(inp, nodes):
    n = inp["kpts"].shape[1]
    flat = inp["kpts"].reshape(-1, 2)
    return [(flat[v], O.record(inp["cams"][v // n], inp["poses"][v // n])) for v in nodes]


# ---------------------------------------------------------------------- the definition on the scenes
def test_oracle_recovers_the_planted_points():
    """The bound, per track, from the noise and the geometry: a pixel error e turns a ray by e / f, which moves the point by D e / f across the ray at depth D
    and by D e / (f sin a) along it when the widest pair of rays meets at the angle a.  With n views the least-squares point averages, but the bound does not
    count on it; e is taken as 5 sigma of the two-dimensional noise of BOTH rays of the widest pair: 5 sqrt(2) sigma."""
    sc = O.main_scene()
    inp, pl = O.oracle_input(sc), sc["planted"]
    out = O.main_oracle()
    assert out["num_tracks"] == 51 and out["state_counts"].tolist() == [0, 51, 1, 0, 0, 0, 0, 0]
    node_of = {k * O.N + r: j for j, at in enumerate(pl["rows"]) for k, r in at.items()}
    worst, angles = 0.0, []
    for t, name in enumerate(out["names"]):
        nodes = np.flatnonzero(out["track_id"].reshape(-1) == t)
        planted = {node_of[v] for v in nodes}
        assert len(planted) == 1                                        # a track of the graph is a part of ONE planted track
        X = pl["X"][planted.pop()]
        obs = observations(inp, nodes)
        a = np.radians(O.widest_angle(obs, X))
        depth = max(np.linalg.norm(X - rec[2]) for _, rec in obs)
        bound = 5 * np.sqrt(2) * O.SIGMA * depth / (O.CAM[0] * np.sin(a))
        err = np.linalg.norm(out["xyz64"][t] - X)
        worst, angles = max(worst, err / bound), angles + [np.degrees(a)]
        assert err <= bound, (t, err, bound)
        # Gauss-Newton never raises the cost
        start = O.start_point(obs)
        assert O.cost(obs, out["xyz64"][t]) <= O.cost(obs, start) * (1 + 1e-12)
    print("planted points: worst error / bound %.3f, widest angles %.1f .. %.1f degrees, largest track error %.2f px" % (worst, min(angles), max(angles), out["error64"].max()))
    assert min(angles) > 5 * O.MIN_ANGLE and out["error64"].max() < O.MAX_ERR / 2        # nothing of the clean scene near a bar


def test_the_scenes_are_what_they_say():
    sc = O.main_scene()
    inp = O.oracle_input(sc)
    assert inp["kpts"].shape == (O.K, O.N, 2) and len(inp["pairs"]) <= 17 and O.N % 64
    only = O.main_oracle(tracks_only=True)
    rows = sc["planted"]["rows"]
    node = lambda j, k: k * O.N + rows[j][k]
    tid, state = only["track_id"].reshape(-1), only["node_state"].reshape(-1)
    a, b = sc["odd"]["conflict"]
    assert {state[node(j, k)] for j in (a, b) for k in rows[j]} == {O.CONFLICT}                       # made through image 4
    j = sc["odd"]["chain"]
    assert (0, 2) in O.MISSING and tid[node(j, 0)] == tid[node(j, 2)] >= 0                            # 0 - 2 hold together through image 1 alone
    j = sc["odd"]["unheld"]
    assert state[node(j, 0)] == state[node(j, 2)] == O.NONE
    assert only["status"].tolist() == [0] * (len(O.PAIRS) - 2) + [O.LG_ERR_INDEX] * 2
    m0 = inp["matches0"]
    live = np.asarray(O.NUM)
    beyond_a = sum(int((m0[p, live[x]:] >= 0).sum()) for p, (x, y) in enumerate(O.PAIRS) if x < O.K and x != y)
    beyond_b = sum(int((m0[p, :live[x]] >= live[y]).sum()) for p, (x, y) in enumerate(O.PAIRS) if max(x, y) < O.K and x != y)
    assert beyond_a >= 2 and beyond_b >= 3 and (m0 >= O.N).any() and (m0 == -1).any()
    # the edges of the list, of the list reversed, permuted and doubled are one set
    edge_set = O.edges(inp["pairs"], m0, O.K, O.N, inp["num"])[0]
    rev, (perm, _) = O.reverse_pairs(inp), O.permute_pairs(inp, 3)
    assert edge_set == O.edges(rev["pairs"], rev["matches0"], O.K, O.N, inp["num"])[0] == O.edges(perm["pairs"], perm["matches0"], O.K, O.N, inp["num"])[0]
    without = [p for p in range(len(O.PAIRS)) if p not in (len(O.REGULAR), O.REVERSED)]              # the pair listed twice and the reversed one add nothing
    assert edge_set == O.edges(inp["pairs"][without], m0[without], O.K, O.N, inp["num"])[0] and len(edge_set) > 150
    # the unread rows would have made edges had they been read
    assert len(O.edges(inp["pairs"], m0, O.K, O.N, None)[0]) > len(edge_set)
    # every rejection state is planted where the scene says, and max_track_length = 4 turns the long tracks away
    rej, want = O.reject_scene(), O.reject_oracle()
    state = want["node_state"].reshape(-1)
    assert sorted(rej["want"]) == [O.TOO_LONG, O.DEGENERATE, O.BEHIND, O.REPROJECTION, O.ANGLE]
    for st, nodes in rej["want"].items():
        assert all(state[v] == st for v in nodes), (st, [state[v] for v in nodes])
    assert want["state_counts"][O.DONE] >= 30 and want["state_counts"][O.CONFLICT] == 0
    big = O.triangulate(O.big_component())
    assert [len(t[1]) for t in big["tracks"]] == [O.BIG_NODES] and len(O.big_component()["pairs"]) == 16
    bad, sub, keep = O.bad_camera_scene()
    assert O.triangulate(bad)["status"].tolist() == np.where(keep, 0, O.LG_ERR_CAMERA).tolist()
    chain = O.triangulate(O.oracle_input(O.chain_scene()))
    assert chain["num_tracks"] == 80 and (chain["track_id"][5] == -1).all()                           # image 5 is held out of the model


def test_host_union_find_names_components_by_their_lowest_node():
    rng = np.random.default_rng(1)
    for _ in range(20):
        nodes = 60
        edge_set = {tuple(sorted(rng.choice(nodes, 2, replace=False).tolist())) for _ in range(int(rng.integers(0, 50)))}
        name = O.components(nodes, edge_set)
        adj = np.eye(nodes, dtype=bool)
        for u, v in edge_set:
            adj[u, v] = adj[v, u] = True
        for _ in range(6):
            adj = (adj.astype(int) @ adj.astype(int)) > 0                # reachability within 64 steps
        assert (name == np.array([np.flatnonzero(adj[v])[0] for v in range(nodes)])).all()


def test_the_prescribed_elimination():
    rng = np.random.default_rng(2)
    for _ in range(100):
        A = rng.standard_normal((3, 3))
        M, b = A @ A.T + 1e-3 * np.eye(3), rng.standard_normal(3)
        assert abs(O.solve3(M, b) - np.linalg.solve(M, b)).max() <= 1e-9 * abs(np.linalg.solve(M, b)).max()
    d = np.array([0.6, 0.0, 0.8])
    assert O.solve3(2 * (np.eye(3) - np.outer(d, d)), np.ones(3)) is None and O.solve3(np.zeros((3, 3)), np.ones(3)) is None
    assert O.solve3(np.full((3, 3), np.nan), np.ones(3)) is None


# ---------------------------------------------------------------------- binding, refusals, workspace
def test_binding_mirrors_the_header():
    scalars = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "float": C.c_float}
    want = [(name, C.c_void_p if pointer else scalars[ctype]) for name, ctype, pointer in typed_fields_of("lg_triangulate_io")]
    assert want == list(_cabi.LgTriangulateIO._fields_)
    for name in ("LG_TRI_REFINE", "LG_TRI_TRACKS_ONLY"):
        assert int(re.search(r"#define %s (\d+)u" % name, HEADER).group(1)) == getattr(_cabi, name)
    assert int(re.search(r"#define LG_TRI_MAX_TRACK_LENGTH (\d+)", HEADER).group(1)) == _cabi.LG_TRI_MAX_TRACK_LENGTH == 1024
    assert [_cabi.LG_TRI_REFINE, _cabi.LG_TRI_TRACKS_ONLY] == [2 * _cabi.LG_ABSPOSE_GIVEN_POSES, 4 * _cabi.LG_ABSPOSE_GIVEN_POSES]
    lib = _cabi.load()
    assert lib.lg_triangulate.argtypes == [C.POINTER(_cabi.LgTriangulateIO), C.c_void_p]
    assert "lg_triangulate" in _cabi.EXPORTED_SYMBOLS and "lg_triangulate_workspace_bytes" in _cabi.EXPORTED_SYMBOLS
    assert lib.lg_version().decode() == "lightglue_amd 0.6 (gfx950)" and HEADER.count("added to ABI 0.6 without a version bump") >= 3
    assert len(STATES) == 8 and (O.LG_ERR_INDEX, O.LG_ERR_CAMERA) == (_cabi.LG_ERR_INDEX, _cabi.LG_ERR_CAMERA)


def good_io(**over):
    io = _cabi.LgTriangulateIO(pairs=4, n=100, images=3, flags=_cabi.LG_TRI_REFINE, max_reproj_error=4.0, min_angle=1.5, max_track_length=128, kpts=256, index0=256,
                               index1=256, matches0=256, cameras=256, poses=256, workspace=256, workspace_bytes=1 << 40, points3d=256, track_id=256, node_state=256,
                               xyz=256, track_length=256, track_error=256, counts=256, status=256)
    for k, v in over.items():
        setattr(io, k, v)
    return io


def test_envelope_is_refused_without_touching_a_gpu():
    """every pointer is a fake non-null value: a refusal that came after anything was dereferenced or launched would have crashed"""
    lib = _cabi.load()
    R, T = _cabi.LG_TRI_REFINE, _cabi.LG_TRI_TRACKS_ONLY
    inv = _cabi.LG_ERR_INVALID
    assert lib.lg_triangulate(None, None) == inv and b"null io" in lib.lg_last_error()
    refused = [
        (dict(flags=1), b"flag"), (dict(flags=R | 1 << 31), b"flag"), (dict(flags=_cabi.LG_FLAG_INDEXED), b"flag"), (dict(flags=_cabi.LG_ABSPOSE_REFINE), b"flag"),
        (dict(flags=4 * T), b"flag"), (dict(flags=_cabi.LG_ABSPOSE_GIVEN_POSES), b"flag"),
        (dict(n=-1), b"LG_MAX_KEYPOINTS"), (dict(n=8193), b"LG_MAX_KEYPOINTS"),
        (dict(images=-1), b"LG_MAX_ROWS"), (dict(images=1025, n=2048), b"LG_MAX_ROWS"), (dict(images=257, n=8192), b"LG_MAX_ROWS"), (dict(images=2 ** 21 + 1, n=0), b"LG_MAX_ROWS"),
        (dict(pairs=-1), b"2^31"), (dict(pairs=2 ** 20, n=2048), b"2^31"), (dict(pairs=2 ** 18, n=8192, images=256), b"2^31"),
        (dict(max_track_length=1), b"max_track_length"), (dict(max_track_length=0), b"max_track_length"), (dict(max_track_length=1025), b"max_track_length"),
        (dict(max_track_length=-4), b"max_track_length"),
        (dict(max_reproj_error=0.0), b"max_reproj_error"), (dict(max_reproj_error=-1.0), b"max_reproj_error"), (dict(max_reproj_error=float("nan")), b"max_reproj_error"),
        (dict(max_reproj_error=float("inf")), b"max_reproj_error"),
        (dict(min_angle=-0.5), b"min_angle"), (dict(min_angle=180.0), b"min_angle"), (dict(min_angle=float("nan")), b"min_angle"),
        (dict(workspace_bytes=1000), b"workspace holds"), (dict(workspace=None), b"null workspace"), (dict(workspace=128), b"256-byte aligned"),
        (dict(flags=T, workspace_bytes=1000), b"workspace holds"),
    ]
    refused += [(dict({k: None}), b"null pointer") for k in ("kpts", "index0", "index1", "matches0", "cameras", "poses", "points3d", "track_id", "node_state", "xyz",
                                                             "track_length", "track_error", "counts", "status")]
    refused += [(dict({k: None}, flags=T), b"null pointer") for k in ("index0", "index1", "matches0", "track_id", "node_state", "track_length", "counts", "status")]
    for over, word in refused:
        assert lib.lg_triangulate(C.byref(good_io(**over)), None) == inv, over
        assert word in lib.lg_last_error() and b"lg_triangulate" in lib.lg_last_error(), (over, lib.lg_last_error())
    # the workspace: 256 bytes, 160 per image, seven int32 per node, 28 bytes per possible track; -1 outside the envelope
    up = lambda b: (b + 255) // 256 * 256
    for images, n in ((1, 0), (1, 1), (6, 96), (16, 2048), (256, 8192), (2 ** 21, 1)):
        nodes = images * n
        want = 256 + up(160 * images) + 7 * up(4 * nodes) + 3 * up(4 * (nodes // 2)) + up(16 * (nodes // 2))
        assert lib.lg_triangulate_workspace_bytes(images, n, R) == want == lib.lg_triangulate_workspace_bytes(images, n, T)
    for bad in ((1, 8193, 0), (-1, 10, 0), (1, -1, 0), (1, 10, 1), (257, 8192, 0), (2 ** 21 + 1, 1, 0)):
        assert lib.lg_triangulate_workspace_bytes(*bad) == -1, bad


def test_python_configuration_errors():
    for bad in (dict(max_reproj_error=0), dict(max_reproj_error=-2.0), dict(max_reproj_error=float("nan")), dict(min_angle=-1), dict(min_angle=180), dict(min_angle=float("nan")),
                dict(max_track_length=1), dict(max_track_length=1025), dict(max_track_length=2.5)):
        with pytest.raises(ValueError):
            Triangulator(**bad)
    tri = Triangulator()
    assert (tri.max_reproj_error, tri.min_angle, tri.max_track_length, tri.refine) == (4.0, 1.5, 128, True)
    assert (O.MAX_ERR, O.MIN_ANGLE, O.MAX_LEN) == (4.0, 1.5, 128)
    Triangulator(min_angle=0, max_track_length=2), Triangulator(max_track_length=1024, refine=False)
    feats = {"keypoints": torch.zeros(2, 8, 2)}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tri.triangulate(feats, [(0, 1)], torch.full((1, 8), -1), torch.tensor([O.CAM, O.CAM]), torch.zeros(2, 3, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tri.build_tracks(feats, [(0, 1)], torch.full((1, 8), -1))
    R, t = torch.eye(3).expand(2, 3, 3), torch.ones(2, 3)
    assert torch.equal(as_poses((R, t), 2, "cpu"), torch.cat([R, t[:, :, None]], 2)) and as_poses(torch.zeros(2, 3, 4, dtype=torch.float64), 2, "cpu").dtype is torch.float32
    for bad in (torch.zeros(2, 4, 4), (R, torch.ones(2, 4)), torch.zeros(3, 3, 4)):
        with pytest.raises(ValueError):
            as_poses(bad, 2, "cpu")


# ---------------------------------------------------------------------- the constants of tests/test_gpu_triangulate.py
def scenes():
    bad, sub, _ = O.bad_camera_scene()
    return [("main", O.oracle_input(O.main_scene()), {}), ("start", O.oracle_input(O.main_scene()), dict(refine_on=False)),
            ("reject", O.oracle_input(O.reject_scene()), dict(max_len=O.REJECT_MAX_LEN)), ("bad cameras", bad, {}), ("bad cameras, without", sub, {}),
            ("chain", O.oracle_input(O.chain_scene()), {})]


@pytest.fixture(scope="module")
def derived():
    q_point = q_error = 0.0
    for name, inp, conf in scenes():
        base = O.triangulate(inp, **conf)
        scale = O.point_scale(inp, base)
        for other in (O.triangulate(inp, order="descending", **conf), O.triangulate(inp, solver=O.solve3_numpy, **conf)):
            assert (other["track_id"] == base["track_id"]).all() and (other["node_state"] == base["node_state"]).all(), name
            q_point = max(q_point, float((abs(other["xyz64"] - base["xyz64"]).max(1) / [O.ulp32(s) for s in scale]).max()))
            q_error = max(q_error, float((abs(other["error64"] - base["error64"]) / [O.ulp32(e) for e in base["error64"]]).max()))
    return q_point, q_error


def test_gpu_constants_are_the_derived_ones(derived):
    """Q_POINT and Q_ERROR of the GPU file's header are the oracle's own figures over that file's inputs (rounded up in the third digit), and both are below
    1e-3 of the ulp they are measured in: the precondition of the one-ulp bar"""
    q_point, q_error = derived
    print("derived: Q_POINT %.4e Q_ERROR %.4e" % (q_point, q_error))
    for got, want in ((G.Q_POINT, q_point), (G.Q_ERROR, q_error)):
        assert want <= got <= want * 1.01, (want, got)
    assert G.Q_POINT < 1e-3 and G.Q_ERROR < 1e-3 and G.MAX_EXCLUDED == 0.02
    for k in ("Q_POINT", "Q_ERROR"):
        assert "%-10s %.2e" % (k, getattr(G, k)) in G.__doc__, k


def test_the_oracle_excludes_no_track_on_these_inputs():
    """decided by the oracle alone: no track of any input of the GPU tests lies within a relative 1e-9 of a bar"""
    for name, inp, conf in scenes():
        out = O.triangulate(inp, **conf)
        assert not any(t[3] for t in out["tracks"]), name
