"""Numpy restatement of the triangulator's definition (include/lightglue_amd.h, lg_triangulate), float64: nodes, edges, statuses, tracks through a host
union-find of its own (union by size with path compression, then renamed to the lowest node), the image records, the rays, the linear start with the prescribed
elimination, the Gauss-Newton refinement, the acceptance tests in their order, the dense ids and every output.  `order` and `solver` vary what the definition
fixes (the accumulation order, the elimination) so that tests/test_triangulate_cpu.py can measure what those choices are worth (Q_POINT).  Also the scenes and
the inputs of every test of tests/test_gpu_triangulate.py, built without a GPU.  No GPU, no torch."""
import functools

import numpy as np

EPS, GN_STEPS, NEAR = 1e-12, 5, 1e-9
LG_OK, LG_ERR_INDEX, LG_ERR_CAMERA = 0, 6, 7
NONE, DONE, CONFLICT, TOO_LONG, DEGENERATE, BEHIND, REPROJECTION, ANGLE = range(8)
MAX_ERR, MIN_ANGLE, MAX_LEN = 4.0, 1.5, 128


# ---------------------------------------------------------------------- nodes, edges, tracks
def live_rows(num, K, N):
    return np.full(K, N, int) if num is None else np.clip(np.asarray(num, int), 0, N)


def image_ok(cam, pose):
    cam, pose = np.asarray(cam, np.float64), np.asarray(pose, np.float64)
    return bool(np.isfinite(cam).all() and (cam[:2] > 0).all() and np.isfinite(pose).all())


def edges(pairs, matches0, K, N, num=None, ok=None):
    """(the edge set {(u, v), u < v}, status [P]); ok [K] bool: the images that pass the camera rule (None: every image, LG_TRI_TRACKS_ONLY)"""
    live = live_rows(num, K, N)
    out, status = set(), np.zeros(len(pairs), int)
    for p, (a, b) in enumerate(np.asarray(pairs, int).reshape(-1, 2)):
        if not (0 <= a < K and 0 <= b < K) or a == b:
            status[p] = LG_ERR_INDEX
            continue
        if ok is not None and not (ok[a] and ok[b]):
            status[p] = LG_ERR_CAMERA
            continue
        for i in range(live[a]):
            m = int(matches0[p][i])
            if 0 <= m < N and m < live[b]:
                u, v = a * N + i, b * N + m
                out.add((min(u, v), max(u, v)))
    return out, status


def components(nodes, edge_set):
    """name [nodes]: the lowest node of every node's component"""
    parent, size = list(range(nodes)), [1] * nodes

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r
    for u, v in sorted(edge_set, reverse=True):                      # any order gives the same components: this one is not the device's
        ru, rv = find(u), find(v)
        if ru != rv:
            if size[ru] < size[rv]:
                ru, rv = rv, ru
            parent[rv] = ru
            size[ru] += size[rv]
    roots = np.array([find(v) for v in range(nodes)], int)
    lowest = np.full(nodes, nodes, int)
    np.minimum.at(lowest, roots, np.arange(nodes))
    return lowest[roots]


def tracks_of(name):
    """[(name, observations ascending)] of the components with at least two nodes, in ascending order of the name"""
    order = np.argsort(name, kind="stable")
    cuts = np.flatnonzero(np.diff(name[order])) + 1
    return [(int(name[g[0]]), g) for g in np.split(order, cuts) if len(g) >= 2]


# ---------------------------------------------------------------------- geometry
def solve3(M, b):
    """the prescribed elimination: x, or None on a pivot that is not above EPS times the largest diagonal entry, or a non-finite x"""
    M = np.concatenate([np.asarray(M, np.float64), np.asarray(b, np.float64)[:, None]], 1)
    bar = EPS * max(M[0, 0], M[1, 1], M[2, 2])
    with np.errstate(all="ignore"):
        for c in range(3):
            for r in range(c + 1, 3):
                if abs(M[r, c]) > abs(M[c, c]):
                    M[[c, r]] = M[[r, c]]
            if not abs(M[c, c]) > bar:
                return None
            for r in range(c + 1, 3):
                f = M[r, c] / M[c, c]
                for j in range(c + 1, 4):
                    M[r, j] = M[r, j] - f * M[c, j]
        x2 = M[2, 3] / M[2, 2]
        x1 = (M[1, 3] - M[1, 2] * x2) / M[1, 1]
        x0 = ((M[0, 3] - M[0, 1] * x1) - M[0, 2] * x2) / M[0, 0]
    x = np.array([x0, x1, x2])
    return x if np.isfinite(x).all() else None


def solve3_numpy(M, b):
    M = np.asarray(M, np.float64)
    if not np.isfinite(M).all() or np.linalg.eigvalsh(M)[0] <= EPS * M.diagonal().max():
        return None
    return np.linalg.solve(M, b)


def record(cam, pose):
    """(R [3, 3], t [3], c [3], cam [4]) in float64 from the float32 inputs"""
    pose, cam = np.asarray(pose, np.float32).astype(np.float64).reshape(3, 4), np.asarray(cam, np.float32).astype(np.float64)
    R, t = pose[:, :3], pose[:, 3]
    c = -np.array([(R[0, j] * t[0] + R[1, j] * t[1]) + R[2, j] * t[2] for j in range(3)])
    return R, t, c, cam


def ray(xy, rec):
    R, _, _, cam = rec
    x, c = np.asarray(xy, np.float32), cam.astype(np.float32)
    xh, yh = np.float64((x[0] - c[2]) / c[0]), np.float64((x[1] - c[3]) / c[1])      # float32 arithmetic, then widened
    w = [(R[0, e] * xh + R[1, e] * yh) + R[2, e] for e in range(3)]
    nrm = np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])                          # of the rotated vector: a float32 R is orthonormal to 1e-7 only
    return np.array([w[e] / nrm for e in range(3)])


def project(rec, X):
    R, t = rec[0], rec[1]
    return np.array([((R[r, 0] * X[0] + R[r, 1] * X[1]) + R[r, 2] * X[2]) + t[r] for r in range(3)])


def start_point(obs, solver=solve3):
    """obs: [(xy, rec)] in accumulation order"""
    S, B = np.zeros((3, 3)), np.zeros(3)
    for xy, rec in obs:
        d, c = ray(xy, rec), rec[2]
        dc = (d[0] * c[0] + d[1] * c[1]) + d[2] * c[2]
        S += np.array([[1.0 - d[0] * d[0], -(d[0] * d[1]), -(d[0] * d[2])], [-(d[0] * d[1]), 1.0 - d[1] * d[1], -(d[1] * d[2])],
                       [-(d[0] * d[2]), -(d[1] * d[2]), 1.0 - d[2] * d[2]]])
        B += c - d * dc
    return solver(S, B)


def residual(xy, rec, X):
    """(rx, ry, pz)"""
    p, cam = project(rec, X), rec[3]
    with np.errstate(all="ignore"):
        iz = 1.0 / p[2]
        return ((cam[0] * p[0]) * iz + cam[2]) - np.float64(np.float32(xy[0])), ((cam[1] * p[1]) * iz + cam[3]) - np.float64(np.float32(xy[1])), p[2]


def cost(obs, X):
    return sum(rx * rx + ry * ry for rx, ry, pz in (residual(xy, rec, X) for xy, rec in obs) if pz > 0)


def refine(obs, X0, solver=solve3):
    """five Gauss-Newton steps; the start comes back if a step is abandoned"""
    Y = np.array(X0, np.float64)
    for _ in range(GN_STEPS):
        H, G = np.zeros((3, 3)), np.zeros(3)
        for xy, rec in obs:
            R, cam = rec[0], rec[3]
            p = project(rec, Y)
            if not p[2] > 0:
                continue
            iz = 1.0 / p[2]
            rx, ry = ((cam[0] * p[0]) * iz + cam[2]) - np.float64(np.float32(xy[0])), ((cam[1] * p[1]) * iz + cam[3]) - np.float64(np.float32(xy[1]))
            ax, az, by, bz = cam[0] * iz, -(((cam[0] * p[0]) * iz) * iz), cam[1] * iz, -(((cam[1] * p[1]) * iz) * iz)
            J0, J1 = ax * R[0] + az * R[2], by * R[1] + bz * R[2]
            H += np.outer(J0, J0) + np.outer(J1, J1)
            G += J0 * rx + J1 * ry
        s = solver(H, -G)
        if s is None or not np.isfinite(Y + s).all():
            return np.array(X0, np.float64)
        Y = Y + s
    return Y


def classify(obs, max_err, min_angle, refine_on, solver=solve3):
    """(state, X, mean error, near: the oracle places the track within a relative NEAR of a bar)"""
    X = start_point(obs, solver)
    if X is None:
        return DEGENERATE, None, None, False
    if refine_on:
        X = refine(obs, X, solver)
    res = [residual(xy, rec, X) for xy, rec in obs]
    near = any(abs(pz) <= NEAR * np.linalg.norm(project(rec, X)) for (_, rec), (_, _, pz) in zip(obs, res))
    if any(not pz > 0 for _, _, pz in res):
        return BEHIND, X, None, near
    err = np.array([np.sqrt(rx * rx + ry * ry) for rx, ry, _ in res])
    near = near or bool((abs(err - max_err) <= NEAR * max_err).any())
    if (~(err <= max_err)).any():
        return REPROJECTION, X, None, near
    mean = functools.reduce(lambda a, b: a + b, err.tolist(), 0.0) / len(err)                # summed in observation order
    if min_angle > 0:
        cos_min = np.cos(np.float64(np.float32(min_angle)) * 3.141592653589793 / 180.0)
        rays = [X - rec[2] for _, rec in obs]
        norms = [np.sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]) for u in rays]
        wide = False
        for i in range(len(obs)):
            for j in range(i + 1, len(obs)):
                dot, bar = (rays[i][0] * rays[j][0] + rays[i][1] * rays[j][1]) + rays[i][2] * rays[j][2], (cos_min * norms[i]) * norms[j]
                near = near or abs(dot - bar) <= NEAR * norms[i] * norms[j]
                wide = wide or dot <= bar
        if not wide:
            return ANGLE, X, None, near
    return DONE, X, mean, near


def widest_angle(obs, X):
    """degrees: the largest angle between two rays of a track (a diagnostic of the scenes, not part of the definition)"""
    rays = [(X - rec[2]) / np.linalg.norm(X - rec[2]) for _, rec in obs]
    return max(np.degrees(np.arccos(np.clip(rays[i] @ rays[j], -1, 1))) for i in range(len(rays)) for j in range(i + 1, len(rays)))


# ---------------------------------------------------------------------- the whole definition
def triangulate(inp, max_err=MAX_ERR, min_angle=MIN_ANGLE, max_len=MAX_LEN, refine_on=True, tracks_only=False, order="ascending", solver=solve3):
    """inp: dict(kpts [K, N, 2] float32, num [K] or None, pairs [P, 2], matches0 [P, N], cams [K, 4], poses [K, 3, 4]) -> dict(points3d [K, N, 3] float32,
    track_id [K, N], node_state [K, N], num_tracks, xyz [T, 3] float32, xyz64 [T, 3], track_length [T], track_error [T] float32, error64 [T], state_counts [8],
    status [P], tracks: [(name, observations, state, near)] of every component with at least two nodes, names [T]: the lowest node of the numbered tracks)"""
    kpts = np.asarray(inp["kpts"], np.float32)
    K, N = kpts.shape[:2]
    ok = None if tracks_only else np.array([image_ok(inp["cams"][k], inp["poses"][k]) for k in range(K)])
    edge_set, status = edges(inp["pairs"], inp["matches0"], K, N, inp.get("num"), ok)
    name = components(K * N, edge_set)
    recs = None if tracks_only else [record(inp["cams"][k], inp["poses"][k]) if ok[k] else None for k in range(K)]
    flat = kpts.reshape(-1, 2)
    pts, tid, state = np.full((K * N, 3), np.nan, np.float32), np.full(K * N, -1, np.int64), np.zeros(K * N, np.uint8)
    xyz, lengths, errors, names, listed, counts = [], [], [], [], [], np.zeros(8, int)
    for root, nodes in tracks_of(name):
        X, mean, near = None, None, False
        if len(nodes) > max_len:
            st = TOO_LONG
        elif len(set((nodes // N).tolist())) < len(nodes):
            st = CONFLICT
        elif tracks_only:
            st = DONE
        else:
            obs = [(flat[v], recs[v // N]) for v in (nodes if order == "ascending" else nodes[::-1])]
            st, X, mean, near = classify(obs, np.float64(np.float32(max_err)), min_angle, refine_on, solver)
        counts[st] += 1
        state[nodes] = st
        listed.append((root, nodes, st, near))
        if st == DONE:
            tid[nodes] = len(names)
            names.append(root)
            lengths.append(len(nodes))
            if not tracks_only:
                pts[nodes] = X.astype(np.float32)
                xyz.append(X)
                errors.append(mean)
    xyz64, err64 = np.asarray(xyz, np.float64).reshape(-1, 3), np.asarray(errors, np.float64)
    return dict(points3d=pts.reshape(K, N, 3), track_id=tid.reshape(K, N), node_state=state.reshape(K, N), num_tracks=len(names), xyz=xyz64.astype(np.float32),
                xyz64=xyz64, track_length=np.asarray(lengths, int), track_error=err64.astype(np.float32), error64=err64, state_counts=counts, status=status,
                tracks=listed, names=np.asarray(names, int))


# ---------------------------------------------------------------------- scenes: 640 x 480 images, camera (500, 500, 320, 240), cameras about 6 units from a box
# of points centred at (100, -50, 20), pixel noise 0.5 (the recipe of tests/abspose_oracle.py)
FRAME, SIGMA, CAM = (640.0, 480.0), 0.5, (500.0, 500.0, 320.0, 240.0)
BOX_CENTRE, BOX_HALF, DISTANCE = np.array([100.0, -50.0, 20.0]), np.array([1.2, 1.2, 1.0]), 6.0
K, N = 6, 96
NUM = (90, 96, 88, 96, 96, 92)


def look_at(centre, target):
    """(R, t) of a camera at `centre` whose z axis points at `target`: X_cam = R X_world + t"""
    z = (target - centre) / np.linalg.norm(target - centre)
    x = np.cross(z, [0.0, 0.0, 1.0])
    x /= np.linalg.norm(x)
    R = np.stack([x, np.cross(z, x), z])
    return R, -R @ centre


def cameras(count=K, seed=0):
    """poses [count, 3, 4] float32 on an arc of about 80 degrees around the box, each looking at a point near its centre; cams [count, 4]"""
    rng = np.random.default_rng(500 + seed)
    poses = []
    for k in range(count):
        phi, theta = np.radians(-40.0 + 80.0 * k / max(count - 1, 1)), np.radians(rng.uniform(-12, 12))
        centre = BOX_CENTRE + (DISTANCE + rng.uniform(-0.4, 0.4)) * np.array([np.cos(phi) * np.cos(theta), np.sin(phi) * np.cos(theta), np.sin(theta)])
        R, t = look_at(centre, BOX_CENTRE + rng.uniform(-0.2, 0.2, 3))
        poses.append(np.concatenate([R, t[:, None]], 1))
    return np.asarray(poses, np.float32), np.tile(np.asarray(CAM, np.float32), (count, 1))


def project_pixels(pose, cam, X):
    p = np.asarray(X, np.float64) @ pose[:, :3].astype(np.float64).T + pose[:, 3].astype(np.float64)
    return np.stack([cam[0] * p[:, 0] / p[:, 2] + cam[2], cam[1] * p[:, 1] / p[:, 2] + cam[3]], 1), p[:, 2]


def plant(poses, cams, views, seed, num=NUM, rows_per_image=N):
    """Tracks planted into empty images.  views: per track the images that see it.  -> dict(kpts [K, N, 2] float32 (unused rows: uniform pixels), X [T, 3],
    views, rows: per track {image: row}, free: per image the unused live rows in a fixed order, clean [K, N, 2]: the projections without noise (NaN elsewhere))"""
    rng = np.random.default_rng(seed)
    count = len(poses)
    kpts = rng.uniform([0, 0], FRAME, (count, rows_per_image, 2)).astype(np.float32)
    clean = np.full((count, rows_per_image, 2), np.nan)
    order = [list(rng.permutation(num[k])) for k in range(count)]
    X = BOX_CENTRE + rng.uniform(-BOX_HALF, BOX_HALF, (len(views), 3))
    rows = []
    for j, seen in enumerate(views):
        at = {}
        for k in seen:
            px, pz = project_pixels(poses[k], cams[k], X[j:j + 1])
            assert pz[0] > 0 and 0 <= px[0, 0] < FRAME[0] and 0 <= px[0, 1] < FRAME[1], (j, k, px, pz)
            at[k] = int(order[k].pop())
            clean[k, at[k]] = px[0]
            kpts[k, at[k]] = px[0] + rng.normal(0, SIGMA, 2)
        rows.append(at)
    return dict(kpts=kpts, X=X, views=views, rows=rows, free=order, clean=clean)


def match_rows(pairs, rows, rows_per_image=N):
    """matches0 [P, N]: row of image a -> row of image b for every planted track both images of a pair see; pairs outside the store or (a, a) stay empty"""
    m0 = np.full((len(pairs), rows_per_image), -1, np.int64)
    for p, (a, b) in enumerate(pairs):
        for at in rows:
            if a != b and a in at and b in at:
                m0[p, at[a]] = at[b]
    return m0


def random_views(count, tracks, rng, lo=2, hi=None):
    hi = count if hi is None else hi
    return [sorted(rng.choice(count, int(rng.integers(lo, hi + 1)), replace=False).tolist()) for _ in range(tracks)]


def reverse_pairs(inp):
    """the same edge set with every pair (a, b) listed as (b, a): its row of matches0 transposed on the host"""
    pairs = np.asarray(inp["pairs"])[:, ::-1].copy()
    m0 = np.full_like(inp["matches0"], -1)
    for p, row in enumerate(inp["matches0"]):
        i = np.flatnonzero((row >= 0) & (row < m0.shape[1]))
        assert len(set(row[i].tolist())) == len(i)                      # one-to-one: the transpose holds the same edges
        m0[p, row[i]] = i
    return dict(inp, pairs=pairs, matches0=m0)


def permute_pairs(inp, seed=0):
    order = np.random.default_rng(seed).permutation(len(inp["pairs"]))
    return dict(inp, pairs=np.asarray(inp["pairs"])[order], matches0=inp["matches0"][order]), order


# the pair list of the main scene: twelve of the fifteen pairs (so that some tracks hold together only through a chain), one of them listed again and one
# listed again reversed, one pair with an index outside the store and one pair (a, a)
MISSING = ((0, 2), (1, 3), (2, 5))
REGULAR = [(a, b) for a in range(K) for b in range(a + 1, K) if (a, b) not in MISSING]
PAIRS = REGULAR + [(3, 4), (1, 0), (2, 9), (4, 4)]
BAD_INDEX, SELF_PAIR, REVERSED = len(REGULAR) + 2, len(REGULAR) + 3, len(REGULAR) + 1


@functools.lru_cache(maxsize=None)
def main_scene():
    """59 planted tracks of 2 - 6 views over six images and the match graph of PAIRS with everything the edge rules name: chains, a conflict made through a
    third image, rows beyond num_keypoints on either side, m >= num[b], m = -1, a pair outside the store, a pair (a, a), a pair listed twice and once reversed.
    -> the oracle's input dict plus `planted` (the plant) and `odd` (what was put where)"""
    rng = np.random.default_rng(7)
    poses, cams = cameras()
    views = random_views(K, 59, rng)
    # the conflict's two tracks, a chain (0 - 1 and 1 - 2 are listed, 0 - 2 is not), a track only the unlisted (0, 2) could hold, a full one
    views[0], views[1], views[2], views[3], views[4] = [0, 1, 4], [0, 1, 4], [0, 1, 2], [0, 2], [0, 1, 2, 3, 4, 5]
    pl = plant(poses, cams, views, 11)
    m0 = match_rows(PAIRS, pl["rows"])                                  # (the reversed pair (1, 0) comes out transposed: row of image 1 -> row of image 0)
    at = {pair: p for p, pair in enumerate(PAIRS[:len(REGULAR)])}
    rows = pl["rows"]
    # a conflict made through a third image: in pair (1, 4) the two tracks' matches are exchanged, so image 4 ties track 0 to track 1 (one-to-one as before)
    m0[at[1, 4], rows[0][1]], m0[at[1, 4], rows[1][1]] = rows[1][4], rows[0][4]
    odd = dict(conflict=(0, 1), chain=2, unheld=3)
    # rows beyond num_keypoints on either side (the dead rows are those of images 0, 2 and 5), a match outside the image; each would be an edge otherwise
    free = [list(v) for v in pl["free"]]
    m0[at[0, 1], NUM[0] + 1] = free[1].pop()                            # i >= num[a]
    m0[at[2, 3], NUM[2]] = free[3].pop()                                # i >= num[a]: the first dead row
    m0[at[1, 2], free[1].pop()] = NUM[2] + 2                            # m >= num[b]
    m0[at[3, 5], free[3].pop()] = NUM[5]                                # m >= num[b]: the first dead row
    m0[at[0, 1], free[0].pop()] = N + 5                                 # m >= n
    # the pairs that contribute nothing carry matches that would merge tracks if they were read
    m0[BAD_INDEX] = m0[at[1, 2]][::-1]
    m0[SELF_PAIR, :NUM[4] - 1] = np.arange(1, NUM[4])
    inp = dict(kpts=pl["kpts"], num=np.asarray(NUM), pairs=np.asarray(PAIRS), matches0=m0, cams=cams, poses=poses)
    return dict(inp, planted=pl, odd=odd)


def oracle_input(sc):
    return {k: sc[k] for k in ("kpts", "num", "pairs", "matches0", "cams", "poses")}


@functools.lru_cache(maxsize=None)
def main_oracle(refine_on=True, tracks_only=False, max_len=MAX_LEN, order="ascending", solver="elim"):
    """The definition's answer on the main scene (shared by the tests; treat as read-only)"""
    return triangulate(oracle_input(main_scene()), refine_on=refine_on, tracks_only=tracks_only, max_len=max_len, order=order,
                       solver=solve3 if solver == "elim" else solve3_numpy)


# ---------------------------------------------------------------------- one large component: K = 8, N = 64, about 300 nodes chained through sixteen pairs
BIG_K, BIG_N, BIG_NODES = 8, 64, 300


@functools.lru_cache(maxsize=None)
def big_component():
    """node j of the chain is row j // 8 of image j % 8; node j is matched onto node j + 1 (pairs (k, k + 1 mod 8)) and onto node j + 2 (pairs (k, k + 2 mod 8)):
    every lane of the union kernel that holds an edge works on the same component"""
    pairs = [(k, (k + 1) % BIG_K) for k in range(BIG_K)] + [(k, (k + 2) % BIG_K) for k in range(BIG_K)]
    m0 = np.full((len(pairs), BIG_N), -1, np.int64)
    for j in range(BIG_NODES):
        for step in (1, 2):
            if j + step < BIG_NODES:
                m0[(step - 1) * BIG_K + j % BIG_K, j // BIG_K] = (j + step) // BIG_K
    poses, cams = cameras(BIG_K, 3)
    kpts = np.random.default_rng(5).uniform([0, 0], FRAME, (BIG_K, BIG_N, 2)).astype(np.float32)
    return dict(kpts=kpts, num=None, pairs=np.asarray(pairs), matches0=m0, cams=cams, poses=poses)


# ---------------------------------------------------------------------- every rejection state, planted
REJECT_PAIRS = [(a, b) for a in range(K) for b in range(a + 1, K)]
REJECT_MAX_LEN = 4


@functools.lru_cache(maxsize=None)
def reject_scene():
    """Six images: 0 and 1 as in the main scene; 3 shares its rotation with 2 (its centre lies 1.5 units to the side); 5 has nearly the centre of 4 (2 mm apart).
    Clean tracks of 2 - 4 views, and planted: a wrong match tens of pixels off (6), a wrong match that puts the point behind a camera (5), tracks seen only
    from images 4 and 5 (7), a track seen at one normalised position by images 2 and 3 (4), tracks of five and six views against max_track_length = 4 (3).
    -> the oracle's input dict plus `want`: {state: the planted tracks' lowest nodes}"""
    rng = np.random.default_rng(21)
    poses, cams = cameras(K, 1)
    poses = poses.astype(np.float64)
    R2, t2 = poses[2][:, :3], poses[2][:, 3]
    c3 = -R2.T @ t2 + R2.T @ np.array([1.5, 0.0, 0.0])
    poses[3] = np.concatenate([R2, (-R2 @ c3)[:, None]], 1)
    R4, t4 = poses[4][:, :3], poses[4][:, 3]
    c5 = -R4.T @ t4 + np.array([0.002, 0.0, 0.0])
    R5, t5 = look_at(c5, BOX_CENTRE + np.array([0.05, 0.0, 0.0]))
    poses[5] = np.concatenate([R5, t5[:, None]], 1)
    poses = poses.astype(np.float32)
    views = [v for v in random_views(K, 40, rng, 2, 4) if v != [4, 5]]
    special = dict(far=len(views), behind=len(views) + 1, narrow=len(views) + 2, narrow2=len(views) + 3, same=len(views) + 4, long5=len(views) + 5, long6=len(views) + 6)
    views += [[0, 1, 2], [0, 1], [4, 5], [4, 5], [2, 3], [0, 1, 2, 3, 4], [0, 1, 2, 3, 4, 5]]
    num = (N,) * K
    pl = plant(poses, cams, views, 23, num)
    kpts, rows = pl["kpts"], pl["rows"]
    kpts[1, rows[special["far"]][1]] += np.float32(45.0)                                  # tens of pixels off
    # behind: the two rays diverge — image 0 sees it at its left edge, image 1 (to the left of image 0's view... whichever side) at the opposite edge; the
    # oracle says which state this is, and tests/test_triangulate_cpu.py asserts it is 5
    kpts[0, rows[special["behind"]][0]] = BEHIND_PIXELS[0]
    kpts[1, rows[special["behind"]][1]] = BEHIND_PIXELS[1]
    # two centres 2 mm apart: under noise 0.5 such rays cross anywhere, also behind the cameras, so these two tracks carry their exact projections
    for j in (special["narrow"], special["narrow2"]):
        for k in (4, 5):
            kpts[k, rows[j][k]] = pl["clean"][k, rows[j][k]]
    # one normalised position in two images that share R: parallel rays
    kpts[3, rows[special["same"]][3]] = kpts[2, rows[special["same"]][2]]
    m0 = match_rows(REJECT_PAIRS, rows)
    inp = dict(kpts=kpts, num=None, pairs=np.asarray(REJECT_PAIRS), matches0=m0, cams=cams, poses=poses)
    lowest = lambda j: min(k * N + r for k, r in rows[j].items())
    want = {REPROJECTION: [lowest(special["far"])], BEHIND: [lowest(special["behind"])], ANGLE: [lowest(special["narrow"]), lowest(special["narrow2"])],
            DEGENERATE: [lowest(special["same"])], TOO_LONG: [lowest(special["long5"]), lowest(special["long6"])]}
    return dict(inp, planted=pl, want=want)


BEHIND_PIXELS = (np.array([40.0, 240.0], np.float32), np.array([600.0, 240.0], np.float32))


@functools.lru_cache(maxsize=None)
def reject_oracle(refine_on=True):
    return triangulate(oracle_input(reject_scene()), max_len=REJECT_MAX_LEN, refine_on=refine_on)


# ---------------------------------------------------------------------- bad cameras: one image with fx = 0 and one with a NaN pose entry
@functools.lru_cache(maxsize=None)
def bad_camera_scene():
    """the main scene's images and REGULAR pairs with image 2's fx = 0 and a NaN in image 5's pose -> (the input, the same input without the flagged pairs)"""
    sc = main_scene()
    cams, poses = sc["cams"].copy(), sc["poses"].copy()
    cams[2, 0], poses[5, 1, 2] = 0.0, np.nan
    regular = np.arange(len(REGULAR))
    inp = dict(oracle_input(sc), pairs=sc["pairs"][regular], matches0=sc["matches0"][regular], cams=cams, poses=poses)
    keep = np.array([2 not in p and 5 not in p for p in REGULAR])
    return inp, dict(inp, pairs=inp["pairs"][keep], matches0=inp["matches0"][keep]), keep


# ---------------------------------------------------------------------- the chain: triangulate five images, localise the sixth against them
@functools.lru_cache(maxsize=None)
def chain_scene():
    """Six images, 80 tracks each seen by image 5 and by two to four of the images 0 .. 4.  -> dict(the triangulator's input over the pairs among images 0 .. 4;
    query_pairs [(5, j)], query_matches0 [5, N]: row of image 5 -> row of image j; planted)"""
    rng = np.random.default_rng(31)
    poses, cams = cameras(K, 2)
    views = [sorted(rng.choice(5, int(rng.integers(2, 5)), replace=False).tolist()) + [5] for _ in range(80)]
    pl = plant(poses, cams, views, 33, (N,) * K)
    model_pairs = [(a, b) for a in range(5) for b in range(a + 1, 5)]
    query_pairs = [(5, j) for j in range(5)]
    inp = dict(kpts=pl["kpts"], num=None, pairs=np.asarray(model_pairs), matches0=match_rows(model_pairs, pl["rows"]), cams=cams, poses=poses)
    return dict(inp, query_pairs=np.asarray(query_pairs), query_matches0=match_rows(query_pairs, pl["rows"]), planted=pl)


# ---------------------------------------------------------------------- what the definition's fixed choices are worth
def ulp32(x):
    """one float32 ulp at magnitude x"""
    return float(np.spacing(np.float32(abs(x))))


def point_scale(inp, out):
    """[T]: per numbered track the largest coordinate magnitude among its point and its cameras' centres — what one float32 ulp is taken of"""
    Kk, Nn = np.asarray(inp["kpts"]).shape[:2]
    scale = []
    for t, name in enumerate(out["names"]):
        nodes = np.flatnonzero(out["track_id"].reshape(-1) == t)
        centres = [record(inp["cams"][v // Nn], inp["poses"][v // Nn])[2] for v in nodes]
        scale.append(max(abs(out["xyz64"][t]).max(), max(abs(c).max() for c in centres)))
    return np.asarray(scale)
