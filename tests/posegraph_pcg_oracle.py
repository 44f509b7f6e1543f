"""Numpy restatement of the global pose estimator with the iterative solver (include/lightglue_amd.h, lg_posegraph_solve_pcg), float64.  Scenes, pair states,
log / exp and the angle are tests/posegraph_oracle.py's; everything outside the two linear solves restates lg_posegraph_solve's definition as that file does;
the two solves follow the header's order of operations: every list sum is 64 lane-strided partials and a halving fold, every image dot 256 strided partials
and a halving fold, and the conjugate-gradient recurrence is the bundle adjuster's.  Sums are vectorised over list position (position k of all images at
once keeps every image's order).

`estimate` runs the definition a second time with the other accumulation order (every list sum one term after the other in list order, every image dot
numpy's pairwise sum) and marks
  near    a stage whose convergence test is decided by rounding (the rule of tests/posegraph_oracle.py);
  moving  the solves (stage, iteration) whose solver-iteration count differs between the two orders: a count of such a solve says nothing about another
          fp64 implementation (at 1e-13 a solve ends near the rounding floor of its recurrences, where the residual stalls for a few iterations);
  own     the spread of the two error outputs between the two runs;
  margins the smallest relative distance of a decision of the FIRST run from its bar: p.q > 0 (`pq`), a block pivot (`pivot`), the solver's stop (`stop`).
Also the calls of tests/test_gpu_posegraph_pcg.py (CALLS): tests/test_posegraph_pcg_cpu.py checks the preconditions of that file's bars on every one."""
import functools

import numpy as np

import posegraph_oracle as G

MAX_IMAGES, MAX_CG, MAX_SOLVER_ITERATIONS = 4096, 1000, 20000
ROTATION_CG_ITERATIONS, POSITION_CG_ITERATIONS, CG_TOLERANCE = 64, 800, 1e-6
TRI_EPS, LANES, PARTIALS = 1e-12, 64, 256


# ---------------------------------------------------------------------- the sums of the definition
class Lists:
    """the sorted adjacency lists flattened: entry e = (image, neighbour, pair, position in the image's list)"""

    def __init__(self, adj, K):
        self.K = K
        self.img = np.asarray([i for i in range(K) for _ in adj[i]], np.int64)
        self.nbr = np.asarray([j for i in range(K) for j, _ in adj[i]], np.int64)
        self.pair = np.asarray([p for i in range(K) for _, p in adj[i]], np.int64)
        self.pos = np.asarray([k for i in range(K) for k in range(len(adj[i]))], np.int64)
        self.longest = int(self.pos.max()) + 1 if len(self.pos) else 0
        self.rounds = max(1, -(-self.longest // LANES))
        self.width = 1                                      # the partials from the longest list's length on are 0 and adding them changes nothing:
        while self.width < min(self.longest, LANES):        # the fold starts at the first power of two that covers the lists
            self.width *= 2
        self.flat = (self.img * self.rounds + self.pos // LANES) * self.width + self.pos % LANES

    def sum(self, terms, taking_part, order):
        """[E, c] terms -> [K, c]: the list sum of the header over the entries that take part (the others add nothing)"""
        c = terms.shape[1]
        terms = np.where(taking_part[:, None], terms, 0.0)
        if order != "ascending":                           # the other order: one term after the other
            table = np.zeros((self.K, max(self.longest, 1), c))
            table[self.img, self.pos] = terms
            acc = np.zeros((self.K, c))
            for k in range(self.longest):
                acc = acc + table[:, k]
            return acc
        rounds, width = self.rounds, self.width
        table = np.zeros((self.K * rounds * width, c))
        table[self.flat] = terms
        table = table.reshape(self.K, rounds, width, c)
        part = table[:, 0].copy()
        for rd in range(1, rounds):
            part = part + table[:, rd]
        h = width // 2
        while h >= 1:
            part[:, :h] = part[:, :h] + part[:, h:2 * h]
            h //= 2
        return part[:, 0]


def image_sum(d, order):
    """the fold of the images' partials: 256 strided partials ascending from 0, then a halving tree"""
    if order != "ascending":
        return float(np.sum(d))
    rounds = -(-len(d) // PARTIALS)
    table = np.zeros(rounds * PARTIALS)
    table[:len(d)] = d
    table = table.reshape(rounds, PARTIALS)
    part = np.zeros(PARTIALS)
    for rd in range(rounds):
        part = part + table[rd]
    h = PARTIALS // 2
    while h >= 1:
        part[:h] = part[:h] + part[h:2 * h]
        h //= 2
    return float(part[0])


def dot3(x, y):
    return (x[:, 0] * y[:, 0] + x[:, 1] * y[:, 1]) + x[:, 2] * y[:, 2]


def ray_block(v, rho):
    """[N, 3], [N] -> [N, 6]: rho (I - v v^T) as (xx, xy, xz, yy, yz, zz)"""
    return np.stack([rho * (1.0 - v[:, 0] * v[:, 0]), rho * (0.0 - v[:, 0] * v[:, 1]), rho * (0.0 - v[:, 0] * v[:, 2]),
                     rho * (1.0 - v[:, 1] * v[:, 1]), rho * (0.0 - v[:, 1] * v[:, 2]), rho * (1.0 - v[:, 2] * v[:, 2])], 1)


def ray_apply(M, x):
    return np.stack([(M[:, 0] * x[:, 0] + M[:, 1] * x[:, 1]) + M[:, 2] * x[:, 2], (M[:, 1] * x[:, 0] + M[:, 3] * x[:, 1]) + M[:, 4] * x[:, 2],
                     (M[:, 2] * x[:, 0] + M[:, 4] * x[:, 1]) + M[:, 5] * x[:, 2]], 1)


def ray_weight(v, e, s):
    ee = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
    ve = (v[:, 0] * e[:, 0] + v[:, 1] * e[:, 1]) + v[:, 2] * e[:, 2]
    r = e - ve[:, None] * v
    q = np.arctan2(np.sqrt((r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]), ve) / s
    return 1.0 / np.maximum(ee, G.MIN_SQ) / (1.0 + q * q)


def tri_inverse3(s):
    """[N, 6] -> the inverses [N, 3, 3] column by column through the 3 x 3 elimination of the triangulator, ok [N], the smallest pivot over its bar less 1"""
    n = len(s)
    bar = TRI_EPS * np.maximum(np.maximum(s[:, 0], s[:, 3]), s[:, 5])
    Mi, ok, margin = np.zeros((n, 3, 3)), np.ones(n, bool), np.inf
    with np.errstate(all="ignore"):
        for c3 in range(3):
            e = [np.full(n, 1.0 if c3 == k else 0.0) for k in range(3)]
            M = [[s[:, 0].copy(), s[:, 1].copy(), s[:, 2].copy(), e[0]], [s[:, 1].copy(), s[:, 3].copy(), s[:, 4].copy(), e[1]],
                 [s[:, 2].copy(), s[:, 4].copy(), s[:, 5].copy(), e[2]]]
            good = np.ones(n, bool)
            for c in range(3):
                for r in range(c + 1, 3):
                    swap = abs(M[r][c]) > abs(M[c][c])
                    for j in range(4):
                        lo, hi = M[c][j], M[r][j]
                        M[c][j], M[r][j] = np.where(swap, hi, lo), np.where(swap, lo, hi)
                good &= abs(M[c][c]) > bar
                away = abs(abs(M[c][c]) / bar - 1.0)
                margin = min([margin] + away[np.isfinite(away)].tolist())
                for r in range(c + 1, 3):
                    f = M[r][c] / M[c][c]
                    for j in range(c + 1, 4):
                        M[r][j] = M[r][j] - f * M[c][j]
            x2 = M[2][3] / M[2][2]
            x1 = (M[1][3] - M[1][2] * x2) / M[1][1]
            x0 = ((M[0][3] - M[0][1] * x1) - M[0][2] * x2) / M[0][0]
            ok &= good & np.isfinite(x0) & np.isfinite(x1) & np.isfinite(x2)
            Mi[:, 0, c3], Mi[:, 1, c3], Mi[:, 2, c3] = x0, x1, x2
    return Mi, ok, margin


# ---------------------------------------------------------------------- the recurrence
def pcg(apply_A, precondition, r, x, free, budget, tol, order, margins):
    """-> x, solver iterations run, ended on the budget, failed.  r is the (warm-started) residual; entries of images that are not free are 0 throughout"""
    z = precondition(r)
    p = z.copy()
    with np.errstate(all="ignore"):
        rz = rz0 = image_sum(dot3(r, z), order)
        if not (np.isfinite(rz) and rz >= 0.0):
            return x, 0, False, True
        if rz == 0.0:
            return x, 0, False, False
        for i in range(1, budget + 1):
            q = apply_A(p)
            pq = image_sum(dot3(p, q), order)
            if not (np.isfinite(pq) and pq > 0.0):
                return x, i - 1, False, True
            margins["pq"] = min(margins["pq"], pq / (np.sqrt(image_sum(dot3(p, p), order)) * np.sqrt(image_sum(dot3(q, q), order))))
            alpha = rz / pq
            x = np.where(free[:, None], x + alpha * p, x)
            r = np.where(free[:, None], r - alpha * q, r)
            z = precondition(r)
            rz_new = image_sum(dot3(r, z), order)
            if not (np.isfinite(rz_new) and rz_new >= 0.0):
                return x, i, False, True
            bar = tol * np.sqrt(rz0)
            margins["stop"] = min(margins["stop"], abs(np.sqrt(rz_new) / bar - 1.0))
            if np.sqrt(rz_new) <= bar:
                return x, i, False, False
            if i == budget:
                return x, i, True, False
            beta = rz_new / rz
            p = np.where(free[:, None], z + beta * p, p)
            rz = rz_new
    raise AssertionError("unreachable")


# ---------------------------------------------------------------------- the definition
def estimate(pairs, R, t, K, **kw):
    """the definition, the decisions rounding takes (`near`, `moving`), the spread of the error outputs (`own`) and the margins of the first run"""
    out, other = estimate_once(pairs, R, t, K, **kw), estimate_once(pairs, R, t, K, order="sequential", **kw)
    near, moving = [], []
    for stage, bar in (("rotation", G.ROT_DONE), ("position", G.POS_DONE)):
        x, y = out["steps"][stage], other["steps"][stage]
        if len(x) != len(y) or any(abs(u - v) > G.NEAR_NOISE * u and bar / G.NEAR_FACTOR < u < bar * G.NEAR_FACTOR for u, v in zip(x, y)):
            near.append(stage)
        a, b = out["cg_counts"][stage], other["cg_counts"][stage]
        moving += [(stage, it) for it in range(max(len(a), len(b))) if it >= min(len(a), len(b)) or a[it] != b[it]]
    with np.errstate(invalid="ignore"):
        own = {k: float(np.nan_to_num(abs(out[k] - other[k])).max()) for k in ("rotation_error64", "direction_error64")}
    return dict(out, near=near, moving=moving, own=own, other=other)


def estimate_once(pairs, R, t, K, origin=0, baseline=None, weights=None, num_inliers=None, num_iterations=12, rotation_scale=5.0, max_rotation_error=15.0,
                  direction_scale=5.0, min_inliers=15, rotation_cg_iterations=ROTATION_CG_ITERATIONS, position_cg_iterations=POSITION_CG_ITERATIONS,
                  cg_tolerance=CG_TOLERANCE, order="ascending"):
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    P, n = len(pairs), int(num_iterations)
    R, t = np.asarray(R, np.float64).reshape(P, 3, 3), np.asarray(t, np.float64).reshape(P, 3)
    if weights is None:
        weights = np.ones(P) if num_inliers is None else np.asarray(num_inliers, np.float64)
    w = np.asarray(weights, np.float64)
    state = G.classify(pairs, R, t, w, num_inliers, min_inliers, K)
    adj = G.adjacency(pairs, state == G.USED, K)
    lists = Lists(adj, K)
    a, b = np.clip(pairs[:, 0], 0, K - 1), np.clip(pairs[:, 1], 0, K - 1)
    margins = dict(pq=np.inf, pivot=np.inf, stop=np.inf)
    counts, on_budget, failures = dict(rotation=[], position=[]), dict(rotation=0, position=0), 0

    # the tree
    level = np.full(K, -1)
    Rot = np.tile(np.eye(3), (K, 1, 1))
    level[origin] = 0
    L = 0
    while True:
        found = []
        for i in np.flatnonzero(level < 0):
            best = None
            for j, p in adj[i]:
                if level[j] == L and (best is None or w[p] > w[best[1]]):
                    best = (j, p)
            if best is not None:
                found.append((i,) + best)
        if not found:
            break
        for i, j, p in found:
            Rot[i] = R[p] @ Rot[j] if pairs[p, 1] == i else R[p].T @ Rot[j]
            level[i] = L + 1
        L += 1
    inside = level >= 0
    state[(state == G.USED) & ~inside[a]] = G.OUTSIDE

    # rotation averaging
    sigma0, rot_iters, steps = np.radians(rotation_scale), 0, dict(rotation=[], position=[])
    free = inside.copy()
    free[origin] = False
    ep, ei, ej = lists.pair, lists.img, lists.nbr
    for it in range(n):
        mult = max(1.0, 2.0 ** (n - 5 - it))
        live = state == G.USED
        om = np.zeros((P, 3))
        om[live] = G.so3_log(np.swapaxes(Rot[b[live]], 1, 2) @ (R[live] @ Rot[a[live]]))
        q = np.sqrt((om[:, 0] * om[:, 0] + om[:, 1] * om[:, 1]) + om[:, 2] * om[:, 2]) / (sigma0 * mult)
        we = w / (1.0 + q * q)
        wom = we[:, None] * om
        part = live[ep] & free[ei]
        sign = np.where(pairs[ep, 1] == ei, 1.0, -1.0)
        D = lists.sum(we[ep][:, None], part, order)[:, 0]
        rhs = lists.sum(sign[:, None] * wom[ep], part, order)
        with np.errstate(all="ignore"):
            inv = np.where(free, 1.0 / np.where(free, D, 1.0), 0.0)

        def apply_A(p):
            acc = lists.sum(we[ep][:, None] * p[ej], part, order)
            return np.where(free[:, None], D[:, None] * p - acc, 0.0)
        x, ran, budget, failed = pcg(apply_A, lambda r: inv[:, None] * r, np.where(free[:, None], rhs, 0.0), np.zeros((K, 3)), free, rotation_cg_iterations,
                                     cg_tolerance, order, margins)
        counts["rotation"].append(ran)
        on_budget["rotation"] += budget
        failures += failed
        Rot[free] = Rot[free] @ G.so3_exp(x[free])
        rot_iters = it + 1
        step = abs(x).max()
        if mult == 1.0:
            steps["rotation"].append(step)
        if mult == 1.0 and np.isfinite(x).all() and step < G.ROT_DONE:
            break
    live = state == G.USED
    rot_err = np.full(P, np.nan)
    rot_err[live] = np.degrees((G.so3_log(np.swapaxes(Rot[b[live]], 1, 2) @ (R[live] @ Rot[a[live]])) ** 2).sum(1) ** 0.5)
    state[live & (rot_err > max_rotation_error)] = G.ROTATION_OUTLIER
    live = state == G.USED

    # the baseline and the images that get a position
    d = np.zeros((P, 3))
    d[live] = -np.einsum("pji,pj->pi", Rot[b[live]], t[live] / np.sqrt((t[live] ** 2).sum(1))[:, None])
    chosen = None
    for j, p in adj[origin]:
        if live[p] and (baseline is None or j == baseline) and (chosen is None or w[p] > w[chosen[1]]):
            chosen = (j, p)
    present = np.zeros(K, bool)
    C = np.zeros((K, 3))
    pos_iters, ok = 0, chosen is not None
    if ok:
        base, pb = chosen
        C[base] = d[pb] if pairs[pb, 0] == origin else -d[pb]
        present = inside.copy()
        while True:
            nxt = present.copy()
            for i in np.flatnonzero(present):
                if i not in (origin, base):
                    nxt[i] = len({j for j, p in adj[i] if live[p] and present[j]}) >= 2
            if (nxt == present).all():
                break
            present = nxt
        state[live & ~(present[a] & present[b])] = G.NO_POSITION
        live = state == G.USED
        # position averaging
        fre = present.copy()
        fre[[origin, base]] = False
        tau0 = np.radians(direction_scale)
        part = live[ep] & fre[ei]
        to_base = ej == base
        for it in range(n):
            mult = max(1.0, 2.0 ** (n - 6 - it))
            rho = np.ones(P)
            if it > 0:
                rho[live] = ray_weight(d[live], C[b[live]] - C[a[live]], tau0 * mult)
            M = ray_block(d, w * rho)
            D = lists.sum(M[ep], part, order)
            rhs = lists.sum(ray_apply(M[ep], np.broadcast_to(C[base], (len(ep), 3))), part & to_base, order)
            tx = lists.sum(ray_apply(M[ep], C[ej]), part & ~to_base, order)
            x0 = np.where(fre[:, None], C, 0.0)
            r0 = np.where(fre[:, None], rhs - (ray_apply(D, x0) - tx), 0.0)
            Di, good, margin = tri_inverse3(D[fre])
            margins["pivot"] = min(margins["pivot"], margin)
            pos_iters = it + 1
            if not good.all():
                ok, failures = False, failures + 1
                break
            inv = np.zeros((K, 3, 3))
            inv[fre] = Di

            def precondition(r):
                return np.stack([(inv[:, s, 0] * r[:, 0] + inv[:, s, 1] * r[:, 1]) + inv[:, s, 2] * r[:, 2] for s in range(3)], 1)

            Mep = M[ep]

            def apply_A(p):
                acc = lists.sum(ray_apply(Mep, p[ej]), part, order)
                return np.where(fre[:, None], ray_apply(D, p) - acc, 0.0)
            x, ran, budget, failed = pcg(apply_A, precondition, r0, x0, fre, position_cg_iterations, cg_tolerance, order, margins)
            counts["position"].append(ran)
            on_budget["position"] += budget
            if failed:
                ok, failures = False, failures + 1
                break
            step = abs(x[fre] - C[fre]).max() if fre.any() else 0.0
            C[fre] = x[fre]
            if mult == 1.0:
                steps["position"].append(step)
            if mult == 1.0 and np.isfinite(step) and step < G.POS_DONE:
                break
    dir_err = np.full(P, np.nan)
    if ok:
        dir_err[live] = np.degrees(G.angle_to(d[live], C[b[live]] - C[a[live]]))
    poses = np.full((K, 3, 4), np.nan)
    poses[inside, :, :3] = Rot[inside]
    posed = present & ok
    poses[posed, :, 3] = -np.einsum("kij,kj->ki", Rot[posed], C[posed])
    image_state = np.where(posed, G.POSED, np.where(inside, G.ROTATION_ONLY, G.NOT_CONNECTED)).astype(np.uint8)
    return dict(poses64=poses, centres64=np.where(posed[:, None], C, np.nan), image_state=image_state, pair_state=state, rotation_error64=rot_err,
                direction_error64=dir_err, origin=int(origin), baseline=int(chosen[0]) if chosen else -1, num_posed=int(posed.sum()),
                rotation_iterations=rot_iters, position_iterations=pos_iters, positions_ok=bool(ok), steps=steps, cg_counts=counts,
                rotation_cg_iterations=sum(counts["rotation"]), position_cg_iterations=sum(counts["position"]),
                rotation_cg_unconverged=on_budget["rotation"], position_cg_unconverged=on_budget["position"], cg_failures=failures, margins=margins)


# ---------------------------------------------------------------------- scenes and the calls of the GPU file
@functools.lru_cache(maxsize=None)
def hub_scene():
    """K = 300: a ring plus 2 100 chords (8 pairs per image: with 3 the position solves take 524 solver iterations at 1e-13, a third of them end on a
    stalled residual and the centres sit 2.6e-3 of a float32 ulp from the dense definition's) with 0.3 degrees of noise; image 7 is paired (exactly) with every image it was not yet paired with: a list of 299
    entries; and the last ring pair is listed again reversed (two entries in either image's list): 300 entries in the hub's list if that pair touches it"""
    sc = G.scene(300, chords=2100, noise=0.3)
    have = {tuple(p) for p in sc["pairs"].tolist()}
    hub = 7
    extra = np.asarray([(min(hub, k), max(hub, k)) for k in range(300) if k != hub and (min(hub, k), max(hub, k)) not in have], np.int64)
    Re, te = G.relative(sc["Rg"], sc["cg"], extra)
    p = sc["pairs"].tolist().index([6, 7])                  # the ring pair (6, 7): listed again as (7, 6)
    again = sc["pairs"][p][::-1][None]
    Ra, ta = sc["R64"][p].T[None], (-sc["R64"][p].T @ sc["t64"][p])[None]
    rng = np.random.default_rng(300)
    pairs = np.concatenate([sc["pairs"], extra, again])
    R, t = np.concatenate([sc["R64"], Re, Ra]), np.concatenate([sc["t64"], te, ta])
    w = np.concatenate([sc["weights"], rng.integers(40, 400, len(extra) + 1).astype(np.float32)])
    return dict(pairs=pairs, R=R.astype(np.float32), t=t.astype(np.float32), weights=w, K=300, origin=0, hub=hub, Rg=sc["Rg"], cg=sc["cg"])


def no_baseline_scene():
    """K = 16 with every pair at the origin given a zero translation (state 2): the origin has no usable pair, so nothing is connected to it"""
    sc = G.scene(16, noise=0.3)
    t = sc["t"].copy()
    t[(sc["pairs"] == sc["origin"]).any(1)] = 0.0
    return dict(sc, t=t)


def permuted(sc, seed=5):
    order = np.random.default_rng(seed).permutation(len(sc["pairs"]))
    return dict(sc, pairs=sc["pairs"][order], R=sc["R"][order], t=sc["t"][order], weights=sc["weights"][order], order=order)


TIGHT = 1e-13
# name -> (scene, settings).  Budgets: a quarter above the oracle's largest count (tests/test_posegraph_pcg_cpu.py checks it), except where a test sets 1
CALLS = {
    "K3 tight": (lambda: G.scene(3, noise=0.3), dict(cg_tolerance=TIGHT)),
    "K16 tight": (lambda: G.scene(16, noise=0.3), dict(cg_tolerance=TIGHT)),
    "K49 tight": (lambda: G.scene(49, noise=0.3), dict(cg_tolerance=TIGHT)),
    "K16 default": (lambda: G.scene(16, noise=0.3), dict()),
    "K16 one": (lambda: G.scene(16, noise=0.3), dict(rotation_cg_iterations=1, position_cg_iterations=1)),
    "hub tight": (hub_scene, dict(cg_tolerance=TIGHT)),
    "big": (lambda: G.scene(1100, chords=7700, noise=0.3), dict(position_cg_iterations=600)),
    "edge": (lambda: G.edge_scene()[0], dict()),
    "edge clean": (lambda: G.edge_scene()[1], dict()),
    "collinear": (G.collinear_scene, dict()),
    "no baseline": (no_baseline_scene, dict()),
    # seed 2: on seeds 0, 1 and 3 the last position solves, whose warm-started residual is rounding already, stop after a count that moves with the order
    "K49 default": (lambda: G.scene(49, seed=2, noise=0.3), dict()),
    "K49 permuted": (lambda: permuted(G.scene(49, seed=2, noise=0.3)), dict()),
}
DENSE = ("K3 tight", "K16 tight", "K49 tight", "hub tight")        # the calls compared with the dense definition too


@functools.lru_cache(maxsize=None)
def answer(name):
    make, conf = CALLS[name]
    inp = make()
    return estimate(inp["pairs"], inp["R"], inp["t"], inp["K"], origin=inp.get("origin", 0), weights=inp["weights"], **conf)


@functools.lru_cache(maxsize=None)
def dense_answer(name):
    inp = CALLS[name][0]()
    return G.estimate(inp["pairs"], inp["R"], inp["t"], inp["K"], origin=inp.get("origin", 0), weights=inp["weights"])
