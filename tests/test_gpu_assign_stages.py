"""The matcher's head, stage by stage: final projection, similarity matrix, 256 -> 1 heads, log-sum-exp sweeps, argmax sweeps and finalize (lg_proj.hip /
lg_tail.hip final projection, lg_gemm.hip sim_kernel, lg_sim.hip, lg_pointwise.hip rowdot, lg_assign.hip) against the definition in tests/assign_oracle.py.

Every test runs ordinary forwards, reads the engine's buffers (lg_engine_debug_read) and compares ONE stage with the definition applied to that stage's own
input as the device holds it, so an error is charged to the kernel that made it and nothing hides behind `exp` or a 2e-4 absolute bar.

Fixtures are built by module-level functions that need no GPU (`fixture`, `head_fixture`); tests/test_assign_oracle_cpu.py sees the same arrays, asserts the
properties the tests below rely on, and measures the floors behind every bound that is not derived:

  MD      err / rms <= _STAGE_TOL[precision] of test_gpu_parity.py (the bound the projection's input x_out already meets), against the float64 oracle.
  SIM     |err| / sum_k |a_k||b_k| <= 4 x SIM_FLOOR (+ 2^-22 for the lo . lo product the split-f16 scheme omits).  SIM_FLOOR is what a np.float32 matmul of the
          oracle's md shows against float64: another summation order moves an fp32 dot product by about its own round-off; a dropped split term (2^-11) or
          a wrong k chunk is 40 x larger or more.
  heads   |err| <= 4 x HEAD_FLOOR x (sum_k |x_k||w_k| + |b|) + 2^-23 |value|: the floor is that of a np.float32 evaluation (dot product, then the stable
          forms) against float64, in the dot product's unit because every output has a slope <= 1 in z; the relative term is expf / log1pf's last place.
  LSE     |err| <= 2^-23 |lse| + 4 x LSE_FLOOR, the floor being the larger of a sequential float32 sum and np.logaddexp.reduce in float32 on the oracle's
          sim of every fixture.  The reduce rounds its running value, of magnitude |lse| = 30 .. 100, once per entry and is the larger by 30 x: a bound
          that wide (7e-4) would pass a sweep that loses one average column of 1300.  The kernels sum exponentials against the maximum like the sequential
          sum, so the tests assert the narrower 2^-23 |lse| + 4 x LSE_SEQ_FLOOR (3.3e-5 at most), which implies the other.
  argmax  exact: indices and the float32 bit patterns of the maxima (the score expression has no multiplication, so numpy float32 computes the same bits).
  outputs indices and counts exact; scores within 4 x 2^-24 relative of float64 exp of the float32 maximum (HIP documents 1 ulp for expf).
Measured values: profiles/assign_stage_tests.md."""
import collections
import functools

import numpy as np
import pytest
import torch

import assign_oracle as A
import gpu_util
from conftest import require_gpu
from lightglue_amd import synthetic as synth
from oracle import lightglue_oracle as O

pytestmark = pytest.mark.gpu

# floors measured by tests/test_assign_oracle_cpu.py::test_floors_behind_the_gpu_bounds (which asserts that they still hold) — see the module docstring
SIM_FLOOR = 1.2e-6        # np.float32 matmul of the oracle's md against float64, per sum_k |a_k||b_k|
HEAD_FLOOR = 4.0e-8       # np.float32 head against float64, per (sum_k |x_k||w_k| + |b|)
LSE_FLOOR = 1.7e-4        # float32 log-sum-exp (sequential sum / logaddexp.reduce, the larger) against float64, absolute
LSE_SEQ_FLOOR = 5.3e-6    # the sequential float32 sum alone
STAGE_TOL = {"fp32": 2e-5, "f16x3": 5e-4}        # test_gpu_parity._STAGE_TOL
EXP_TOL = 4 * 2.0 ** -24

MODES = collections.OrderedDict([("fp32", ("fp32", {})), ("f16x3", ("f16x3", {})), ("f16x3-rows", ("f16x3", {"sim_planes": 0}))])

# ---------------------------------------------------------------------------------------------------------------- fixtures (no GPU)
Fixture = collections.namedtuple("Fixture", "sd data conf num0 num1")
CONF1 = dict(n_layers=1, depth_confidence=-1, width_confidence=-1)
SHAPES = {"1x1025": (1, 1025), "33x1021": (33, 1021), "1057x5": (1057, 5), "5x700": (5, 700), "300x1300": (300, 1300), "600x1025": (600, 1025)}
RAGGED0, RAGGED1 = (300, 31, 0), (1300, 1025, 77)
# identical image-1 rows (columns of sim): the same float4 of one thread / two lanes of a wave / two waves of a pass / the two passes / three places
DUP_COLS = ((40, 42), (10, 201), (20, 600), (30, 1100), (50, 700, 1200))
# identical image-0 rows: inside a 32-row tile / tiles 1, 2 (waves 1, 2 of the column merge) / tiles 3, 7 (both wave 3) / tiles 4, 9 (waves 0, 1)
DUP_ROWS = ((3, 9), (40, 70), (100, 230), (130, 290))
FIXTURES = tuple(SHAPES) + ("ragged", "tie-33x1025", "tie-1057x5", "dups", "adaptive")


@functools.lru_cache(maxsize=None)
def one_layer_sd(tie=False):
    sd = synth.make_state_dict(0, recipe="A", n_layers=1)
    if tie:   # every MD row is the bias and every matchability logit the bias: exact ties wherever a row sits
        sd["log_assignment.0.final_proj.weight"] = np.zeros_like(sd["log_assignment.0.final_proj.weight"])
        sd["log_assignment.0.matchability.weight"] = np.zeros_like(sd["log_assignment.0.matchability.weight"])
    return sd


def _shuffled_columns(data, seed):
    """make_batch puts the true partners in the first min(n0, n1) rows of image 1: spread them over all of them (and so over both column passes)"""
    for b in range(data["image1"]["keypoints"].shape[0]):
        perm = np.random.Generator(np.random.PCG64(seed + b)).permutation(data["image1"]["keypoints"].shape[1])
        for key in ("keypoints", "descriptors"):
            data["image1"][key][b] = data["image1"][key][b][perm]
    return data


@functools.lru_cache(maxsize=None)
def fixture(name):
    if name in SHAPES:
        n0, n1 = SHAPES[name]
        data = synth.make_batch(3, 1, n0, n1)
        if name == "300x1300":
            data = _shuffled_columns(data, 100)
        return Fixture(one_layer_sd(), data, {**CONF1, **({"filter_threshold": 0.0} if name == "600x1025" else {})}, None, None)
    if name == "ragged":   # dead row tiles, an empty image, sim entries beyond len1 that are garbage by construction; padding rows are NaN
        data = _shuffled_columns(synth.make_batch(11, 3, 300, 1300), 200)
        for key, counts in (("image0", RAGGED0), ("image1", RAGGED1)):
            for b, c in enumerate(counts):
                data[key]["keypoints"][b, c:] = np.nan
                data[key]["descriptors"][b, c:] = np.nan
        return Fixture(one_layer_sd(), data, CONF1, RAGGED0, RAGGED1)
    if name.startswith("tie-"):
        n0, n1 = (int(v) for v in name[4:].split("x"))
        return Fixture(one_layer_sd(True), synth.make_batch(7, 1, n0, n1), {**CONF1, "filter_threshold": 0.0}, None, None)
    if name == "dups":     # the partners of image 0's rows are image 1's first 300 rows: every source below has a row (column) whose best score it is
        data = synth.make_batch(13, 1, 300, 1300)
        for key, groups in (("image1", DUP_COLS), ("image0", DUP_ROWS)):
            for g in groups:
                for k in ("keypoints", "descriptors"):
                    data[key][k][0, list(g[1:])] = data[key][k][0, g[0]]
        return Fixture(one_layer_sd(), data, CONF1, None, None)
    if name == "adaptive":  # pruned index sets (IND scatter) and the FINAL_LAYER weight select
        return Fixture(synth.make_state_dict(0, recipe="C", n_layers=3), synth.make_batch(9, 1, 600, 520),
                       dict(n_layers=3, pruning_min_kpts=64, filter_threshold=0.0), None, None)
    raise KeyError(name)


def pair_inputs(fx, b):
    """pair b of a fixture as the oracle takes it: (kpts0, kpts1, desc0, desc1, size0, size1), cut to the pair's own counts"""
    d0, d1 = fx.data["image0"], fx.data["image1"]
    c0 = d0["keypoints"].shape[1] if fx.num0 is None else fx.num0[b]
    c1 = d1["keypoints"].shape[1] if fx.num1 is None else fx.num1[b]
    return d0["keypoints"][b, :c0], d1["keypoints"][b, :c1], d0["descriptors"][b, :c0], d1["descriptors"][b, :c1], d0["image_size"][b], d1["image_size"][b]


@functools.lru_cache(maxsize=None)
def oracle_traces(name, dtype=np.float64):
    """[(output dict, trace)] per pair: the oracle's forward with the assignment's inputs traced (md0, md1, sim, z0, z1, ind0, ind1, scores_full)"""
    fx, res = fixture(name), []
    for b in range(fx.data["image0"]["keypoints"].shape[0]):
        tr = {}
        out = O.forward_pair(fx.sd, O.make_conf(**fx.conf), *pair_inputs(fx, b), dtype=dtype, trace=tr)
        res.append((out, tr))
    return res


HEAD_SHAPES = ((1, 65), (129, 17))
# two layers, so that layer 0 has a token head; depth_confidence 1 never stops and width_confidence 1 keeps every point (sigmoid > 0), so both adaptive
# heads run and no row moves; recipe C spreads the logits over both signs
HEAD_CONF = dict(n_layers=2, depth_confidence=1.0, width_confidence=1.0, pruning_min_kpts=-1)


@functools.lru_cache(maxsize=None)
def head_fixture(shape):
    return Fixture(synth.make_state_dict(0, recipe="C", n_layers=2), synth.make_batch(7, 2, *shape), HEAD_CONF, None, None)


def head_weights(sd, kind, layer):
    pre = f"token_confidence.{layer}.token.0." if kind == "token" else f"log_assignment.{layer}.matchability."
    return sd[pre + "weight"], sd[pre + "bias"]


def head_scale(x, w, b):
    """sum_k |x_k||w_k| + |b| per row: the unit of a head's rounding error"""
    return np.abs(np.asarray(x, np.float64)) @ np.abs(np.asarray(w, np.float64).reshape(-1)) + abs(float(np.asarray(b).reshape(-1)[0]))


def split_f16(x):
    """the operand the split-f16 kernels multiply: hi + lo, both f16 (lg_common.h split8)"""
    return O.round_fp16x2(np.asarray(x, np.float32)).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------- device snapshots
def _run(fx, mode, fused_tail=1, log_assignment=False, stop=-1):
    precision, options = MODES[mode]
    model = gpu_util.make_model(fx.sd, precision, **fx.conf)
    model.set_option("fused_tail", fused_tail)
    for key, value in options.items():
        model.set_option(key, value)
    model.return_log_assignment = log_assignment
    tdata = gpu_util.to_torch(fx.data)
    if fx.num0 is not None:
        tdata["image0"]["num_keypoints"] = torch.tensor(fx.num0, dtype=torch.int32)
        tdata["image1"]["num_keypoints"] = torch.tensor(fx.num1, dtype=torch.int32)
    model.debug_stop_after(stop)
    out = model(tdata)
    return model, out


def _rows(model, fx):
    B, n0 = fx.data["image0"]["keypoints"].shape[:2]
    return gpu_util.Rows(B, n0, fx.data["image1"]["keypoints"].shape[1], *model.debug_caps())


@functools.lru_cache(maxsize=None)
def snapshot(name, mode):
    """One full forward of a fixture; per pair, every buffer of the head cut to the pair's live rows (LEN), and the pair's outputs."""
    fx = fixture(name)
    model, out = _run(fx, mode)
    rows = _rows(model, fx)
    B, c0, c1, R = rows.B, rows.c0, rows.c1, rows.R
    planes = MODES[mode][0] == "f16x3" and MODES[mode][1].get("sim_planes", 1)
    if planes:      # f16 hi plane, then f16 lo plane, [2][R][256]
        md = model.debug_read("MD", np.float16).astype(np.float64).reshape(2, R, 256).sum(0)
    else:
        md = model.debug_read("MD", np.float32).reshape(R, 256)
    sim = model.debug_read("SIM", np.float32).reshape(B, c0, c1)
    row = {k: model.debug_read(k, np.float32) for k in ("LS", "X")}
    per0 = {k: model.debug_read(k, t).reshape(B, c0) for k, t in (("LSE_R", np.float32), ("MAX0", np.float32), ("ARG0", np.int32))}
    per1 = {k: model.debug_read(k, t).reshape(B, c1) for k, t in (("LSE_C", np.float32), ("MAX1", np.float32), ("ARG1", np.int32))}
    ind, length = model.debug_read("IND", np.int32), model.debug_read("LEN", np.int32).reshape(B, 2)
    final_layer = model.debug_read("FINAL_LAYER", np.int32)
    pairs = []
    for b in range(B):
        len0, len1 = int(length[b, 0]), int(length[b, 1])
        s0, s1 = rows.sl(b, 0), rows.sl(b, 1)
        live0, live1 = slice(s0.start, s0.start + len0), slice(s1.start, s1.start + len1)
        p = dict(len0=len0, len1=len1, md0=md[live0], md1=md[live1], sim=sim[b, :len0, :len1], ls0=row["LS"][live0], ls1=row["LS"][live1],
                 x0=row["X"].reshape(R, 256)[live0], x1=row["X"].reshape(R, 256)[live1], ind0=ind[live0], ind1=ind[live1], final_layer=int(final_layer[b]))
        if MODES[mode][0] == "f16x3" and not planes:   # fp32 rows, split into hi + lo where sim_kernel stages them
            p["md0_op"], p["md1_op"] = split_f16(p["md0"]), split_f16(p["md1"])
        else:
            p["md0_op"], p["md1_op"] = p["md0"], p["md1"]
        p.update({k: v[b, :len0] for k, v in per0.items()})
        p.update({k: v[b, :len1] for k, v in per1.items()})
        for key in ("matches0", "matches1", "matching_scores0", "matching_scores1"):
            p[key] = out[key][b].cpu().numpy()
        p["matches"], p["scores"] = out["matches"][b].cpu().numpy(), out["scores"][b].cpu().numpy()
        pairs.append(p)
    return pairs


def live_pairs(name, mode):
    return [(b, p) for b, p in enumerate(snapshot(name, mode)) if p["len0"] > 0 and p["len1"] > 0]


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- 1. final projection, similarity
@pytest.mark.parametrize("mode", MODES)
def test_final_projection_against_the_oracle(mode):
    """MD (the final projection, / 256^(1/4) included; with the weights FINAL_LAYER selects in the adaptive pair) against the float64 oracle's md0 / md1."""
    require_gpu()
    tol, bad, compared = STAGE_TOL[MODES[mode][0]], {}, 0
    for name in FIXTURES:
        for b, p in live_pairs(name, mode):
            out, tr = oracle_traces(name)[b]
            if name == "adaptive":   # rows are in pruned order: comparable when the device kept the oracle's rows (it must in fp32, test_gpu_parity.py)
                same = np.array_equal(p["ind0"], tr["ind0"]) and np.array_equal(p["ind1"], tr["ind1"]) and p["final_layer"] + 1 == out["stop"]
                assert same or mode != "fp32", "fp32 pruning differs from the oracle's"
                assert len(tr["ind0"]) < 600 or len(tr["ind1"]) < 520, "fixture never pruned"
                if not same:
                    print(f"MD {mode} adaptive: the device pruned other rows than the float64 oracle, pair not compared")
                    continue
            for im in (0, 1):
                e = gpu_util.err(p[f"md{im}"], tr[f"md{im}"])
                compared += 1
                print(f"MD {mode} {name}[{b}] image {im}: max abs {e[0]:.3e}  err/rms {e[1]:.3e}  (bound {tol:g})")
                if not e[1] <= tol:
                    bad[(name, b, im)] = e
    assert not bad, bad
    assert compared >= 2 * (len(FIXTURES) + 1) - 2


@pytest.mark.parametrize("mode", MODES)
def test_similarity_of_the_devices_own_md(mode):
    """SIM[:len0, :len1] against the float64 product of the device's own MD operands, per sum_k |a_k||b_k|."""
    require_gpu()
    tol, bad = 4 * SIM_FLOOR + (2.0 ** -22 if MODES[mode][0] == "f16x3" else 0.0), {}
    for name in FIXTURES:
        for b, p in live_pairs(name, mode):
            e = float((np.abs(p["sim"] - A.sim(p["md0_op"], p["md1_op"])) / A.sim_scale(p["md0_op"], p["md1_op"])).max())
            print(f"SIM {mode} {name}[{b}]: max |err| / sum|a||b| {e:.3e}  (bound {tol:.3e})")
            if not e <= tol:
                bad[(name, b)] = e
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------- 2. heads
def _head_errors(tag, got, want, scale, bad):
    err = np.abs(got.astype(np.float64) - want)
    bound = 4 * HEAD_FLOOR * scale + 2.0 ** -23 * np.abs(want)
    worst = int(np.argmax(err / bound)) if err.size else 0
    print(f"heads {tag}: max |err| {err.max():.3e}  worst err / bound {float((err / bound).max()):.3f}")
    if not (err <= bound).all():
        bad[tag] = (float(err[worst]), float(bound[worst]))


@pytest.mark.parametrize("fused", [1, 0], ids=["tail", "rowdot"])
@pytest.mark.parametrize("mode", ["fp32", "f16x3"])
def test_heads_of_the_crossblock_tail(mode, fused):
    """CONF, MSCORE, LS, LSNEG against heads() of the device's own X: from the fused tail's head block (stopped behind layer 0's CrossBlock), and from
    rowdot (fused_tail = 0: CONF / MSCORE in the adaptive step behind layer 0, LS / LSNEG in the assignment's own pass over the last layer's X)."""
    require_gpu()
    bad = {}
    for shape in HEAD_SHAPES:
        fx = head_fixture(shape)
        # (step the forward stops behind, buffers that step leaves, layer whose weights they were made with)
        runs = [(12, ("CONF", "MSCORE", "LS", "LSNEG"), 0)] if fused else [(13, ("CONF", "MSCORE"), 0), (-1, ("LS", "LSNEG"), 1)]
        for stop, names, layer in runs:
            model, _ = _run(fx, mode, fused_tail=fused, log_assignment=True, stop=stop)
            rows = _rows(model, fx)
            length = model.debug_read("LEN", np.int32).reshape(rows.B, 2)
            assert (length == np.array(shape)).all(), "a row was pruned: X is not the heads' input any more"
            x = model.debug_read("X", np.float32).reshape(rows.R, 256)
            bufs = {k: model.debug_read(k, np.float32) for k in names}
            for b in range(rows.B):
                for im in (0, 1):
                    sl = rows.sl(b, im)
                    for kind, outs in (("token", {"CONF": 1}), ("match", {"MSCORE": 1, "LS": 2, "LSNEG": 3})):
                        if not set(outs) & set(bufs):
                            continue
                        w, bias = head_weights(fx.sd, kind, layer)
                        ref = A.heads(x[sl], w, bias)
                        for key, which in outs.items():
                            if key in bufs:
                                _head_errors(f"{mode} {'tail' if fused else 'rowdot'} {shape}[{b}] image {im} {key}", bufs[key][sl], ref[which], head_scale(x[sl], w, bias), bad)
            model.debug_stop_after(-1)
    assert not bad, bad


@pytest.mark.parametrize("mode", ["fp32", "f16x3"])
def test_matchability_term_after_a_full_forward(mode):
    """LS as the assignment reads it, against heads() of the device's own final X, at every fixed-depth fixture."""
    require_gpu()
    bad = {}
    for name in FIXTURES:
        if name == "adaptive":     # its final rows may sit in the gather path's second buffer set
            continue
        fx = fixture(name)
        w, bias = head_weights(fx.sd, "match", 0)
        for b, p in live_pairs(name, mode):
            for im in (0, 1):
                _head_errors(f"{mode} {name}[{b}] image {im} LS", p[f"ls{im}"], A.heads(p[f"x{im}"], w, bias)[2], head_scale(p[f"x{im}"], w, bias), bad)
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------- 3. log-sum-exp
@pytest.mark.parametrize("mode", MODES)
def test_log_sum_exp_of_the_devices_own_sim(mode):
    """LSE_R / LSE_C against float64 log-sum-exp of the device's own SIM; the all-tie fixtures also against their closed form c + log(len)."""
    require_gpu()
    bad = {}
    for name in FIXTURES:
        for b, p in live_pairs(name, mode):
            for key, want in (("LSE_R", A.lse_rows(p["sim"])), ("LSE_C", A.lse_cols(p["sim"]))):
                err, bound = np.abs(p[key].astype(np.float64) - want), 2.0 ** -23 * np.abs(want) + 4 * LSE_SEQ_FLOOR     # <= ... + 4 * LSE_FLOOR
                print(f"LSE {mode} {name}[{b}] {key}: max |err| {err.max():.3e}  worst err / bound {float((err / bound).max()):.3f}")
                if not (err <= bound).all():
                    bad[(name, b, key)] = float(err.max())
            if name.startswith("tie-"):
                c = float(p["sim"][0, 0])
                assert (bits(p["sim"]) == bits(p["sim"])[0, 0]).all(), "all-tie fixture: sim is not constant"
                for key, n in (("LSE_R", p["len1"]), ("LSE_C", p["len0"])):
                    want = c + np.log(n)
                    assert np.abs(p[key] - want).max() <= 2.0 ** -23 * abs(want) + 4 * LSE_SEQ_FLOOR, (name, key, float(np.abs(p[key] - want).max()))
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------- 4. argmax
def _argmax_of_device_inputs(p):
    return A.argmax_first(A.scores_f32(p["sim"], p["LSE_R"], p["LSE_C"], p["ls0"], p["ls1"]))


@pytest.mark.parametrize("mode", MODES)
def test_argmax_is_exact_and_takes_the_first_index(mode):
    """MAX0 / ARG0 / MAX1 / ARG1 equal, to the bit and to the index, the first-index argmax of the float32 scores of the device's own SIM, LSE_R, LSE_C and
    LS — every live row and column of every fixture, near-ties included."""
    require_gpu()
    bad = []
    for name in FIXTURES:
        for b, p in live_pairs(name, mode):
            max0, arg0, max1, arg1 = _argmax_of_device_inputs(p)
            for key, want in (("ARG0", arg0), ("ARG1", arg1)):
                if not np.array_equal(p[key], want):
                    bad.append((name, b, key, int((p[key] != want).sum()), np.where(p[key] != want)[0][:8].tolist()))
            for key, want in (("MAX0", max0), ("MAX1", max1)):
                if not np.array_equal(bits(p[key]), bits(want)):
                    bad.append((name, b, key, int((bits(p[key]) != bits(want)).sum())))
            if name.startswith("tie-"):
                assert (p["ARG0"] == 0).all() and (p["ARG1"] == 0).all(), (name, "an all-tie row or column did not take index 0")
    assert not bad, bad
    p = snapshot("300x1300", mode)[0]
    assert (p["ARG0"] >= 1024).any() and (p["ARG0"] < 1024).any(), "no row of the 300 x 1300 fixture has its best column in the second pass"


@pytest.mark.parametrize("mode", MODES)
def test_duplicate_rows_and_columns_tie_to_the_lowest_index(mode):
    """Identical keypoints give bit-identical SIM rows / columns and LS entries wherever they sit (the kernels' arithmetic does not depend on a row's position),
    and whenever a row's (column's) best score belongs to a duplicate group, the winner is the group's lowest index — for groups inside one lane, across
    lanes, across waves and across the two column passes; inside a row tile, across tiles of different merge waves and of the same one."""
    require_gpu()
    p = snapshot("dups", mode)[0]
    for g in DUP_COLS:
        for j in g[1:]:
            assert np.array_equal(bits(p["sim"][:, j]), bits(p["sim"][:, g[0]])), f"sim columns {g[0]} and {j} of identical keypoints differ"
            assert bits(p["ls1"][j]) == bits(p["ls1"][g[0]]) and bits(p["LSE_C"][j]) == bits(p["LSE_C"][g[0]]), f"LS / LSE_C of columns {g[0]} and {j} differ"
    for g in DUP_ROWS:
        for i in g[1:]:
            assert np.array_equal(bits(p["sim"][i]), bits(p["sim"][g[0]])), f"sim rows {g[0]} and {i} of identical keypoints differ"
            assert bits(p["ls0"][i]) == bits(p["ls0"][g[0]]) and bits(p["LSE_R"][i]) == bits(p["LSE_R"][g[0]]), f"LS / LSE_R of rows {g[0]} and {i} differ"
    for key, groups in (("ARG0", DUP_COLS), ("ARG1", DUP_ROWS)):
        for g in groups:
            winners = p[key][np.isin(p[key], g)]
            assert winners.size, f"{key}: no winner comes from the duplicate group {g}"
            assert (winners == min(g)).all(), f"{key}: group {g} was won by {sorted(set(winners.tolist()))}"


# ---------------------------------------------------------------------------------------------------------------- 5. finalize and outputs
@pytest.mark.parametrize("mode", MODES)
def test_outputs_are_finalize_of_the_devices_own_argmax(mode):
    """matches0 / matches1 / matches / n_matches of the returned dict against finalize() of the device's own MAX0, ARG0, ARG1, IND, LEN: ragged (an empty
    image, dead row tiles), pruned index sets, one match among exact ties, valid matches in each of three 256-row blocks, a last workgroup without rows."""
    require_gpu()
    for name in FIXTURES:
        fx = fixture(name)
        n0, n1 = fx.data["image0"]["keypoints"].shape[1], fx.data["image1"]["keypoints"].shape[1]
        for b, p in enumerate(snapshot(name, mode)):
            if p["len0"] == 0 or p["len1"] == 0:      # ref :539-540, :568-588: nothing was computed for the pair
                p = {**p, "MAX0": np.zeros(0, np.float32), "ARG0": np.zeros(0, np.int32), "ARG1": np.zeros(0, np.int32), "ind0": np.zeros(0, np.int32), "ind1": np.zeros(0, np.int32)}
            want = A.finalize(p["MAX0"], p["ARG0"], p["ARG1"], p["ind0"], p["ind1"], n0, n1, fx.conf.get("filter_threshold", 0.1))
            tag = (name, b)
            np.testing.assert_array_equal(p["matches0"], want["matches0"], err_msg=str(tag))
            np.testing.assert_array_equal(p["matches1"], want["matches1"], err_msg=str(tag))
            assert len(p["matches"]) == want["n_matches"], tag
            np.testing.assert_array_equal(p["matches"].reshape(-1, 2), want["matches"], err_msg=str(tag))
            for key, ref in (("matching_scores0", want["scores0"]), ("matching_scores1", want["scores1"]), ("scores", want["match_scores"])):
                assert ((p[key] == 0) == (ref == 0)).all(), (tag, key)
                assert (np.abs(p[key] - ref) <= EXP_TOL * ref).all(), (tag, key, float(np.abs(p[key] - ref).max()))
            print(f"outputs {mode} {name}[{b}]: live {p['len0']} x {p['len1']}, {want['n_matches']} matches")
            if name.startswith("tie-"):
                assert p["matches"].tolist() == [[0, 0]], tag
            if name == "600x1025":
                blocks = np.bincount(want["matches"][:, 0] // 256, minlength=3)
                assert (blocks > 0).all(), f"valid matches per 256-row block {blocks.tolist()}: the count of the rows below is not exercised"
            if name == "adaptive":
                assert p["len0"] < n0 or p["len1"] < n1, "fixture never pruned"
            if name == "ragged" and b == 2:
                assert want["n_matches"] == 0 and (p["matches0"] == -1).all() and (p["matches1"] == -1).all()
