"""The oracle (oracle/lightglue_oracle.py) against the golden vectors produced by the real reference
(tools/make_golden.py), and against the reference's recorded output on a case outside that set."""
import numpy as np
import pytest

from conftest import golden_names, load_golden, oracle_conf_for
from oracle import lightglue_oracle as O
from lightglue_amd import synthetic as synth
import make_golden


def oracle_score_atol(name):
    """Two fp32 evaluations of the same network (the reference on ATen, this oracle on numpy / ATen kernels in another order) differ by
    summation order alone.  Recipes A - D: <= 1.4e-4.  The confident-match fixtures (recipe E: residual rms 27 AND scores spread over
    (0, 1), where d score / d logit is largest) have a wider fp32 floor — measured here (round 4): numpy 5.6e-4, ATen backend 4.4e-4,
    and the float64 evaluation of the oracle is itself 7.1e-4 away from the reference's fp32 output (2048x512).  Indices are identical
    in every case.  The 1e-3 bar therefore leaves the GPU path ~3e-4 of its own on those fixtures."""
    return 7e-4 if name.startswith("trained_stats_confident") else 2e-4


@pytest.mark.parametrize("name", golden_names())
def test_oracle_matches_reference_golden(name):
    meta, gold = load_golden(name)
    case = meta["case"]
    sd, data = make_golden.case_inputs(case)
    assert synth.state_dict_digest(sd) == meta["weights_sha256"], "seeded weight generator drifted"
    out = O.forward(sd, oracle_conf_for(case), data)
    np.testing.assert_array_equal(out["matches0"], gold["matches0"])
    np.testing.assert_array_equal(out["matches1"], gold["matches1"])
    atol = oracle_score_atol(name)
    np.testing.assert_allclose(out["matching_scores0"], gold["matching_scores0"], atol=atol, rtol=0)
    np.testing.assert_allclose(out["matching_scores1"], gold["matching_scores1"], atol=atol, rtol=0)
    assert out["stop"] == gold["stop"].tolist()
    np.testing.assert_array_equal(np.asarray(out["prune0"], np.float32), gold["prune0"])
    np.testing.assert_array_equal(np.asarray(out["prune1"], np.float32), gold["prune1"])
    assert [len(m) for m in out["matches"]] == gold["n_matches"].tolist()
    for b, ml in enumerate(out["matches"]):  # sorted by index0 (torch.where order, ref :596)
        assert np.all(np.diff(ml[:, 0]) > 0)
        np.testing.assert_array_equal(ml[:, 1], out["matches0"][b][ml[:, 0]])


# the torch-kernel backend of the oracle (the timed cpu_baseline leg of bench.py) is pinned against the same fixtures: small / edge cases,
# both adaptive paths, trained statistics, 128-d and scale/orientation inputs, and the bench batch's own fixture
TORCH_BACKEND_CASES = [n for n in golden_names() if any(t in n for t in ("bbox_300x200", "empty", "1x17", "5x3", "adaptive_9x30", "adaptive_1024",
                                                                          "trained_stats_512", "trained_stats_confident_512", "trained_stats_confident_adaptive_1024", "sift", "disk128_256", "mutualnn", "nonadaptive_1024_b4"))]


@pytest.mark.parametrize("name", TORCH_BACKEND_CASES)
def test_torch_backend_matches_reference_golden(name):
    meta, gold = load_golden(name)
    sd, data = make_golden.case_inputs(meta["case"])
    out = O.forward(sd, oracle_conf_for(meta["case"]), data, backend="torch")
    np.testing.assert_array_equal(out["matches0"], gold["matches0"])
    np.testing.assert_array_equal(out["matches1"], gold["matches1"])
    atol = oracle_score_atol(name)
    np.testing.assert_allclose(out["matching_scores0"], gold["matching_scores0"], atol=atol, rtol=0)
    np.testing.assert_allclose(out["matching_scores1"], gold["matching_scores1"], atol=atol, rtol=0)
    assert out["stop"] == gold["stop"].tolist()
    np.testing.assert_array_equal(np.asarray(out["prune0"], np.float32), gold["prune0"])
    np.testing.assert_array_equal(np.asarray(out["prune1"], np.float32), gold["prune1"])


def test_oracle_live_against_reference():
    """The oracle against the reference's own output on a case outside the fixture set (weights seed 5, N = 160, M = 140), recorded by
    tools/make_golden.py's run_reference in tests/golden/reference_live_160x140.json."""
    import json
    from pathlib import Path
    rec = json.loads((Path(__file__).resolve().parent / "golden" / "reference_live_160x140.json").read_text())
    case = rec["case"]
    assert case == dict(recipe="A", wseed=5, dseed=123, B=1, n=160, m=140, dim=256, conf=dict(depth_confidence=-1, width_confidence=-1))
    ref = {k: np.asarray([p[k] for p in rec["pairs"]]) for k in ("matches0", "matching_scores0")}
    sd, data = make_golden.case_inputs(case)
    out = O.forward(sd, oracle_conf_for(case), data)
    np.testing.assert_array_equal(out["matches0"], ref["matches0"])
    np.testing.assert_allclose(out["matching_scores0"], ref["matching_scores0"].astype(np.float32), atol=2e-4)


def test_float64_truth_agrees_with_fp32_reference():
    meta, gold = load_golden("nonadaptive_bbox_300x200")
    sd, data = make_golden.case_inputs(meta["case"])
    out = O.forward(sd, oracle_conf_for(meta["case"]), data, dtype=np.float64)
    assert (out["matches0"] != gold["matches0"]).sum() == 0
    assert np.abs(out["matching_scores0"] - gold["matching_scores0"]).max() < 2e-4


def test_operand_rounding_emulation_orders():
    """What justifies the HIP path's precision allocation, on a diffuse-attention fixture (recipe A) and on a
    trained-statistics one (recipe D): plain bf16 breaks the bar everywhere; the fast opt-in (one f16 plane on the q.k / P.V
    path) holds it only while attention is diffuse; the default (split f16 everywhere) holds it on both."""
    e = {}
    for name in ("nonadaptive_bbox_300x200", "trained_stats_512"):
        meta, gold = load_golden(name)
        sd, data = make_golden.case_inputs(meta["case"])
        conf = oracle_conf_for(meta["case"])
        for tag, q in (("bf16", "bf16"), ("fast", O.FAST_ATTENTION_QUANT), ("default", O.DEFAULT_PRECISION_QUANT)):
            out = O.forward(sd, conf, data, quant=q)
            same = out["matches0"] == gold["matches0"]
            e[name, tag] = np.abs(out["matching_scores0"] - gold["matching_scores0"])[same].max()
    A, D = "nonadaptive_bbox_300x200", "trained_stats_512"
    assert e[A, "default"] < 1e-3 and e[A, "fast"] < 1e-3 < e[A, "bf16"], e
    assert e[D, "default"] < 1e-3 < e[D, "fast"] < e[D, "bf16"], e
    assert e[D, "fast"] > 10 * e[D, "default"], e      # an order of magnitude: sharp logits need the split on the whole q.k / P.V path


def test_oracle_matches_the_reference_on_the_trained_checkpoint_when_present():
    """The synthetically trained checkpoint (tools/train_synthetic_checkpoint.py; git-ignored, build container only): the oracle restatement against the unmodified
    reference on it — what lets the oracle stand in for the reference on the GPU box for these weights (tools/verify_pretrained.py --cpu-only)."""
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parents[1]
    ck = root / "tests" / "golden" / "_local" / "synthetic_trained_L9.pth"
    if not ck.exists() or not Path("/root/reference/lightglue/lightglue.py").exists():
        pytest.skip("needs the trained checkpoint and the reference checkout (build container)")
    p = subprocess.run([sys.executable, str(root / "tools" / "verify_pretrained.py"), str(ck), "--cpu-only", "--sizes", "256", "--pairs", "1"],
                       capture_output=True, text=True, timeout=900, cwd=str(root))
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    rows = [ln for ln in p.stdout.splitlines() if ln.startswith("| synthetic")]
    assert len(rows) == 2 and all("| 0 / 0 |" in ln and "equal | equal" in ln for ln in rows), rows
