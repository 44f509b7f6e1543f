"""Host side of LightGlue.match_pairs (no GPU): the chunk planner, the constants of the indexed C-ABI call, and the checks that run before any launch."""
import re
from pathlib import Path

import pytest
import torch

from lightglue_amd import LightGlue, _cabi
from lightglue_amd.lightglue import plan_pair_chunks

HEADER = (Path(__file__).resolve().parent.parent / "include" / "lightglue_amd.h").read_text()
MAX_ROWS, MAX_SIM = 2 ** 21, 2 ** 31 - 1


def _cap(n):
    return (n + 127) // 128 * 128


def _fits(pairs, n0, n1, max_rows, max_sim):
    return pairs * (_cap(n0) + _cap(n1)) <= max_rows and pairs * _cap(n0) * _cap(n1) <= max_sim


@pytest.mark.parametrize("P,n0,n1,max_rows,max_sim", [
    (256, 4096, 4096, MAX_ROWS, MAX_SIM), (7, 200, 200, 1536, MAX_SIM), (7, 200, 200, MAX_ROWS, 131072), (1, 8192, 8192, MAX_ROWS, MAX_SIM),
    (4950, 2048, 2048, MAX_ROWS, MAX_SIM), (1000, 1, 8192, MAX_ROWS, MAX_SIM), (33, 129, 127, 384, MAX_SIM), (5, 0, 300, 384, MAX_SIM), (12, 0, 0, 1, 1),
    (100, 1024, 1024, 2048, MAX_SIM), (101, 300, 77, 5000, 400000)])
def test_plan_covers_the_list_within_the_limits_in_the_fewest_even_chunks(P, n0, n1, max_rows, max_sim):
    plan = plan_pair_chunks(P, n0, n1, max_rows, max_sim)
    assert plan[0][0] == 0 and plan[-1][1] == P and all(a[1] == b[0] for a, b in zip(plan, plan[1:]))       # covers range(P) in order
    sizes = [stop - start for start, stop in plan]
    assert min(sizes) >= 1 and all(_fits(s, n0, n1, max_rows, max_sim) for s in sizes)                       # every chunk satisfies both limits
    assert max(sizes) - min(sizes) <= 1 and sizes == sorted(sizes, reverse=True)                              # even, larger chunks first
    largest = max(k for k in range(1, P + 1) if _fits(k, n0, n1, max_rows, max_sim))                          # pairs one call can take
    assert len(plan) == -(-P // largest)                                                                     # no plan has fewer chunks


def test_plan_examples():
    sizes = lambda plan: [stop - start for start, stop in plan]
    assert sizes(plan_pair_chunks(256, 4096, 4096, MAX_ROWS, MAX_SIM)) == [86, 85, 85]     # 127 pairs is the similarity limit, 256 the row limit
    assert sizes(plan_pair_chunks(256, 4096, 4096)) == [86, 85, 85]                        # the defaults are the header's limits
    assert plan_pair_chunks(7, 200, 200, max_rows=1536) == [(0, 3), (3, 5), (5, 7)]
    assert sizes(plan_pair_chunks(7, 200, 200, max_sim_elems=131072)) == [2, 2, 2, 1]
    assert plan_pair_chunks(0, 200, 200) == []
    assert plan_pair_chunks(32, 1024, 1024) == [(0, 32)]
    with pytest.raises(AssertionError, match="LG_MAX_KEYPOINTS"):
        plan_pair_chunks(3, 8193, 100)
    with pytest.raises(AssertionError, match="LG_MAX_KEYPOINTS"):
        plan_pair_chunks(3, 100, 8193)
    with pytest.raises(ValueError, match="max_rows"):
        plan_pair_chunks(3, 200, 200, max_rows=500)                                        # not even one pair fits the lowered limit


def test_constants_of_the_indexed_call_equal_the_header():
    define = lambda name: re.search(r"#define %s (\d+)" % name, HEADER).group(1)
    assert int(define("LG_FLAG_INDEXED")) == _cabi.LG_FLAG_INDEXED == 8
    assert int(define("LG_ERR_INDEX")) == _cabi.LG_ERR_INDEX == 6
    assert (int(define("LG_MAX_KEYPOINTS")), int(define("LG_MAX_ROWS")), int(define("LG_MAX_SIM_ELEMS"))) == \
        (_cabi.LG_MAX_KEYPOINTS, _cabi.LG_MAX_ROWS, _cabi.LG_MAX_SIM_ELEMS)
    names = [f[0] for f in _cabi.LgForwardIO._fields_]
    assert names[-5:] == ["status", "index0", "index1", "images0", "images1"]              # appended behind `status`: older callers' structs stay valid


def _store(K=3, N=8, dim=256):
    g = torch.Generator().manual_seed(0)
    return {"keypoints": torch.rand(K, N, 2, generator=g), "descriptors": torch.rand(K, N, dim, generator=g), "keypoint_scores": torch.rand(K, N, generator=g)}


@pytest.mark.parametrize("pairs", [[[0, 1, 2]], [0, 1], torch.zeros(2, 2, 2, dtype=torch.int64), [[0.0, 1.0]], torch.tensor([[0, 1]], dtype=torch.float64),
                                   torch.tensor([[True, False]]), [[0, 3]], [[3, 0]], [[0, 1], [-1, 2]], torch.tensor([[1, 1], [2, -1]], dtype=torch.int32)])
def test_malformed_pairs_raise_before_the_device_check(pairs):
    """Wrong shape, non-integer dtype, index K, index -1: ValueError — on CPU stores, i.e. before the 'no CPU fallback' check and so before any launch."""
    with pytest.raises(ValueError, match="pairs"):
        LightGlue(features=None).match_pairs(_store(), pairs)


def test_range_is_checked_per_store():
    small = _store(K=2)
    model = LightGlue(features=None)
    with pytest.raises(ValueError, match=r"pairs \[1\]"):
        model.match_pairs(_store(K=3), [[2, 1], [2, 2]], small)                            # side 1 indexes the second store: 2 images
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.match_pairs(_store(K=3), [[2, 1]], small)


def test_valid_pairs_on_cpu_stores_hit_the_no_fallback_rule():
    model = LightGlue(features=None)
    for pairs in ([[0, 1], [2, 2]], torch.tensor([[0, 1]]), [], torch.zeros(0, 2, dtype=torch.int64)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            model.match_pairs(_store(), pairs)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.match_pairs(_store(), [[0, 7]], validate=False)                              # unchecked on the host; still no CPU path


def test_per_call_limits_above_the_envelope_are_refused():
    model = LightGlue(features=None)
    assert model.max_rows_per_call is None and model.max_sim_elems_per_call is None and model.last_pair_chunks is None
    for name, top in (("max_rows_per_call", MAX_ROWS), ("max_sim_elems_per_call", MAX_SIM)):
        for bad in (top + 1, 0, -5):
            setattr(model, name, bad)
            with pytest.raises(ValueError, match=name):
                model.match_pairs(_store(), [[0, 1]])
        setattr(model, name, top)                                                          # the header's own value is the default
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            model.match_pairs(_store(), [[0, 1]])


def test_glue_match_pairs_collates_once_and_trims_per_pair():
    """glue.match_pairs with a stub matcher: a list of per-image dicts becomes ONE store, and every pair's result is cut to its two images' keypoint counts."""
    from lightglue_amd import match_pairs
    g = torch.Generator().manual_seed(1)
    feats = [{"keypoints": torch.rand(n, 2, generator=g), "descriptors": torch.rand(n, 256, generator=g)} for n in (5, 9, 0)]
    seen = []

    class Stub:
        def match_pairs(self, store0, pairs, store1=None):
            seen.append((store0, store1))
            P, N = len(pairs), store0["keypoints"].shape[1]
            row = torch.arange(N).repeat(P, 1)
            return {"matches0": row, "matches1": row + 100, "matching_scores0": row.float(), "matching_scores1": row.float(), "prune0": row, "prune1": row,
                    "matches": [torch.zeros(b, 2, dtype=torch.long) for b in range(P)], "scores": [torch.zeros(b) for b in range(P)],
                    "stop": torch.arange(P) + 1 if P > 1 else 4}

    out = match_pairs(Stub(), feats, [(0, 1), (1, 2), (1, 1)])
    assert len(seen) == 1 and seen[0][1] is None and seen[0][0]["keypoints"].shape == (3, 9, 2) and seen[0][0]["num_keypoints"].tolist() == [5, 9, 0]
    assert [(len(r["matches0"]), len(r["matches1"]), len(r["prune0"]), len(r["matching_scores1"])) for r in out] == [(5, 9, 5, 9), (9, 0, 9, 0), (9, 9, 9, 9)]
    assert [r["stop"] for r in out] == [1, 2, 3] and out[2]["matches"].shape == (2, 2) and out[0]["matches1"][0] == 100
    one = match_pairs(Stub(), seen[0][0], [(2, 0)])                                        # a store passes through as it is; B = 1: `stop` is an int
    assert seen[1][0] is seen[0][0] and one[0]["stop"] == 4 and len(one[0]["matches0"]) == 0 and len(one[0]["matches1"]) == 5
