"""The forward enqueues what its plan says (lightglue_amd/csrc/lg_forward_plan.h): launch sites per kernel class of one forward, read back through the
profile brackets, against tests/golden/forward_launch_sites.json — recorded by tools/record_launch_sites.py on the library as it was before the forward
was split into plan + stages.  The host enqueues every layer whatever stops early, so the counts do not depend on the data and equality is exact.
B = 2, (n0, n1) = (129, 17), recipe A, f16x3: one forward per option set."""
import json
import sys
from pathlib import Path

import pytest

from conftest import require_gpu
from test_gpu_match_pairs import _assert_same_dict

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tools"))
import record_launch_sites as rec

pytestmark = pytest.mark.gpu

GOLDEN = json.loads(rec.GOLDEN.read_text())
# what test_fused_next_projection_is_bit_identical, test_fused_prep_is_bit_identical and test_gather_projection_equals_the_in_place_compaction compare bit for
# bit with the option off.  No test claims bit-identity of the per-op path (fused_tail = 0: other kernels, another summation order), so none is asserted here.
_BIT_IDENTICAL_OFF = ("fused_next=0", "fused_prep=0", "adapt_gather=0")
_COMPARED = ("matches0", "matches1", "matching_scores0", "matching_scores1", "prune0", "prune1", "stop")


def test_golden_covers_every_case():
    keys = {rec.case_key(m, d, o) for m in rec.MODES for d in rec.DIMS for o in rec.OPTION_SETS} | {"match_pairs/fixed/dim256/defaults"}
    assert set(GOLDEN) == keys


@pytest.mark.parametrize("dim", rec.DIMS)
@pytest.mark.parametrize("mode", list(rec.MODES))
def test_launch_sites_per_kernel_class(mode, dim):
    require_gpu()
    got = rec.forward_cases(mode, dim)
    for name, (counts, _) in got.items():
        assert counts == GOLDEN[rec.case_key(mode, dim, name)], (mode, dim, name)
    want = {k: got["defaults"][1][k] for k in _COMPARED}
    for name in _BIT_IDENTICAL_OFF:
        _assert_same_dict({k: got[name][1][k] for k in _COMPARED}, want, (mode, dim, name))
    assert (want["matches0"] > -1).any(), "the equality above must compare something"


def test_launch_sites_of_an_indexed_call():
    require_gpu()
    counts, out = rec.match_pairs_case()
    assert counts == GOLDEN["match_pairs/fixed/dim256/defaults"]
    assert out["matches0"].shape == (len(rec.PAIRS), rec.SHAPE[1])
