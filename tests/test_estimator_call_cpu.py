"""The four steps `_call` writes once for the geometry estimators over a match list (TwoViewVerifier, RelativePoseEstimator, AbsolutePoseEstimator; the
Triangulator reads matches0 through the same one): the constructor check, the matches0 coercion, the ragged `matches` lists and the error that carries the
call's outputs.  Plain tensor code on CPU tensors: no GPU."""
import pytest
import torch

from lightglue_amd import AbsolutePoseEstimator, RelativePoseEstimator, TwoViewVerifier, _cabi, _call

CPU = torch.device("cpu")


def test_settings_are_returned_as_float_int_int():
    got = _call.ransac_settings("2.5", 512.0, True)
    assert got == (2.5, 512, 1) and [type(v) for v in got] == [float, int, int]
    assert _call.ransac_settings(1e-30, 65536, 2 ** 32 - 1) == (1e-30, 65536, 2 ** 32 - 1)


@pytest.mark.parametrize("kwargs, text", [
    (dict(threshold=0.0), "threshold must be > 0, got 0.0"),
    (dict(threshold=float("nan")), "threshold must be > 0, got nan"),
    (dict(threshold=-1), "threshold must be > 0, got -1"),
    (dict(num_hypotheses=0), "num_hypotheses must be a multiple of 256 in [256, 65536], got 0"),
    (dict(num_hypotheses=300), "num_hypotheses must be a multiple of 256 in [256, 65536], got 300"),
    (dict(num_hypotheses=65536 + 256), "num_hypotheses must be a multiple of 256 in [256, 65536], got 65792"),
    (dict(seed=-1), "seed must lie in [0, 2^32), got -1"),
    (dict(seed=2 ** 32), "seed must lie in [0, 2^32), got 4294967296"),
])
def test_the_three_refusals_of_the_settings(kwargs, text):
    settings = {"threshold": 3.0, "num_hypotheses": 1024, "seed": 0, **kwargs}
    with pytest.raises(ValueError) as err:
        _call.ransac_settings(**settings)
    assert str(err.value) == text
    for cls in (TwoViewVerifier, RelativePoseEstimator, AbsolutePoseEstimator):         # every estimator answers with the same error
        with pytest.raises(ValueError) as err:
            cls(**kwargs)
        assert str(err.value) == text, cls.__name__


def test_the_refusals_come_in_the_order_threshold_budget_seed():
    with pytest.raises(ValueError, match="threshold"):
        _call.ransac_settings(0, 1, -1)
    with pytest.raises(ValueError, match="num_hypotheses"):
        _call.ransac_settings(1, 1, -1)
    est = RelativePoseEstimator(threshold=2, num_hypotheses=256, refine=0, seed=7)
    assert (est.threshold, est.num_hypotheses, est.refine, est.seed) == (2.0, 256, False, 7)


def test_matches0_of_a_dict_a_tensor_and_a_deferred_result():
    m0 = torch.arange(6, dtype=torch.int64).reshape(2, 3)
    assert _call.as_matches0(m0, 2, 3, CPU) is m0                                     # qualifies: untouched
    assert _call.as_matches0({"matches0": m0, "matches1": None}, 2, 3, CPU) is m0

    class Done:
        waited = 0

        def synchronize(self):
            Done.waited += 1
    deferred = _call.DeferredMatches(Done(), torch.zeros(1), lambda host: {"matches0": m0})
    assert _call.as_matches0(deferred, 2, 3, CPU) is m0 and Done.waited == 1
    assert _call.as_matches0(deferred, 2, 3, CPU) is m0 and Done.waited == 1          # the handle keeps its result


def test_matches0_is_coerced_to_contiguous_int64():
    m0 = torch.tensor([[2, -1, 0], [1, 1, -1]], dtype=torch.int32)
    got = _call.as_matches0(m0, 2, 3, CPU)
    assert got.dtype is torch.int64 and got.is_contiguous() and got.tolist() == m0.tolist() and got.data_ptr() != m0.data_ptr()
    wide = torch.arange(12, dtype=torch.int64).reshape(2, 6)[:, ::2]                  # the right dtype, not contiguous
    got = _call.as_matches0(wide, 2, 3, CPU)
    assert got.is_contiguous() and got.tolist() == [[0, 2, 4], [6, 8, 10]]
    meta = _call.as_matches0(torch.zeros(2, 3, dtype=torch.int64), 2, 3, torch.device("meta"))      # another device: moved there
    assert meta.device.type == "meta" and meta.dtype is torch.int64 and tuple(meta.shape) == (2, 3)
    with pytest.raises(AssertionError) as err:
        _call.as_matches0(torch.zeros(2, 4, dtype=torch.int64), 2, 3, CPU)
    assert str(err.value) == "matches0 must have shape [2, 3], got (2, 4)"
    with pytest.raises(AssertionError, match=r"matches0 must have shape \[3, 3\], got \(2, 3\)"):
        _call.as_matches0({"matches0": m0}, 3, 3, CPU)


def test_ragged_matches_of_a_mask_with_an_empty_and_a_full_row():
    mask = torch.tensor([[0, 1, 0, 1, 1], [0, 0, 0, 0, 0], [1, 1, 1, 1, 1]], dtype=torch.bool)
    verified = torch.tensor([[-1, 7, -1, 0, 3], [-1, -1, -1, -1, -1], [4, 3, 2, 1, 0]])
    before = (mask.clone(), verified.clone())
    got = _call.ragged_matches(mask, verified, [3, 0, 5])
    assert [g.tolist() for g in got] == [[[1, 7], [3, 0], [4, 3]], [], [[0, 4], [1, 3], [2, 2], [3, 1], [4, 0]]]
    assert [tuple(g.shape) for g in got] == [(3, 2), (0, 2), (5, 2)] and all(g.dtype is torch.int64 for g in got)
    assert torch.equal(mask, before[0]) and torch.equal(verified, before[1])
    assert _call.ragged_matches(mask[:0], verified[:0], []) == []


def test_the_raised_error_carries_the_outputs():
    out = {"models": torch.zeros(2, 3, 3), "num_inliers": torch.tensor([5, 0])}
    assert _call.raise_with_outputs([_cabi.LG_OK, _cabi.LG_OK], out) is out
    with pytest.raises(_cabi.LightGlueAmdError) as err:
        _call.raise_with_outputs([_cabi.LG_OK, _cabi.LG_ERR_INDEX, _cabi.LG_ERR_CAMERA], out)
    assert err.value.outputs is out
    with pytest.raises(_cabi.LightGlueAmdError) as plain:
        _call.raise_on_status([_cabi.LG_OK, _cabi.LG_ERR_INDEX, _cabi.LG_ERR_CAMERA])
    assert str(err.value) == str(plain.value) and str(err.value).startswith("pair 1: an image index outside its feature store (LG_ERR_INDEX)")
    assert "pair 2: a camera whose focal length" in str(err.value) and not hasattr(plain.value, "outputs")
