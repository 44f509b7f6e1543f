"""Host side of the matcher's one call path (no GPU): the side normaliser on CPU tensors (plain tensor code), the checks `forward` and `match_pairs` share
and their order, the carve plan of the output allocations, and the sharded forward as a statement of its own."""
import ast
from pathlib import Path

import pytest
import torch

from lightglue_amd import LightGlue, NearestNeighborMatcher, TwoViewVerifier, _call
from lightglue_amd._call import carve_plan, normalise_side

CPU = torch.device("cpu")
K, N = 3, 8


def _side(dim=256, scale_ori=False, **over):
    g = torch.Generator().manual_seed(0)
    d = {"keypoints": torch.rand(K, N, 2, generator=g), "descriptors": torch.rand(K, N, dim, generator=g)}
    if scale_ori:
        d["scales"], d["oris"] = torch.rand(K, N, generator=g), torch.rand(K, N, generator=g)
    d.update(over)
    return {k: v for k, v in d.items() if v is not None}


def test_qualifying_tensors_pass_through_untouched():
    d = _side(dim=128, scale_ori=True, image_size=torch.rand(K, 2))
    s = normalise_side(d, CPU, 128, True)
    assert (s.K, s.N, s.desc_f16, s.num) == (K, N, False, None)
    for got, key in ((s.kpts, "keypoints"), (s.desc, "descriptors"), (s.scales, "scales"), (s.oris, "oris")):
        assert got is d[key] and got.data_ptr() == d[key].data_ptr(), key
    assert s.size.data_ptr() == d["image_size"].data_ptr() and s.size.shape == (K, 2)     # a [-1, 2] view of the same memory
    plain = normalise_side(_side(), CPU, 256, False)
    assert plain.size is None and plain.scales is None and plain.oris is None           # scales / oris are read iff add_scale_ori
    half = normalise_side(_side(descriptors=torch.rand(K, N, 256).half()), CPU, 256, False)
    assert half.desc.dtype is torch.float16 and half.desc_f16
    f64 = normalise_side(_side(keypoints=torch.rand(K, N, 2, dtype=torch.float64)), CPU, 256, False)
    assert f64.kpts.dtype is torch.float32 and f64.kpts.is_contiguous()


@pytest.mark.parametrize("given", [torch.tensor([640.0, 480.0]), torch.tensor([[640.0, 480.0]]), torch.tensor([[640.0, 480.0]] * K), [640, 480]])
def test_image_size_is_broadcast_over_the_images(given):
    s = normalise_side(_side(image_size=given), CPU, 256, False)
    assert s.size.shape == (K, 2) and s.size.dtype is torch.float32 and s.size.is_contiguous() and s.size.tolist() == [[640.0, 480.0]] * K


def test_num_keypoints_is_clamped_into_the_rows():
    s = normalise_side(_side(num_keypoints=torch.tensor([-2, 5, N + 7])), CPU, 256, False)
    assert s.num.dtype is torch.int32 and s.num.tolist() == [0, 5, N]
    assert normalise_side(_side(num_keypoints=[1, 2, 3]), CPU, 256, False).num.tolist() == [1, 2, 3]


MALFORMED = [                                   # (dim, add_scale_ori, what is wrong, exception, the key its message names)
    (256, False, dict(image_size=torch.rand(2, 2)), AssertionError, "image_size"),
    (256, False, dict(num_keypoints=torch.tensor([1, 2])), AssertionError, "num_keypoints"),
    (256, False, dict(num_keypoints=torch.tensor([[1, 2, 3]])), AssertionError, "num_keypoints"),
    (256, False, dict(descriptors=torch.rand(K, N, 128)), AssertionError, "descriptors"),
    (256, False, dict(descriptors=torch.rand(K, N + 1, 256)), AssertionError, "descriptors"),
    (256, False, dict(descriptors=torch.rand(K * N, 256)), AssertionError, "descriptors"),
    (256, False, dict(keypoints=torch.rand(K, N, 3)), AssertionError, "keypoints"),
    (256, False, dict(keypoints=torch.rand(N, 2)), AssertionError, "keypoints"),
    (128, True, dict(scales=torch.rand(K, N + 1)), AssertionError, "scales"),
    (128, True, dict(oris=torch.rand(K, N, 1)), AssertionError, "oris"),
    (128, True, dict(scales=torch.rand(K * N)), AssertionError, "scales"),
    (128, True, dict(scales=None), KeyError, "scales"),
]


@pytest.mark.parametrize("dim,scale_ori,wrong,exc,key", MALFORMED)
def test_malformed_side_is_refused(dim, scale_ori, wrong, exc, key):
    with pytest.raises(exc, match=key):
        normalise_side(_side(dim, scale_ori, **wrong), CPU, dim, scale_ori)


def test_float16_on_one_side_sets_that_sides_flag_only():
    model = LightGlue(features=None)
    h, w = _side(descriptors=torch.rand(K, N, 256).half()), _side()
    for f0, f1, want in ((h, w, (True, False)), (w, h, (False, True)), (h, h, (True, True)), (w, w, (False, False))):
        s0, s1 = (normalise_side(f, CPU, model.conf.input_dim, model.conf.add_scale_ori) for f in (f0, f1))
        assert (s0.desc_f16, s1.desc_f16) == want


class _Reached(Exception):
    """the call got as far as the launch path"""


@pytest.fixture
def past_the_device_check(monkeypatch):
    """CPU tensors reach the side normaliser through the public methods: the device check passes, and the launch path (which needs the engine) ends the call."""
    def launch(self, *a, **k):
        raise _Reached
    monkeypatch.setattr(_call, "require_gpu", lambda device, what="keypoints": None)
    for cls in (LightGlue, NearestNeighborMatcher, TwoViewVerifier):
        monkeypatch.setattr(cls, "_launch", launch)


@pytest.mark.parametrize("dim,scale_ori,wrong,exc,key", MALFORMED)
@pytest.mark.parametrize("side", [0, 1])
def test_forward_and_match_pairs_refuse_the_same_side(past_the_device_check, dim, scale_ori, wrong, exc, key, side):
    model = LightGlue(features=None, input_dim=dim, add_scale_ori=scale_ori)
    feats = [_side(dim, scale_ori), _side(dim, scale_ori)]
    with pytest.raises(_Reached):                                                       # both routes take the well-formed sides
        model({"image0": feats[0], "image1": feats[1]})
    with pytest.raises(_Reached):
        model.match_pairs(feats[0], [(0, 1)], feats[1])
    feats[side] = _side(dim, scale_ori, **wrong)
    for call in (lambda: model({"image0": feats[0], "image1": feats[1]}), lambda: model.forward_raw({"image0": feats[0], "image1": feats[1]}),
                 lambda: model.forward_deferred({"image0": feats[0], "image1": feats[1]}), lambda: model.match_pairs(feats[0], [(0, 0)], feats[1], validate=False)):
        with pytest.raises(exc, match=key):
            call()


OTHERS_MALFORMED = [                            # (class, what is wrong with something the class reads, the key the message names)
    (NearestNeighborMatcher, dict(descriptors=torch.rand(K * N, 256)), "descriptors"),
    (NearestNeighborMatcher, dict(num_keypoints=torch.tensor([1, 2])), "num_keypoints"),
    (NearestNeighborMatcher, dict(num_keypoints=torch.tensor([[1, 2, 3]])), "num_keypoints"),
    (NearestNeighborMatcher, dict(descriptor_transform="hellinger"), "descriptor_transform"),
    (TwoViewVerifier, dict(keypoints=torch.rand(K, N, 3)), "keypoints"),
    (TwoViewVerifier, dict(keypoints=torch.rand(N, 2)), "keypoints"),
    (TwoViewVerifier, dict(num_keypoints=torch.tensor([1, 2])), "num_keypoints"),
    (TwoViewVerifier, dict(num_keypoints=torch.tensor([[1, 2, 3]])), "num_keypoints"),
]


@pytest.mark.parametrize("cls,wrong,key", OTHERS_MALFORMED)
@pytest.mark.parametrize("side", [0, 1])
def test_nn_matcher_and_verifier_refuse_the_same_side(past_the_device_check, cls, wrong, key, side):
    """every route of the weight-free matcher and of the verifier refuses a malformed side with the exception type LightGlue raises for it, naming the same key"""
    with pytest.raises(Exception) as lightglue_says:
        LightGlue(features=None)({"image0": _side(**wrong), "image1": _side()})
    exc = type(lightglue_says.value)
    assert exc is not _Reached and key in str(lightglue_says.value)
    m, m0 = cls(), torch.full((K, N), -1)
    if cls is NearestNeighborMatcher:
        routes = lambda f: (lambda: m({"image0": f[0], "image1": f[1]}), lambda: m.match_pairs(f[0], [(0, 0)], f[1], validate=False))
    else:
        routes = lambda f: (lambda: m({"image0": f[0], "image1": f[1]}, m0), lambda: m.verify_pairs(f[0], [(0, 0)], m0[:1], f[1], validate=False),
                            lambda: m.score_models(f[0], [(0, 0)], m0[:1], torch.zeros(1, 256, 3, 3), f[1], validate=False))
    feats = [_side(), _side()]
    for call in routes(feats):                                                          # every route takes the well-formed sides
        with pytest.raises(_Reached):
            call()
    feats[side] = _side(**wrong)
    for call in routes(feats):
        with pytest.raises(exc, match=key):
            call()


def test_forward_refuses_sides_of_different_batch_size(past_the_device_check):
    model = LightGlue(features=None)
    one = {k: v[:1] for k, v in _side().items()}
    with pytest.raises(AssertionError, match="image0 and image1"):
        model({"image0": _side(), "image1": one})
    with pytest.raises(_Reached):
        model.match_pairs(_side(), [(2, 0)], one)                                       # two stores may differ in size; two sides of a batch may not


def test_order_of_checks_on_cpu_inputs():
    model = LightGlue(features=None)
    bad = _side(keypoints=torch.rand(K, N, 3))
    with pytest.raises(AssertionError, match="Missing key image1"):
        model({"image0": bad})
    for call in (model.forward, model.forward_raw, model.forward_deferred):
        with pytest.raises(RuntimeError, match="no CPU fallback"):                      # the device comes before the sides
            call({"image0": bad, "image1": bad})
    model.max_rows_per_call = 0
    with pytest.raises(ValueError, match="max_rows_per_call"):                          # the limits come before the pair list
        model.match_pairs(bad, [[0, 9]])
    model.max_rows_per_call = None
    with pytest.raises(ValueError, match="pairs"):                                      # the pair list comes before the device
        model.match_pairs(bad, [[0, 9]])
    with pytest.raises(RuntimeError, match="no CPU fallback"):                          # the device comes before the stores
        model.match_pairs(bad, [[0, 1]])


# what the class's own per-shape plan returned for these arguments before it became a function: sizes and offsets of the int32, fp32 and int64 pieces
PARENT_PLAN = {
    False: ([1000, 1000, 2000, 0, 0, 15], [0, 1000, 2000, 4000, 4000, 4000, 4016], [1000, 1000, 1000, 1000, 1000], [0, 1000, 2000, 3000, 4000, 5000],
            [1000, 1000, 2000, 5, 0, 0], [0, 1000, 2000, 4000, 4008, 4008, 4008]),
    True: ([1000, 1000, 2000, 1000, 1000, 15], [0, 1000, 2000, 4000, 5000, 6000, 6016], [1000, 1000, 1000, 0, 0], [0, 1000, 2000, 3000, 3000, 3000],
           [1000, 1000, 2000, 5, 1000, 1000], [0, 1000, 2000, 4000, 4008, 5008, 6008]),
}


@pytest.mark.parametrize("pruning", [False, True])
def test_carve_plan_is_a_pure_cached_function(pruning):
    plan = carve_plan(5, 200, 200, pruning)
    assert [list(x) for x in plan] == [list(x) for x in PARENT_PLAN[pruning]]
    assert all(off % 4 == 0 for offsets in plan[1::2] for off in offsets)
    assert carve_plan(5, 200, 200, pruning) is plan
    odd = carve_plan(3, 131, 17, pruning)                                               # sizes that are no multiple of 4: every piece still starts 16-byte aligned
    assert all(off % 4 == 0 for offsets in odd[1::2] for off in offsets) and all(b - a >= s for sz, off in zip(odd[0::2], odd[1::2]) for a, b, s in zip(off, off[1:], sz))


def test_the_sharded_forward_is_a_statement_of_its_own():
    """PairShardedMatcher.issue_local must run `forward_raw` under `python -O` too.  That route needs a GPU tensor, so this reads the source instead: no call of
    `raw(...)` in lightglue_amd/parallel.py sits inside an `assert` statement."""
    tree = ast.parse((Path(_call.__file__).parent / "parallel.py").read_text())
    is_raw_call = lambda node: isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id == "raw"
    calls = [node for node in ast.walk(tree) if is_raw_call(node)]
    asserted = [node for stmt in ast.walk(tree) if isinstance(stmt, ast.Assert) for node in ast.walk(stmt) if is_raw_call(node)]
    assert len(calls) == 1 and not asserted
