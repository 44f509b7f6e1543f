"""GPU tests of float16 descriptors (include/lightglue_amd.h LG_FLAG_DESC0_F16 / LG_FLAG_DESC1_F16, LG_EXTRACT_DESC_F16 of lg_sp_sample_descriptors / lg_aliked_describe).

The engine reads a float16 descriptor tensor in place and widens every value exactly where the descriptors enter it, so every comparison here is bit for bit:
outputs on `d16` against outputs on `d16.float()`, and an extractor's float16 descriptors against `.half()` of its fp32 ones.  Shapes, stores and pair lists are
those of tests/test_gpu_match_pairs.py (N = 200: caps of 256, counts 200 / 131 / 64 / 1 / 0, NaN in every padding row — of the float16 tensors too); a few live
values are replaced by the float16 values a wrong widening would lose: subnormals, both zeros, and 65504 in a row of its own."""
import pytest
import torch

import gpu_util
from conftest import require_gpu
from lightglue_amd import _cabi
from lightglue_amd._call import normalise_side
from lightglue_amd import synthetic as synth
from test_gpu_match_pairs import ADAPTIVE, COUNTS, FIXED, PAIRS, _assert_same_dict, _stacked, _store

pytestmark = pytest.mark.gpu


def _model(dim=256, scale_ori=False, adaptive=False, precision="f16x3"):
    sd = synth.make_state_dict(0, input_dim=dim, add_scale_ori=scale_ori, recipe="C" if adaptive else "A")
    model = gpu_util.make_model(sd, precision, input_dim=dim, add_scale_ori=scale_ori, **(ADAPTIVE if adaptive else FIXED))
    model.check_finite = False   # the planted 65504 sits ON the edge of the guard's range; the guard has its own test below
    return model


def _halves(store, big=2, poisoned=True):
    """(store with float16 descriptors, the same store with those descriptors widened to fp32).  Special values go into live rows: subnormals and zeros into
    image 0, and 65504 into a row of its own of image `big` — a keypoint that far out drowns the attention of its image, so it stays out of the two largest
    images, whose pairs show that the comparison is not one of empty results."""
    d = store["descriptors"].clone()
    d[0, 3, 5], d[0, 3, 6], d[0, 3, 7] = 3e-6, -3e-6, 6e-8          # float16 subnormals (|x| < 6.1e-5), the last one the smallest (2^-24)
    d[0, 4, 0], d[0, 4, 1] = 0.0, -0.0
    assert int(store["num_keypoints"][big]) > 7
    d[big, 7] = 0.0
    d[big, 7, 9] = 65504.0                                            # the largest finite float16
    d16 = d.half()
    sub = d16[0, 3, 5:8].float()
    assert (sub != 0).all() and (sub.abs() < 6.1e-5).all() and float(d16[big, 7, 9]) == 65504.0
    assert not poisoned or torch.isnan(d16[1, int(store["num_keypoints"][1]):]).all(), "the padding rows of the float16 tensor hold NaN too"
    return {**store, "descriptors": d16}, {**store, "descriptors": d16.float()}


def _not_all_unmatched(out, pairs=2):
    assert (out["matches0"][:pairs] > -1).any(1).all(), "the pairs of the two largest images must produce matches"


I0, I1 = [0, 1, 2, 3, 4, 0], [1, 0, 4, 2, 3, 0]    # a ragged batch of six pairs out of the store's images, the empty image and the one-keypoint image included


@pytest.mark.parametrize("adaptive", [False, True])
@pytest.mark.parametrize("dim,scale_ori", [(256, False), (128, False), (128, True)])
def test_forward_bitwise(dim, scale_ori, adaptive):
    """forward on float16 descriptors == forward on the same values as fp32: the fused first projection (256-d) and the staged preparation kernel (128-d)."""
    require_gpu()
    model = _model(dim, scale_ori, adaptive)
    h, w = _halves(_store(3, COUNTS, 200, dim, scale_ori))
    got = model({"image0": _stacked(h, I0), "image1": _stacked(h, I1)})
    want = model({"image0": _stacked(w, I0), "image1": _stacked(w, I1)})
    _assert_same_dict(got, want, (dim, scale_ori, adaptive))
    _not_all_unmatched(got)
    mixed = model({"image0": _stacked(h, I0), "image1": _stacked(w, I1)})     # one side only
    _assert_same_dict(mixed, want, "image0 float16, image1 fp32")


@pytest.mark.parametrize("precision", ["f16x3", "fp32", "f16x3/fp16"])
def test_forward_bitwise_every_precision(precision):
    """The three instantiations of the first projection's load: 8 halves per 16-byte load (16-bit operands, split or single plane), 4 per 8-byte load (fp32)."""
    require_gpu()
    model = _model(precision=precision)
    h, w = _halves(_store(3, COUNTS, 200))
    got = model({"image0": _stacked(h, I0), "image1": _stacked(h, I1)})
    _assert_same_dict(got, model({"image0": _stacked(w, I0), "image1": _stacked(w, I1)}), precision)
    _not_all_unmatched(got)


def test_debug_tap_sees_the_widened_descriptors():
    """A debug stop takes the staged preparation kernel also at 256-d: the residual stream behind it holds exactly the widened values."""
    require_gpu()
    model = _model()
    h, w = _halves(_store(3, COUNTS, 200))
    data = lambda s: {"image0": _stacked(s, I0), "image1": _stacked(s, I1)}
    model.debug_stop_after(0)
    model(data(h)); x16 = model.debug_read("X").reshape(-1, 256)
    c0, c1 = model.debug_caps()
    model(data(w)); x32 = model.debug_read("X").reshape(-1, 256)
    model.debug_stop_after(-1)
    for b, (i, j) in enumerate(zip(I0, I1)):
        for image, src in ((0, i), (1, j)):
            base, n = b * (c0 + c1) + image * c0, COUNTS[src]
            want = w["descriptors"][src, :n].cpu().numpy()
            assert (x16[base:base + n].view("u4") == want.view("u4")).all() and (x32[base:base + n].view("u4") == want.view("u4")).all(), (b, image)


@pytest.mark.parametrize("adaptive", [False, True])
@pytest.mark.parametrize("dim,scale_ori", [(256, False), (128, True)])
def test_match_pairs_bitwise(dim, scale_ori, adaptive):
    require_gpu()
    model = _model(dim, scale_ori, adaptive)
    h, w = _halves(_store(3, COUNTS, 200, dim, scale_ori))
    want = model.match_pairs(w, PAIRS)
    got = model.match_pairs(h, PAIRS)
    _assert_same_dict(got, want, (dim, scale_ori, adaptive))
    _not_all_unmatched(got)


def test_match_pairs_two_stores_one_of_them_float16():
    require_gpu()
    model = _model()
    h0, w0 = _halves(_store(3, COUNTS, 200))
    h1, w1 = _halves(_store(4, [136, 70, 0], 136), big=1)
    pairs = [(0, 0), (1, 1), (4, 0), (0, 2), (3, 1), (2, 0), (1, 0), (0, 0)]
    want = model.match_pairs(w0, pairs, w1)
    _not_all_unmatched(want, 1)
    _assert_same_dict(model.match_pairs(h0, pairs, w1), want, "float16 x fp32")
    _assert_same_dict(model.match_pairs(w0, pairs, h1), want, "fp32 x float16")
    _assert_same_dict(model.match_pairs(h0, pairs, h1), want, "float16 x float16")


def test_store_is_read_in_place():
    require_gpu()
    model = _model()
    h, w = _halves(_store(3, COUNTS, 200))
    st = normalise_side(h, h["descriptors"].device, 256, False)
    assert st.desc.dtype is torch.float16 and st.desc.data_ptr() == h["descriptors"].data_ptr() and st.desc_f16
    st = normalise_side(w, w["descriptors"].device, 256, False)
    assert st.desc.dtype is torch.float32 and st.desc.data_ptr() == w["descriptors"].data_ptr() and not st.desc_f16


def _kernels_of(call):
    from torch.profiler import ProfilerActivity, profile
    call(); torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        call(); torch.cuda.synchronize()
    kernels = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "Memcpy" not in e.name and "Memset" not in e.name]
    foreign = [k for k in kernels if any(tag in k for tag in ("at::", "at_cuda", "c10::", "rocprim", "hipcub", "elementwise", "Elementwise"))]
    ours = [k for k in kernels if "lg::" in k or "anonymous namespace" in k]
    return ours, foreign


def test_no_framework_kernel_inside_match_pairs_on_a_float16_store():
    """As tests/test_gpu_round5.py::test_no_framework_kernels_between_engine_launches: the profiler sees memcpy / memset activity and kernels of namespace lg only —
    the store is not converted.  A dense store (no num_keypoints to clamp) and one pair given as a device int32 tensor (no [2, P] transposition) leave the call
    without any kernel of the framework's; on the ragged store and the whole list the float16 store launches exactly what the fp32 store launches."""
    require_gpu()
    model = _model()
    dense = _store(3, [200] * 5, 200, poison=False)
    h, _ = _halves(dense, poisoned=False)
    del h["num_keypoints"]
    one = torch.tensor([PAIRS[1]], device="cuda", dtype=torch.int32)
    ours, foreign = _kernels_of(lambda: model.match_pairs(h, one))
    assert len(ours) >= 20 and not foreign, f"framework kernels inside match_pairs: {sorted(set(foreign))}"
    h, w = _halves(_store(3, COUNTS, 200))
    pairs = torch.tensor(PAIRS, device="cuda", dtype=torch.int32)
    ours16, foreign16 = _kernels_of(lambda: model.match_pairs(h, pairs))
    ours32, foreign32 = _kernels_of(lambda: model.match_pairs(w, pairs))
    assert sorted(foreign16) == sorted(foreign32) and len(ours16) == len(ours32), (foreign16, foreign32)


def test_chunked_equals_one_call():
    require_gpu()
    model = _model()
    h, _ = _halves(_store(5, [200, 131, 64, 1, 0, 177], 200))
    pairs = [(0, 1), (1, 5), (4, 2), (5, 0), (2, 2), (3, 1), (5, 1)]
    whole = model.match_pairs(h, pairs)
    assert model.last_pair_chunks == [(0, 7)]
    model.max_rows_per_call = 1536
    _assert_same_dict(model.match_pairs(h, pairs), whole)
    assert model.last_pair_chunks == [(0, 3), (3, 5), (5, 7)]


def test_views():
    """A contiguous view offset by whole rows is read where it lies; a non-contiguous one goes through ONE float16 copy."""
    require_gpu()
    model = _model()
    h, w = _halves(_store(3, COUNTS, 200))
    pairs = [(0, 0), (0, 1), (2, 3), (3, 0), (1, 1)]
    vh, vw = {k: v[1:] for k, v in h.items()}, {k: v[1:] for k, v in w.items()}
    assert vh["descriptors"].is_contiguous() and vh["descriptors"].data_ptr() == h["descriptors"].data_ptr() + 200 * 256 * 2
    assert normalise_side(vh, vh["keypoints"].device, 256, False).desc.data_ptr() == vh["descriptors"].data_ptr()
    want = model.match_pairs(vw, pairs)
    got = model.match_pairs(vh, pairs)
    _assert_same_dict(got, want, "view [1:]")
    assert (got["matches0"][0] > -1).any()
    nc = vh["descriptors"].transpose(1, 2).contiguous().transpose(1, 2)
    assert not nc.is_contiguous() and torch.equal(nc[0, :131], vh["descriptors"][0, :131])
    st = normalise_side({**vh, "descriptors": nc}, nc.device, 256, False)
    assert st.desc.dtype is torch.float16 and st.desc.is_contiguous() and st.desc_f16
    _assert_same_dict(model.match_pairs({**vh, "descriptors": nc}, pairs), want, "non-contiguous")
    data = {"image0": {**_stacked(vh, [0, 2]), "descriptors": nc[[0, 2]].transpose(1, 2).contiguous().transpose(1, 2)}, "image1": _stacked(vh, [1, 3])}
    assert not data["image0"]["descriptors"].is_contiguous()
    _assert_same_dict(model(data), model({"image0": _stacked(vw, [0, 2]), "image1": _stacked(vw, [1, 3])}), "forward, non-contiguous")


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_range_guard_reads_float16(bad):
    """LG_FLAG_CHECK_FINITE on float16 input: an inf / a NaN in one live row of pair 1 is that pair's LG_ERR_RANGE; in range, the guard changes no output bit."""
    require_gpu()
    from test_gpu_round5 import _forward_with_guard
    model, td = _forward_with_guard(1.0)
    for side in ("image0", "image1"):
        td[side]["descriptors"] = td[side]["descriptors"].half()
    a = model(td)
    model.check_finite = False
    _assert_same_dict(model(td), a, "guard on / off")
    assert (a["matches0"] > -1).any(1).all()
    model.check_finite = True
    td["image0"]["descriptors"][1, 5, 7] = bad
    raw = model.forward_raw(td)
    torch.cuda.synchronize()
    assert raw["status"].cpu().tolist() == [_cabi.LG_OK, _cabi.LG_ERR_RANGE]
    with pytest.raises(_cabi.LightGlueAmdError, match="pair 1"):
        model(td)


def _same_but_descriptors(f16, f32):
    assert f16["descriptors"].dtype is torch.float16 and f32["descriptors"].dtype is torch.float32
    assert torch.equal(f16["descriptors"], f32["descriptors"].half())
    assert f16["num_keypoints"].dtype == f32["num_keypoints"].dtype and torch.equal(f16["num_keypoints"], f32["num_keypoints"])
    counts = f16["num_keypoints"].tolist()
    for b, c in enumerate(counts):
        for k in ("keypoints", "keypoint_scores"):     # live rows: what lies behind an image's count comes from uninitialised memory in either run
            assert f16[k].dtype == f32[k].dtype and f16[k].shape == f32[k].shape and torch.equal(f16[k][b, :c], f32[k][b, :c]), (k, b)
        assert c > 0 and f16["descriptors"][b, :c].float().norm(dim=-1).sub(1).abs().max() < 2e-3      # unit rows, rounded
        assert not f16["descriptors"][b, c:].any(), "padding rows are zero"
    return counts


def _superpoint_case(ragged):
    import make_golden_superpoint as G
    from lightglue_amd import SuperPoint
    sd, img = G.encoder_state_dict(0), torch.from_numpy(G.encoder_image(10, 2, 64, 96)).cuda()
    conf = dict(max_num_keypoints=50)
    if ragged:    # threshold mode, the threshold at the 90th percentile of the batch's score map: the two images keep different numbers of detections
        scores, _ = SuperPoint(weights=sd).cuda().eval().encode(img)
        conf = dict(max_num_keypoints=None, detection_threshold=float(scores.flatten().quantile(0.9)))
    make = lambda **kw: SuperPoint(weights=sd, **conf, **kw).cuda().eval()
    return make, img


@pytest.mark.parametrize("ragged", [False, True])
def test_superpoint_writes_float16_descriptors(ragged):
    require_gpu()
    make, img = _superpoint_case(ragged)
    f32, f16 = make()({"image": img}), make(descriptor_dtype=torch.float16)({"image": img})
    counts = _same_but_descriptors(f16, f32)
    assert counts[0] != counts[1] or not ragged, counts


def _aliked_case(model_name, ragged):
    import make_golden_aliked as G
    from lightglue_amd import ALIKED
    sd = G.aliked_state_dict(1, model_name)
    img = torch.cat([G.aliked_image(s, 1, 64, 96, 3) for s in (3, 4)], 0).cuda()
    conf = dict(detection_threshold=0.2, max_num_keypoints=-1) if ragged else dict(detection_threshold=-1, max_num_keypoints=50)
    return (lambda **kw: ALIKED(weights=sd, model_name=model_name, **conf, **kw).eval().cuda()), img


@pytest.mark.parametrize("model_name,ragged", [("aliked-n16", False), ("aliked-n16", True), ("aliked-n32", False)])
def test_aliked_writes_float16_descriptors(model_name, ragged):
    require_gpu()
    make, img = _aliked_case(model_name, ragged)
    f32, f16 = make()({"image": img}), make(descriptor_dtype=torch.float16)({"image": img})
    counts = _same_but_descriptors(f16, f32)
    assert counts[0] != counts[1] or not ragged, counts
    ext = make()
    scores, levels = ext.encode(img)
    _, _, knorm, cnt = ext.detect(scores)
    knorm = knorm[:, :int(cnt.max())].contiguous()
    assert torch.equal(ext.describe(levels, (2, 64, 96), knorm, cnt, dtype=torch.float16), ext.describe(levels, (2, 64, 96), knorm, cnt).half())


def test_extractor_to_matcher_end_to_end():
    """match_pairs over an extractor's float16 store == match_pairs over `.half().float()` of its fp32 store; extract() passes the dtype through."""
    require_gpu()
    make, img = _superpoint_case(False)
    f32, f16 = make()({"image": img}), make(descriptor_dtype=torch.float16)({"image": img})
    model = _model()
    pairs = [(0, 1), (1, 0), (0, 0)]
    got = model.match_pairs(f16, pairs)
    _assert_same_dict(got, model.match_pairs({**f32, "descriptors": f32["descriptors"].half().float()}, pairs))
    assert (got["matches0"][2] > -1).any(), "an image matches itself"
    one, ref = make(descriptor_dtype=torch.float16).extract(img[0]), make().extract(img[0])
    assert one["descriptors"].dtype is torch.float16 and torch.equal(one["descriptors"], ref["descriptors"].half()) and torch.equal(one["keypoints"], ref["keypoints"])
