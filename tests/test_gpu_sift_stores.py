"""GPU tests of SIFT feature stores (include/lightglue_amd.h: LG_FLAG_DESC0_U8 / _DESC1_U8, LG_FLAG_ROOTSIFT0 / _ROOTSIFT1, lg_rootsift, lg_sift_filter).

The engine reads uint8 descriptor rows in place and widens them exactly, and applies RootSIFT from the same device code as `sift_to_rootsift`, so every engine
comparison here is bit for bit: outputs on the uint8 store against outputs on `store.float()`, and outputs with descriptor_transform = "rootsift" against outputs
on the pre-transformed fp32 rows.  `lg_rootsift` and `filter_dog_point` are held to the reference's own outputs (tests/golden/sift/sift_helpers.npz).

Stores: K images of one synthetic scene — every image a re-ordered, perturbed copy of the same uint8 descriptor rows (sparse, SIFT-like: most bins small, a few
large), so pairs do match.  n0 = 70 and n1 = 130 cross the 64- and 128-row tiles and are no multiple of the 4 rows per workgroup of the preparation kernel."""
from pathlib import Path

import numpy as np
import pytest
import torch

import gpu_util
from conftest import require_gpu
from lightglue_amd import _cabi, _call, filter_dog_point, sift_features, sift_to_rootsift
from lightglue_amd import synthetic as synth
from lightglue_amd._call import normalise_side
from test_gpu_match_pairs import ADAPTIVE, FIXED, _assert_same_dict

pytestmark = pytest.mark.gpu

GOLDEN = np.load(Path(__file__).resolve().parent / "golden" / "sift" / "sift_helpers.npz")
_PER_IMAGE = ("keypoints", "descriptors", "scales", "oris", "image_size", "num_keypoints")


def _model(dim=128, adaptive=False):
    sd = synth.make_state_dict(0, input_dim=dim, add_scale_ori=True, recipe="C" if adaptive else "A")
    model = gpu_util.make_model(sd, "f16x3", input_dim=dim, add_scale_ori=True, **(ADAPTIVE if adaptive else FIXED))
    model.check_finite = False
    return model


SCENE = 130    # keypoints of the scene every store of one seed shows


def _u8_store(seed, counts, N, dim=128):
    """K = len(counts) images of N <= SCENE rows, counts[i] of them live; the rows past an image's count hold 255 (uint8 has no NaN to poison them with).  The
    scene depends on the seed alone, so stores of different N match each other."""
    g = torch.Generator().manual_seed(seed)
    K = len(counts)
    base_k = torch.rand(SCENE, 2, generator=g) * torch.tensor([1024.0, 768.0])
    base_d = (torch.randn(SCENE, dim, generator=g).abs() ** 3 * 12.0).clamp(0, 255)
    st = {"keypoints": torch.empty(K, N, 2), "descriptors": torch.empty(K, N, dim, dtype=torch.uint8),
          "scales": 1.0 + 4.0 * torch.rand(K, N, generator=g), "oris": (torch.rand(K, N, generator=g) * 2 - 1) * 3.14159}
    for i in range(K):
        perm = torch.randperm(SCENE, generator=g)[:N]
        st["keypoints"][i] = base_k[perm] + 2.0 * torch.randn(N, 2, generator=g)
        st["descriptors"][i] = (base_d[perm] + 2.0 * torch.randn(N, dim, generator=g)).clamp(0, 255).to(torch.uint8)
        st["descriptors"][i, counts[i]:] = 255
    st["image_size"] = torch.tensor([[1024.0, 768.0]]).expand(K, 2).contiguous()
    st["num_keypoints"] = torch.tensor(counts, dtype=torch.int32)
    return {k: v.cuda() for k, v in st.items()}


def _sparse_u8_store(seed, counts, N, dim=128):
    """The same layout with rows the matcher can use WITHOUT RootSIFT: two bins of value 1 per row (norm 1.41, every scene point its own pair of bins), copied
    exactly into every image — raw 0 .. 255 rows have norms of several hundred, far from what the synthetic weights separate.  The full value range goes
    through the same load in the RootSIFT tests below and, bit for bit, in test_rootsift_kernel_against_the_reference."""
    st = _u8_store(seed, counts, N, dim)
    g = torch.Generator().manual_seed(seed + 1000)
    bins = torch.combinations(torch.arange(dim), 2)[torch.randperm(dim * (dim - 1) // 2, generator=g)[:SCENE]]
    base_d = torch.zeros(SCENE, dim, dtype=torch.uint8).scatter_(1, bins, 1)
    base_k = torch.rand(SCENE, 2, generator=g) * torch.tensor([1024.0, 768.0])
    for i in range(len(counts)):
        perm = torch.randperm(SCENE, generator=g)[:N]
        st["keypoints"][i] = (base_k[perm] + 2.0 * torch.randn(N, 2, generator=g)).cuda()
        st["descriptors"][i] = base_d[perm].cuda()
        st["descriptors"][i, counts[i]:] = 255
    return st


def _with(store, **kw):
    return {**store, **kw}


def _pair_data(n0=70, n1=130, dim=128):
    """B = 2 pairs, image0 with 70 rows (counts 70 / 61), image1 with 130 (130 / 97)."""
    a, b = _u8_store(5, [n0, n0 - 9], n0, dim), _u8_store(5, [n1, n1 - 33], n1, dim)
    return a, b


def _has_matches(out):
    assert (out["matches0"] > -1).any(1).all(), "every pair must produce matches: the equality compares something"


@pytest.mark.parametrize("dim,adaptive", [(128, False), (256, False), (128, True)])
def test_engine_reads_uint8_rows_in_place(dim, adaptive, monkeypatch):
    """Outputs on a uint8 store == outputs on store.float(), and the pointer handed to the engine is the store's own.  At input_dim = 256 the launch plan takes
    prep_kernel + proj_kernel for the flagged call and the fused first projection for the fp32 one: the two forms are bit-identical."""
    require_gpu()
    model = _model(dim, adaptive)
    a, b = _sparse_u8_store(5, [70, 61], 70, dim), _sparse_u8_store(5, [130, 97], 130, dim)
    st = normalise_side(a, a["keypoints"].device, dim, True)
    assert st.desc.dtype is torch.uint8 and st.desc.data_ptr() == a["descriptors"].data_ptr() and st.desc_u8 and not st.desc_f16 and not st.rootsift
    fa, fb = _with(a, descriptors=a["descriptors"].float()), _with(b, descriptors=b["descriptors"].float())
    want = model({"image0": fa, "image1": fb})
    print(f"uint8 rows, dim {dim}, adaptive {adaptive}: matches per pair {(want['matches0'] > -1).sum(1).tolist()}")
    _has_matches(want)
    ios, build = [], _call.Outputs.io          # the struct _launch hands to lg_engine_forward
    monkeypatch.setattr(_call.Outputs, "io", lambda self, *args, **kw: ios.append(build(self, *args, **kw)) or ios[-1])
    got = model({"image0": a, "image1": b})
    monkeypatch.undo()
    assert len(ios) == 1 and ios[0].desc0 == a["descriptors"].data_ptr() and ios[0].desc1 == b["descriptors"].data_ptr()
    assert ios[0].flags & _cabi.LG_FLAG_DESC0_U8 and ios[0].flags & _cabi.LG_FLAG_DESC1_U8 and not ios[0].flags & (_cabi.LG_FLAG_ROOTSIFT0 | _cabi.LG_FLAG_ROOTSIFT1)
    _assert_same_dict(got, want, (dim, adaptive))
    _assert_same_dict(model({"image0": a, "image1": fb}), want, "image0 uint8, image1 fp32")
    _assert_same_dict(model({"image0": fa, "image1": _with(b, descriptors=b["descriptors"].half())}), want, "image0 fp32, image1 float16")
    assert torch.isfinite(got["matching_scores0"]).all()


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float16, torch.float32])
def test_rootsift_on_entry_bitwise(dtype):
    """descriptor_transform = "rootsift" on a uint8 / float16 / fp32 store == the same call on sift_to_rootsift(store) as fp32 without the key: one side only,
    both sides, and a uint8 store joined with an fp32 one."""
    require_gpu()
    model = _model()
    a, b = _pair_data()
    ra, rb = _with(a, descriptors=sift_to_rootsift(a["descriptors"])), _with(b, descriptors=sift_to_rootsift(b["descriptors"]))
    assert ra["descriptors"].dtype is torch.float32 and "descriptor_transform" not in ra
    want = model({"image0": ra, "image1": rb})
    _has_matches(want)
    ta, tb = (_with(s, descriptors=s["descriptors"].to(dtype), descriptor_transform="rootsift") for s in (a, b))
    st = normalise_side(ta, ta["keypoints"].device, 128, True)
    assert st.rootsift and st.desc.data_ptr() == ta["descriptors"].data_ptr() and st.desc_u8 == (dtype is torch.uint8) and st.desc_f16 == (dtype is torch.float16)
    _assert_same_dict(model({"image0": ta, "image1": tb}), want, "both sides")
    _assert_same_dict(model({"image0": ta, "image1": rb}), want, "image0 on entry, image1 pre-transformed")
    _assert_same_dict(model({"image0": ra, "image1": tb}), want, "image0 pre-transformed, image1 on entry")
    if dtype is torch.uint8:
        fb = _with(b, descriptors=b["descriptors"].float(), descriptor_transform="rootsift")
        _assert_same_dict(model({"image0": ta, "image1": fb}), want, "a uint8 store joined with an fp32 one")
        wrong = model({"image0": ta, "image1": _with(b, descriptors=b["descriptors"].float())})      # the key is per side: image1 without it is another input
        assert not torch.equal(wrong["matching_scores0"], want["matching_scores0"])


def test_rootsift_on_entry_at_256_and_adaptive():
    require_gpu()
    for dim, adaptive in ((256, False), (128, True)):
        model = _model(dim, adaptive)
        a, b = _pair_data(dim=dim)
        want = model({"image0": _with(a, descriptors=sift_to_rootsift(a["descriptors"])), "image1": _with(b, descriptors=sift_to_rootsift(b["descriptors"]))})
        got = model({"image0": _with(a, descriptor_transform="rootsift"), "image1": _with(b, descriptor_transform="rootsift")})
        _assert_same_dict(got, want, (dim, adaptive))
        _has_matches(got)


@pytest.mark.parametrize("dim", [128, 256])
def test_one_preparation_launch_serves_any_two_formats_and_transforms(dim):
    """The preparation kernel picks storage format and transform per side inside one launch: every pair of storage kinds (fp32, float16, uint8) on the two
    sides, with descriptor_transform = "rootsift" on image0 only, on image1 only and on both, == the call on fp32 tensors converted (exact: the values are
    0 .. 255) and transformed beforehand.  n0 = 70 / n1 = 130 cross a 64-row tile, and pair 1 has an empty image0."""
    require_gpu()
    model = _model(dim)
    a, b = _u8_store(5, [70, 0], 70, dim), _u8_store(5, [130, 97], 130, dim)
    kinds = (torch.float32, torch.float16, torch.uint8)
    matched = []
    for root0, root1 in ((True, False), (False, True), (True, True)):
        pre = lambda s, root: _with(s, descriptors=sift_to_rootsift(s["descriptors"]) if root else s["descriptors"].float())
        want = model({"image0": pre(a, root0), "image1": pre(b, root1)})
        matched.append((want["matches0"] > -1).sum(1).tolist())
        assert matched[-1][1] == 0, "the pair with an empty image has no match"
        side = lambda s, kind, root: _with(s, descriptors=s["descriptors"].to(kind), **({"descriptor_transform": "rootsift"} if root else {}))
        for k0 in kinds:
            for k1 in kinds:
                _assert_same_dict(model({"image0": side(a, k0, root0), "image1": side(b, k1, root1)}), want, (dim, root0, root1, k0, k1))
    print(f"dim {dim}: matches per pair with RootSIFT on image0 / image1 / both {matched}")
    assert matched[2][0] > 0, "with both sides transformed pair 0 must produce matches: the equality compares something"


def test_match_pairs_over_an_indexed_uint8_rootsift_store():
    """K = 3, P = 4 with a repeated image and a self pair == forward on the stacked, pre-transformed fp32 tensors; deferred and raw calls carry the key too."""
    require_gpu()
    model = _model()
    store = _u8_store(7, [130, 97, 70], 130)
    pairs = [(0, 1), (1, 2), (0, 2), (1, 1)]
    i0, i1 = torch.tensor([p[0] for p in pairs], device="cuda"), torch.tensor([p[1] for p in pairs], device="cuda")
    pre = _with(store, descriptors=sift_to_rootsift(store["descriptors"]))
    stacked = lambda s, idx: {k: s[k][idx] for k in _PER_IMAGE}
    want = model({"image0": stacked(pre, i0), "image1": stacked(pre, i1)})
    _has_matches(want)
    tagged = _with(store, descriptor_transform="rootsift")
    got = model.match_pairs(tagged, pairs)
    _assert_same_dict(got, want)
    _assert_same_dict(model.match_pairs(tagged, pairs, deferred=True).result(), want, "deferred")
    data = {"image0": _with(stacked(store, i0), descriptor_transform="rootsift"), "image1": _with(stacked(store, i1), descriptor_transform="rootsift")}
    _assert_same_dict(model.forward_deferred(data).result(), want, "forward_deferred")
    raw = model.forward_raw(data)
    torch.cuda.synchronize()
    assert torch.equal(raw["matches0"].long(), want["matches0"]) and torch.equal(raw["matching_scores0"], want["matching_scores0"])
    from lightglue_amd import InflightMatcher, PairShardedMatcher, collate_features, match_batch
    _assert_same_dict(InflightMatcher(model, depth=1).submit(data).result(), want, "InflightMatcher")
    from test_parallel_gpu import _check
    _check(PairShardedMatcher(model)(data), want)      # a world of one: its shard of the batch keeps the key (parallel._take) and the wire row carries the result
    # match_batch collates per-image dicts: the key and the uint8 rows survive the collation (the same lists pre-transformed are the yardstick)
    items = lambda s, idx, **kw: [{**{k: s[k][i][: int(s["num_keypoints"][i])] for k in ("keypoints", "descriptors", "scales", "oris")},
                                   "image_size": s["image_size"][i], **kw} for i in idx.tolist()]
    tag = dict(descriptor_transform="rootsift")
    assert collate_features(items(store, i0, **tag))["descriptors"].dtype is torch.uint8
    per_pair, per_pair_want = match_batch(model, items(store, i0, **tag), items(store, i1, **tag)), match_batch(model, items(pre, i0), items(pre, i1))
    for p, (res, ref) in enumerate(zip(per_pair, per_pair_want)):
        _assert_same_dict(res, ref, ("match_batch", p))
    assert all((res["matches0"] > -1).any() for res in per_pair)


# ---------------------------------------------------------------------------------------------------- lg_rootsift
ROOTSIFT_BOUND = 1e-5    # absolute; outputs lie in [0, 1] and a 128-term fp32 sum of non-negative terms is within 127 * 2^-24 = 7.6e-6 relative in any order


@pytest.mark.parametrize("key,dim", [("desc", 128), ("desc64", 64)])
@pytest.mark.parametrize("rows", [0, 1, 5, 260])
def test_rootsift_kernel_against_the_reference(rows, key, dim):
    require_gpu()
    x = torch.from_numpy(GOLDEN[key][:rows]).cuda()
    want = torch.from_numpy(GOLDEN[f"rootsift_{key}"][:rows]).cuda()
    got = sift_to_rootsift(x)
    assert got.dtype is torch.float32 and got.shape == (rows, dim)
    err = float((got - want).abs().max()) if rows else 0.0
    print(f"lg_rootsift rows {rows} dim {dim}: max |d| against the reference {err:.3e} (bound {ROOTSIFT_BOUND:.0e})")
    assert err <= ROOTSIFT_BOUND
    assert torch.equal(sift_to_rootsift(x.float()), got) and torch.equal(sift_to_rootsift(x.half()), got), "uint8, float32 and float16 rows of the same values"
    assert torch.equal(sift_to_rootsift(x, out_dtype=torch.float16), got.half()), "float16 output: the fp32 result rounded once"
    if rows:
        assert torch.equal(sift_to_rootsift(x.reshape(1, rows, dim))[0], got), "leading dimensions"
        assert float((got.norm(dim=-1) - 1).abs().max()) < 1e-6
    if rows == 260:
        view = x[3:]                                                      # rows are 128 / 64 bytes: a view by whole rows is read where it lies
        assert torch.equal(sift_to_rootsift(view), got[3:])
        odd = torch.empty(4 + x[:8].numel(), dtype=torch.uint8, device="cuda")[4:].view(8, dim).copy_(x[:8])     # 4 bytes off: still four elements
        assert odd.data_ptr() % 16 == 4 and torch.equal(sift_to_rootsift(odd), got[:8])
    if rows == 5 and dim == 128:
        assert float((got[0] - 1 / np.sqrt(128)).abs().max()) < 1e-7, "the all-zero row is uniform"
        with pytest.raises(ValueError, match="eps"):
            sift_to_rootsift(x, eps=1e-7)
        with pytest.raises(ValueError, match="multiple of 4"):
            sift_to_rootsift(x[:, :126])


# ---------------------------------------------------------------------------------------------------- filter_dog_point, sift_features
def _detections(image):
    g = GOLDEN
    return tuple(torch.from_numpy(g[f"{k}_{image}"]).cuda() for k in ("points", "scales", "angles", "scores")) + (tuple(int(v) for v in g[f"shape_{image}"]),)


@pytest.mark.parametrize("by", ["scale", "score"])
@pytest.mark.parametrize("radius", [0, 1, 3])
def test_filter_dog_point_equals_the_reference(radius, by):
    require_gpu()
    pts, scales, angles, scores, shape = _detections("a")
    keep = filter_dog_point(pts, scales, angles, shape, radius, scores=scores if by == "score" else None)
    want = GOLDEN[f"keep_a_r{radius}_{by}"]
    assert keep.dtype is torch.int64 and keep.is_cuda and np.array_equal(keep.cpu().numpy(), want) and 0 < len(want) < len(pts)


def test_filter_dog_point_ragged_batch():
    """K = 2 images of different sizes and counts in one call: every row equals the reference's keep of its image, -1 behind the count."""
    require_gpu()
    a, b = _detections("a"), _detections("b")
    N = 300
    pad = lambda t: torch.cat([t, torch.full((N - len(t),) + tuple(t.shape[1:]), 3.0, device="cuda")])      # rows past the count: inside the image, never read
    stack = lambda i: torch.stack([a[i], pad(b[i])])
    for radius, by in ((1, "score"), (0, "scale"), (3, "score")):
        keep, counts = filter_dog_point(stack(0), stack(1), stack(2), [a[4], b[4]], radius, scores=stack(3) if by == "score" else None,
                                        num_keypoints=torch.tensor([300, 200]))
        assert keep.shape == (2, N) and keep.dtype is torch.int64 and counts.dtype is torch.int64
        for k, name in enumerate("ab"):
            want = GOLDEN[f"keep_{name}_r{radius}_{by}"]
            assert int(counts[k]) == len(want) and np.array_equal(keep[k, : len(want)].cpu().numpy(), want) and (keep[k, len(want):] == -1).all(), (radius, by, name)


def test_filter_dog_point_drops_points_outside_the_image():
    """The documented difference: the reference wraps a negative pixel index and raises on a large one; here such a detection is dropped and the rest is
    filtered as if it were not there."""
    require_gpu()
    pts, scales, angles, scores, shape = _detections("a")
    h, w = shape
    out = torch.tensor([[-0.6, 5.0], [5.0, -3.0], [w + 0.6, 5.0], [5.0, h + 0.51], [1e9, 1e9], [-1e9, 2.0]], device="cuda")
    big = torch.full((len(out),), 100.0, device="cuda")                      # they would win every window they fell into
    zero = torch.zeros(len(out), device="cuda")
    for radius in (0, 3):
        keep = filter_dog_point(torch.cat([out, pts]), torch.cat([big, scales]), torch.cat([zero, angles]), shape, radius, scores=torch.cat([big, scores]))
        assert np.array_equal(keep.cpu().numpy(), GOLDEN[f"keep_a_r{radius}_score"] + len(out))
    edge = torch.tensor([[0.0, 0.0], [w - 0.01, h - 0.01], [0.5, 0.5]], device="cuda")      # the corners are inside: round_half_even(-0.5) = 0; (0.5, 0.5) is pixel 0 too
    keep = filter_dog_point(edge, torch.tensor([1.0, 1.0, 2.0], device="cuda"), torch.zeros(3, device="cuda"), shape, 0)
    assert keep.tolist() == [1, 2]
    assert filter_dog_point(torch.zeros(0, 2, device="cuda"), torch.zeros(0, device="cuda"), torch.zeros(0, device="cuda"), shape, 1).shape == (0,)


def test_sift_features_builds_the_store_the_matcher_reads():
    """Filter + top-k on the golden detections returns the rows the reference's filter + torch.topk would, in its order; the store stays uint8 and goes straight
    into match_pairs."""
    require_gpu()
    topk = int(GOLDEN["topk"])
    desc = torch.from_numpy(GOLDEN["desc"]).cuda()
    pts, scales, angles, scores, (h, w) = _detections("a")
    bp, bs, ba, bsc, (bh, bw) = _detections("b")
    store = sift_features([pts, bp], [scales, bs], [angles, ba], [desc, desc[:200]], [(w, h), (bw, bh)], scores=[scores, bsc], nms_radius=0, max_num_keypoints=topk)
    assert store["descriptors"].dtype is torch.uint8 and store["descriptors"].shape == (2, topk, 128) and store["descriptor_transform"] == "rootsift"
    assert store["num_keypoints"].tolist() == [topk, topk] and store["image_size"].tolist() == [[w, h], [bw, bh]]
    want = GOLDEN["topk_a"]
    got_scores = store["keypoint_scores"][0].cpu().numpy()
    assert (np.diff(got_scores) < 0).all(), "descending score"
    assert set(got_scores.tolist()) == set(GOLDEN["scores_a"][want].tolist())
    assert np.array_equal(store["keypoints"][0].cpu().numpy(), GOLDEN["points_a"][want]) and np.array_equal(store["descriptors"][0].cpu().numpy(), GOLDEN["desc"][want])
    assert np.array_equal(store["scales"][0].cpu().numpy(), GOLDEN["scales_a"][want]) and np.array_equal(store["oris"][0].cpu().numpy(), GOLDEN["angles_a"][want])
    out = _model().match_pairs(store, [(0, 1), (0, 0)])
    assert out["matches0"].shape == (2, topk) and (out["matches0"][1] > -1).any(), "an image matches itself"
    # without scores nothing is cut; rootsift = True transforms now, False leaves the rows alone
    keep = GOLDEN["keep_a_r1_scale"]
    now = sift_features(pts, scales, angles, desc, (w, h), nms_radius=1, rootsift=True)
    assert now["descriptors"].dtype is torch.float32 and "descriptor_transform" not in now and "keypoint_scores" not in now and now["num_keypoints"].tolist() == [len(keep)]
    assert torch.equal(now["descriptors"][0], sift_to_rootsift(desc[torch.from_numpy(keep).cuda()]))
    raw = sift_features(pts, scales, angles, desc, (w, h), nms_radius=None, rootsift=False)
    assert raw["descriptors"].dtype is torch.uint8 and "descriptor_transform" not in raw and torch.equal(raw["descriptors"][0], desc)
